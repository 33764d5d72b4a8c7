"""The device overlap and fm-merge at the shapes that the 50-base sets of test_overlap_host and test_fmmerge_host never reach,
checked without a GPU: chains of more than 64 blocks, reads of unequal length in one call, reads at the length limit, the
boundary of a read's output.  The yardsticks are those modules' (plain_overlap_exact, brute_edge_lines, plain_fmmerge); every
comparison is exact.  test_gpu_overlap_shapes and test_gpu_fmmerge_shapes run the same sets through the kernels.

What each set reaches in csrc/fm_overlap.h and capi_overlap.cpp:

  trim_in_the_second_tile   reads of 300 bases at step 2, m = 20: a chain emits up to 140 blocks of interval size 1, ascending.
                            TrimOBLInterval's sum reaches 128 at block 127, the last lane of the second 64-lane tile, with 64
                            carried from the first tile in ov_reduce_read's `acc`.
  trim_carries_127          the 63 farthest followers of read 0 twice, the next once: the first tile sums to 127, and the first
                            lane of the second tile hits.
  trim_at_the_tile_s_end    every read twice: the sum is exactly 128 at block 63, the last lane of the first tile.
  trim_sizes_one_and_two    every second start twice: sizes 1, 2, 1, 2, ...; the first tile sums to 96, the hit is at block 84.
  monotone_mixed_lengths    reads of 40 .. 400 bases of both strands and both haplotypes, starts and ends strictly increasing: no
                            read is a substring of another, so the edges are also those of the definition (brute_edge_lines).
                            A chain's slots are sized from the call's longest read while each read emits by its own length, and
                            OverlapProcess's coordinates take the query's and the target's length, which differ here.
  joined_list_above_64      reads of 300 bases at step 2 on alternating strands, with a periodic stretch at the end of read 0 and
                            a short read that starts with two suffixes of it: suffixFwd of read 0 has more than 64 blocks and a
                            removeSubMaximalBlocks resolution (ov_rank_sort and ov_resolve_serial above one tile), and suffixFwd
                            joined with suffixRev has more than 128 (the compaction, the join and ov_irreducible in three tiles).
  at_the_limits             three reads of kOvMaxRead = 2000 bases that overlap by 1990 and 1000 among 50-base reads, with m = 20
                            and with m = kOvMaxMinOverlap = 2000 (containments only).
  out_cap_boundary          _fan(n): read 0 ends with exactly kOvOutCap = 256 final blocks, and with 257, which is the overflow.
  two_chunks_by_length      (GPU) the index of the `random` set and the three 2000-base reads, one call of 800 query reads: with
                            max_len = 2000 overlap_plan's chunk is 704 reads, so lrsc_overlap_exact's own chunk loop runs twice.
  fm-merge                  monotone_mixed_lengths of one haplotype, in shuffled order on random strands, whole and with holes:
                            the sequences are the genome's pieces.  Long chains whose last read has 2000 bases: lrsc_fmmerge
                            takes two chunks below the cap of 32768.

The sum that TrimOBLInterval walks grows by at least 1 per block, so it reaches 128 at block 127 at the latest: whatever a chain
holds, the trim's hit lies in its first or second tile.  A set with a hit in a third tile cannot be built; the lists above 128
blocks (joined_list_above_64) run the other loops there.
"""
from __future__ import annotations

import re
import subprocess

import numpy as np
import pytest

from .conftest import REPO
from .test_fmmerge_host import REVERSED, _fan, check_invariant, plain_fmmerge, run_fmmerge_driver
from .test_fmmerge_host import _build as _build_fmmerge
from .test_index_filter_host import LAYOUTS, _image_input, _rand, revcomp
from .test_index_locate_host import naive_sa
from .test_index_merge_host import CODE
from .test_overlap_host import (COMP, M, OV_SETS, OVERLAP_BLOCK_DTYPE, OVERLAP_READ_DTYPE, PATH, PRE_PRE, SUF_PRE, Index, _const, brute_edge_lines,
                                find_overlap_blocks_exact, plain_overlap_exact, plain_overlap_text, reads_input)
from .test_overlap_host import _build as _build_overlap

LRSC_OVERLAP_OVERFLOW = 1
LANES = 64


# ---- the plan's chunk, from the constants of fm_overlap.h and capi_overlap.cpp -----------------------------------------------------
def _capi_const(name: str) -> int:
    m = re.search(rf"constexpr uint64_t {name} = (\d+)ull << (\d+);", (REPO / "longreadselfcorrect_amd/csrc/capi_overlap.cpp").read_text())
    assert m, name
    return int(m.group(1)) << int(m.group(2))


def _sizeof(name: str) -> int:
    m = re.search(rf"sizeof\({name}\) == (\d+)", (REPO / "longreadselfcorrect_amd/csrc/fm_overlap.h").read_text())
    assert m, name
    return int(m.group(1))


def plan_chunk(max_len: int, m: int) -> int:
    """overlap_plan's chunk before it is cut to the number of reads: what the chains of a chunk leave stays below kOvChainBytes"""
    header = (REPO / "longreadselfcorrect_amd/csrc/fm_overlap.h").read_text()
    assert "constexpr uint32_t kOvReadsPerWave = kOvLanes / kOvChains;" in header and "constexpr uint32_t kOvLanes = kWaveLanes;" in header
    chains, per_wave = _const("kOvChains"), LANES // _const("kOvChains")
    slots = max_len - m if max_len > m else 0
    per_read = chains * (slots * _sizeof("OvBlock") + _sizeof("OvChainHead"))
    return min(_capi_const("kOvChunkReads"), max(per_wave, _capi_const("kOvChainBytes") // per_read // per_wave * per_wave))


def test_the_chunk_follows_the_longest_read():
    assert plan_chunk(50, 20) == plan_chunk(55, 20) == plan_chunk(50, 10) == _capi_const("kOvChunkReads") == 32768      # every set of the two older modules
    assert plan_chunk(2000, 20) == 704 and plan_chunk(2000, 30) == 704 and plan_chunk(400, 20) == 3664
    assert plan_chunk(2000, 2000) == 32768 and plan_chunk(2000, 2) == 16 * (plan_chunk(2000, 2) // 16) < 704


# ---- the sets ----------------------------------------------------------------------------------------------------------------
_G1 = _rand(0x1E01, 600)
_LONG = _rand(0x1E04, 3010)
LONG_READS = [_LONG[0:2000], _LONG[10:2010], _LONG[1010:3010]]    # overlaps of 1990, of 1000 and of 990
_UNIT = "ACGTT"
# joined_list_above_64: read 0 ends with six units, the genome goes on with other bases; the short read starts with five units
_G3 = _rand(0x1E05, 270) + _UNIT * 6 + _rand(0x1E06, 300)
_SHORT_PERIODIC = _UNIT * 5 + _rand(0x1E07, 25)


def _step2(genome: str, n: int, copies=lambda i: 1) -> list[str]:
    return [genome[2 * i: 2 * i + 300] for i in range(n) for _ in range(copies(i))]


def _monotone(seed: int, n: int, m: int, genomes: list[str], flip: bool = True) -> tuple[list[str], list[tuple]]:
    """n reads whose starts and ends both increase strictly, consecutive ones overlapping by m bases or more, each from one of
    the genomes and, where flip, on a random strand: (the reads, their (start, end))"""
    rng = np.random.default_rng(seed)
    reads, spans, start, end = [], [], 0, 0
    for i in range(n):
        # a read that is shorter than the one before starts later by more than the difference: the lengths follow a wave between
        # 40 and 400 bases, 80 reads from crest to crest, with steps of up to 30 bases
        wave = 40 + 9 * abs(i % 80 - 40)
        if i:
            start += int(rng.integers(1, min(30, spans[-1][1] - spans[-1][0] - m) + 1))
        end = max(end + 1, start + min(400, max(40, wave + int(rng.integers(-12, 13)))))
        assert end <= len(genomes[0])
        r = genomes[int(rng.integers(len(genomes)))][start: end]
        reads.append(revcomp(r) if flip and rng.integers(2) else r)
        spans.append((start, end))
    return reads, spans


_G2 = _rand(0x1E08, 4000)
_SITES = (700, 1500, 2300)
_H2 = "".join("ACGT"[("ACGT".index(b) + 1) % 4] if i in _SITES else b for i, b in enumerate(_G2))
FAN_FITS, FAN_OVERFLOWS = 254, 255                                # _fan(n): read 0's two containment blocks and n blocks on its sense end

SHAPE_SETS = {
    "trim_in_the_second_tile": lambda: (_step2(_G1, 136), M),
    "trim_carries_127": lambda: (_step2(_G1, 76, lambda i: 2 if i >= 13 else 1), M),
    "trim_at_the_tile_s_end": lambda: (_step2(_G1, 68, lambda i: 2), M),
    "trim_sizes_one_and_two": lambda: (_step2(_G1, 92, lambda i: 1 + (i & 1)), M),
    "monotone_mixed_lengths": lambda: (_monotone(0x1E09, 160, M, [_G2, _H2])[0], M),
    "joined_list_above_64": lambda: ([revcomp(r) if i & 1 else r for i, r in enumerate(_step2(_G3, 142))] + [_SHORT_PERIODIC], M),
    "at_the_limits": lambda: (PATH[:8] + LONG_READS + PATH[8:], M),
    "at_the_limits_m_2000": lambda: (PATH[:8] + LONG_READS + PATH[8:] + [revcomp(LONG_READS[1])], 2000),
    "out_cap_fits": lambda: (_fan(FAN_FITS), M),
    "out_cap_overflows": lambda: (_fan(FAN_OVERFLOWS), M),
    "random_and_the_long_reads": lambda: (OV_SETS["random"]()[0] + LONG_READS, M),
}
TRIMS = [n for n in SHAPE_SETS if n.startswith("trim_")]
HOST_SETS = [n for n in SHAPE_SETS if n != "random_and_the_long_reads"]              # that one is the two-chunk call's index
SANITIZED = TRIMS + ["joined_list_above_64", "at_the_limits", "at_the_limits_m_2000", "out_cap_fits", "out_cap_overflows"]
_SH: dict = {}


def shape_case(name: str) -> dict:
    """the set with its yardstick, computed once and left unchanged: names, reads, m, ix, results, traces, asqg, edges, and the
    drivers' input up to the reads (both strands' images, which overlap_driver and fmmerge_driver read alike)"""
    if name not in _SH:
        reads, m = SHAPE_SETS[name]()
        names = [f"read{i}" for i in range(len(reads))]
        ix = Index(reads)
        traces = [[] for _ in reads]
        results = [plain_overlap_exact(ix, r, m, t) for r, t in zip(reads, traces)]
        asqg, edges = plain_overlap_text(names, reads, m, f"{name}.fa", results, ix)
        _SH[name] = dict(names=names, reads=reads, m=m, ix=ix, results=results, traces=traces, asqg=asqg, edges=edges)
    return _SH[name]


def expected_status(name: str) -> list[dict]:
    """what the entry gives per read: the yardstick's result with status 0, or the overflow and no blocks where the yardstick has
    more final blocks than a read's output holds"""
    cap = _const("kOvOutCap")
    return [dict(r, status=0) if len(r["blocks"]) <= cap else dict(is_substring=r["is_substring"], blocks=[], status=LRSC_OVERLAP_OVERFLOW) for r in shape_case(name)["results"]]


def chain_list(name: str, read: int, rev: bool) -> tuple[list, list]:
    """(the blocks, the containment blocks) that findOverlapBlocksExact leaves of the read's suffixFwd chain, or suffixRev's, in the
    order of the search: ascending overlap length"""
    c = shape_case(name)
    blocks, contain = [], []
    if rev:
        find_overlap_blocks_exact(c["reads"][read].translate(COMP), c["ix"].rbwt, c["ix"].bwt, PRE_PRE, c["m"], blocks, contain, {})
    else:
        find_overlap_blocks_exact(c["reads"][read], c["ix"].bwt, c["ix"].rbwt, SUF_PRE, c["m"], blocks, contain, {})
    return blocks, contain


def _sizes(blocks: list) -> list[int]:
    return [b.r[3] - b.r[2] + 1 for b in blocks]


def _trims(name: str, read: int) -> list[tuple]:
    """(erased, kept) of the read's trim events"""
    return [(len(t[1]), len(t[2])) for t in shape_case(name)["traces"][read] if t[0] == "trim"]


def test_the_trim_sets_hold_what_they_are_named_for():
    assert _const("kOvTrimSum") == 128
    # 135 followers of read 0, a row each: the sum is 128 at block 127, which goes with the seven longer ones
    blocks, _ = chain_list("trim_in_the_second_tile", 0, False)
    assert len(blocks) == 135 and set(_sizes(blocks)) == {1} and [b.len for b in blocks] == list(range(30, 300, 2))
    assert _trims("trim_in_the_second_tile", 0)[0] == (8, 127)
    assert sum(1 for r in range(136) if (k := _trims("trim_in_the_second_tile", r)) and k[0][1] == 127 and k[0][0] >= 1) >= 8
    # the first tile's 64 blocks sum to 127: the hit is block 64, with nothing but the carried sum to show for it
    blocks, _ = chain_list("trim_carries_127", 0, False)
    sizes = _sizes(blocks)
    assert len(blocks) == 75 and sizes[:63] == [2] * 63 and sizes[63:] == [1] * 12 and sum(sizes[:LANES]) == 127
    assert _trims("trim_carries_127", 0)[0] == (11, 64)
    # every block holds two rows: exactly 128 at the first tile's last lane
    blocks, _ = chain_list("trim_at_the_tile_s_end", 0, False)
    assert len(blocks) == 67 and set(_sizes(blocks)) == {2} and _trims("trim_at_the_tile_s_end", 0)[0] == (4, 63)
    # sizes 2, 1, 2, 1, ... from the shortest overlap: 96 after the first tile, 128 at block 84 in the second
    blocks, _ = chain_list("trim_sizes_one_and_two", 0, False)
    sizes = _sizes(blocks)
    assert len(blocks) == 91 and sizes[:4] == [2, 1, 2, 1] and sum(sizes[:LANES]) == 96 and sum(sizes[:84]) == 126 and sum(sizes[:85]) == 128
    assert _trims("trim_sizes_one_and_two", 0)[0] == (7, 84)
    # with the block count alone (one row each) that list would not be trimmed at all
    assert len(blocks) < 128


def test_the_mixed_length_set_holds_what_it_is_named_for():
    c = shape_case("monotone_mixed_lengths")
    _, spans = _monotone(0x1E09, 160, M, [_G2, _H2])
    assert all(a[0] < b[0] and a[1] < b[1] for a, b in zip(spans, spans[1:])) and [len(r) for r in c["reads"]] == [e - s for s, e in spans]
    lengths = [len(r) for r in c["reads"]]
    assert min(lengths) <= 40 and max(lengths) >= 400 and len(set(lengths)) > 80 and sum(1 for a, b in zip(_G2, _H2) if a != b) == 3
    assert not any(r["is_substring"] for r in c["results"]) and not any(t[0] == "trim" for tr in c["traces"] for t in tr)
    assert sum(1 for tr in c["traces"] for t in tr if t[0] == "split") >= 1
    # the independent check, by definition
    lines = c["edges"].splitlines(keepends=True)
    assert set(lines) == brute_edge_lines(c["names"], c["reads"], c["m"]) and len(lines) == len(set(lines)) and len(lines) > 150
    # an edge between the strands whose two reads differ in length: swapping queryLen and targetLen would show in its coordinates
    crossed = [f for f in (line[3:].split() for line in lines) if f[8] == "1" and f[4] != f[7]]
    assert len(crossed) > 20 and any(int(f[5]) != 0 for f in crossed) and any(int(f[2]) == 0 for f in crossed)


def test_the_joined_list_set_holds_what_it_is_named_for():
    c = shape_case("joined_list_above_64")
    assert c["reads"][0] == _G3[:300] and c["reads"][0].endswith(_UNIT * 6) and c["reads"][142] == _SHORT_PERIODIC and c["results"][0]["is_substring"] == 0
    fwd, fwd_contain = chain_list("joined_list_above_64", 0, False)
    rev, rev_contain = chain_list("joined_list_above_64", 0, True)
    # suffixFwd: the 70 overlap lengths of the reads of its own strand, and 23 and 25, the second overlaps that the periodic stretch
    # gives the read that starts 28 bases before read 0's end and the short read; suffixRev: 70 of the other strand, and 20, 21, 25;
    # no trim
    assert len(fwd) == 72 and len(rev) == 73 and sum(_sizes(fwd)) < 128 and sum(_sizes(rev)) < 128 and not _trims("joined_list_above_64", 0)
    assert {b.len for b in fwd} == set(range(20, 300, 4)) | {23, 25} and {b.len for b in rev} == set(range(22, 300, 4)) | {20, 21, 25}
    assert len(fwd_contain) == 1 and len(rev_contain) == 0
    # the resolutions, on lists of more than 64: a read leaves the block of its shorter overlap, which is then empty
    resolved = [t for t in c["traces"][0] if t[0] == "submaximal"]
    assert resolved[0] == ("submaximal", 25, 20, 1) and len(resolved) == 5 and all(t[3] == 1 for t in resolved)
    # the join of both, a resolution taking a block at the most
    assert len(fwd) + len(rev) - len(resolved) == 140 > 2 * LANES
    assert sum(1 for r in range(143) if len(chain_list("joined_list_above_64", r, False)[0]) + len(chain_list("joined_list_above_64", r, True)[0]) > 2 * LANES) >= 1


def test_the_limit_sets_hold_what_they_are_named_for():
    assert _const("kOvMaxRead") == 2000 == _const("kOvMaxMinOverlap") and [len(r) for r in LONG_READS] == [2000] * 3
    c = shape_case("at_the_limits")
    assert c["reads"][8: 11] == LONG_READS and not any(r["is_substring"] for r in c["results"])
    assert "ED\tread9 read8 0 1989 2000 10 1999 2000 0 0\n" in c["edges"] and "ED\tread9 read10 1000 1999 2000 0 999 2000 0 0\n" in c["edges"]
    assert "read8 read10" not in c["edges"] and "read10 read8" not in c["edges"]                  # the overlap of 990 is transitive
    blocks, _ = chain_list("at_the_limits", 8, False)
    assert [b.len for b in blocks] == [990, 1990]
    # m at the limit: the reads below it have no result, the long ones their containment blocks, one edge for the pair
    e = shape_case("at_the_limits_m_2000")
    assert all(b["contained"] for r in e["results"] for b in r["blocks"]) and [len(r["blocks"]) for r in e["results"]][8: 11] == [2, 4, 2]
    assert all(r == dict(is_substring=0, blocks=[]) for i, r in enumerate(e["results"]) if len(e["reads"][i]) == 50)
    assert e["edges"] == "ED\tread9 read29 0 1999 2000 0 1999 2000 1 0\n"
    # the boundary of a read's output
    cap = _const("kOvOutCap")
    assert len(shape_case("out_cap_fits")["results"][0]["blocks"]) == cap and len(shape_case("out_cap_overflows")["results"][0]["blocks"]) == cap + 1
    assert max(len(r["blocks"]) for r in shape_case("out_cap_overflows")["results"][1:]) < cap
    assert [x["status"] for x in expected_status("out_cap_overflows")] == [LRSC_OVERLAP_OVERFLOW] + [0] * FAN_OVERFLOWS
    assert all(x["status"] == 0 for x in expected_status("out_cap_fits"))


# ---- the overlap driver ----------------------------------------------------------------------------------------------------------
def status_dicts(per_read: np.ndarray, blocks: np.ndarray) -> list[dict]:
    """test_overlap_host's result_dicts with the read's status returned, not asserted; first_block is contiguous and ascending in
    read order"""
    out, at = [], 0
    for q in per_read:
        assert q["pad"] == 0 and int(q["first_block"]) == at, (at, q)
        mine = blocks[at: at + int(q["n_blocks"])]
        at += int(q["n_blocks"])
        out.append(dict(is_substring=int(q["is_substring"]), blocks=[{k: int(b[k]) for k in OVERLAP_BLOCK_DTYPE.names} for b in mine], status=int(q["status"])))
    assert at == len(blocks)
    return out


def _images(c: dict) -> bytes:
    if "images" not in c:
        c["images"] = _image_input(naive_sa(c["reads"])[0]) + _image_input(naive_sa([r[::-1] for r in c["reads"]])[0])
    return c["images"]


def run_shape_driver(exe: str, name: str, wide: int) -> list[dict]:
    c = shape_case(name)
    bases, off = reads_input(c["reads"])
    n = len(c["reads"])
    blob = b"".join([_images(c), np.array([c["m"]], dtype=np.int32).tobytes(), np.array([n], dtype=np.uint64).tobytes(), off.tobytes(), bytes(CODE[chr(x)] - 1 for x in bases)])
    r = subprocess.run([exe, str(wide)], input=blob, capture_output=True)
    assert r.returncode == 0, (name, wide, r.returncode, r.stderr[-2000:])
    per_read = np.frombuffer(r.stdout, dtype=OVERLAP_READ_DTYPE, count=n)
    total = int(per_read["n_blocks"].sum())
    blocks = np.frombuffer(r.stdout, dtype=OVERLAP_BLOCK_DTYPE, count=total, offset=n * 24)
    assert n * 24 + total * 24 + 16 == len(r.stdout)
    return status_dicts(per_read, blocks)


def _run_sets(exe: str, wide: int, names) -> int:
    for name in names:
        got, want = run_shape_driver(exe, name, wide), expected_status(name)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, wide, i)
    return len(names)


@pytest.fixture(scope="module")
def overlap_driver(tmp_path_factory):
    return _build_overlap(tmp_path_factory.mktemp("overlap_shapes") / "overlap_driver")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_field_equals_the_yardstick(overlap_driver, layout):
    assert _run_sets(overlap_driver, LAYOUTS[layout], HOST_SETS) == 10


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: the trims, the long lists, the 2000-base reads (the largest slices and chain arrays) and
    the full output, both layouts"""
    exe = _build_overlap(tmp_path / "overlap_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        _run_sets(exe, wide, SANITIZED)


# ---- fm-merge: mixed lengths ---------------------------------------------------------------------------------------------------
_G4 = _rand(0x1E0A, 4200)
_G5 = _rand(0x1E0B, 9500)


def _pieces(spans: list[tuple], holes: list[int], width: int, m: int) -> tuple[list[int], list[tuple]]:
    """`width` reads taken out from every hole on -> (the reads kept, (first, last) kept read of every piece); the reads on both
    sides of a hole share fewer than m bases"""
    gone = {h + i for h in holes for i in range(width)}
    kept = [i for i in range(len(spans)) if i not in gone]
    pieces, start = [], 0
    for h in holes + [len(spans)]:
        pieces.append((start, h - 1))
        start = h + width
    for first, last in pieces[:-1]:
        assert spans[last][1] - spans[last + width + 1][0] < m, "the hole is too narrow"
    return kept, pieces


def _merge_set(genome: str, spans: list[tuple], kept: list[int], pieces: list[tuple], seed: int) -> dict:
    """the kept reads in shuffled order, each on a random strand, and the sequences they merge into by construction: the genome's
    pieces, each on the strand of its lowest-numbered read, in the order of those reads"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(kept))
    flip = rng.integers(0, 2, size=len(kept))
    which = [kept[i] for i in order]
    reads = [revcomp(genome[spans[p][0]: spans[p][1]]) if f else genome[spans[p][0]: spans[p][1]] for p, f in zip(which, flip)]
    number = {p: i for i, p in enumerate(which)}
    want = []
    for first, last in pieces:
        members = [number[p] for p in range(first, last + 1)]
        root = min(members)
        text = genome[spans[first][0]: spans[last][1]]
        want.append((root, dict(bases=revcomp(text) if flip[root] else text, n_reads=len(members), root=root, circular=0)))
    want = [w for _, w in sorted(want, key=lambda x: x[0])]
    offsets = {}
    for first, last in pieces:
        for p in range(first, last + 1):
            offsets[number[p]] = (spans[p][0] - spans[first][0], spans[last][1] - spans[p][1])   # from the piece's left end, from its right end
    return dict(reads=reads, flip=[int(f) for f in flip], want=want, offsets=offsets)


def _mixed_merge(holes: list[int]):
    _, spans = _monotone(0x1E0C, 170, M, [_G4], flip=False)
    kept, pieces = _pieces(spans, holes, 12, M)
    return _merge_set(_G4, spans, kept, pieces, 0x1E0D), M


def _long_chain_merge():
    """50-base reads at step 10 as in test_gpu_fmmerge's long chains, m = 30, and a last read of 2000 bases that overlaps its
    neighbour by 40: three holes, four pieces, 724 reads; overlap_plan's chunk is 704"""
    n_pos, m = 733, 30
    spans = [(10 * p, 10 * p + 50) for p in range(n_pos - 1)] + [(10 * (n_pos - 1), 10 * (n_pos - 1) + 2000)]
    kept, pieces = _pieces(spans, [100, 380, 700], 3, m)
    return _merge_set(_G5, spans, kept, pieces, 0x1E0E), m


MERGE_SETS = {
    "monotone_mixed_lengths": lambda: _mixed_merge([]),
    "monotone_mixed_lengths_with_holes": lambda: _mixed_merge([44, 124]),
    "two_chunks_by_length": _long_chain_merge,
}
_MG: dict = {}


def merge_case(name: str) -> dict:
    """reads, m, ix, results, merged (plain_fmmerge), and by construction: want (the sequences), flip, offsets"""
    if name not in _MG:
        built, m = MERGE_SETS[name]()
        ix = Index(built["reads"])
        c = dict(built, names=[f"read{i}" for i in range(len(built["reads"]))], m=m, ix=ix, results=[plain_overlap_exact(ix, r, m) for r in built["reads"]])
        c["merged"] = plain_fmmerge(c)
        _MG[name] = c
    return _MG[name]


def check_merged(c: dict, got: dict):
    """the sequences are those of the construction and the yardstick's, every read stands where the construction puts it, on the
    strand that its piece's lowest-numbered read decides"""
    assert got["seqs"] == c["want"] and got["seqs"] == c["merged"]["seqs"]
    assert got["per_read"] == c["merged"]["per_read"] and got["fasta"] == c["merged"]["fasta"]
    check_invariant(c["reads"], got["per_read"], got["seqs"])
    for i, (seq, flags, offset) in enumerate(got["per_read"]):
        root_flipped = c["flip"][c["want"][seq]["root"]]
        assert flags == (REVERSED if c["flip"][i] != root_flipped else 0), i
        assert offset == c["offsets"][i][root_flipped], i


@pytest.mark.parametrize("name", list(MERGE_SETS))
def test_the_merge_sets_hold_what_they_are_named_for(name):
    c = merge_case(name)
    lengths = [len(r) for r in c["reads"]]
    if name == "two_chunks_by_length":
        chunk = plan_chunk(max(lengths), c["m"])
        assert max(lengths) == 2000 and sorted(lengths)[-2] == 50 and chunk == 704 < len(c["reads"]) == 724 < 2 * chunk and len(c["want"]) == 4
        assert c["want"][-1]["bases"] in (_G5[7030: 9320], revcomp(_G5[7030: 9320])) or any(len(w["bases"]) == 2290 for w in c["want"])
    else:
        assert min(lengths) <= 41 and max(lengths) >= 399 and len(set(lengths)) > 60
        assert len(c["want"]) == (3 if name.endswith("holes") else 1) and sum(w["n_reads"] for w in c["want"]) == len(c["reads"]) == (146 if name.endswith("holes") else 170)
    assert 0 < sum(c["flip"]) < len(c["reads"]) and any(p[1] & REVERSED for p in c["merged"]["per_read"])
    check_merged(c, c["merged"])


@pytest.fixture(scope="module")
def fmmerge_driver(tmp_path_factory):
    return _build_fmmerge(tmp_path_factory.mktemp("fmmerge_shapes") / "fmmerge_driver")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_merge_driver_equals_the_yardstick_and_the_construction(fmmerge_driver, layout):
    for name in MERGE_SETS:
        c = merge_case(name)
        check_merged(c, run_fmmerge_driver(fmmerge_driver, c["reads"], c["m"], LAYOUTS[layout], c["ix"]))


def test_the_merge_driver_refuses_the_read_whose_output_overflows(fmmerge_driver):
    """256 final blocks fit: read 0 has 254 blocks on one end, no link, and the set is one of singletons; 257 are the overflow"""
    fits = shape_case("out_cap_fits")
    got = run_fmmerge_driver(fmmerge_driver, fits["reads"], M, 0, fits["ix"])
    assert got == plain_fmmerge(fits) and [s["n_reads"] for s in got["seqs"]] == [1] * (FAN_FITS + 1) and [s["bases"] for s in got["seqs"]] == fits["reads"]
    over = shape_case("out_cap_overflows")
    for wide in LAYOUTS.values():
        assert run_fmmerge_driver(fmmerge_driver, over["reads"], M, wide, over["ix"]) == (1, 0)


def test_merge_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: the mixed-length sets, both layouts"""
    exe = _build_fmmerge(tmp_path / "fmmerge_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        for name in ("monotone_mixed_lengths", "monotone_mixed_lengths_with_holes"):
            c = merge_case(name)
            check_merged(c, run_fmmerge_driver(exe, c["reads"], c["m"], wide, c["ix"]))
