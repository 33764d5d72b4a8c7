"""The device duplicate check and read removal (csrc/fm_dup.h, fm_dup.hip, fm_remove.h, fm_remove.hip) checked without a GPU.

1. The per-lane functions that the kernels call, compiled for the CPU (tests/host_tools/dup_driver.cpp, remove_driver.cpp) and
   run in the kernels' order on images made by build_strand_image.  The yardsticks are written out here: for the duplicate check
   the plain definition (plain_dupcheck: proper-substring test, the reads sorted by (sequence, id) for the '$' ranks, the first
   in input order wins), for the removal the suffix sort of the kept reads (naive_sa).  Classes and both '$' intervals of every
   read, the compacted codes and the packed image exactly; both layouts, both strands, the kernels' tile and one of 384 rows.
2. The drivers again under AddressSanitizer and UBSan, as stand-alone programs.
3. The four entries and the result record are declared, exported and bound, the ABI version is still 2; `stride filter` refuses
   what it must and is listed.
4. The kernels compile for gfx950 without scratch, spills or AGPRs, the walks within the registers their launch is sized for.
"""
from __future__ import annotations

import bisect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_gpu_index_build import EDGE_SETS
from .test_index_locate_host import naive_sa
from .test_index_merge_host import CODE, _random_reads
from .test_index_unrle_host import encode

LLVM = Path("/opt/rocm/lib/llvm/bin")
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
LAYOUTS = {"block32": 0, "block64": 1}                           # the drivers' <wide>
SHAPES = {"kernel_tile": 0, "small_tile": 1}                     # remove_driver's <small>
SMALL_TILE = 384
DUP_DTYPE = np.dtype([("fwd_lower", "<i8"), ("fwd_upper", "<i8"), ("rvc_lower", "<i8"), ("rvc_upper", "<i8"), ("cls", "<i4"), ("pad", "<u4")])
UNIQUE, SUBSTRING, FULL_LENGTH, ABSENT = range(4)


def _const(header: str, name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", (REPO / "longreadselfcorrect_amd/csrc" / header).read_text())
    assert m, name
    return int(m.group(1))


def kernel_tile() -> int:
    assert re.search(r"kRemoveTile = kRemoveLanes \* 16;", (REPO / "longreadselfcorrect_amd/csrc/fm_remove.h").read_text())
    return _const("fm_remove.h", "kRemoveLanes") * 16


def revcomp(s: str) -> str:
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _rand(seed: int, n: int, alphabet: str = "ACGT") -> str:
    return "".join(np.random.default_rng(seed).choice(list(alphabet), size=n))


# ---- the yardstick of the duplicate check: the plain definition -------------------------------------------------------
def plain_dupcheck(index_reads: list[str], calls: list[list[str]]) -> list[np.ndarray]:
    """One DUP_DTYPE array per call of one session.  A read w with reverse complement rc is SUBSTRING when w or rc is a proper
    substring of a read of the index, ABSENT when neither is a read of it; otherwise its canonical index is the smaller valid
    lower of the two '$' intervals, UNIQUE when that bit is clear (the read sets it), FULL_LENGTH when it is set.  The '$'
    interval of a string is the range it takes among the index's reads sorted by (sequence, id), {0, -1} when it is none of
    them; reads are taken in input order, calls in call order."""
    order = [s for s, _ in sorted((s, i) for i, s in enumerate(index_reads))]
    distinct = sorted(set(index_reads), key=len, reverse=True)

    def dollar(s):
        lo, hi = bisect.bisect_left(order, s), bisect.bisect_right(order, s) - 1
        return (lo, hi) if hi >= lo else (0, -1)

    def contained(s):
        return any(len(r) > len(s) and s in r for r in distinct)

    bits = set()
    out = []
    for reads in calls:
        res = np.zeros(len(reads), dtype=DUP_DTYPE)
        for i, w in enumerate(reads):
            rc = revcomp(w)
            f, r = dollar(w), dollar(rc)
            res[i]["fwd_lower"], res[i]["fwd_upper"], res[i]["rvc_lower"], res[i]["rvc_upper"] = f + r
            if contained(w) or contained(rc):
                res[i]["cls"] = SUBSTRING
            elif f[1] < f[0] and r[1] < r[0]:
                res[i]["cls"] = ABSENT
            else:
                canonical = min(x[0] for x in (f, r) if x[1] >= x[0])
                res[i]["cls"] = FULL_LENGTH if canonical in bits else UNIQUE
                bits.add(canonical)
        out.append(res)
    return out


# ---- the sets of the duplicate check: (reads of the index, calls of one session) ---------------------------------------
X, Y, Z, B = _rand(101, 40), _rand(102, 43), _rand(103, 37), _rand(104, 60)
PAL = "ACGTTGCAAC" + revcomp("ACGTTGCAAC")                        # w == revcomp(w)
NOT_THERE = ("C" if B[0] != "C" else "G") + B[1:]                 # B with another first base: its search dies at the last step


def _whole(reads):
    return reads, [reads]


def _short_and_below_k():
    rng = np.random.default_rng(33)
    reads = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(1, 13, size=60)]
    return reads + reads[:10] + [revcomp(r) for r in reads[10:20]]


DUP_SETS = {
    "three_copies": lambda: _whole([X, Y, X, Z, X]),
    "rc_second": lambda: _whole([X, Y, revcomp(X), Z]),
    "rc_first": lambda: _whole([revcomp(X), Y, X, Z]),
    "palindrome_alone": lambda: _whole([PAL, Y]),
    "palindrome_twice": lambda: _whole([PAL, Y, PAL]),
    "substrings": lambda: _whole([B, B[:20], B[40:], B[20:40], revcomp(B[:25]), revcomp(B[35:]), revcomp(B[10:30]), Y]),
    "substring_with_twin": lambda: _whole([B, B[5:25], Y, B[5:25]]),
    "absent": lambda: ([B, Y], [[B, NOT_THERE, Y, Z, revcomp(NOT_THERE)]]),
    "one_base": lambda: (["G"], [["G", "C", "A", "G"]]),
    "one_base_reads": lambda: _whole(["A", "C", "G", "T", "A"]),
    "below_k": lambda: _whole(_short_and_below_k()),
    "all_A_all_T": lambda: _whole(["A" * 50, "T" * 50, "A" * 50, "A" * 20, "T" * 7, "AT", "T" * 50]),
    "dollar_dense": lambda: _whole(EDGE_SETS["dollar_dense"]()),
    "pathological": lambda: _whole(EDGE_SETS["pathological"]()),
    "split_calls": lambda: ([X, Y, X, revcomp(Y), Z], [[X, Y], [X, revcomp(Y), Z]]),
    "split_calls_second_alone": lambda: ([X, Y, X, revcomp(Y), Z], [[X, revcomp(Y), Z]]),
}
_DUP: dict = {}


def dup_case(name: str):
    """(index reads, calls, [codes of .bwt, codes of .rbwt], expected per call), computed once per set"""
    if name not in _DUP:
        reads, calls = DUP_SETS[name]()
        codes = [naive_sa(reads)[0], naive_sa([r[::-1] for r in reads])[0]]
        _DUP[name] = (reads, calls, codes, plain_dupcheck(reads, calls))
    return _DUP[name]


def test_the_duplicate_sets_hold_what_they_are_named_for():
    cls = lambda name, call=0: dup_case(name)[3][call]["cls"].tolist()
    assert cls("three_copies") == [UNIQUE, UNIQUE, FULL_LENGTH, UNIQUE, FULL_LENGTH]
    assert cls("rc_second") == cls("rc_first") == [UNIQUE, UNIQUE, FULL_LENGTH, UNIQUE] and revcomp(X) != X
    assert PAL == revcomp(PAL) and cls("palindrome_alone") == [UNIQUE, UNIQUE] and cls("palindrome_twice") == [UNIQUE, UNIQUE, FULL_LENGTH]
    assert cls("substrings") == [UNIQUE] + [SUBSTRING] * 6 + [UNIQUE]
    assert cls("substring_with_twin") == [UNIQUE, SUBSTRING, UNIQUE, SUBSTRING]
    assert cls("absent") == [UNIQUE, ABSENT, UNIQUE, ABSENT, ABSENT] and NOT_THERE[1:] == B[1:] and NOT_THERE not in B
    res = dup_case("absent")[3][0]
    assert (res["fwd_lower"][1], res["fwd_upper"][1], res["rvc_lower"][1], res["rvc_upper"][1]) == (0, -1, 0, -1)
    # "C" is no read of ["G"], its reverse complement is: it shares G's slot
    assert cls("one_base") == [UNIQUE, FULL_LENGTH, ABSENT, FULL_LENGTH]
    assert cls("one_base_reads") == [UNIQUE, UNIQUE, FULL_LENGTH, FULL_LENGTH, FULL_LENGTH]
    reads = dup_case("below_k")[0]
    assert max(len(r) for r in reads) < 13 and min(len(r) for r in reads) == 1 and len(set(cls("below_k"))) >= 3
    assert cls("all_A_all_T") == [UNIQUE, FULL_LENGTH, FULL_LENGTH, SUBSTRING, SUBSTRING, UNIQUE, FULL_LENGTH]
    reads = dup_case("dollar_dense")[0]
    assert len(reads) == 3000 and max(len(r) for r in reads) == 2 and {UNIQUE, SUBSTRING, FULL_LENGTH} == set(cls("dollar_dense"))
    assert {UNIQUE, SUBSTRING, FULL_LENGTH} == set(cls("pathological"))
    # across the calls of one session the first copy wins; a fresh session calls the second call's copies UNIQUE again
    assert cls("split_calls", 0) == [UNIQUE, UNIQUE] and cls("split_calls", 1) == [FULL_LENGTH, FULL_LENGTH, UNIQUE]
    assert cls("split_calls_second_alone") == [UNIQUE, UNIQUE, UNIQUE]
    # the '$' ranks: the k-th '$' row of .bwt is the k-th read by (sequence, id)
    reads, _, codes, want = dup_case("three_copies")
    sa = naive_sa(reads)[1]
    order = sa["read"][sa["pos"] == 0].tolist()
    assert order == [i for _, i in sorted((s, i) for i, s in enumerate(reads))]
    assert [order[k] for k in range(want[0]["fwd_lower"][0], want[0]["fwd_upper"][0] + 1)] == [0, 2, 4]


# ---- the duplicate check's driver --------------------------------------------------------------------------------------
def _build(exe: Path, source: str, *flags: str) -> str:
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools" / source),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def dup_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("dup_driver") / "dup_driver", "dup_driver.cpp")


@pytest.fixture(scope="module")
def remove_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("remove_driver") / "remove_driver", "remove_driver.cpp")


def _image_input(codes: np.ndarray) -> bytes:
    units = encode(codes)
    return np.array([codes.size, units.size], dtype=np.uint64).tobytes() + units.tobytes()


def _read_codes(reads: list[str]) -> bytes:
    return bytes(CODE[c] - 1 for r in reads for c in r)


def run_dup_driver(exe: str, name: str, wide: int):
    """-> [DUP_DTYPE array per call], Occ queries, block loads"""
    reads, calls, codes, _ = dup_case(name)
    parts = [_image_input(codes[0]), _image_input(codes[1]), np.array([len(calls)], dtype=np.uint64).tobytes()]
    for call in calls:
        off = np.concatenate([[0], np.cumsum([len(r) for r in call])]).astype(np.uint64)
        parts += [np.array([len(call)], dtype=np.uint64).tobytes(), off.tobytes(), _read_codes(call)]
    r = subprocess.run([exe, str(wide)], input=b"".join(parts), capture_output=True)
    assert r.returncode == 0, (name, wide, r.returncode, r.stderr[-2000:])
    out, p = [], 0
    for call in calls:
        out.append(np.frombuffer(r.stdout, dtype=DUP_DTYPE, count=len(call), offset=p))
        p += len(call) * DUP_DTYPE.itemsize
    ranks, loads = np.frombuffer(r.stdout, dtype=np.uint64, count=2, offset=p)
    assert p + 16 == len(r.stdout)
    return out, int(ranks), int(loads)


def assert_same_dup(got: np.ndarray, want: np.ndarray, what: str):
    for field in ("cls", "fwd_lower", "fwd_upper", "rvc_lower", "rvc_upper"):
        np.testing.assert_array_equal(got[field], want[field], err_msg=f"{what}: {field}")


def _run_all_dup_sets(exe: str, wide: int) -> int:
    for name in DUP_SETS:
        got, ranks, loads = run_dup_driver(exe, name, wide)
        want = dup_case(name)[3]
        for k, (g, w) in enumerate(zip(got, want)):
            assert_same_dup(g, w, f"{name} call {k}")
        assert ranks // 2 <= loads <= ranks
    return len(DUP_SETS)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_classes_and_dollar_intervals_equal_the_plain_definition(dup_driver, layout):
    assert _run_all_dup_sets(dup_driver, LAYOUTS[layout]) >= 16


def test_a_narrow_interval_costs_one_block_load_per_step(dup_driver):
    """once the interval of a chain lies in one rank block a step is one block load: on reads of a random 60-mer set nearly all"""
    _, ranks, loads = run_dup_driver(dup_driver, "substrings", 0)
    assert ranks > 0 and loads < 0.75 * ranks


# ---- the sets of the removal: (reads, drop[]) ---------------------------------------------------------------------------
def _kept_total(total: int, seed: int):
    """a set whose kept reads' symbols, sentinels included, add up to total, with dropped reads between them"""
    kept = _random_reads(seed, total, 3 + total // 150)
    dropped = _random_reads(seed + 1, 700, 4)
    reads, drop = [], []
    for i, r in enumerate(kept):
        if i % 3 == 0 and dropped:
            reads.append(dropped.pop())
            drop.append(1)
        reads.append(r)
        drop.append(0)
    return reads, drop


def _remove_sets() -> dict:
    path = EDGE_SETS["pathological"]
    n = len(path())
    s = {
        "drop_none": lambda: (path(), [0] * n),
        "drop_first": lambda: (path(), [1] + [0] * (n - 1)),
        "drop_last": lambda: (path(), [0] * (n - 1) + [1]),
        "all_but_one": lambda: (path(), [1] * 4 + [0] + [1] * (n - 5)),
        "every_second": lambda: (path(), [i & 1 for i in range(n)]),
        "copies_but_one": lambda: (path(), [int(i in (0, 9)) for i in range(n)]),      # reads 0, 1 and 9 are equal
        "every_all_A": lambda: (path(), [int(set(r) == {"A"}) for r in path()]),
        "dollar_dense_every_third": lambda: (EDGE_SETS["dollar_dense"](), [int(i % 3 == 0) for i in range(3000)]),
        # the rows of A^1 .. A^5000 follow one another from row 6 on: across tile and block edges of every shape
        "straddle": lambda: (["A" * 5000] + [_rand(200 + i, 300, "CGT") for i in range(5)], [1, 0, 0, 0, 0, 0]),
    }
    for t in (SMALL_TILE, kernel_tile()):
        for total in (t - 1, t, t + 1, 3 * t + 7):
            s[f"kept{total}"] = lambda total=total: _kept_total(total, total)
    return s


REMOVE_SETS = _remove_sets()
_REMOVE: dict = {}


def remove_case(name: str):
    """(reads, drop, per strand (codes of all reads, SA of all reads, codes of the kept reads)), computed once per set"""
    if name not in _REMOVE:
        reads, drop = REMOVE_SETS[name]()
        kept = [r for r, d in zip(reads, drop) if not d]
        strands = []
        for rev in (False, True):
            flip = (lambda x: [r[::-1] for r in x]) if rev else list
            strands.append(naive_sa(flip(reads)) + (naive_sa(flip(kept))[0],))
        _REMOVE[name] = (reads, np.array(drop, dtype=np.uint8), strands)
    return _REMOVE[name]


def test_the_removal_sets_hold_what_they_are_named_for():
    t = kernel_tile()
    assert t % 192 == 0 and t % 128 == 0 and t > SMALL_TILE
    for total in (SMALL_TILE - 1, SMALL_TILE, SMALL_TILE + 1, 3 * SMALL_TILE + 7, t - 1, t, t + 1, 3 * t + 7):
        reads, drop, strands = remove_case(f"kept{total}")
        assert strands[0][2].size == strands[1][2].size == total and 0 < drop.sum() < len(reads)
    reads, drop, _ = remove_case("copies_but_one")
    assert reads[0] == reads[1] == reads[9] and drop.tolist().count(1) == 2 and not drop[1]
    reads, drop, _ = remove_case("every_all_A")
    assert drop.sum() == 3 and all(set(r) == {"A"} for r, d in zip(reads, drop) if d)
    assert remove_case("all_but_one")[1].tolist().count(0) == 1 and remove_case("drop_none")[1].sum() == 0
    # deleting the rows of the dropped reads leaves the BWT of the kept reads: the claim the removal rests on
    for name in ("every_second", "straddle", f"kept{3 * SMALL_TILE + 7}"):
        _, drop, strands = remove_case(name)
        for codes, sa, kept_codes in strands:
            np.testing.assert_array_equal(codes[drop[sa["read"]] == 0], kept_codes)
    _, drop, strands = remove_case("straddle")
    rows = np.flatnonzero(drop[strands[0][1]["read"]] != 0)
    for edge in (t, SMALL_TILE, 192, 128):
        assert edge - 1 in rows and edge in rows, edge


def run_remove_driver(exe: str, name: str, strand: int, wide: int, small: int) -> np.ndarray:
    _, drop, strands = remove_case(name)
    codes, _, kept_codes = strands[strand]
    ids = np.flatnonzero(drop).astype(np.uint32)
    blob = _image_input(codes) + np.array([ids.size], dtype=np.uint64).tobytes() + ids.tobytes() + _image_input(kept_codes)
    r = subprocess.run([exe, str(wide), str(small), "0"], input=blob, capture_output=True)
    assert r.returncode == 0, (name, strand, wide, small, r.returncode, r.stderr[-2000:])
    n = int(np.frombuffer(r.stdout, dtype=np.uint64, count=1)[0])
    assert len(r.stdout) == 8 + n
    return np.frombuffer(r.stdout, dtype=np.uint8, offset=8)


def _run_all_remove_sets(exe: str, wide: int, small: int) -> int:
    n = 0
    for name in REMOVE_SETS:
        for strand in (0, 1):
            got = run_remove_driver(exe, name, strand, wide, small)          # the driver itself holds the packed image against build_strand_image
            np.testing.assert_array_equal(got, remove_case(name)[2][strand][2], err_msg=f"{name} strand {strand}: compacted codes")
            n += 1
    return n


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_compacted_codes_and_packed_image_equal_the_suffix_sort_of_the_kept_reads(remove_driver, shape, layout):
    assert _run_all_remove_sets(remove_driver, LAYOUTS[layout], SHAPES[shape]) == 2 * len(REMOVE_SETS) >= 34


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_walk_that_never_meets_its_dollar_row_ends_in_the_format_path(remove_driver, layout):
    """defect = 1: the image's '$' list is emptied; the walks end at their bound or at the strand's end, inside the bitmap"""
    _, drop, strands = remove_case("every_second")
    codes = strands[0][0]
    ids = np.flatnonzero(drop).astype(np.uint32)
    blob = _image_input(codes) + np.array([ids.size], dtype=np.uint64).tobytes() + ids.tobytes() + _image_input(strands[0][2])
    r = subprocess.run([remove_driver, str(LAYOUTS[layout]), "0", "1"], input=blob, capture_output=True)
    assert r.returncode == 3 and r.stdout == b"FORMAT", (r.returncode, r.stdout[:100], r.stderr[-2000:])


def test_drivers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """stand-alone programs, CPU only: every set, both layouts, both tile shapes, the defective input"""
    san = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    dup = _build(tmp_path / "dup_driver_san", "dup_driver.cpp", *san)
    rem = _build(tmp_path / "remove_driver_san", "remove_driver.cpp", *san)
    for wide in LAYOUTS.values():
        _run_all_dup_sets(dup, wide)
        for small in SHAPES.values():
            _run_all_remove_sets(rem, wide, small)
        test_a_walk_that_never_meets_its_dollar_row_ends_in_the_format_path(rem, "block64" if wide else "block32")


# ---- the ABI, the command line, the kernels ----------------------------------------------------------------------------
ENTRIES = ("lrsc_dupcheck_create", "lrsc_dupcheck_reads", "lrsc_dupcheck_destroy", "lrsc_index_remove")


def test_filter_entries_are_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    for name in ENTRIES:
        assert name in capi.declared_symbols()
        assert f" T {name}\n" in exported
    assert "enum lrsc_dup_class { LRSC_DUP_UNIQUE = 0, LRSC_DUP_SUBSTRING = 1, LRSC_DUP_FULL_LENGTH = 2, LRSC_DUP_ABSENT = 3 };" in header
    assert "typedef struct lrsc_dupcheck lrsc_dupcheck;" in header
    assert "int  lrsc_dupcheck_create(lrsc_ctx* ctx, lrsc_dupcheck** out);" in header
    assert "int  lrsc_dupcheck_reads(lrsc_dupcheck* dc, const char* reads, const uint64_t* read_off, uint32_t n_reads, lrsc_dup_result* out);" in header
    assert "void lrsc_dupcheck_destroy(lrsc_dupcheck* dc);" in header
    assert "int lrsc_index_remove(lrsc_index* idx, const uint8_t* drop, uint64_t n_reads, int device, lrsc_index** out);" in header
    assert "does not race" in header
    assert re.search(r"LRSC_K_LOCATE = 10, LRSC_K_COUNT = 11 \}", header) and "#define LRSC_ABI_VERSION 2\n" in header
    assert api.lib.lrsc_abi_version() == 2
    assert capi.DUP_DTYPE == DUP_DTYPE and capi.DUP_DTYPE.itemsize == 40
    assert (capi.DUP_UNIQUE, capi.DUP_SUBSTRING, capi.DUP_FULL_LENGTH, capi.DUP_ABSENT) == (UNIQUE, SUBSTRING, FULL_LENGTH, ABSENT)
    assert callable(capi.Ctx.dupcheck) and callable(capi.DupCheck.reads) and callable(capi.DupCheck.close) and callable(capi.Index.remove)


def test_stride_filter_usage(api, tmp_path):
    stride = str(STRIDE)
    run = lambda *args: subprocess.run([stride, *args], cwd=tmp_path, capture_output=True, text=True, input="")
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n")
    for args, message in ((["filter"], "filter: missing arguments"),
                          (["filter", "reads.fa", "more.fa"], "filter: too many arguments"),
                          (["filter", "-t", "0", "reads.fa"], "filter: invalid number of threads: 0"),
                          (["filter", "-k", "0", "reads.fa"], "filter: invalid kmer length: 0, must be greater than zero"),
                          (["filter", "-x", "-2", "reads.fa"], "filter: invalid kmer threshold: -2, must be greater than zero"),
                          (["filter", "--frobnicate", "reads.fa"], "")):
        r = run(*args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert message in r.stderr and "Usage: StriDe filter [OPTION] ... READSFILE" in r.stdout + r.stderr, (args, r.stdout, r.stderr)
        assert "--substring-only" in r.stdout + r.stderr and "--device=N" in r.stdout + r.stderr
    r = run("filter", "--help")
    assert r.returncode == 0 and "Usage: StriDe filter" in r.stdout + r.stderr
    for args in (["help"], []):                                  # the two `Commands:` lines
        r = run(*args)
        lines = [l for l in (r.stdout + r.stderr).split("\n") if l.startswith("Commands:")]
        assert len(lines) == 1 and " filter" in lines[0] and all(f" {c}," in lines[0] for c in ("merge", "sai", "grep")), (args, r.stdout, r.stderr)


def _kernel_notes(tmp_path, unit: str) -> str:
    import __graft_entry__ as g

    g.build()
    obj = REPO / "longreadselfcorrect_amd" / "_build" / "obj" / f"{unit}.hip.o"
    assert obj.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp_path / f"{unit}.fatbin", tmp_path / f"{unit}.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    return subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout


def _kernels(notes: str, pattern: str):
    """{kernel: [(mangled name, metadata)]} of the unit's own kernels, each held to no scratch, no spills, no AGPRs"""
    seen = {}
    for b in re.split(r"\n\s+- \.", notes):
        m = re.search(rf"\.name:\s+(_ZN4lrsc\d+({pattern})\S*)\s", b + "\n")
        if not m or m.group(1).endswith(".kd"):
            continue
        md = {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, (m.group(1), md)
        assert md.get("agpr_count", 0) == 0
        seen.setdefault(m.group(2), []).append((m.group(1), md))
    return seen


def _assert_sized_as_a_walk(instances, waves: int, threads: int):
    """the launch is sized for `waves` wavefronts per SIMD: 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of LDS per
    CU for the workgroups of its four SIMDs; both <WIDE> instances"""
    assert waves == 8 and threads == 128
    for name, md in instances:
        lds = md["group_segment_fixed_size"]
        assert md["max_flat_workgroup_size"] == threads
        assert md["vgpr_count"] <= 512 // waves // 8 * 8 == 64, (name, md)
        assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (name, md)
    assert {re.search(r"ILb([01])E", n).group(1) for n, _ in instances} == {"0", "1"}


def test_dup_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_dup"), r"dup_[a-z]+_kernel")
    assert {k: len(v) for k, v in seen.items()} == {"dup_chain_kernel": 2, "dup_combine_kernel": 1, "dup_classify_kernel": 1, "dup_commit_kernel": 1}, seen
    _assert_sized_as_a_walk(seen["dup_chain_kernel"], _const("fm_dup.h", "kDupWavesPerSimd"), _const("fm_dup.h", "kDupThreads"))


def test_remove_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_remove"), r"remove_[a-z]+_kernel")
    assert {k: len(v) for k, v in seen.items()} == {"remove_mark_kernel": 2, "remove_count_kernel": 1, "remove_compact_kernel": 2}, seen
    _assert_sized_as_a_walk(seen["remove_mark_kernel"], _const("fm_remove.h", "kRemoveWalkWavesPerSimd"), _const("fm_remove.h", "kRemoveWalkThreads"))
    for name, md in seen["remove_compact_kernel"]:
        assert md["max_flat_workgroup_size"] == _const("fm_remove.h", "kRemoveLanes")
        assert 0 < md["group_segment_fixed_size"] <= 160 * 1024 // 8, "eight workgroups of three wavefronts per CU"
    assert {re.search(r"ILb([01])E", n).group(1) for n, _ in seen["remove_compact_kernel"]} == {"0", "1"}
