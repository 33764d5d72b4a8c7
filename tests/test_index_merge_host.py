"""The device index merge (csrc/fm_merge.h, fm_merge.hip) checked without a GPU.

1. The per-lane functions that the kernels call, compiled for the CPU (tests/host_tools/merge_driver.cpp) and run in the
   kernels' order on images made by build_strand_image, against a naive suffix sort of A's reads followed by B's: the merged
   codes and rank[] exactly, both strands, all four layout combinations, the kernels' tile and one of two rank blocks.
2. dollar_origin against the same sort.
3. lrsc_index_merge is declared, exported and bound, the ABI version is still 2; `stride merge` and `--merge-index` refuse
   what they must and are listed.
4. The merge kernels compile for gfx950 without scratch or spills, the walk within the registers its launch is sized for.
5. The driver again under AddressSanitizer and UBSan, as a stand-alone program.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_gpu_index_build import EDGE_SETS, _pathological
from .test_index_unrle_host import encode

LLVM = Path("/opt/rocm/lib/llvm/bin")
HDR = (REPO / "longreadselfcorrect_amd/csrc/fm_merge.h").read_text()
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
COMBOS = {"a32_b32": (0, 0), "a32_b64": (0, 1), "a64_b32": (1, 0), "a64_b64": (1, 1)}     # the driver's <wide_a> <wide_b>
SHAPES = {"kernel_tile": 0, "small_tile": 1}                                              # the driver's <small>
SMALL_TILE = 384
CODE = {c: i for i, c in enumerate("$ACGT")}


def _const(name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", HDR)
    assert m, name
    return int(m.group(1))


def kernel_tile() -> int:
    assert re.search(r"kMergeTile = kMergeLanes \* 16;", HDR)
    return _const("kMergeLanes") * 16


# ---- the yardstick: a suffix sort --------------------------------------------------------------------------------------
def naive_bwt(reads: list[str], n_a: int | None = None):
    """BWT codes ($ACGT = 0..4) of the string set, sentinels in input order and below every base.  With n_a also: for every
    row of reads[n_a:]'s own BWT the number of suffixes of reads[:n_a] below it (rank[]), and for every '$' row of the
    BWT whether it belongs to reads[n_a:]."""
    suf = sorted((r[k:], i, k) for i, r in enumerate(reads) for k in range(len(r) + 1))
    codes = np.array([CODE[reads[i][k - 1]] if k else 0 for _, i, k in suf], dtype=np.uint8)
    if n_a is None:
        return codes
    from_b = np.array([i >= n_a for _, i, _ in suf])
    rank = np.cumsum(~from_b)[from_b].astype(np.uint64)
    return codes, rank, from_b[codes == 0].astype(np.uint8)


_SORTS: dict = {}


def sorted_case(name: str):
    """(codes A, codes B, codes of the union, rank[], origin) per strand, computed once per case"""
    if name not in _SORTS:
        a, b = CASES[name]()
        out = []
        for rev in (False, True):
            ra, rb = ([r[::-1] for r in x] if rev else list(x) for x in (a, b))
            out.append((naive_bwt(ra), naive_bwt(rb)) + naive_bwt(ra + rb, len(ra)))
        _SORTS[name] = out
    return _SORTS[name]


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _random_reads(seed: int, total: int, n_reads: int) -> list[str]:
    """n_reads reads whose symbols, sentinels included, add up to total"""
    rng = np.random.default_rng(seed)
    bases = total - n_reads
    assert bases >= n_reads
    cuts = np.sort(rng.choice(np.arange(1, bases), size=n_reads - 1, replace=False)) if n_reads > 1 else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([[0], cuts, [bases]]))
    genome = "".join(rng.choice(list("ACGT"), size=400))          # reads of one short genome share long suffixes
    reads = []
    for n in lens:
        s = int(rng.integers(0, 400))
        reads.append((genome[s:] + genome * (int(n) // 400 + 1))[: int(n)])
    assert sum(len(r) + 1 for r in reads) == total
    return reads


def _cases() -> dict:
    c = {}
    for name, make in EDGE_SETS.items():
        n = len(make())
        for at in sorted({1, n // 2, n - 1} - {0, n}):
            c[f"{name}-split{at}"] = (lambda make=make, at=at: (make()[:at], make()[at:]))
    c["one_base-twice"] = lambda: (["G"], ["G"])
    c["a_equals_b"] = lambda: (_pathological(), _pathological())
    c["a_equals_b-dollar_dense"] = lambda: (EDGE_SETS["dollar_dense"]()[:700], EDGE_SETS["dollar_dense"]()[:700])
    c["b_all_A"] = lambda: (_pathological(), ["A" * 50, "A", "A" * 230, "AA"])
    c["b_all_T"] = lambda: (_pathological(), ["T" * 50, "T", "T" * 230, "TT"])
    c["a_all_A"] = lambda: (["A" * 7, "A" * 300], _pathological())
    c["duplicates_across"] = lambda: (_pathological()[:6] + ["ACGT" * 40], ["ACGT" * 40] + _pathological()[:6][::-1])
    for t in (SMALL_TILE, kernel_tile()):
        for total in (t - 1, t, t + 1, 3 * t + 7):
            n_reads = 3 + total // 150
            c[f"total{total}"] = (lambda total=total, n_reads=n_reads: (lambda r: (r[: 2 * n_reads // 3], r[2 * n_reads // 3:]))(_random_reads(total, total, n_reads)))
    c["multiple_of_384_minus_1"] = lambda: (lambda r: (r[:5], r[5:]))(_random_reads(8, 384 * 5 - 1, 12))
    c["b_in_one_tile_of_a"] = lambda: (_random_reads(9, 3 * SMALL_TILE + 7, 9), ["ACGTTGCAAC"])
    return c


CASES = _cases()


def test_the_cases_hold_what_they_are_named_for():
    t = kernel_tile()
    assert t % 384 == 0 or t % 128 == 0
    for total in (SMALL_TILE - 1, SMALL_TILE, SMALL_TILE + 1, 3 * SMALL_TILE + 7, t - 1, t, t + 1, 3 * t + 7):
        a, b = CASES[f"total{total}"]()
        assert a and b and sum(len(r) + 1 for r in a + b) == total
    for name, mod in (("multiple_of_384-split1", 0), ("multiple_of_384_plus_1-split1", 1), ("multiple_of_384_minus_1", 383)):
        a, b = CASES[name]()
        assert sum(len(r) + 1 for r in a + b) % 384 == mod
    a, b = CASES["dollar_dense-split1500"]()
    assert len(a) == len(b) == 1500 and max(len(r) for r in a + b) == 2
    assert len(CASES["pathological-split11"]()[1]) == 1 and len(CASES["pathological-split1"]()[0]) == 1
    # all of B below A's first base row, and above its last
    _, _, _, rank, _ = sorted_case("b_all_A")[0]
    n_a = len(_pathological())
    assert (rank[:4] == n_a).all() and rank.max() <= n_a + sum(r.count("A") for r in _pathological())
    codes_a, _, _, rank, _ = sorted_case("b_all_T")[0]
    assert (rank[:4] == n_a).all() and rank[4:].min() >= codes_a.size - sum(r.count("T") for r in _pathological())
    # every suffix tied: a row of B stands behind as many rows of A as its own number says
    _, codes_b, _, rank, origin = sorted_case("a_equals_b")[0]
    assert (np.diff(rank.astype(np.int64)) >= 0).all() and rank[-1] == codes_b.size
    assert origin.size == 2 * n_a and origin.sum() == n_a and origin[0] == 0 and origin[-1] == 1


def test_the_suffix_sort_is_the_oracle_builder_s(oracle, tmp_path):
    """once, on a set with duplicates, prefixes and runs: the naive sort is the BWT that the pinned builder writes"""
    from oracle.oracle_py import pack_reads

    a, b = CASES["pathological-split6"]()
    bases, off = pack_reads(a + b)
    oracle.build_index(bases, off, str(tmp_path / "u"))
    for rev, ext in ((False, "bwt"), (True, "rbwt")):
        units = np.fromfile(tmp_path / f"u.{ext}", dtype=np.uint8)[30:]
        np.testing.assert_array_equal(units, encode(sorted_case("pathological-split6")[int(rev)][2]))


# ---- the driver --------------------------------------------------------------------------------------------------------
def _build_driver(exe: Path, *flags: str):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/merge_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build_driver(tmp_path_factory.mktemp("merge_driver") / "merge_driver")


def _driver_input(codes_a: np.ndarray, codes_b: np.ndarray) -> bytes:
    parts = []
    for codes in (codes_a, codes_b):
        units = encode(codes)
        parts += [np.array([codes.size, units.size], dtype=np.uint64).tobytes(), units.tobytes()]
    return b"".join(parts)


def _driver_output(blob: bytes):
    out, p = [], 0
    for dtype in (np.uint8, np.uint64, np.uint8):
        n = int(np.frombuffer(blob, dtype=np.uint64, count=1, offset=p)[0])
        out.append(np.frombuffer(blob, dtype=dtype, count=n, offset=p + 8))
        p += 8 + n * np.dtype(dtype).itemsize
    assert p == len(blob)
    return out


def _run_all_cases(exe: str, wide_a: int, wide_b: int, small: int) -> int:
    n = 0
    for name in CASES:
        for strand, (codes_a, codes_b, want, want_rank, want_origin) in enumerate(sorted_case(name)):
            r = subprocess.run([exe, str(wide_a), str(wide_b), str(small)], input=_driver_input(codes_a, codes_b), capture_output=True)
            assert r.returncode == 0, (name, strand, r.returncode, r.stderr[-2000:])
            merged, rank, origin = _driver_output(r.stdout)
            assert (np.diff(rank.astype(np.int64)) >= 0).all(), (name, strand)
            np.testing.assert_array_equal(rank, want_rank, err_msg=f"{name} strand {strand}: rank[]")
            np.testing.assert_array_equal(merged, want, err_msg=f"{name} strand {strand}: merged codes")
            np.testing.assert_array_equal(origin, want_origin, err_msg=f"{name} strand {strand}: dollar_origin")
            n += 1
    return n


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_merged_codes_ranks_and_origin_equal_the_suffix_sort_of_the_union(driver, shape, combo):
    assert _run_all_cases(driver, *COMBOS[combo], SHAPES[shape]) == 2 * len(CASES) >= 50


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: the same cases, every layout combination, the tile shapes alternating"""
    exe = _build_driver(tmp_path / "merge_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for small in SHAPES.values():
        for k, (wide_a, wide_b) in enumerate(COMBOS.values()):
            if (k ^ small) & 1:                                   # each shape with two combinations that cover both layouts of A and of B
                _run_all_cases(exe, wide_a, wide_b, small)


# ---- the ABI, the command line, the kernels ----------------------------------------------------------------------------
def test_index_merge_is_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    assert "lrsc_index_merge" in capi.declared_symbols()
    assert " T lrsc_index_merge\n" in exported
    assert re.search(r"int lrsc_index_merge\(lrsc_index\* a, lrsc_index\* b, int device, lrsc_index\*\* out, uint8_t\* dollar_origin\);",
                     (REPO / "include/lrsc.h").read_text())
    assert api.lib.lrsc_abi_version() == 2
    assert callable(capi.Lrsc.index_merge)


def test_stride_merge_and_merge_index_usage(api, tmp_path):
    stride = str(STRIDE)
    run = lambda *args: subprocess.run([stride, *args], cwd=tmp_path, capture_output=True, text=True)
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n")
    for args in (["merge", "-p", "M", "A"], ["merge", "-p", "M"], ["merge", "A", "B"]):
        r = run(*args)
        assert r.returncode != 0, args
        assert "Usage: StriDe merge" in r.stderr and "PREFIX_A PREFIX_B" in r.stderr, (args, r.stderr)
    r = run("merge", "--help")
    assert r.returncode == 0 and "Usage: StriDe merge" in r.stderr + r.stdout
    r = run("pbcorrect", "--merge-index=A", "-p", "A", "-o", "o", "reads.fa")
    assert r.returncode != 0
    assert "--merge-index" in r.stderr and "--build-index" in r.stderr and "Usage: StriDe PacBioSelfCorrection" in r.stderr
    assert "--merge-index" in run("pbcorrect", "--help").stderr
    for args in (["help"], []):                                  # the two `Commands:` lines
        r = run(*args)
        lines = [l for l in (r.stdout + r.stderr).split("\n") if l.startswith("Commands:")]
        assert len(lines) == 1 and " merge," in lines[0], (args, r.stdout, r.stderr)


def test_merge_kernels_build_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as g

    g.build()
    obj = REPO / "longreadselfcorrect_amd" / "_build" / "obj" / "fm_merge.hip.o"
    assert obj.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp_path / "fm_merge.fatbin", tmp_path / "fm_merge.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    waves, threads = _const("kMergeWalkWavesPerSimd"), _const("kMergeWalkThreads")
    assert 1 <= waves <= 8 and threads % 64 == 0
    seen = {}
    for b in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(_ZN4lrsc\d+(merge_\w+_kernel)\S*)\s", b + "\n")
        if not m or m.group(1).endswith(".kd"):
            continue
        md = {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
        kernel = m.group(2)
        seen.setdefault(kernel, []).append(m.group(1))
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, (m.group(1), md)
        assert md.get("agpr_count", 0) == 0
        lds = md["group_segment_fixed_size"]
        if kernel == "merge_rank_kernel":
            # the launch is sized for `waves` wavefronts per SIMD: 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of
            # LDS per CU for the workgroups of its four SIMDs
            assert md["max_flat_workgroup_size"] == threads
            assert md["vgpr_count"] <= 512 // waves // 8 * 8, (m.group(1), md)
            assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (m.group(1), md)
        if kernel == "merge_interleave_kernel":
            assert md["max_flat_workgroup_size"] == _const("kMergeLanes")
            assert 0 < lds <= 64 * 1024 and lds <= 160 * 1024 // 8, "eight workgroups of four wavefronts fill a CU"
    assert {k: len(v) for k, v in seen.items()} == {"merge_rank_kernel": 4, "merge_interleave_kernel": 4, "merge_tile_kernel": 1,
                                                     "merge_origin_kernel": 1}, seen
    # all four <WIDE_A, WIDE_B> instances of the walk
    assert {re.search(r"ILb([01])ELb([01])E", n).groups() for n in seen["merge_rank_kernel"]} == {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}
