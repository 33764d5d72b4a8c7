"""The device locate (csrc/fm_locate.h, fm_locate.hip) checked without a GPU.

1. The per-lane functions that the kernels call, compiled for the CPU (tests/host_tools/locate_driver.cpp) and run in the
   kernels' order on images made by build_strand_image, against a naive suffix sort with the sentinels in input order: order[],
   the read lengths, every sample and the located (read, pos) of every row exactly; both strands, both layouts, rates 0, 1, 7, 16
   and 192.
2. Sampling pays: on 2 kb reads the LF steps of locating every row at rate 16 are at most a quarter of those at rate 0.
3. The driver again under AddressSanitizer and UBSan, as a stand-alone program.
4. The three entries are declared, exported and bound, the ABI version is still 2; `stride sai` and `stride grep` refuse what they
   must and are listed.
5. The locate kernels compile for gfx950 without scratch or spills, within the registers their launch is sized for.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_gpu_index_build import EDGE_SETS
from .test_index_merge_host import CASES, CODE, _random_reads
from .test_index_unrle_host import encode

LLVM = Path("/opt/rocm/lib/llvm/bin")
HDR = (REPO / "longreadselfcorrect_amd/csrc/fm_locate.h").read_text()
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
LAYOUTS = {"block32": 0, "block64": 1}                           # the driver's <wide>
RATES = (0, 1, 7, 16, 192)
SA_DTYPE = np.dtype([("read", "<u4"), ("pos", "<u4")])
LCM = 7 * 192                                                     # a multiple of every rate above


def _const(name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", HDR)
    assert m, name
    return int(m.group(1))


# ---- the yardstick: a suffix sort --------------------------------------------------------------------------------------
def naive_sa(reads: list[str]):
    """(BWT codes $ACGT = 0..4, SA as SA_DTYPE) of the string set, sentinels in input order and below every base: row r is the
    suffix of read SA[r].read that starts at SA[r].pos (pos == the read's length: its sentinel alone).  test_index_merge_host's
    naive_bwt, which is held once against the pinned builder, with the (read, k) of every row kept."""
    suf = sorted((r[k:], i, k) for i, r in enumerate(reads) for k in range(len(r) + 1))
    codes = np.array([CODE[reads[i][k - 1]] if k else 0 for _, i, k in suf], dtype=np.uint8)
    sa = np.array([(i, k) for _, i, k in suf], dtype=SA_DTYPE)
    return codes, sa


def expected(sa: np.ndarray, n_reads: int, rate: int):
    """order[], read_len[], the samples of a rate: num_symbols // rate + 1 slots as SampledSuffixArray::build sizes them, the last
    one left empty (all bits set) when it stands for the row behind the last"""
    order = sa["read"][sa["pos"] == 0]
    read_len = np.zeros(n_reads, dtype=np.uint32)
    np.maximum.at(read_len, sa["read"], sa["pos"])
    samples = np.full(sa.size // rate + 1 if rate else 0, 2 ** 64 - 1, dtype=np.uint64).view(SA_DTYPE)
    if rate:
        samples[: -(-sa.size // rate)] = sa[::rate]
    return order, read_len, samples


LOCATE_SETS = dict(EDGE_SETS)
LOCATE_SETS["b_all_T"] = lambda: CASES["b_all_T"]()[1]
LOCATE_SETS["rate_times_m"] = lambda: _random_reads(31, 2 * LCM, 9)
LOCATE_SETS["rate_times_m_plus_1"] = lambda: _random_reads(32, 2 * LCM + 1, 9)
_SORTS: dict = {}


def sorted_set(name: str):
    """[(codes, SA) of the reads, (codes, SA) of the reversed reads], computed once per set"""
    if name not in _SORTS:
        reads = LOCATE_SETS[name]()
        _SORTS[name] = (len(reads), [naive_sa(reads), naive_sa([r[::-1] for r in reads])])
    return _SORTS[name]


def test_the_sets_hold_what_they_are_named_for():
    for name, extra in (("rate_times_m", 0), ("rate_times_m_plus_1", 1)):
        n = sorted_set(name)[1][0][0].size
        assert all(n % r == extra for r in RATES if r > 1), name
    assert all(set(r) == {"T"} for r in LOCATE_SETS["b_all_T"]())
    n_reads, strands = sorted_set("dollar_dense")
    assert n_reads == 3000 and strands[0][0].size // 192 > 3 * 8
    codes, sa = sorted_set("pathological")[1][0]
    # row i < n is read i's sentinel alone; equal reads keep their input order among the '$' rows
    n = sorted_set("pathological")[0]
    assert (sa["read"][:n] == np.arange(n)).all()
    order, read_len, _ = expected(sa, n, 0)
    reads = LOCATE_SETS["pathological"]()
    assert sorted(order.tolist()) == list(range(n)) and read_len.tolist() == [len(r) for r in reads]
    assert reads[0] == reads[1] == reads[9] and [int(x) for x in order if x in (0, 1, 9)] == [0, 1, 9]
    assert (codes[sa["pos"] == 0] == 0).all() and (codes == 0).sum() == n


# ---- the driver --------------------------------------------------------------------------------------------------------
def _build_driver(exe: Path, *flags: str):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/locate_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build_driver(tmp_path_factory.mktemp("locate_driver") / "locate_driver")


def run_driver(exe: str, codes: np.ndarray, wide: int, rate: int):
    """-> order, read_len, samples, located, LF steps"""
    units = encode(codes)
    blob = np.array([codes.size, units.size], dtype=np.uint64).tobytes() + units.tobytes()
    r = subprocess.run([exe, str(wide), str(rate)], input=blob, capture_output=True)
    assert r.returncode == 0, (wide, rate, r.returncode, r.stderr[-2000:])
    out, p = [], 0
    for dtype in (np.uint32, np.uint32, SA_DTYPE, SA_DTYPE, np.uint64):
        n = int(np.frombuffer(r.stdout, dtype=np.uint64, count=1, offset=p)[0])
        out.append(np.frombuffer(r.stdout, dtype=dtype, count=n, offset=p + 8))
        p += 8 + n * np.dtype(dtype).itemsize
    assert p == len(r.stdout)
    return out[0], out[1], out[2], out[3], int(out[4][0])


def _run_all_sets(exe: str, wide: int, rate: int) -> int:
    n = 0
    for name in LOCATE_SETS:
        n_reads, strands = sorted_set(name)
        for strand, (codes, sa) in enumerate(strands):
            order, read_len, samples, located, steps = run_driver(exe, codes, wide, rate)
            want_order, want_len, want_samples = expected(sa, n_reads, rate)
            what = f"{name} strand {strand}"
            np.testing.assert_array_equal(order, want_order, err_msg=f"{what}: order[]")
            np.testing.assert_array_equal(read_len, want_len, err_msg=f"{what}: read_len[]")
            assert samples.size == (codes.size // rate + 1 if rate else 0), what
            np.testing.assert_array_equal(samples, want_samples, err_msg=f"{what}: samples")
            np.testing.assert_array_equal(located, sa, err_msg=f"{what}: located (read, pos)")
            if rate == 1:
                assert steps == 0
            if rate == 0:                                       # every row walks to its read's '$' row
                assert steps == int(sa["pos"].astype(np.int64).sum())
            n += 1
    return n


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_order_lengths_samples_and_located_pairs_equal_the_suffix_sort(driver, layout, rate):
    assert _run_all_sets(driver, LAYOUTS[layout], rate) == 2 * len(LOCATE_SETS) >= 16


def test_sampling_at_16_takes_at_most_a_quarter_of_the_lf_steps_on_2kb_reads(driver):
    rng = np.random.default_rng(5)
    reads = ["".join(rng.choice(list("ACGT"), size=2000)) for _ in range(6)]
    codes, sa = naive_sa(reads)
    _, _, _, located0, steps0 = run_driver(driver, codes, 0, 0)
    _, _, _, located16, steps16 = run_driver(driver, codes, 0, 16)
    np.testing.assert_array_equal(located0, sa)
    np.testing.assert_array_equal(located16, sa)
    print(f"LF steps per row: {steps0 / codes.size:.1f} at rate 0, {steps16 / codes.size:.1f} at rate 16")
    assert steps0 == int(sa["pos"].astype(np.int64).sum()) and 0 < 4 * steps16 <= steps0


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: the same sets, both strands, both layouts, every rate"""
    exe = _build_driver(tmp_path / "locate_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        for rate in RATES:
            _run_all_sets(exe, wide, rate)


# ---- the ABI, the command line, the kernels ----------------------------------------------------------------------------
def test_locate_entries_are_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    for name in ("lrsc_index_locate_prepare", "lrsc_index_lexico_order", "lrsc_locate"):
        assert name in capi.declared_symbols()
        assert f" T {name}\n" in exported
    assert "int lrsc_index_locate_prepare(lrsc_index* idx, int device, uint32_t sample_rate);" in header
    assert "int lrsc_index_lexico_order(lrsc_index* idx, int strand, int device, uint32_t* order, uint32_t* read_len);" in header
    assert "int lrsc_locate(lrsc_ctx* ctx, int strand, const uint64_t* rows, uint64_t n, lrsc_sa_elem* out);" in header
    assert "typedef struct lrsc_sa_elem { uint32_t read, pos; } lrsc_sa_elem;" in header
    assert re.search(r"LRSC_K_LOCATE = 10, LRSC_K_COUNT = 11 \}", header) and "#define LRSC_ABI_VERSION 2\n" in header
    assert api.lib.lrsc_abi_version() == 2
    assert capi.K_LOCATE == 10 and capi.SA_DTYPE.itemsize == 8
    assert callable(capi.Index.locate_prepare) and callable(capi.Index.lexico_order) and callable(capi.Ctx.locate)


def test_stride_sai_and_grep_usage(api, tmp_path):
    stride = str(STRIDE)
    run = lambda *args: subprocess.run([stride, *args], cwd=tmp_path, capture_output=True, text=True, input="")
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n")
    for args in (["sai"], ["sai", "--frobnicate", "-p", "P"], ["sai", "-p"], ["sai", "-p", "P", "extra"]):
        r = run(*args)
        assert r.returncode != 0, args
        assert "Usage: StriDe sai" in r.stderr and "-p PREFIX" in r.stderr, (args, r.stderr)
    for args in (["grep"], ["grep", "--frobnicate", "reads.fa"], ["grep", "-p"], ["grep", "reads.fa", "more.fa"], ["grep", "--sample-rate=x", "reads.fa"]):
        r = run(*args)
        assert r.returncode != 0, args
        assert "Usage: StriDe grep" in r.stderr and "READSFILE" in r.stderr and "--sample-rate" in r.stderr, (args, r.stderr)
    for cmd in ("sai", "grep"):
        r = run(cmd, "--help")
        assert r.returncode == 0 and f"Usage: StriDe {cmd}" in r.stderr + r.stdout
    for args in (["help"], []):                                  # the two `Commands:` lines
        r = run(*args)
        lines = [l for l in (r.stdout + r.stderr).split("\n") if l.startswith("Commands:")]
        assert len(lines) == 1 and all(f" {c}," in lines[0] for c in ("merge", "sai", "grep")), (args, r.stdout, r.stderr)


def test_locate_kernels_build_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as g

    g.build()
    obj = REPO / "longreadselfcorrect_amd" / "_build" / "obj" / "fm_locate.hip.o"
    assert obj.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp_path / "fm_locate.fatbin", tmp_path / "fm_locate.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    waves, threads = _const("kLocateWavesPerSimd"), _const("kLocateThreads")
    assert waves == 8 and threads == 128
    seen = {}
    for b in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(_ZN4lrsc\d+(locate_(?:[a-z]+_)?kernel)\S*)\s", b + "\n")
        if not m or m.group(1).endswith(".kd"):
            continue
        md = {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
        kernel = m.group(2)
        seen.setdefault(kernel, []).append(m.group(1))
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, (m.group(1), md)
        assert md.get("agpr_count", 0) == 0
        if kernel in ("locate_prepare_kernel", "locate_kernel"):
            # the launch is sized for `waves` wavefronts per SIMD: 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of
            # LDS per CU for the workgroups of its four SIMDs
            lds = md["group_segment_fixed_size"]
            assert md["max_flat_workgroup_size"] == threads
            assert md["vgpr_count"] <= 512 // waves // 8 * 8 == 64, (m.group(1), md)
            assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (m.group(1), md)
    assert {k: len(v) for k, v in seen.items()} == {"locate_prepare_kernel": 2, "locate_kernel": 2, "locate_fixup_kernel": 1}, seen
    for kernel in ("locate_prepare_kernel", "locate_kernel"):     # both <WIDE> instances
        assert {re.search(r"ILb([01])E", n).group(1) for n in seen[kernel]} == {"0", "1"}
