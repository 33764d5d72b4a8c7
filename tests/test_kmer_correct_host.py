"""The device k-mer corrector (csrc/fm_kcorrect.h, fm_kcorrect.hip, capi_kcorrect.cpp) checked without a GPU.

1. The yardstick, plain_kmer_correct: ErrorCorrectProcess::kmerCorrection restated in plain Python, the count of a k-mer taken
   from a dictionary of all k-mers of the index's reads.  The named sets, each with an assertion that it holds what it is named
   for.
2. The per-lane and per-read code that the kernel calls, compiled for the CPU (tests/host_tools/kcorrect_driver.cpp) and run in the
   kernel's order on an image made by build_strand_image: corrected reads, kmer_qc, n_changed and passes equal the yardstick's on
   every set, for both layouts.  The driver again under AddressSanitizer and UBSan, as a stand-alone program.
3. The entry and its structs are declared, exported and bound, the ABI version is still 2.
4. The kernels compile for gfx950 without scratch, spills or AGPRs, within the registers and the LDS their launch is sized for.

One set of the issue cannot exist: "the original base is the last qualifier".  A base qualifies with count >= 2 * max(count of the
k-mer as it stands, t), and the k-mer with the original base is the k-mer as it stands, so the original base never qualifies while
t > 0.  `left_fails_right_succeeds` keeps what that set was for, a left attempt that fails and a right one that is tried and
succeeds, and the named-sets test asserts the impossibility on every attempt the yardstick makes.
"""
from __future__ import annotations

import re
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_index_filter_host import LAYOUTS, _image_input, _kernel_notes, _kernels, _rand, revcomp
from .test_index_locate_host import naive_sa
from .test_index_merge_host import CODE

KC_DTYPE = np.dtype([("kmer_qc", "<u4"), ("n_changed", "<u4"), ("passes", "<u4"), ("pad", "<u4")])
CUTOFF = 20


def _const(name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", (REPO / "longreadselfcorrect_amd/csrc/fm_kcorrect.h").read_text())
    assert m, name
    return int(m.group(1))


LDS_BASES = _const("kKcLdsBases")


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def kmer_counter(index_reads: list[str], k: int):
    """count(w): the occurrences of w among the index's reads plus those of its reverse complement"""
    table = Counter(r[i: i + k] for r in index_reads for i in range(len(r) - k + 1))
    return lambda w: table[w] + table[revcomp(w)]


def plain_kmer_correct(count, seq: str, qual: str | None, k: int, x: int, rounds_max: int, attempts: list | None = None):
    """-> (corrected, kmer_qc, n_changed, passes).  attempts, when given, collects (original base, qualifying bases) of every attempt."""
    n = len(seq)
    if n < k:
        return seq, False, 0, 0
    phred = [ord(c) - 33 for c in qual] if qual is not None else [15] * n
    support = lambda p: x if p >= CUTOFF else x + 1
    nk = n - k + 1
    min_phred = [min(phred[i: i + k]) for i in range(nk)]
    s = list(seq)

    def attempt(i, k_idx, min_count):
        original, best, qualifying = s[i], None, []
        for b in "ACGT":
            w = s[k_idx: k_idx + k]
            w[i - k_idx] = b
            if count("".join(w)) >= 2 * min_count:
                best = b
                qualifying.append(b)
        if attempts is not None:
            attempts.append((original, qualifying))
        if best is not None and best != original:
            s[i] = best
            return True
        return False

    rounds = passes = 0
    all_solid = False
    while True:
        cnt = [count("".join(s[i: i + k])) for i in range(nk)]
        passes += 1
        solid = [False] * n
        for i in range(nk):
            if cnt[i] >= support(min_phred[i]):
                solid[i: i + k] = [True] * k
        all_solid = all(solid)
        if all_solid:
            break
        rounds += 1
        if rounds - 1 > rounds_max:                              # if(rounds++ > maxAttempts) break;
            break
        corrected = False
        for i in range(n):
            if solid[i]:
                continue
            t = support(phred[i])
            left = i + 1 - k if i + 1 >= k else 0
            corrected = attempt(i, left, max(cnt[left], t))
            if not corrected:
                right = min(i, n - k)
                corrected = attempt(i, right, max(cnt[right], t))
            if corrected:
                break
        if not corrected:
            break
    if not all_solid:
        return seq, False, 0, passes
    out = "".join(s)
    return out, True, sum(a != b for a, b in zip(out, seq)), passes


# ---- the indexes of the sets -----------------------------------------------------------------------------------------------
GENOME = _rand(0xC0DE, 3000)


def _tiling():
    """100-base reads every 4 bases of a random 3 kb genome, alternate reads reverse-complemented: k-mer counts of 17 to 20"""
    reads = [GENOME[s: s + 100] for s in range(0, len(GENOME) - 99, 4)]
    return [revcomp(r) if i & 1 else r for i, r in enumerate(reads)]


Z60 = _rand(0x2A, 60)
LEFT40, RIGHT40 = _rand(0x2B, 40), _rand(0x2C, 40)
HALF10 = _rand(0x2D, 10)
PAL20 = HALF10 + revcomp(HALF10)
PLAIN20 = _rand(0x2E, 20)
INDEXES = {
    "tiling": _tiling,
    "exact_x": lambda: [Z60] * 3 + [_rand(0x30, 50)],
    # more copies with C than with G: the later base wins all the same
    "two_qualify": lambda: [LEFT40 + "C" + RIGHT40] * 12 + [LEFT40 + "G" + RIGHT40] * 9,
    # the whole segment four times, its right part from the base on ten times more
    "right_only": lambda: [LEFT40 + "T" + RIGHT40] * 4 + ["T" + RIGHT40] * 10,
    "palindrome": lambda: [PAL20] * 2 + [PLAIN20] * 2,
}
_INDEX: dict = {}


def index_case(key: str):
    """(reads of the index, BWT codes of .bwt), computed once per index"""
    if key not in _INDEX:
        reads = INDEXES[key]()
        _INDEX[key] = (reads, naive_sa(reads)[0])
    return _INDEX[key]


# ---- the sets: index, reads, qualities (None: FASTA), k, x, rounds ----------------------------------------------------------
def _sub(s: str, *positions: int) -> str:
    """s with another base at every position"""
    s = list(s)
    for p in positions:
        s[p % len(s)] = "ACGT"[("ACGT".index(s[p % len(s)]) + 1 + p % 3) % 4]
    return "".join(s)


def _g(start: int, n: int) -> str:
    return GENOME[start: start + n]


def _set(index, reads, k, quals=None, x=3, rounds=10):
    return dict(index=index, reads=list(reads), quals=quals, k=k, x=x, rounds=rounds)


def _tiling_sets(k: int) -> dict:
    nks = (63, 64, 65, 127, 128, 129)
    return {
        f"untouched_k{k}": lambda: _set("tiling", [_g(600, 100), revcomp(_g(901, 100))], k),
        f"one_error_k{k}": lambda: _set("tiling", [_sub(_g(700, 100), p) for p in (50, 0, 5, -1, -10)], k),
        f"two_errors_k{k}": lambda: _set("tiling", [_sub(_g(800, 100), 45, 50), _sub(_g(1000, 100), 35, 75)], k),
        f"length_k_k{k}": lambda: _set("tiling", [_sub(_g(1100, k), k // 2), _g(1200, k)], k),
        f"length_k_minus_1_k{k}": lambda: _set("tiling", [_g(1300, k - 1), _sub(_g(1300, k - 1), 3)], k),
        f"eleven_errors_i10_k{k}": lambda: _set("tiling", [_sub(_g(1400, 200), *range(40, 40 + 11 * 12, 12))], k),
        f"twelve_errors_i10_k{k}": lambda: _set("tiling", [_sub(_g(1400, 200), *range(40, 40 + 12 * 12, 12))], k),
        f"two_errors_i1_k{k}": lambda: _set("tiling", [_sub(_g(1600, 120), 40, 80)], k, rounds=1),
        f"three_errors_i1_k{k}": lambda: _set("tiling", [_sub(_g(1600, 120), 40, 60, 80)], k, rounds=1),
        f"nk_edges_k{k}": lambda: _set("tiling", [_sub(_g(500 + 7 * nk, nk + k - 1), (nk + k - 1) // 2) for nk in nks], k),
        f"beyond_lds_k{k}": lambda: _set("tiling", [_sub(_g(900, LDS_BASES + 44), 100, LDS_BASES + 24), _g(2000, LDS_BASES + 1), _sub(_g(1700, LDS_BASES), 70)], k),
        f"not_of_the_genome_k{k}": lambda: _set("tiling", [_rand(0x99, 100), _g(1500, 60) + _rand(0x9A, 40)], k),
    }


KC_SETS = {**_tiling_sets(21), **_tiling_sets(31)}
KC_SETS.update({
    "k_1": lambda: _set("tiling", [_g(600, 30), "A", _rand(0x9B, 7)], 1),
    "k_41": lambda: _set("tiling", [_sub(_g(2000, 100), 60), _g(2100, 100), _g(2200, 40)], 41),
    "fastq_low_and_high_k21": lambda: _set("tiling", [_sub(_g(700, 100), 50), _g(600, 100)], 21, quals=["I" * 100, "#" * 50 + "I" * 50]),
    # every 21-mer of Z60 occurs exactly x = 3 times
    "exact_x_fastq": lambda: _set("exact_x", [Z60, Z60], 21, quals=["I" * 60, "I" * 30 + "4" + "I" * 29]),
    "exact_x_fasta": lambda: _set("exact_x", [Z60], 21),
    "two_qualify": lambda: _set("two_qualify", [LEFT40 + "A" + RIGHT40, LEFT40 + "T" + RIGHT40], 21),
    "left_fails_right_succeeds": lambda: _set("right_only", [LEFT40 + "A" + RIGHT40, LEFT40 + "G" + RIGHT40], 21),
    "palindrome_counted_twice": lambda: _set("palindrome", [PAL20, PLAIN20], 20),
})
_KC: dict = {}


def kc_case(name: str):
    """(the set, [(corrected, kmer_qc, n_changed, passes) per read] by the yardstick), computed once per set"""
    if name not in _KC:
        s = KC_SETS[name]()
        count = kmer_counter(index_case(s["index"])[0], s["k"])
        quals = s["quals"] or [None] * len(s["reads"])
        _KC[name] = (s, [plain_kmer_correct(count, r, q, s["k"], s["x"], s["rounds"]) for r, q in zip(s["reads"], quals)])
    return _KC[name]


def phred_of(quals: list[str] | None):
    """the scores of a set's reads back to back, or None"""
    return None if quals is None else np.frombuffer("".join(quals).encode(), dtype=np.uint8) - 33


def test_the_sets_hold_what_they_are_named_for():
    qc_passes = lambda name: [(w[1], w[3]) for w in kc_case(name)[1]]
    fixed = lambda name: [w[0] for w in kc_case(name)[1]]
    counts = kmer_counter(index_case("tiling")[0], 31)
    inner = [counts(GENOME[p: p + 31]) for p in range(500, 2400)]
    assert 700 <= len(index_case("tiling")[0]) <= 760 and 17 <= min(inner) and max(inner) <= 20
    for k in (21, 31):
        assert qc_passes(f"untouched_k{k}") == [(True, 1)] * 2
        assert qc_passes(f"one_error_k{k}") == [(True, 2)] * 5 and fixed(f"one_error_k{k}") == [_g(700, 100)] * 5
        assert [w[2] for w in kc_case(f"one_error_k{k}")[1]] == [1] * 5
        assert qc_passes(f"two_errors_k{k}") == [(True, 3)] * 2 and fixed(f"two_errors_k{k}") == [_g(800, 100), _g(1000, 100)]
        assert qc_passes(f"length_k_k{k}") == [(True, 2), (True, 1)] and fixed(f"length_k_k{k}") == [_g(1100, k), _g(1200, k)]
        assert all(len(r) == k for r in kc_case(f"length_k_k{k}")[0]["reads"])
        assert qc_passes(f"length_k_minus_1_k{k}") == [(False, 0)] * 2 and fixed(f"length_k_minus_1_k{k}") == kc_case(f"length_k_minus_1_k{k}")[0]["reads"]
        assert qc_passes(f"eleven_errors_i10_k{k}") == [(True, 12)] and fixed(f"eleven_errors_i10_k{k}") == [_g(1400, 200)]
        assert kc_case(f"eleven_errors_i10_k{k}")[1][0][2] == 11
        twelve = kc_case(f"twelve_errors_i10_k{k}")
        assert qc_passes(f"twelve_errors_i10_k{k}") == [(False, 12)] and twelve[1][0][0] == twelve[0]["reads"][0] and twelve[1][0][2] == 0
        assert sum(a != b for a, b in zip(twelve[0]["reads"][0], _g(1400, 200))) == 12
        assert qc_passes(f"two_errors_i1_k{k}") == [(True, 3)] and qc_passes(f"three_errors_i1_k{k}") == [(False, 3)]
        assert [len(r) - k + 1 for r in kc_case(f"nk_edges_k{k}")[0]["reads"]] == [63, 64, 65, 127, 128, 129]
        assert qc_passes(f"nk_edges_k{k}") == [(True, 2)] * 6
        long_reads = kc_case(f"beyond_lds_k{k}")[0]["reads"]
        assert [len(r) for r in long_reads] == [LDS_BASES + 44, LDS_BASES + 1, LDS_BASES]
        assert qc_passes(f"beyond_lds_k{k}") == [(True, 3), (True, 1), (True, 2)] and fixed(f"beyond_lds_k{k}")[0] == _g(900, LDS_BASES + 44)
        assert long_reads[0][100] != GENOME[1000] and long_reads[0][LDS_BASES + 24] != GENOME[900 + LDS_BASES + 24]
        # no substitute of a random read is a k-mer of the genome; a random tail is walked back onto the genome a base a pass
        assert qc_passes(f"not_of_the_genome_k{k}") == [(False, 1), (False, 12)]
    assert qc_passes("k_1") == [(True, 1)] * 3 and qc_passes("k_41") == [(True, 2), (True, 1), (False, 0)]
    # phred 40 everywhere: support 3; the second read's first half has phred 2, support 4: the counts of 17 to 20 reach both
    assert qc_passes("fastq_low_and_high_k21") == [(True, 2), (True, 1)]
    exact = kmer_counter(index_case("exact_x")[0], 21)
    assert {exact(Z60[i: i + 21]) for i in range(40)} == {3} == {kc_case("exact_x_fastq")[0]["x"]}
    assert ord("4") - 33 == 19 and ord("I") - 33 >= CUTOFF
    assert qc_passes("exact_x_fastq") == [(True, 1), (False, 1)] and qc_passes("exact_x_fasta") == [(False, 1)]
    two = kmer_counter(index_case("two_qualify")[0], 21)
    at = lambda b: two((LEFT40 + b + RIGHT40)[20:41])
    assert (at("A"), at("C"), at("G"), at("T")) == (0, 12, 9, 0) and min(at("C"), at("G")) >= 2 * 4
    assert fixed("two_qualify") == [LEFT40 + "G" + RIGHT40] * 2 and qc_passes("two_qualify") == [(True, 2)] * 2
    right = kmer_counter(index_case("right_only")[0], 21)
    truth = LEFT40 + "T" + RIGHT40
    assert right(truth[20:41]) == 4 < 2 * 4 <= right(truth[40:61]) == 14 and min(right(truth[i: i + 21]) for i in range(60)) >= 4
    assert fixed("left_fails_right_succeeds") == [truth] * 2 and qc_passes("left_fails_right_succeeds") == [(True, 2)] * 2
    pal = kmer_counter(index_case("palindrome")[0], 20)
    assert PAL20 == revcomp(PAL20) and PLAIN20 != revcomp(PLAIN20) and (pal(PAL20), pal(PLAIN20)) == (4, 2)
    assert qc_passes("palindrome_counted_twice") == [(True, 1), (False, 1)]
    # the base that stands in the read never qualifies in an attempt
    seen = 0
    for name in KC_SETS:
        s = kc_case(name)[0]
        count = kmer_counter(index_case(s["index"])[0], s["k"])
        attempts: list = []
        for r, q in zip(s["reads"], s["quals"] or [None] * len(s["reads"])):
            plain_kmer_correct(count, r, q, s["k"], s["x"], s["rounds"], attempts)
        assert all(original not in qualifying for original, qualifying in attempts), name
        seen += len(attempts)
    assert seen > 500


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _build(exe: Path, *flags: str) -> str:
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/kcorrect_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def kcorrect_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("kcorrect_driver") / "kcorrect_driver")


def run_kcorrect_driver(exe: str, name: str, wide: int):
    """-> [(corrected, kmer_qc, n_changed, passes) per read], Occ queries, block loads"""
    s = kc_case(name)[0]
    reads = s["reads"]
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    phred = phred_of(s["quals"])
    blob = b"".join([_image_input(index_case(s["index"])[1]), np.array([s["k"], s["x"], s["rounds"], CUTOFF], dtype=np.int32).tobytes(),
                     np.array([len(reads)], dtype=np.uint64).tobytes(), off.tobytes(), bytes(CODE[c] - 1 for r in reads for c in r),
                     np.array([phred is not None], dtype=np.uint64).tobytes(), b"" if phred is None else phred.tobytes()])
    r = subprocess.run([exe, str(wide)], input=blob, capture_output=True)
    assert r.returncode == 0, (name, wide, r.returncode, r.stderr[-2000:])
    res = np.frombuffer(r.stdout, dtype=KC_DTYPE, count=len(reads))
    p = len(reads) * KC_DTYPE.itemsize
    total = int(off[-1])
    text = "".join("ACGT"[c] for c in r.stdout[p: p + total])
    ranks, loads = np.frombuffer(r.stdout, dtype=np.uint64, count=2, offset=p + total)
    assert p + total + 16 == len(r.stdout)
    got = [(text[int(a): int(b)], bool(q["kmer_qc"]), int(q["n_changed"]), int(q["passes"])) for a, b, q in zip(off[:-1], off[1:], res)]
    return got, int(ranks), int(loads)


def _run_all_sets(exe: str, wide: int) -> int:
    for name in KC_SETS:
        got, ranks, loads = run_kcorrect_driver(exe, name, wide)
        assert got == kc_case(name)[1], (name, wide)
        assert ranks // 2 <= loads <= ranks
    return len(KC_SETS)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_corrected_reads_qc_changes_and_passes_equal_the_yardstick(kcorrect_driver, layout):
    assert _run_all_sets(kcorrect_driver, LAYOUTS[layout]) >= 30


def test_a_later_pass_recounts_only_the_k_mers_that_cover_the_changed_base(kcorrect_driver):
    """a read of n bases with one error mid-read: nk k-mers, then 16 chains for the base, then at most k k-mers again; a chain is at
    most k - 1 steps of two Occ queries"""
    k, n = 21, 100
    got, ranks, _ = run_kcorrect_driver(kcorrect_driver, "one_error_k21", 0)
    assert len(got) == 5
    chains = 5 * (2 * (n - k + 1) + 2 * k) + (1 + 2 + 1 + 1 + 1) * 64      # the error at base 5 is found in the second group of four
    assert 0 < ranks <= chains * 2 * (k - 1)
    assert ranks < 5 * 2 * (2 * (n - k + 1)) * 2 * (k - 1), "two whole passes would cost this much"


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: every set, both layouts; the state of every read is an allocation of its own"""
    exe = _build(tmp_path / "kcorrect_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        _run_all_sets(exe, wide)


# ---- the ABI, the kernels ---------------------------------------------------------------------------------------------------
def test_kmer_correct_entry_is_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    assert "lrsc_kmer_correct" in capi.declared_symbols() and " T lrsc_kmer_correct\n" in exported
    assert "typedef struct lrsc_kcorrect_params { int32_t kmer_length, kmer_threshold, kmer_rounds, quality_cutoff; } lrsc_kcorrect_params;" in header
    assert "typedef struct lrsc_kcorrect_result { uint32_t kmer_qc, n_changed, passes, pad; } lrsc_kcorrect_result;" in header
    assert re.search(r"int lrsc_kmer_correct\(lrsc_ctx\* ctx, const char\* reads, const uint64_t\* read_off, uint32_t n_reads,\s+const uint8_t\* phred", header)
    assert "ErrorCorrectProcess.cpp:287-438" in header
    assert re.search(r"LRSC_K_LOCATE = 10, LRSC_K_COUNT = 11 \}", header) and "#define LRSC_ABI_VERSION 2\n" in header
    assert api.lib.lrsc_abi_version() == 2
    assert capi.KCORRECT_DTYPE == KC_DTYPE and capi.KCORRECT_DTYPE.itemsize == 16
    assert callable(capi.Ctx.kmer_correct)


def test_kmer_correct_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_kcorrect"), r"kmer_[a-z]+_kernel")
    assert {k: len(v) for k, v in seen.items()} == {"kmer_correct_kernel": 2}, seen
    waves, threads = _const("kKcWavesPerSimd"), _const("kKcThreads")
    assert waves >= 4 and threads % 64 == 0
    for name, md in seen["kmer_correct_kernel"]:
        lds = md["group_segment_fixed_size"]
        assert md["max_flat_workgroup_size"] == threads
        # 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of LDS per CU for the workgroups of its four SIMDs
        assert md["vgpr_count"] <= 512 // waves // 8 * 8, (name, md)
        assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (name, md)
        assert lds >= (threads // 64) * (10 * LDS_BASES + 256)
    assert {re.search(r"ILb([01])E", n).group(1) for n, _ in seen["kmer_correct_kernel"]} == {"0", "1"}


# ---- `stride correct`: the command line and the post-processing ---------------------------------------------------------------
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
CORRECT_USAGE = "Usage: StriDe correct [OPTION] ... READSFILE"


def test_stride_correct_usage(api, tmp_path):
    run = lambda *args: subprocess.run([str(STRIDE), "correct", *args], cwd=tmp_path, capture_output=True, text=True, input="")
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n")
    kmer = ["-a", "kmer"]
    for args, message in ((kmer, "correct: missing arguments"),
                          (kmer + ["reads.fa", "more.fa"], "correct: too many arguments"),
                          (kmer + ["-t", "0", "reads.fa"], "correct: invalid number of threads: 0"),
                          (kmer + ["-r", "0", "reads.fa"], "correct: invalid number of overlap rounds: 0, must be at least 1"),
                          (kmer + ["-i", "0", "reads.fa"], "correct: invalid number of kmer rounds: 0, must be at least 1"),
                          (kmer + ["-k", "0", "reads.fa"], "correct: invalid kmer length: 0, must be greater than zero"),
                          (kmer + ["-x", "-2", "reads.fa"], "correct: invalid kmer threshold: -2, must be greater than zero"),
                          (["-a", "best", "reads.fa"], "correct: unrecognized -a,--algorithm parameter: best"),
                          (["-a", "overlap", "reads.fa"], "correct: -a overlap is not built here"),
                          (["--algorithm=hybrid", "reads.fa"], "correct: -a hybrid is not built here"),
                          (["reads.fa"], "correct: without -a the reference runs its overlap algorithm, which is not built here"),
                          (kmer + ["--learn", "reads.fa"], "correct: --learn is not built here"),
                          (kmer + ["--frobnicate", "reads.fa"], "correct: unrecognized option '--frobnicate'")):       # getopt's own line
        r = run(*args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert message in r.stderr and len([l for l in r.stderr.split("\n") if l.startswith("correct: ")]) == 1, (args, r.stderr)
        assert CORRECT_USAGE in r.stdout, (args, r.stdout, r.stderr)
        for option in ("--discard", "--metrics=FILE", "--kmer-rounds=N", "--learn", "--device=N", "--build-index", "--branch-cutoff=N", "(default: READSFILE.ec.fa)"):
            assert option in r.stdout, (args, option)
    r = run(*kmer, "-e", "2", "reads.fa")
    assert r.returncode == 1 and "Invalid error-rate parameter: 2" in r.stderr and CORRECT_USAGE not in r.stdout
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith(CORRECT_USAGE) and r.stderr == ""
    for args in (["help"], []):                                  # the two `Commands:` lines
        r = subprocess.run([str(STRIDE), *args], cwd=tmp_path, capture_output=True, text=True, input="")
        lines = [l for l in (r.stdout + r.stderr).split("\n") if l.startswith("Commands:")]
        assert lines == ["Commands: index, merge, sai, grep, filter, correct, pbcorrect, kmerfreq, kmercheck"], (args, r.stdout, r.stderr)


def metrics_reads():
    """20 reads with qualities over the tiling index: untouched, with one to three errors, and two that fail QC; what the yardstick
    makes of them with k = 21"""
    rng = np.random.default_rng(0x3E7)
    count = kmer_counter(index_case("tiling")[0], 21)
    records = []
    for i in range(20):
        truth = _g(520 + 90 * i, 100)
        seq = _rand(0x500 + i, 100) if i in (6, 13) else _sub(truth, *rng.choice(np.arange(3, 97, 7), size=i % 4, replace=False).tolist())
        qual = "".join(rng.choice(list("I5#4"), size=100, p=[0.7, 0.1, 0.1, 0.1]))
        corrected, qc, changed, _ = plain_kmer_correct(count, seq, qual, 21, 3, 10)
        assert qc == (i not in (6, 13)) and changed == (i % 4 if qc else 0) and (not qc or corrected == truth)
        records.append((f"read{i}/1", seq, qual, corrected, qc))
    return records


def _g6(x: float) -> str:
    """a double as an ostream prints it"""
    return "%g" % x


def plain_metrics(records) -> tuple[str, list[str]]:
    """the metrics file and the two summary lines: collectMetrics and writeMetrics over the reads that passed QC"""
    tables = {name: {} for name in ("pos", "base", "kmer", "quality")}
    total = errors = 0

    def bump(name, key, error):
        s = tables[name].setdefault(key, [0, 0])
        s[0] += 1
        s[1] += int(error)

    for _, seq, qual, corrected, qc in records:
        if not qc:
            continue
        for i, (a, b) in enumerate(zip(seq, corrected)):
            total += 1
            errors += a != b
            bump("pos", i, a != b)
            bump("base", a, a != b)
            if qual:
                bump("quality", qual[i], a != b)
            if i > 2:                                              # not i >= 2: the reference's test
                bump("kmer", seq[i - 2: i], a != b)
    leaders = {"pos": "Bases corrected by position\n", "base": "\nOriginal base that was corrected\n", "kmer": "\nkmer preceding the corrected base\n",
               "quality": "\nBases corrected by quality value\n\n"}
    text = ""
    for name in ("pos", "base", "kmer", "quality"):
        text += leaders[name] + f"{name}\tsamples\terrors\tfraction\n"
        text += "".join(f"{key}\t{s}\t{e}\t{_g6(e / s)}\n" for key, (s, e) in sorted(tables[name].items()))
    kept = len(records)
    return text, [f"ErrorCorrect -- Corrected {errors} out of {total} bases ({_g6(errors / total)})", f"Kept {kept} reads. Discarded 0 reads (0)"]


def fastx(records, keep=lambda qc: True, corrected=True) -> str:
    """the records as SeqRecord::write writes them: FASTQ with qualities, else FASTA"""
    out = ""
    for rid, seq, qual, fixed, qc in records:
        if keep(qc) and (fixed if corrected else seq):
            s = fixed if corrected else seq
            out += f"@{rid}\n{s}\n+\n{qual}\n" if qual else f">{rid}\n{s}\n"
    return out


def count_lines(records) -> list[str]:
    passed = sum(1 for r in records if r[4])
    return [f"Reads passed kmer QC check: {passed}", "Reads passed overlap QC check: 0", f"Reads failed QC: {len(records) - passed}"]


@pytest.fixture(scope="module")
def ecpost_driver(api, tmp_path_factory):
    exe = tmp_path_factory.mktemp("ecpost_driver") / "ecpost_driver"
    subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(REPO / "tests/host_tools/ecpost_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/host/ErrorCorrectProcess.cpp"), f"-L{api.path.parent}", "-llrsc_hip", f"-Wl,-rpath,{api.path.parent}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return str(exe)


def _run_post(exe, tmp_path, records, discard: bool, metrics: bool):
    lines = "".join("\t".join([rid, seq, qual or "-", fixed or "-", str(int(qc))]) + "\n" for rid, seq, qual, fixed, qc in records)
    r = subprocess.run([exe, "out.fx", "discard.fx" if discard else "-", "metrics.txt" if metrics else "-"], cwd=tmp_path, input=lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip().split("\n")


def test_metrics_equal_a_plain_computation_of_the_four_tables(ecpost_driver, tmp_path):
    records = metrics_reads()
    want, summary = plain_metrics(records)
    assert want.count("\n") > 100 + 4 + 16 + 4 and "\nread" not in want
    stdout = _run_post(ecpost_driver, tmp_path, records, False, True)
    assert (tmp_path / "metrics.txt").read_text() == want
    assert stdout == summary + count_lines(records)
    assert (tmp_path / "out.fx").read_text() == fastx(records)      # without --discard a read that failed QC is written too, as it came
    # the 2-mer before base 2 is never taken: every read gives 97 samples, not 98
    kmer_samples = sum(int(l.split("\t")[1]) for l in want.split("kmer preceding the corrected base\n")[1].split("\n\n")[0].split("\n")[1:])
    assert kmer_samples == 97 * sum(1 for r in records if r[4])


def test_discard_splits_the_records_and_an_empty_read_is_not_written(ecpost_driver, tmp_path):
    records = metrics_reads()[:8]
    records.insert(3, ("empty", "", "", "", False))
    records += [(rid + "_fa", seq, "", fixed, qc) for rid, seq, _, fixed, qc in metrics_reads()[5:8]]      # FASTA records between FASTQ ones
    stdout = _run_post(ecpost_driver, tmp_path, records, True, False)
    assert (tmp_path / "out.fx").read_text() == fastx(records, lambda qc: qc)
    assert (tmp_path / "discard.fx").read_text() == fastx(records, lambda qc: not qc)
    assert stdout == count_lines(records) and stdout[2] == "Reads failed QC: 3"
    assert "@empty" not in (tmp_path / "discard.fx").read_text() and ">read6/1_fa\n" in (tmp_path / "discard.fx").read_text()
