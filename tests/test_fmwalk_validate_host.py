"""fmwalk's validate algorithm (csrc/fm_validate.h, fm_validate.hip, capi_fmwalk.cpp) checked without a GPU.

1. The yardstick: SAIntervalTree::validate with the single-read constructor, FMIndexWalkProcess::ValidateReads and
   splitRead(std::string&) restated statement by statement in plain Python over strings, the growing interval of the split with
   its restarts included.  The count of a string comes from test_fmwalk_host's Counts, isSimple and isLowComplexity from
   test_fmwalk_hybrid_host.  An interval is known by its string and by whether it is valid, as in test_fmwalk_host; where
   mergeTwoReads' shortcut does not apply, validate()'s walk is held against that module's plain_walk.  The serial countQualified
   is held against independent per-position counts on every set.  The named sets, each with an assertion that it holds what it
   is named for.
2. The per-lane and per-read code that the kernels call, compiled for the CPU (tests/host_tools/fmwalk_validate_driver.cpp) and
   run in the kernels' order: every field equals the yardstick's on every set, for both layouts.  The driver again under
   AddressSanitizer and UBSan, as a stand-alone program.
3. The entry and its struct are declared, exported and bound, the ABI version is still 2, the limits are as they were.
4. `stride fmwalk --validate`: usage, errors, and that `-a validate` is still refused; the three files and the summary lines of the
   command's post-processor on a tiny input (tests/host_tools/fmwalk_post_driver.cpp: the command itself needs a device).
5. The kernels compile for gfx950 without scratch, spills or AGPRs, within the registers and the LDS their launch is sized for.

The threshold.  ValidateReads takes `threshold = getRequiredSupport(0) - 1`, the line MergePairedReads and KmerizeReads have too, and
setBaseMinSupport(x) makes getRequiredSupport(0) x + 1: the walks' threshold is -x itself, the value lrsc_fmwalk_merge is given,
and the split's is (size_t)x - 1.  So every k-mer qualifies at -x 1 (x_is_1_all_qualify), and the unsigned wrap that leaves none
qualified needs a threshold of 0, which the command line and the entry refuse as they do for merge: threshold_0_none_qualifies
shows it on the yardstick and the CPU driver alone.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_fmwalk_host import GENOME, HAP2, K, M_MIN, SNP2, X, Counts, _alt, index_case, plain_walk
from .test_fmwalk_hybrid_host import (PIECE_DTYPE, READ_DTYPE, _codes, check_unwritten, is_simple, literal_low_complexity, piece_slots, read_record,
                                      reads_input)
from .test_index_filter_host import LAYOUTS, _image_input, _kernel_notes, _kernels, revcomp

VALIDATE_DTYPE = np.dtype([("merged", "<u4"), ("length", "<u4"), ("status", "<i4", (2,)), ("max_used_leaves", "<u4", (2,)), ("coverage", "<u8", (2,)),
                           ("walk_length", "<u4", (2,)), ("chosen", "<i4"), ("read", READ_DTYPE)], align=True)
SIZE_MAX = 2 ** 64 - 1


def _const(name: str, unit: str = "fm_validate.h") -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", (REPO / "longreadselfcorrect_amd/csrc" / unit).read_text())
    assert m, name
    return int(m.group(1))


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def plain_validate_walk(c: Counts, s: str, m: int, max_overlap: int, depth: int, leaves_max: int, x: int, trace: list | None = None):
    """SAIntervalTree(&s, m, max_overlap, depth, leaves_max, indices, x).validate (SAIntervalTree.cpp:59-94, 173-237) -> (code,
    mergedseq, maxUsedLeaves, maxKmerCoverage).  A leaf is (its string, is fwd valid, is rvc valid), the intervals those of its last
    `kmer` bases; m_secondread is empty, so a result's string is the thread."""
    root, e = s[:m], s[len(s) - m:]
    leaves = [(root, c.single(root) > 0, c.single(revcomp(root)) > 0)]
    cur_len, kmer, max_used, results = len(root), m, 0, []

    def extend(kmer):                                             # attempToExtend with getFMIndexExtensions
        new = []
        for t, f, r in leaves:
            u = t[len(t) - kmer:]
            for b in "ACGT":
                fs = c.single(u + b) if f else 0
                rs = c.single(revcomp(u + b)) if r else 0
                if fs + rs >= x:
                    new.append((t + b, fs > 0, rs > 0))
        return new

    def refine(ls):                                               # refineSAInterval(m_minOverlap)
        return [(t, c.single(t[-m:]) > 0, c.single(revcomp(t[-m:])) > 0) for t, _, _ in ls]

    while leaves and len(leaves) <= leaves_max and cur_len <= depth:
        new = extend(kmer)                                        # extendLeaves
        if not new:
            leaves, kmer = refine(leaves), m
            new = extend(kmer)
            if trace is not None:
                trace.append(("retry", cur_len, len(new)))
        if new:
            kmer += 1
            cur_len += 1
        leaves = new
        if leaves and kmer >= max_overlap:
            leaves, kmer = refine(leaves), m
        max_used = max(max_used, len(leaves))
        results = [t for t, f, r in leaves if t[len(t) - kmer:].endswith(e) and (f or r)]         # isTerminated
        if results:
            break
    if results:
        if trace is not None:
            trace.append(("results", len(results), len(leaves)))
        best, best_cov = "", 0
        for t in results:
            cov = sum(c.both(t[i: i + m]) for i in range(0, len(t) - m + 1, m // 2))             # calculateKmerCoverage
            if trace is not None:
                trace.append(("cov", t, cov))
            if cov > best_cov:
                best, best_cov = t, cov
        return 1, best, max_used, best_cov
    return (-1 if not leaves else -2 if cur_len > depth else -3 if len(leaves) > leaves_max else -4), "", max_used, 0


def serial_count_qualified(c: Counts, seq: str, k: int, threshold: int):
    """the first loop of splitRead(std::string&) (617-684), statement by statement: fwdInterval and rvcInterval are those of
    `grown`, a stretch of the read that ends with k-mer i -> (countQualified, the recomputations at a k-mer that had grown)"""
    cq = [0] * (len(seq) - k + 1)
    grown = seq[:k]                                               # startingKmer
    size = k                                                      # currKmerSize
    freq = c.single(grown) + c.single(revcomp(grown))             # an invalid interval adds nothing, and stays invalid
    restarts = 0
    i = 0
    while i <= len(seq) - k:
        if freq >= threshold:
            cq[i] += 1
            if i < len(seq) - k:
                grown += seq[i + k]
                size += 1
                freq = c.single(grown) + c.single(revcomp(grown))
            i += 1
            continue
        elif size > k and freq < threshold:                       # unsatisfied due to too large kmer
            grown = seq[i: i + k]
            size = k
            freq = c.single(grown) + c.single(revcomp(grown))
            restarts += 1
            continue                                              # i--; continue: this iteration again
        elif size == k and freq < threshold:                      # bad kmer at i
            if i < len(seq) - k:
                grown = seq[i + 1: i + 1 + k]
                size = k
                freq = c.single(grown) + c.single(revcomp(grown))
        else:
            assert False
        i += 1
    assert all(q in (0, 1) for q in cq)
    return cq, restarts


def plain_split_string(c: Counts, seq: str, k: int, threshold: int):
    """splitRead(std::string&) (613-722), len(seq) >= k -> ([(first k-mer, the piece's string)], mainSeedIdx)"""
    nk = len(seq) - k + 1
    cq, _ = serial_count_qualified(c, seq, k, threshold)
    intervals, start = [], 0
    for p in range(1, nk):
        if cq[p - 1] == 1 and cq[p] == 1:
            continue
        if not is_simple(c, seq[p - 1: p - 1 + k], seq[p: p + k]):
            intervals.append((start, p - 1))
            start = p
    intervals.append((start, nk - 1))
    max_size, main, pieces = 0, -1, []
    for i, (a, b) in enumerate(intervals):
        if max_size < b - a:
            max_size, main = b - a, i
        pieces.append((a, seq[a: b + k]))
    return pieces, main


def plain_validate(c: Counts, read: str, k: int = K, x: int = X, m: int = M_MIN, max_overlap: int = -1, leaves_max: int = 32, trace: list | None = None) -> dict:
    """ValidateReads (269-391), x being its `threshold` -> the fields of lrsc_fmwalk_validate_result, the sequence of a merged read,
    and the read's record as test_fmwalk_hybrid_host's read_record gives it"""
    n = len(read)
    rd = dict(kmerize=0, head=0, length=n, main=-1, whole=0, pieces=[], correct="", kmerized=[])
    out = dict(merged=0, length=0, seq="", status=[0, 0], max_used_leaves=[0, 0], coverage=[0, 0], walk_length=[0, 0], chosen=-1, read=rd)
    if n <= m:
        rd.update(whole=1, correct=read, kmerize=0 if literal_low_complexity(read) else 1)
        return out
    mo = max_overlap if max_overlap != -1 else int(n * 0.9)
    depth = int(n * 1.1)
    w1 = plain_validate_walk(c, read, m, mo, depth, leaves_max, x, trace)
    w2 = plain_validate_walk(c, revcomp(read), m, mo, depth, leaves_max, x, trace)
    out.update(status=[w1[0], w2[0]], max_used_leaves=[w1[2], w2[2]], coverage=[w1[3], w2[3]], walk_length=[len(w1[1]), len(w2[1])])
    s1, s2 = w1[1], w2[1]
    diff1, diff2 = len(s1) / n, len(s2) / n
    seq = None
    if s1 and not s2 and w2[0] != -2:
        seq, out["chosen"] = (s1, 0) if diff1 >= 1 else (read, -1)
    elif s2 and not s1 and w1[0] != -2:
        seq, out["chosen"] = (s2, 1) if diff2 >= 1 else (read, -1)
    elif s1 and s2:
        seq, out["chosen"] = (s1, 0) if diff1 >= 1 else (s2, 1) if diff2 >= 1 else (read, -1)
    if seq is not None:
        out.update(merged=1, length=len(seq), seq=seq)
        return out
    if n < k:                                                     # the reference asserts; here: nothing
        return out
    pieces, main = plain_split_string(c, read, k, (x - 1) % 2 ** 64)
    rd["kmerize"], rd["main"] = 1, main                           # firstKR is never empty
    for i, (a, s) in enumerate(pieces):
        kept = not literal_low_complexity(s)
        rd["pieces"].append((a, len(s), int(kept)))
        if not kept:
            continue
        if i == main:
            rd["correct"] = s
        else:
            rd["kmerized"].append(s)
    return out


def written_files(records, quals: bool = False) -> tuple[str, str, str]:
    """FMIndexWalkPostProcess::process(SequenceWorkItem) (922-969) with the validate algorithm's three writers: [(id, the read,
    plain_validate's dict)] -> (the -o file, .kmerized.fa, LowComplexityReads.fa).  quals: the records are FASTQ, and SeqRecord::write
    gives the read's own quality line whatever the sequence; a merged read is SeqItem::write's FASTA either way."""
    record = lambda rid, read, seq: f"@{rid}\n{seq}\n+\n{'I' * len(read)}\n" if quals else f">{rid}\n{seq}\n"
    origin, kmerized, low = [], [], []
    for rid, read, w in records:
        rd = w["read"]
        if w["merged"]:
            origin.append(f">{rid}\n{w['seq']}\n")
        elif rd["kmerize"]:
            if rd["correct"]:
                kmerized.append(record(rid, read, rd["correct"]))
            kmerized += [f">{rid}:{i}\n{s}\n" for i, s in enumerate(rd["kmerized"])]
        else:
            low.append(record(rid, read, rd["correct"]))
    return "".join(origin), "".join(kmerized), "".join(low)


def summary_lines(wants) -> list[str]:
    kmerized = sum(1 for w in wants if w["read"]["kmerize"])
    merged = sum(1 for w in wants if not w["read"]["kmerize"] and w["merged"])
    return [f"Reads are kmerized: {kmerized}", f"Reads are merged : {merged}", f"Reads failed to kmerize or merge: {len(wants) - kmerized - merged}"]


# ---- the sets: single reads and options ------------------------------------------------------------------------------------
def _sub(read: str, at: int, d: int = 2) -> str:
    return read[:at] + _alt(read[at], d) + read[at + 1:]


def _vd(reads, k=K, x=X, m=M_MIN, max_overlap=-1, leaves=32):
    return dict(reads=list(reads), k=k, x=x, m=m, max_overlap=max_overlap, leaves=leaves)


CLEAN = GENOME[100:200]                                          # away from the copied stretch and from both SNPs
BOTH_ENDS_BAD = _sub(_sub(CLEAN, 5), 95)
NINE_TENTHS = "AAAAAACAAAAAACAAAAAA"                              # 18 of 20 bases: the float quotient is below the double 0.9
AROUND_SNP = [GENOME[540:630], HAP2[540:630], GENOME[1140:1230], HAP2[1140:1230]]
END_MER = GENOME[310:331]
G_RUN = GENOME[900:914]                                          # ...CGGGGGGT...: with -k 5 the only piece of two k-mers is GGGGGG
VD_SETS = {
    "short_kept": lambda: _vd([GENOME[100:100 + M_MIN], GENOME[100:110], NINE_TENTHS, "ACGT"]),
    "short_low_complexity": lambda: _vd(["A" * 20, "A" * 19 + "C", "T" * M_MIN, "G"]),
    "both_walks_agree": lambda: _vd([CLEAN, GENOME[1000:1160], revcomp(GENOME[700:780]), GENOME[1250:1470]]),
    "interior_error_is_walked_over": lambda: _vd([_sub(CLEAN, 50), _sub(GENOME[1000:1160], 80)]),
    "walk_longer_than_read": lambda: _vd([GENOME[100:150] + GENOME[152:200]]),
    "walk_shorter_keeps_read": lambda: _vd([GENOME[100:150] + "AC" + GENOME[150:200]]),
    "only_walk0": lambda: _vd([GENOME[231:361], GENOME[252:322]], leaves=1),
    "only_walk1": lambda: _vd([revcomp(GENOME[231:361]), GENOME[301:371]], leaves=1),
    # the last m-mer holds the thinner haplotype's allele; walk 0 comes to the site with a k-mer too long for that haplotype's reads
    "one_string_other_depth_falls_to_split": lambda: _vd([HAP2[1110:SNP2 + 1], HAP2[1086:SNP2 + 1]]),
    "bubble_two_results_coverage_picks": lambda: _vd(AROUND_SNP, max_overlap=30),
    "leaves_overflow": lambda: _vd(AROUND_SNP, max_overlap=30, leaves=1),
    "equal_end_mers_still_walked": lambda: _vd([END_MER + GENOME[331:380] + END_MER]),
    "bad_first_end_splits": lambda: _vd([_sub(CLEAN, 5), _sub(CLEAN, 95)]),
    "split_with_restart": lambda: _vd([_sub(_sub(GENOME[100:220], 5), 115), _sub(_sub(_sub(GENOME[1000:1160], 5), 80), 155)]),
    "main_piece_low_complexity": lambda: _vd([G_RUN], k=5, x=175, m=8),
    "x_is_1_all_qualify": lambda: _vd([BOTH_ENDS_BAD, _sub(BOTH_ENDS_BAD, 50)], x=1),
    "threshold_0_none_qualifies": lambda: _vd([CLEAN, BOTH_ENDS_BAD], x=0),
    "depth_truncation": lambda: _vd([GENOME[100:150] + GENOME[160:205], GENOME[100:150] + GENOME[161:206]]),
    "between_m_and_k": lambda: _vd([GENOME[100:180], _sub(_sub(GENOME[100:180], 5), 75)], k=100),
}
ENTRY_SETS = [n for n in VD_SETS if n != "threshold_0_none_qualifies"]     # what lrsc_fmwalk_validate takes
DEFAULT_SETS = [n for n in ENTRY_SETS if all(v == d for v, d in zip(list(VD_SETS[n]().values())[1:], (K, X, M_MIN, -1, 32)))]
_VD: dict = {}


def vd_options(s: dict) -> dict:
    return dict(k=s["k"], x=s["x"], m=s["m"], max_overlap=s["max_overlap"], leaves_max=s["leaves"])


def vd_case(name: str):
    """(the set, [plain_validate's dict per read], [its trace per read]), computed once per set"""
    if name not in _VD:
        s = VD_SETS[name]()
        c = index_case()[1]
        traces = [[] for _ in s["reads"]]
        _VD[name] = (s, [plain_validate(c, r, trace=t, **vd_options(s)) for r, t in zip(s["reads"], traces)], traces)
    return _VD[name]


def test_the_sets_hold_what_they_are_named_for():
    c = index_case()[1]
    reads = lambda name: vd_case(name)[0]["reads"]
    want = lambda name: vd_case(name)[1]
    events = lambda name, i, kind: [t for t in vd_case(name)[2][i] if t[0] == kind]
    status = lambda name: [tuple(w["status"]) for w in want(name)]
    split = lambda w: not w["merged"] and w["read"]["kmerize"] == 1 and len(w["read"]["pieces"]) >= 1
    strings = lambda name, i: [reads(name)[i][a: a + n] for a, n, _ in want(name)[i]["read"]["pieces"]]
    # n <= m: no walk, the read is its own correctSequence, kmerize says whether it is of low complexity; nine tenths exactly is not
    for name, km in (("short_kept", 1), ("short_low_complexity", 0)):
        assert all(len(r) <= M_MIN for r in reads(name)) and any(len(r) == M_MIN for r in reads(name))
        for r, w in zip(reads(name), want(name)):
            assert (w["merged"], w["status"], w["read"]["kmerize"], w["read"]["whole"], w["read"]["correct"], w["read"]["pieces"]) == (0, [0, 0], km, 1, r, [])
    assert NINE_TENTHS.count("A") * 10 == 9 * len(NINE_TENTHS) and NINE_TENTHS in reads("short_kept") and "A" * 19 + "C" in reads("short_low_complexity")
    # both walks find the read: walk 0's string is taken, diff0 being exactly 1
    for r, w in zip(reads("both_walks_agree"), want("both_walks_agree")):
        assert (w["merged"], w["chosen"], w["seq"], w["status"], w["walk_length"]) == (1, 0, r, [1, 1], [len(r)] * 2) and w["read"]["kmerize"] == 0
    assert 60 <= min(len(r) for r in reads("both_walks_agree")) and max(len(r) for r in reads("both_walks_agree")) == 220
    for r, w in zip(reads("interior_error_is_walked_over"), want("interior_error_is_walked_over")):
        assert w["merged"] and w["chosen"] == 0 and w["seq"] != r and len(w["seq"]) == len(r) and sum(a != b for a, b in zip(w["seq"], r)) == 1
        assert w["seq"] in GENOME
    (r,), (w,) = reads("walk_longer_than_read"), want("walk_longer_than_read")
    assert w["merged"] and w["chosen"] == 0 and w["seq"] == GENOME[100:200] and len(r) == 98 and w["length"] == 100
    (r,), (w,) = reads("walk_shorter_keeps_read"), want("walk_shorter_keeps_read")
    assert w["merged"] and w["chosen"] == -1 and w["seq"] == r and w["walk_length"] == [100, 100] and len(r) == 102 and w["status"] == [1, 1]
    # one walk alone, the other out of leaves: merged, with walk 1's string as it is, on the reverse strand
    assert status("only_walk0") == [(1, -3)] * 2 and all(w["merged"] and w["chosen"] == 0 and w["seq"] == r for r, w in zip(reads("only_walk0"), want("only_walk0")))
    assert status("only_walk1") == [(-3, 1)] * 2
    assert all(w["merged"] and w["chosen"] == 1 and w["seq"] == revcomp(r) for r, w in zip(reads("only_walk1"), want("only_walk1")))
    # one walk alone, the other out of depth: not merged, split
    o = want("one_string_other_depth_falls_to_split")
    assert status("one_string_other_depth_falls_to_split") == [(-2, 1)] * 2 and all(split(w) and w["walk_length"][0] == 0 < w["walk_length"][1] for w in o)
    assert all(r[-M_MIN:] in HAP2 and r[-M_MIN:] not in GENOME for r in reads("one_string_other_depth_falls_to_split"))
    # two results in one step of each walk; the strictly greater coverage wins, the first on a tie
    b = want("bubble_two_results_coverage_picks")
    for i, w in enumerate(b):
        res, covs = events("bubble_two_results_coverage_picks", i, "results"), events("bubble_two_results_coverage_picks", i, "cov")
        assert [t[1:] for t in res] == [(2, 2), (2, 2)] and len(covs) == 4 and w["status"] == [1, 1] and w["merged"] and w["chosen"] == 0
        first = covs[0] if covs[0][2] >= covs[1][2] else covs[1]
        assert w["seq"] == first[1] and w["coverage"][0] == max(covs[0][2], covs[1][2])
    assert any(events("bubble_two_results_coverage_picks", i, "cov")[0][2] != events("bubble_two_results_coverage_picks", i, "cov")[1][2] for i in range(4))
    assert any(w["seq"] != r for r, w in zip(AROUND_SNP, b)), "a read of the thinner haplotype is given the thicker one's allele"
    assert status("leaves_overflow") == [(-3, -3)] * 4 and all(split(w) for w in want("leaves_overflow"))
    # first m-mer == last m-mer: mergeTwoReads would return at once, validate walks
    (r,), (w,) = reads("equal_end_mers_still_walked"), want("equal_end_mers_still_walked")
    assert r[:M_MIN] == r[-M_MIN:] and plain_walk(c, r[:M_MIN], r[-M_MIN:], M_MIN, int(len(r) * 0.9), int(len(r) * 1.1), 32, X) == (1, r[:M_MIN], 0, 0)
    assert w["status"] == [-2, -2] and min(w["max_used_leaves"]) >= 1 and split(w)
    # an error in an end m-mer: that walk's root is in no read, the other never meets its terminal; the read is cut around the error
    bad = want("bad_first_end_splits")
    assert status("bad_first_end_splits") == [(-1, -2), (-2, -1)] and all(split(w) and len(w["read"]["pieces"]) > 1 for w in bad)
    # the k-mer that begins or ends with the wrong base still links simply to its neighbour on the clean side
    assert bad[0]["read"]["correct"] == reads("bad_first_end_splits")[0][5:] and bad[1]["read"]["correct"] == reads("bad_first_end_splits")[1][:96]
    for name in ("split_with_restart",):
        for r, w in zip(reads(name), want(name)):
            cq, restarts = serial_count_qualified(c, r, K, X - 1)
            assert split(w) and restarts >= 2 and 0 in cq and cq.count(1) > len(r) // 2
    (w,) = want("main_piece_low_complexity")
    rd = w["read"]
    assert split(w) and rd["main"] >= 0 and rd["pieces"][rd["main"]][2] == 0 and rd["correct"] == "" and strings("main_piece_low_complexity", 0)[rd["main"]] == "GGGGGG"
    assert len(rd["kmerized"]) == len(rd["pieces"]) - 1 and w["status"] == [-1, -1]
    # threshold - 1 of the split: 0 at -x 1, where every k-mer qualifies, erroneous ones too, and nothing is examined
    for r, w in zip(reads("x_is_1_all_qualify"), want("x_is_1_all_qualify")):
        assert serial_count_qualified(c, r, K, 0)[0] == [1] * (len(r) - K + 1) and any(c.both(r[i: i + K]) == 0 for i in range(len(r) - K + 1))
        assert split(w) and w["read"]["pieces"] == [(0, len(r), 1)] and w["read"]["main"] == 0 and w["read"]["correct"] == r and w["status"] == [-1, -1]
    # ... and wraps to the greatest size_t at 0: none qualifies, every boundary is examined (and with a threshold of 0 every base
    # extends a walk, which runs out of leaves)
    for r, w in zip(reads("threshold_0_none_qualifies"), want("threshold_0_none_qualifies")):
        assert serial_count_qualified(c, r, K, SIZE_MAX)[0] == [0] * (len(r) - K + 1) and w["status"] == [-3, -3] and split(w)
    assert want("threshold_0_none_qualifies")[0]["read"]["pieces"] == [(0, 100, 1)], "every link of a clean read is simple"
    assert len(want("threshold_0_none_qualifies")[1]["read"]["pieces"]) > 1
    # n = 95: n * 1.1 = 104.5, the depth is 104 and the longest string 105 bases
    d = want("depth_truncation")
    assert [len(r) for r in reads("depth_truncation")] == [95, 95] and int(95 * 1.1) == 104 and 95 * 11 % 10 != 0
    assert (d[0]["merged"], d[0]["walk_length"], d[0]["chosen"], d[0]["seq"]) == (1, [105, 105], 0, GENOME[100:205]) and d[1]["status"] == [-2, -2] and split(d[1])
    # m < n < k
    mk = want("between_m_and_k")
    assert all(M_MIN < len(r) < 100 for r in reads("between_m_and_k")) and mk[0]["merged"] == 1 and mk[0]["seq"] == reads("between_m_and_k")[0]
    assert (mk[1]["merged"], mk[1]["status"], mk[1]["read"]["kmerize"], mk[1]["read"]["pieces"], mk[1]["read"]["correct"]) == (0, [-1, -1], 0, [], "")
    assert len(DEFAULT_SETS) >= 11 and "threshold_0_none_qualifies" not in ENTRY_SETS and len(VD_SETS) == 19


def test_the_serial_count_equals_per_position_counts():
    """countQualified from the growing interval with its restarts == (occurrences of k-mer i + of its reverse complement >=
    threshold) at every position: on every read of every set with its own threshold, and with 0, 1, 5 and the wrapped one"""
    c = index_case()[1]
    n = restarts = 0
    for name in VD_SETS:
        s = vd_case(name)[0]
        for r in s["reads"]:
            if len(r) < s["k"]:
                continue
            for threshold in {(s["x"] - 1) % 2 ** 64, 0, 1, 5, SIZE_MAX}:
                cq, rs = serial_count_qualified(c, r, s["k"], threshold)
                assert cq == [1 if c.both(r[i: i + s["k"]]) >= threshold else 0 for i in range(len(r) - s["k"] + 1)], (name, threshold)
                restarts += rs
                n += 1
    assert n > 150 and restarts > 100


def test_validates_walk_is_merges_walk_where_the_shortcut_does_not_apply():
    c = index_case()[1]
    n = 0
    for name in DEFAULT_SETS + ["bubble_two_results_coverage_picks", "leaves_overflow", "only_walk0"]:
        s = vd_case(name)[0]
        for r in s["reads"]:
            if len(r) <= s["m"] or r[: s["m"]] == r[-s["m"]:]:
                continue
            mo = s["max_overlap"] if s["max_overlap"] != -1 else int(len(r) * 0.9)
            for t in (r, revcomp(r)):
                assert plain_validate_walk(c, t, s["m"], mo, int(len(t) * 1.1), s["leaves"], s["x"]) == \
                    plain_walk(c, t[: s["m"]], t[-s["m"]:], s["m"], mo, int(len(t) * 1.1), s["leaves"], s["x"])
                n += 1
    assert n >= 50


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _build(exe: Path, *flags: str) -> str:
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/fmwalk_validate_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def validate_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fmwalk_validate_driver") / "fmwalk_validate_driver")


def default_stride(reads) -> int:
    return int(max(len(r) for r in reads) * 1.1) + 1


def validate_dicts(res: np.ndarray, rows, pieces: np.ndarray, slots, reads, unwritten: int) -> list[dict]:
    """VALIDATE_DTYPE records, the merged rows as text and the pieces -> what plain_validate returns"""
    out = []
    for i, (q, row, read) in enumerate(zip(res, rows, reads)):
        out.append(dict(merged=int(q["merged"]), length=int(q["length"]), seq=row[: int(q["length"])] if q["merged"] else "", status=q["status"].tolist(),
                        max_used_leaves=q["max_used_leaves"].tolist(), coverage=q["coverage"].tolist(), walk_length=q["walk_length"].tolist(),
                        chosen=int(q["chosen"]), read=read_record(q["read"], pieces, int(slots[i]), read, unwritten)))
    check_unwritten(pieces, slots, [int(q["read"]["n_pieces"]) for q in res], unwritten)
    return out


def run_validate_driver(exe: str, name: str, wide: int):
    """-> [dict per read], Occ queries, block loads"""
    s = vd_case(name)[0]
    _, _, bwt, rbwt = index_case()
    reads = s["reads"]
    bases, off = reads_input(reads)
    n = len(reads)
    blob = b"".join([_image_input(bwt), _image_input(rbwt), np.array([s["k"], s["x"], s["m"], s["max_overlap"], 0, s["leaves"]], dtype=np.int32).tobytes(),
                     np.array([n], dtype=np.uint64).tobytes(), off.tobytes(), _codes(bases)])
    r = subprocess.run([exe, str(wide)], input=blob, capture_output=True)
    assert r.returncode == 0, (name, wide, r.returncode, r.stderr[-2000:])
    slots, stride = piece_slots(reads, s["k"]), default_stride(reads)
    res = np.frombuffer(r.stdout, dtype=VALIDATE_DTYPE, count=n)
    at = n * VALIDATE_DTYPE.itemsize
    rows = np.frombuffer(r.stdout, dtype=np.uint8, count=n * stride, offset=at).reshape(n, stride)
    at += n * stride
    pieces = np.frombuffer(r.stdout, dtype=PIECE_DTYPE, count=int(slots[-1]), offset=at)
    at += int(slots[-1]) * PIECE_DTYPE.itemsize
    ranks, loads = np.frombuffer(r.stdout, dtype=np.uint64, count=2, offset=at)
    assert at + 16 == len(r.stdout)
    for q, row in zip(res, rows):                                 # nothing is written beyond the sequence
        assert (row[int(q["length"]) if q["merged"] else 0:] == 0xFF).all()
    text = ["".join("ACGT"[c & 3] for c in row) for row in rows]
    return validate_dicts(res, text, pieces, slots, reads, 0xFFFFFFFF), int(ranks), int(loads)


def _run_sets(exe: str, wide: int) -> int:
    for name in VD_SETS:
        got, ranks, loads = run_validate_driver(exe, name, wide)
        want = vd_case(name)[1]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, wide, i)
        assert len(got) == len(want) and ranks // 2 <= loads <= ranks
    return len(VD_SETS)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_field_equals_the_yardstick(validate_driver, layout):
    assert VALIDATE_DTYPE.itemsize == 80
    assert _run_sets(validate_driver, LAYOUTS[layout]) == 19


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: every set, both layouts; workspaces, read, sequence and pieces are allocations of their own"""
    exe = _build(tmp_path / "fmwalk_validate_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        _run_sets(exe, wide)


# ---- the ABI, the kernels ---------------------------------------------------------------------------------------------------
def test_validate_entry_is_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    assert "lrsc_fmwalk_validate" in capi.declared_symbols() and " T lrsc_fmwalk_validate\n" in exported
    assert ("typedef struct lrsc_fmwalk_validate_result { uint32_t merged, length; int32_t status[2]; uint32_t max_used_leaves[2]; uint64_t coverage[2]; "
            "uint32_t walk_length[2]; int32_t chosen /* 0, 1: that walk's string; -1: the read itself or none */; lrsc_fmwalk_read_result read; } "
            "lrsc_fmwalk_validate_result;") in header
    assert re.search(r"int lrsc_fmwalk_validate\(lrsc_ctx\* ctx, const char\* reads, const uint64_t\* read_off, uint32_t n_reads, const lrsc_fmwalk_params\* p "
                     r"/\* max_insert ignored \*/,\s+char\* merged /\* n_reads \* stride \*/, uint64_t stride, lrsc_fmwalk_validate_result\* out, "
                     r"lrsc_fmwalk_piece\* pieces, uint64_t n_piece_slots\);", header)
    for lines in ("FMIndexWalkProcess.cpp:269-391", "613-722", "418-445", "855-881", "SAIntervalTree.cpp:59-94", "173-237", "248-350", "397-507", "318-352"):
        assert lines in header, lines
    for clause in (" 1. n <= m", " 2. Otherwise two walks", " 3. The decision", " 4. Everything else", " 5. m < n < k"):
        assert clause in header, clause
    limits = {n: int(v) for n, v in re.findall(r"#define LRSC_FMWALK_MAX_(\w+) (\d+)", header)}
    assert limits == {"LEAVES": 64, "INSERT": 2000, "MIN_OVERLAP": 255, "KMER": 255}
    assert "#define LRSC_ABI_VERSION 2\n" in header and api.lib.lrsc_abi_version() == 2
    assert capi.FMWALK_VALIDATE_DTYPE == VALIDATE_DTYPE and capi.FMWALK_VALIDATE_DTYPE.itemsize == 80
    assert callable(capi.Ctx.fmwalk_validate)


def test_validate_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_validate"), r"validate_[a-z]+_kernel")
    assert {k: len(v) for k, v in seen.items()} == {"validate_walk_kernel": 2, "validate_split_kernel": 2}, seen
    waves, threads = _const("kVdWavesPerSimd"), _const("kVdThreads")
    assert waves >= 4 and threads % 64 == 0
    for kernel in seen.values():
        for name, md in kernel:
            lds = md["group_segment_fixed_size"]
            assert md["max_flat_workgroup_size"] == threads
            # 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of LDS per CU for the workgroups of its four SIMDs
            assert md["vgpr_count"] <= 512 // waves // 8 * 8 == 128, (name, md)
            assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (name, md)
        assert {re.search(r"ILb([01])E", n).group(1) for n, _ in kernel} == {"0", "1"}
    make = (REPO / "longreadselfcorrect_amd/csrc/Makefile").read_text()
    assert "fm_validate.hip" in make and "fast-math" not in make


# ---- the command line --------------------------------------------------------------------------------------------------------
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"


def test_stride_fmwalk_validate_usage(api, tmp_path):
    from .test_fmwalk_host import FMWALK_USAGE

    run = lambda *args: subprocess.run([str(STRIDE), "fmwalk", *args], cwd=tmp_path, capture_output=True, text=True, input="")
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n")
    for args, message in ((["--validate", "-a", "merge", "reads.fa"], "FMIndexWalk: -a is not given together with --validate"),
                          (["--validate", "--algorithm=validate", "reads.fa"], "FMIndexWalk: -a is not given together with --validate"),
                          (["--validate", "--hybrid", "reads.fa"], "FMIndexWalk: --validate and --hybrid are two algorithms: give one"),
                          (["--kmerize", "--validate", "reads.fa"], "FMIndexWalk: --validate and --kmerize are two algorithms: give one"),
                          (["--validate"], "FMIndexWalk: missing arguments"),
                          (["--validate", "-x", "0", "reads.fa"], "FMIndexWalk: invalid kmer threshold: 0, must be greater than zero"),
                          (["--validate", "-m", "1", "reads.fa"], "FMIndexWalk: invalid min overlap: 1"),
                          # the refusal that test_fmwalk_host pins still holds, word for word
                          (["-a", "validate", "reads.fa"], "FMIndexWalk: -a validate is not built here: only -a merge is")):
        r = run(*args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert message in r.stderr and len([l for l in r.stderr.split("\n") if l.strip()]) == 1, (args, r.stderr)
        assert FMWALK_USAGE in r.stdout, (args, r.stdout, r.stderr)
        assert not [p.name for p in tmp_path.iterdir() if p.name != "reads.fa"], args
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith(FMWALK_USAGE) and r.stderr == ""
    usage = r.stdout.split("\n")
    assert len([l for l in usage if l.startswith("      --validate ")]) == 1 and "hybrid (default), merge, kmerize, or validate" in r.stdout
    # without an index the run ends before a file is opened; the command end to end is test_gpu_fmwalk_validate's
    r = run("--validate", "reads.fa")
    assert r.returncode == 1 and not [p.name for p in tmp_path.iterdir() if p.name != "reads.fa"]


TINY = ["short_kept", "short_low_complexity", "both_walks_agree", "only_walk1", "bad_first_end_splits", "main_piece_low_complexity", "between_m_and_k"]


def test_the_three_files_and_the_summary_lines_on_a_tiny_input(api, tmp_path):
    """the command's post-processor (host/FMIndexWalkProcess.cpp) fed the yardstick's results of a few reads as text, FASTA and
    FASTQ records: PREFIX.origin.fa, PREFIX.kmerized.fa, LowComplexityReads.fa and the three lines against written_files"""
    exe = tmp_path / "fmwalk_post_driver"
    lib = Path(api.path)
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(REPO / "tests/host_tools/fmwalk_post_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/host/FMIndexWalkProcess.cpp"), f"-L{lib.parent}", "-llrsc_hip", f"-Wl,-rpath,{lib.parent}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    records = [(f"{name}.{i}", r, w) for name in TINY for i, (r, w) in enumerate(zip(vd_case(name)[0]["reads"], vd_case(name)[1]))]
    assert {(w["merged"], w["read"]["kmerize"]) for _, _, w in records} == {(1, 0), (0, 1), (0, 0)}
    assert any(not w["merged"] and w["read"]["kmerize"] and not w["read"]["correct"] for _, _, w in records), "a kmerized read without a correctSequence"
    text = "".join(f"{rid} {r} - {w['merged']} {w['read']['kmerize']} {(w['seq'] if w['merged'] else w['read']['correct']) or '-'} "
                   f"{len(w['read']['kmerized'])} {' '.join(w['read']['kmerized'])}\n" for rid, r, w in records)
    r = subprocess.run([str(exe), "tiny.origin.fa", "tiny.kmerized.fa", "LowComplexityReads.fa"], cwd=tmp_path, input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    origin, kmerized, low = written_files(records)
    assert origin and kmerized and low
    assert ((tmp_path / "tiny.origin.fa").read_text(), (tmp_path / "tiny.kmerized.fa").read_text(), (tmp_path / "LowComplexityReads.fa").read_text()) == \
        (origin, kmerized, low)
    assert r.stdout.split("\n")[:3] == summary_lines([w for _, _, w in records])
    # a FASTQ record: merged reads are FASTA whatever the record (SeqItem::write), the others keep the record's quality line
    text = "m ACGT IIII 1 0 ACGTT 0\nk ACGT IIII 0 1 ACG 1 GT\nn ACGT IIII 0 0 - 0\n"
    r = subprocess.run([str(exe), "q.origin.fa", "q.kmerized.fa", "q.low.fa"], cwd=tmp_path, input=text, capture_output=True, text=True)
    assert r.returncode == 0 and (tmp_path / "q.origin.fa").read_text() == ">m\nACGTT\n"
    assert (tmp_path / "q.kmerized.fa").read_text() == "@k\nACG\n+\nIIII\n>k:0\nGT\n" and (tmp_path / "q.low.fa").read_text() == "@n\n\n+\nIIII\n"
    assert r.stdout.split("\n")[:3] == ["Reads are kmerized: 1", "Reads are merged : 1", "Reads failed to kmerize or merge: 1"]
