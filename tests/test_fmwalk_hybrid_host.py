"""fmwalk's hybrid and kmerize algorithms and the sampled k-mer counts (csrc/fm_kmerize.h, fm_kmerize.hip, capi_fmwalk.cpp) checked
without a GPU.

1. The yardstick: FMIndexWalkProcess::splitRead(KmerContext&), KmerizeReads, MergeAndKmerize, isLowComplexity, maxCon and
   BWTAlgorithms::sampleKmerCounts' body restated line by line in plain Python over strings, the count of a string taken from
   test_fmwalk_host's Counts; the trim and the walk are that module's plain_trim and plain_walk.  The named sets, each with an
   assertion that it holds what it is named for.
2. The per-lane, per-read and per-pair code that the kernels call, compiled for the CPU (tests/host_tools/fmwalk_hybrid_driver.cpp)
   and run in the kernels' order: every field equals the yardstick's on every set, for both layouts.  The driver again under
   AddressSanitizer and UBSan, as a stand-alone program.
3. The yardstick against the definition: the k-mer counts against brute force, the sample counts against LF steps over the literal
   BWT and against the read the row belongs to.
4. The entries and their structs are declared, exported and bound, the ABI version is still 2.
5. The kernels compile for gfx950 without scratch, spills or AGPRs, within the registers and the LDS their launch is sized for.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_fmwalk_host import GENOME, HAP2, INSERT, K, M_MIN, SNP, X, Counts, _alt, ends, index_case, plain_trim, plain_walk
from .test_index_filter_host import LAYOUTS, _image_input, _kernel_notes, _kernels, revcomp
from .test_index_merge_host import CODE

PIECE_DTYPE = np.dtype([("start", "<u4"), ("length", "<u4"), ("kept", "<u4")])
READ_DTYPE = np.dtype([("kmerize", "<u4"), ("head", "<i4"), ("length", "<u4"), ("n_pieces", "<u4"), ("main_piece", "<i4"), ("whole", "<u4")])
WALK_DTYPE = np.dtype([("merged", "<u4"), ("length", "<u4"), ("status", "<i4", (2,)), ("max_used_leaves", "<u4", (2,)), ("coverage", "<u8", (2,)),
                       ("trimmed_length", "<u4", (2,))], align=True)
HYBRID_DTYPE = np.dtype([("walk", WALK_DTYPE), ("read", READ_DTYPE, (2,))], align=True)
WALK_X = 3                                                       # SAIntervalTree's default SA_threshold


def _const(name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", (REPO / "longreadselfcorrect_amd/csrc/fm_kmerize.h").read_text())
    assert m, name
    return int(m.group(1))


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def literal_max_con(s: str) -> int:
    """maxCon (FMIndexWalkProcess.cpp:448-477), statement by statement"""
    c, mx = 1, 1
    for i in range(1, len(s)):
        if s[i] == "N":
            continue
        if s[i] != s[i - 1]:
            if c > mx:
                mx = c
            c = 1
        else:
            c += 1
            if i == len(s) - 1:
                if c > mx:
                    mx = c
            elif s[i] != s[i + 1]:
                if c > mx:
                    mx = c
    return mx


def literal_low_complexity(s: str) -> bool:
    """isLowComplexity (418-445): (float) count / seqLen >= 0.9, a float quotient against the double 0.9"""
    n = np.float32(len(s))
    return any(float(np.float32(s.count(b)) / n) >= 0.9 for b in "ATCG")


def num_next_kmer(c: Counts, kmer: str, end: bool, threshold: int) -> int:
    """numNextKmer (855-870)"""
    return sum(1 for b in "ATCG" if c.both(kmer[1:] + b if end else b + kmer[:-1]) >= threshold)


def is_simple(c: Counts, left: str, right: str) -> bool:
    """isSimple (873-881) with its threshold of 1"""
    return num_next_kmer(c, left, True, 1) == 1 and num_next_kmer(c, right, False, 1) == 1


def count_qualified(c: Counts, seq: str, k: int, x: int) -> list[int]:
    """KmerContext's two counts per k-mer against the threshold (FMIndexWalkProcess.h:74-92, .cpp:559-565)"""
    kmers = [seq[i: i + k] for i in range(len(seq) - k + 1)]
    return [(1 if c.single(w) >= x else 0) + (1 if c.single(revcomp(w)) >= x else 0) for w in kmers]


def plain_split(c: Counts, seq: str, k: int, x: int):
    """splitRead(KmerContext(seq, k)) (555-609), len(seq) >= k -> ([(first k-mer, the piece's string)], mainSeedIdx)"""
    nk = len(seq) - k + 1
    cq = count_qualified(c, seq, k, x)
    intervals, start = [], 0
    for p in range(1, nk):
        if cq[p - 1] == 2 and cq[p] == 2:
            continue
        if not is_simple(c, seq[p - 1: p - 1 + k], seq[p: p + k]):
            intervals.append((start, p - 1))
            start = p
    intervals.append((start, nk - 1))
    max_num, main, pieces = 0, -1, []
    for i, (a, b) in enumerate(intervals):
        if any(cq[j] == 2 for j in range(a, b + 1)):
            if max_num < b - a:
                max_num, main = b - a, i
        pieces.append((a, seq[a: b + k]))
    return pieces, main


def _read_record(head: int, trimmed: str) -> dict:
    return dict(kmerize=0, head=head, length=len(trimmed), main=-1, whole=0, pieces=[], correct="", kmerized=[])


def _split_into(c: Counts, rd: dict, seq: str, k: int, x: int, filters: bool):
    """the loops over firstKR (126-135, 255-264): the pieces as (start in the untrimmed read, length, kept)"""
    pieces, main = plain_split(c, seq, k, x)
    rd["kmerize"], rd["main"] = 1, main
    for i, (a, s) in enumerate(pieces):
        kept = not (filters and (literal_low_complexity(s) or literal_max_con(s) * 3 > len(s)))
        rd["pieces"].append((rd["head"] + a, len(s), int(kept)))
        if not kept:
            continue
        if i == main:
            rd["correct"] = s
        else:
            rd["kmerized"].append(s)


def plain_kmerize(c: Counts, read: str, k: int = K, x: int = X) -> dict:
    """KmerizeReads (229-267)"""
    if len(read) < k:
        return _read_record(0, "")
    rd = _read_record(0, read)
    _split_into(c, rd, read, k, x, False)
    return rd


def trim_at(c: Counts, read: str, k: int):
    """(head, trimRead's string); a read shorter than k, on which the reference throws, counts as trimmed to nothing"""
    if len(read) < k:
        return 0, ""
    t = plain_trim(c, read, k)
    if not t:
        return 0, ""
    heads = [h for h in range(len(read) - len(t) + 1) if read[h: h + len(t)] == t]
    # trimRead's own head: the first position from the left that it stops at
    def num_next(p):
        return num_next_kmer(c, read[p: p + k], False, 1)
    head = 0
    if num_next(0) == 0:
        head = 1
        while head <= len(read) - k and num_next(head) < 2:
            head += 1
    assert head in heads
    return head, t


def plain_merge_and_kmerize(c: Counts, r1: str, r2: str, repeat: int, k: int = K, x: int = X, m: int = M_MIN, max_overlap: int = -1, insert: int = INSERT,
                            leaves_max: int = 32) -> dict:
    """MergeAndKmerize (29-150) -> the walk's record as plain_fmwalk_merge gives it, and a record per read"""
    (h1, s1), (h2, s2) = trim_at(c, r1, k), trim_at(c, r2, k)
    walk = dict(merged=0, length=0, seq="", status=[0, 0], max_used_leaves=[0, 0], coverage=[0, 0], trimmed_length=[len(s1), len(s2)])
    reads = [_read_record(h1, s1), _read_record(h2, s2)]
    out = dict(walk=walk, reads=reads)
    if (k <= len(s1) <= m) or (k <= len(s2) <= m):
        for rd, s in zip(reads, (s1, s2)):
            rd.update(kmerize=1, whole=1, correct=s)
    elif len(s1) < k or len(s2) < k:
        return out
    a, b = s1[:m], s2[:m]
    if len(a) >= m and len(b) >= m and c.both(a) < repeat and c.both(b) < repeat:             # isSuitableForFMWalk (394-415)
        mo = max_overlap if max_overlap != -1 else int(((len(r1) + len(r2)) // 2) * 0.95)
        w1 = plain_walk(c, a, revcomp(b), m, mo, insert, leaves_max, WALK_X)
        w2 = plain_walk(c, b, revcomp(a), m, mo, insert, leaves_max, WALK_X)
        walk["status"], walk["max_used_leaves"], walk["coverage"] = [w1[0], w2[0]], [w1[2], w2[2]], [w1[3], w2[3]]
        q1, q2, few = w1[1], w2[1], w1[2] <= 1 and w2[2] <= 1
        seq = ""
        if q1 and not q2 and few:
            seq = q1
        elif not q1 and q2 and few:
            seq = q2
        elif q1 and q2 and q1 == revcomp(q2):
            seq = q1 if w1[3] > w2[3] else q2
        if seq:
            walk.update(merged=1, length=len(seq), seq=seq)
            return out
    for rd, s in zip(reads, (s1, s2)):                            # case 3
        if len(s) >= k:
            _split_into(c, rd, s, k, x, True)
    return out


def plain_sample_count(c: Counts, reads: list[str], row: int, length: int) -> int:
    """extractString(pRBWT, row, length) and countSequenceOccurrences of it in .rbwt (BWTAlgorithms.cpp:454-469, 135-141): the
    '$' row `row` of .rbwt is read `row`'s reverse, the LF steps give its last bases first, the string is their reverse: the
    reverse of the read's first `length` bases.  Its occurrences in the reversed reads, and its reverse complement's, are those
    of the read's prefix and of the prefix's reverse complement in the reads."""
    return c.both(reads[row][:length])


# ---- the sets --------------------------------------------------------------------------------------------------------------
def _sub(read: str, at: int, d: int = 2) -> str:
    return read[:at] + _alt(read[at], d) + read[at + 1:]


NINE_TENTHS = "AAAAAACAAAAAACAAAAAA"                              # 18 of 20 bases: not low complexity; runs of 6: 18 <= 20
LONG_RUN = "ACGTACG" + "T" * 8 + "ACGTA"                         # half T, a run of 8: 24 > 20
POLY_A = "A" * 20
K20 = 20

KMERIZE_SETS = {
    # (reads, k, x)
    "solid_and_exact": lambda: ([GENOME[400:470], GENOME[400:400 + K], GENOME[1000:1131], "ACGTACGT", "A"], K, X),
    "weak_but_simple": lambda: ([GENOME[1430:1495], revcomp(GENOME[5:70])], K, X),
    "substitutions": lambda: ([_sub(GENOME[400:470], at) for at in (20, 34, 35, 49)] + [_sub(GENOME[400:471], 35), _sub(_sub(GENOME[400:490], 30), 61)], K, X),
    "haplotypes_x5": lambda: ([HAP2[SNP - 40: SNP + 40], GENOME[1160:1240], HAP2[1160:1240]], K, 5),
    "k21": lambda: ([GENOME[400:470], _sub(GENOME[400:470], 35), GENOME[250:380]], 21, X),
}


def _junk_read(junk: str) -> str:
    return GENOME[400:440] + junk + GENOME[460:500]


def _hy(pairs, repeat, k=K, x=X, m=M_MIN, max_overlap=-1, insert=INSERT, leaves=32):
    return dict(pairs=list(pairs), repeat=repeat, k=k, x=x, m=m, max_overlap=max_overlap, insert=insert, leaves=leaves)


NO_WALK = 0                                                      # a repeat cutoff below every count: no pair is walked
ANY_WALK = 10 ** 6
U1, U2 = ends(GENOME, 100, 130)
RUN_OF_SIX = GENOME[485:502]                                     # 17 bases around AAAAAA: 6 * 3 > 17
_both_ways = lambda p: [p, (p[1], p[0])]
HYBRID_SETS = {
    "merges_as_merge_does": lambda: _hy([ends(GENOME, 100, 130), ends(GENOME, 1407, 70), ends(GENOME, 7, 70), ends(GENOME, 100, 100)], ANY_WALK),
    "one_walk_alone_merges": lambda: _hy(_both_ways(ends(HAP2, 880, 65)) + _both_ways(ends(HAP2, 1197, 114)), ANY_WALK, leaves=2),
    "one_walk_alone_with_two_leaves": lambda: _hy([ends(GENOME, 231, 130), ends(GENOME, 252, 70), ends(GENOME, 301, 70)], ANY_WALK, leaves=1),
    "bubble": lambda: _hy([ends(GENOME, 540, 90), ends(HAP2, 540, 90), ends(GENOME, 1140, 90), ends(HAP2, 1140, 90)], ANY_WALK, max_overlap=30),
    "bubble_l1": lambda: _hy([ends(GENOME, 540, 90), ends(HAP2, 1140, 90)], ANY_WALK, max_overlap=30, leaves=1),
    "too_deep": lambda: _hy([ends(GENOME, 100, 130)], ANY_WALK, insert=90),
    "repeat_cutoff_0": lambda: _hy([ends(GENOME, 100, 130), ends(GENOME, 1407, 70)], NO_WALK),
    "repeat_cutoff_at_the_count": lambda: _hy([(U1, U2)], 20),
    "repeat_cutoff_above_the_count": lambda: _hy([(U1, U2)], 21),
    "x_is_not_the_walks": lambda: _hy([ends(GENOME, 100, 130), ends(GENOME, 1407, 70), ends(GENOME, 231, 130)], ANY_WALK, x=12, leaves=1),
    "length_gate": lambda: _hy([(U1[:M_MIN], U2), (U1[:K], U2[:K]), (U1[:M_MIN], U2[:M_MIN]), (U1[:K + 3], _sub(_sub(U2, 0), 49))], ANY_WALK),
    "trimmed_below_k": lambda: _hy([(_sub(_sub(U1, 0), 49), U2), (U1, "ACGTACGT"), ("ACGT", "A"), (_sub(U1, 0), U2)], ANY_WALK),
    "filters_k20": lambda: _hy([(_junk_read(NINE_TENTHS), _junk_read(LONG_RUN)), (_junk_read(POLY_A), GENOME[700:760])], NO_WALK, k=K20),
    "main_filtered_after_the_gate": lambda: _hy([(RUN_OF_SIX, U2), (U2, RUN_OF_SIX)], ANY_WALK),
    "substitutions": lambda: _hy([(_sub(U1, 25), U2), (U1, _sub(U2, 30)), (_sub(U1, 10), _sub(U2, 40))], ANY_WALK),
}
_KM: dict = {}
_HY: dict = {}


def km_case(name: str):
    """((reads, k, x), [plain_kmerize's record per read]), computed once per set"""
    if name not in _KM:
        s = KMERIZE_SETS[name]()
        c = index_case()[1]
        _KM[name] = (s, [plain_kmerize(c, r, s[1], s[2]) for r in s[0]])
    return _KM[name]


def hy_options(s: dict) -> dict:
    return dict(k=s["k"], x=s["x"], m=s["m"], max_overlap=s["max_overlap"], insert=s["insert"], leaves_max=s["leaves"])


def hy_case(name: str):
    """(the set, [plain_merge_and_kmerize's record per pair]), computed once per set"""
    if name not in _HY:
        s = HYBRID_SETS[name]()
        c = index_case()[1]
        _HY[name] = (s, [plain_merge_and_kmerize(c, r1, r2, s["repeat"], **hy_options(s)) for r1, r2 in s["pairs"]])
    return _HY[name]


def test_the_sets_hold_what_they_are_named_for():
    c = index_case()[1]
    km = lambda name: km_case(name)[1]
    hy = lambda name: hy_case(name)[1]
    span = lambda rd, i: rd["pieces"][i][1] - km_case("substitutions")[0][1]
    # kmerize: an all-solid read is one piece and the main one; a read of exactly k bases is one piece and not the main one,
    # maxIntervalNum starting at 0; a read shorter than k gives nothing
    s = km("solid_and_exact")
    assert [(len(w["pieces"]), w["main"], w["kmerize"]) for w in s] == [(1, 0, 1), (1, -1, 1), (1, 0, 1), (0, -1, 0), (0, -1, 0)]
    assert s[1]["correct"] == "" and s[1]["kmerized"] == [GENOME[400:400 + K]] and s[0]["correct"] == GENOME[400:470] and s[0]["kmerized"] == []
    assert all(q == 2 for q in count_qualified(c, GENOME[400:470], K, X))
    # a stretch whose k-mers are below the threshold on a strand, with one way on either side of every boundary: not cut
    for r, w in zip(km_case("weak_but_simple")[0][0], km("weak_but_simple")):
        assert sum(1 for q in count_qualified(c, r, K, X) if q < 2) >= 4 and len(w["pieces"]) == 1 and w["main"] == 0
    # a substitution: the k-mer that ends with it still links simply to the one before, the others stand alone; pieces on both sides
    sub = km("substitutions")
    assert [len(w["pieces"]) for w in sub] == [15, 15, 15, 15, 15, 29]
    assert sub[1]["pieces"][0] == (0, 35, 1) and sub[1]["pieces"][-1] == (34, 36, 1) and sub[1]["main"] == 14
    assert sub[2]["pieces"][0] == (0, 36, 1) and sub[2]["pieces"][-1] == (35, 35, 1) and sub[2]["main"] == 0
    assert all(p[1] == K for w in sub for p in w["pieces"][1:-1][:13]) and all(len(w["kmerized"]) == len(w["pieces"]) - 1 for w in sub)
    # two intervals of 22 k-mers each: the first is the main one
    assert span(sub[4], 0) == span(sub[4], -1) == 21 and sub[4]["main"] == 0
    assert sub[5]["main"] not in (0, 28) and span(sub[5], sub[5]["main"]) > max(span(sub[5], 0), span(sub[5], -1))
    # -x 5: the thinner haplotype's k-mers are weak at its allele and the read is cut there, the thicker one's are not
    h = km("haplotypes_x5")
    assert [len(w["pieces"]) for w in h] == [1, 1, 3] and len(km("k21")[1]["pieces"]) == 21 and km("k21")[1]["pieces"][1][1] == 21
    # hybrid: what merge mode merges by two walks of equal length is merged here when one string is the other's reverse
    # complement, and the coverage picks
    m = hy("merges_as_merge_does")
    assert all(w["walk"]["merged"] and w["walk"]["status"] == [1, 1] and not any(rd["kmerize"] for rd in w["reads"]) for w in m)
    assert m[1]["walk"]["coverage"][0] > m[1]["walk"]["coverage"][1] and m[1]["walk"]["seq"] == GENOME[1407:1477]
    assert m[2]["walk"]["coverage"][0] < m[2]["walk"]["coverage"][1] and revcomp(m[2]["walk"]["seq"]) == GENOME[7:77]
    # one walk alone, neither with more than a leaf: merged, whichever of the two it is
    one = [w["walk"] for w in hy("one_walk_alone_merges")]
    assert all(w["merged"] and max(w["max_used_leaves"]) <= 1 for w in one) and {tuple(w["status"]) for w in one} == {(1, -2), (-2, 1)}
    # the same with two leaves somewhere: refused, and the reads are split
    two = hy("one_walk_alone_with_two_leaves")
    assert [tuple(w["walk"]["status"]) for w in two] == [(1, -3), (1, -3), (-3, 1)] and not any(w["walk"]["merged"] for w in two)
    assert two[1]["walk"]["max_used_leaves"] == [1, 2] and all(rd["kmerize"] and rd["pieces"] for w in two for rd in w["reads"])
    # both walks find, and the strings are not each other's reverse complement (each took its own side of the bubble)
    b = hy("bubble")
    assert [(w["walk"]["merged"], tuple(w["walk"]["status"])) for w in b] == [(0, (1, 1)), (0, (1, 1)), (1, (1, 1)), (1, (1, 1))]
    assert all(not w["walk"]["merged"] and w["walk"]["status"] == [-3, -3] for w in hy("bubble_l1"))
    assert hy("too_deep")[0]["walk"]["status"] == [-2, -2]
    # the repeat gate: strictly below the cutoff
    assert c.both(U1[:M_MIN]) == c.both(U2[:M_MIN]) == 20
    assert hy("repeat_cutoff_at_the_count")[0]["walk"]["status"] == [0, 0] and hy("repeat_cutoff_above_the_count")[0]["walk"]["merged"] == 1
    assert all(w["walk"]["status"] == [0, 0] and all(rd["main"] == 0 and rd["correct"] == r for rd, r in zip(w["reads"], p))
               for w, p in zip(hy("repeat_cutoff_0"), hy_case("repeat_cutoff_0")[0]["pairs"]))
    # -x 12: the walks still go with 3 (with 12 they would not find: a 21-mer occurs about ten times)
    xs = hy("x_is_not_the_walks")
    assert [w["walk"]["merged"] for w in xs] == [1, 1, 0] and xs[1]["walk"] == m[1]["walk"]
    assert plain_walk(c, ends(GENOME, 1407, 70)[0][:M_MIN], revcomp(ends(GENOME, 1407, 70)[1][:M_MIN]), M_MIN, 47, INSERT, 1, 12)[0] != 1
    # the [k, m] gate marks both reads and goes on: to a merge, or to the split, whose lone piece of one k-mer is no main piece
    g = hy("length_gate")
    assert [w["walk"]["merged"] for w in g] == [1, 0, 1, 0] and all(rd["whole"] == 1 and rd["kmerize"] == 1 for w in g for rd in w["reads"])
    assert [rd["length"] for rd in g[0]["reads"]] == [M_MIN, 50] and [(rd["main"], rd["correct"], rd["kmerized"]) for rd in g[1]["reads"]] == \
        [(-1, U1[:K], [U1[:K]]), (-1, U2[:K], [U2[:K]])]
    assert [(rd["length"], rd["kmerize"], rd["correct"], len(rd["pieces"])) for rd in g[3]["reads"]] == [(K + 3, 1, U1[:K + 3], 1), (0, 1, "", 0)]
    # a trimmed read below k without the gate: nothing
    t = hy("trimmed_below_k")
    assert [w["walk"]["trimmed_length"] for w in t] == [[0, 50], [50, 0], [0, 0], [0, 50]]
    assert all(not rd["kmerize"] and not rd["pieces"] and not rd["whole"] for w in t for rd in w["reads"])
    # the filters
    f = hy("filters_k20")
    strings = lambda rd, r: [r[a: a + n] for a, n, kept in rd["pieces"]]
    (r1, r2), (r3, _) = hy_case("filters_k20")[0]["pairs"]
    assert NINE_TENTHS in f[0]["reads"][0]["kmerized"] and NINE_TENTHS.count("A") * 10 == 9 * len(NINE_TENTHS) and literal_max_con(NINE_TENTHS) * 3 <= 20
    assert not literal_low_complexity(NINE_TENTHS) and literal_low_complexity("A" * 19 + "C")
    at = strings(f[0]["reads"][1], r2).index(LONG_RUN)
    assert f[0]["reads"][1]["pieces"][at][2] == 0 and not literal_low_complexity(LONG_RUN) and literal_max_con(LONG_RUN) * 3 > 20
    at = strings(f[1]["reads"][0], r3).index(POLY_A)
    assert f[1]["reads"][0]["pieces"][at][2] == 0 and literal_low_complexity(POLY_A)
    assert f[0]["reads"][0]["main"] == 0 and f[0]["reads"][0]["correct"] == r1[:41], "the k-mer that ends with the first foreign base"
    # numbers of the other pieces: the index into kmerizedReads, which a dropped piece does not take
    assert len(f[1]["reads"][0]["kmerized"]) < len(f[1]["reads"][0]["pieces"]) - 1
    # a main piece that the filter drops leaves the gate's correctSequence
    for w, e in zip(hy("main_filtered_after_the_gate"), (0, 1)):
        rd = w["reads"][e]
        assert (rd["whole"], rd["main"], rd["pieces"], rd["correct"], rd["kmerized"]) == (1, 0, [(0, 17, 0)], RUN_OF_SIX, [])
        assert literal_max_con(RUN_OF_SIX) == 6 and w["reads"][1 - e]["correct"] == U2


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _build(exe: Path, *flags: str) -> str:
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/fmwalk_hybrid_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def hybrid_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fmwalk_hybrid_driver") / "fmwalk_hybrid_driver")


def reads_input(reads) -> tuple[np.ndarray, np.ndarray]:
    """(the ASCII bases of the reads back to back, their n + 1 offsets)"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8), off


def piece_slots(reads, k: int) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([max(len(r) - k + 1, 0) for r in reads])]).astype(np.int64)


def read_record(rec, pieces: np.ndarray, slot: int, read: str, unwritten: int) -> dict:
    """a READ_DTYPE record and the read's slots of the pieces -> what the yardstick gives of the read"""
    n, main = int(rec["n_pieces"]), int(rec["main_piece"])
    ps = [(int(q["start"]), int(q["length"]), int(q["kept"])) for q in pieces[slot: slot + n]]
    trimmed = read[int(rec["head"]): int(rec["head"]) + int(rec["length"])]
    correct = trimmed if rec["whole"] else ""
    if main >= 0 and ps[main][2]:
        correct = read[ps[main][0]: ps[main][0] + ps[main][1]]
    kmerized = [read[a: a + ln] for i, (a, ln, kept) in enumerate(ps) if kept and i != main]
    return dict(kmerize=int(rec["kmerize"]), head=int(rec["head"]), length=int(rec["length"]), main=main, whole=int(rec["whole"]), pieces=ps, correct=correct,
                kmerized=kmerized)


def check_unwritten(pieces: np.ndarray, slots: np.ndarray, counts, unwritten: int):
    raw = pieces.view(np.uint32).reshape(-1, 3)
    for i, n in enumerate(counts):
        assert (raw[int(slots[i]) + n: int(slots[i + 1])] == unwritten).all(), i


def hybrid_dicts(res: np.ndarray, rows, pieces: np.ndarray, slots, pairs, unwritten: int) -> list[dict]:
    out = []
    for i, (q, row, pair) in enumerate(zip(res, rows, pairs)):
        w = q["walk"]
        walk = dict(merged=int(w["merged"]), length=int(w["length"]), seq=row[: int(w["length"])] if w["merged"] else "", status=w["status"].tolist(),
                    max_used_leaves=w["max_used_leaves"].tolist(), coverage=w["coverage"].tolist(), trimmed_length=w["trimmed_length"].tolist())
        out.append(dict(walk=walk, reads=[read_record(q["read"][e], pieces, int(slots[2 * i + e]), pair[e], unwritten) for e in range(2)]))
    check_unwritten(pieces, slots, [int(q["read"][e]["n_pieces"]) for q in res for e in range(2)], unwritten)
    return out


def _codes(bases: np.ndarray) -> bytes:
    return bytes(CODE[chr(b)] - 1 for b in bases)


def _run(exe: str, wide: int, mode: str, blob: bytes) -> bytes:
    _, _, bwt, rbwt = index_case()
    r = subprocess.run([exe, str(wide), mode], input=_image_input(bwt) + _image_input(rbwt) + blob, capture_output=True)
    assert r.returncode == 0, (mode, wide, r.returncode, r.stderr[-2000:])
    return r.stdout


def run_kmerize_driver(exe: str, name: str, wide: int):
    """-> [record per read], Occ queries, block loads"""
    (reads, k, x), _ = km_case(name)
    bases, off = reads_input(reads)
    out = _run(exe, wide, "kmerize", np.array([k, x], dtype=np.int32).tobytes() + np.array([len(reads)], dtype=np.uint64).tobytes() + off.tobytes() + _codes(bases))
    slots = piece_slots(reads, k)
    res = np.frombuffer(out, dtype=READ_DTYPE, count=len(reads))
    at = len(reads) * READ_DTYPE.itemsize
    pieces = np.frombuffer(out, dtype=PIECE_DTYPE, count=int(slots[-1]), offset=at)
    at += int(slots[-1]) * PIECE_DTYPE.itemsize
    ranks, loads = np.frombuffer(out, dtype=np.uint64, count=2, offset=at)
    assert at + 16 == len(out)
    check_unwritten(pieces, slots, [int(q["n_pieces"]) for q in res], 0xFFFFFFFF)
    return [read_record(q, pieces, int(slots[i]), reads[i], 0xFFFFFFFF) for i, q in enumerate(res)], int(ranks), int(loads)


def run_hybrid_driver(exe: str, name: str, wide: int):
    s, _ = hy_case(name)
    reads = [r for p in s["pairs"] for r in p]
    bases, off = reads_input(reads)
    n = len(s["pairs"])
    out = _run(exe, wide, "hybrid", np.array([s["k"], s["x"], s["m"], s["max_overlap"], s["insert"], s["leaves"]], dtype=np.int32).tobytes() +
               np.array([s["repeat"], n], dtype=np.uint64).tobytes() + off.tobytes() + _codes(bases))
    slots, stride = piece_slots(reads, s["k"]), max(s["insert"] + 1, s["m"])
    res = np.frombuffer(out, dtype=HYBRID_DTYPE, count=n)
    at = n * HYBRID_DTYPE.itemsize
    rows = np.frombuffer(out, dtype=np.uint8, count=n * stride, offset=at).reshape(n, stride)
    at += n * stride
    pieces = np.frombuffer(out, dtype=PIECE_DTYPE, count=int(slots[-1]), offset=at)
    at += int(slots[-1]) * PIECE_DTYPE.itemsize
    ranks, loads = np.frombuffer(out, dtype=np.uint64, count=2, offset=at)
    assert at + 16 == len(out)
    for q, row in zip(res, rows):                                 # nothing is written beyond the merged string
        assert (row[int(q["walk"]["length"]) if q["walk"]["merged"] else 0:] == 0xFF).all()
    text = ["".join("ACGT"[c & 3] for c in row) for row in rows]
    return hybrid_dicts(res, text, pieces, slots, s["pairs"], 0xFFFFFFFF), int(ranks), int(loads)


def _run_sets(exe: str, wide: int) -> int:
    for name in KMERIZE_SETS:
        got, ranks, loads = run_kmerize_driver(exe, name, wide)
        assert got == km_case(name)[1], (name, wide)
        assert ranks // 2 <= loads <= ranks
    for name in HYBRID_SETS:
        got, ranks, loads = run_hybrid_driver(exe, name, wide)
        for i, (g, w) in enumerate(zip(got, hy_case(name)[1])):
            assert g == w, (name, wide, i)
        assert len(got) == len(hy_case(name)[1]) and ranks // 2 <= loads <= ranks
    return len(KMERIZE_SETS) + len(HYBRID_SETS)


def sample_rows():
    """every '$' row of the index, and the lengths: 1, m, and more than the longest read"""
    reads = index_case()[0]
    return np.arange(len(reads), dtype=np.uint64), (1, M_MIN, max(len(r) for r in reads) + 10)


def run_sample_driver(exe: str, wide: int, rows: np.ndarray, length: int) -> np.ndarray:
    out = _run(exe, wide, "sample", np.array([length], dtype=np.uint32).tobytes() + np.array([rows.size], dtype=np.uint64).tobytes() + rows.tobytes())
    assert len(out) == 4 * rows.size + 16
    return np.frombuffer(out, dtype=np.uint32, count=rows.size)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_field_equals_the_yardstick(hybrid_driver, layout):
    assert HYBRID_DTYPE.itemsize == 96 and READ_DTYPE.itemsize == 24 and PIECE_DTYPE.itemsize == 12
    assert _run_sets(hybrid_driver, LAYOUTS[layout]) >= 19
    reads, c, _, _ = index_case()
    rows, lengths = sample_rows()
    for length in lengths:
        want = [plain_sample_count(c, reads, int(r), length) for r in rows]
        assert run_sample_driver(hybrid_driver, LAYOUTS[layout], rows, length).tolist() == want, length


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: every set, both layouts; workspaces, reads, merged string and pieces are allocations of their own"""
    exe = _build(tmp_path / "fmwalk_hybrid_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    rows, lengths = sample_rows()
    for wide in LAYOUTS.values():
        _run_sets(exe, wide)
        for length in lengths:
            run_sample_driver(exe, wide, rows[::7], length)


def test_the_filters_equal_their_literal_transcription(hybrid_driver):
    """km_max_con against maxCon as written on every string over {A, C} of up to 12 bases; km_low_complexity against the float32
    quotient for every count of A among up to 200 bases, nine tenths exactly among them; and the unit is built without fast-math"""
    strings = ["".join("AC"[(v >> i) & 1] for i in range(n)) for n in range(1, 13) for v in range(1 << n)]
    strings += ["A" * a + ("CGT" * 70)[: n - a] for n in range(1, 201) for a in range(n + 1)]
    bases, off = reads_input(strings)
    out = _run(hybrid_driver, 0, "filters", np.array([len(strings)], dtype=np.uint64).tobytes() + off.tobytes() + _codes(bases))
    got = np.frombuffer(out, dtype=np.uint64, count=2 * len(strings)).reshape(-1, 2)
    assert got[:, 0].tolist() == [literal_max_con(s) for s in strings]
    assert got[:, 1].tolist() == [int(literal_low_complexity(s)) for s in strings]
    longest_run = lambda s: max(len(m.group()) for m in re.finditer(r"A+|C+|G+|T+", s))
    assert all(literal_max_con(s) == longest_run(s) for s in strings[:8190])
    assert sum(1 for s in strings[8190:] if s.count("A") * 10 == len(s) * 9 and not literal_low_complexity(s)) == 20
    make = (REPO / "longreadselfcorrect_amd/csrc/Makefile").read_text()
    assert "fast-math" not in make and "-Ofast" not in make and "unsafe-fp" not in make and "fm_kmerize.hip" in make


# ---- the yardstick against the definition ------------------------------------------------------------------------------------
def test_the_counts_equal_brute_force():
    reads, c, _, _ = index_case()
    brute = lambda w: sum(1 for r in reads for i in range(len(r) - len(w) + 1) if r[i: i + len(w)] == w)
    for seq in (GENOME[400:440], _sub(GENOME[400:440], 20), HAP2[1185:1225]):
        for k in (K, 21):
            for i in range(len(seq) - k + 1):
                w = seq[i: i + k]
                assert c.single(w) == brute(w) and c.single(revcomp(w)) == brute(revcomp(w)) and c.both(w) == brute(w) + brute(revcomp(w))


def test_the_sample_counts_equal_lf_steps_over_the_literal_bwt():
    """extractString and countSequenceOccurrences as BWTAlgorithms has them, over the BWT of the reversed reads with Occ by counting"""
    from .test_fmwalk_host import FmIndex

    reads, c, _, _ = index_case()
    rev = [r[::-1] for r in reads]
    fm = FmIndex(rev)
    from .test_index_locate_host import naive_sa

    codes = naive_sa(rev)[0]
    letters = "$ACGT"
    for row in list(range(0, len(reads), 37)) + [len(reads) - 1]:
        for length in (1, 5, M_MIN, 60):
            out, lo = "", row
            while len(out) < length:
                b = letters[codes[lo]]
                if b == "$":
                    break
                out += b
                lo = fm.update((lo, lo), b)[0]
            s = out[::-1]
            assert s == rev[row][len(rev[row]) - len(s):] and len(s) == min(length, len(reads[row]))
            size = lambda iv: max(iv[1] - iv[0], 0)
            assert size(fm.find(s)) + size(fm.find(revcomp(s))) == plain_sample_count(c, reads, row, length), (row, length)


# ---- the ABI, the kernels ---------------------------------------------------------------------------------------------------
def test_hybrid_entries_are_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    for name in ("lrsc_fmwalk_hybrid", "lrsc_fmwalk_kmerize", "lrsc_kmer_sample_counts"):
        assert name in capi.declared_symbols() and f" T {name}\n" in exported, name
    assert "typedef struct lrsc_fmwalk_piece { uint32_t start, length, kept; } lrsc_fmwalk_piece;" in header
    assert ("typedef struct lrsc_fmwalk_read_result { uint32_t kmerize; int32_t head; uint32_t length, n_pieces; int32_t main_piece; uint32_t whole; } "
            "lrsc_fmwalk_read_result;") in header
    assert "typedef struct lrsc_fmwalk_hybrid_result { lrsc_fmwalk_result walk; lrsc_fmwalk_read_result read[2]; } lrsc_fmwalk_hybrid_result;" in header
    for lines in ("FMIndexWalkProcess.cpp:29-150", "229-267", "555-609", "BWTAlgorithms.cpp:527-539", "454-469", "135-141", "394-415", "418-445", "448-477"):
        assert lines in header, lines
    assert f"#define LRSC_KMER_SAMPLE_MAX_LENGTH {_const('kKmMaxSampleLength')}\n" in header and _const("kKmWalkThreshold") == WALK_X
    assert "#define LRSC_ABI_VERSION 2\n" in header and api.lib.lrsc_abi_version() == 2
    assert capi.FMWALK_HYBRID_DTYPE == HYBRID_DTYPE and capi.FMWALK_READ_DTYPE == READ_DTYPE and capi.FMWALK_PIECE_DTYPE == PIECE_DTYPE
    assert callable(capi.Ctx.fmwalk_hybrid) and callable(capi.Ctx.fmwalk_kmerize) and callable(capi.Ctx.kmer_sample_counts)
    reads = ["ACGTACGTAC", "ACG", "ACGTA"]
    assert capi.piece_slots(reads_input(reads)[1], 5).tolist() == piece_slots(reads, 5).tolist() == [0, 6, 6, 7]


def test_hybrid_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_kmerize"), r"(?:kmerize|hybrid|kmer_sample)_[a-z]+_kernel|kmer_sample_kernel")
    assert {k: len(v) for k, v in seen.items()} == {"kmerize_split_kernel": 2, "hybrid_gate_kernel": 2, "hybrid_walk_kernel": 2, "kmer_sample_kernel": 2}, seen
    waves, threads = _const("kKmWavesPerSimd"), _const("kKmThreads")
    assert waves >= 4 and threads % 64 == 0
    for kernel in seen.values():
        for name, md in kernel:
            lds = md["group_segment_fixed_size"]
            assert md["max_flat_workgroup_size"] == threads
            # 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of LDS per CU for the workgroups of its four SIMDs
            assert md["vgpr_count"] <= 512 // waves // 8 * 8, (name, md)
            assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (name, md)
        assert {re.search(r"ILb([01])E", n).group(1) for n, _ in kernel} == {"0", "1"}
    # the fmwalk unit's own kernels are as they were
    assert set(_kernels(_kernel_notes(tmp_path, "fm_fmwalk"), r"fmwalk_[a-z]+_kernel")) == {"fmwalk_trim_kernel", "fmwalk_walk_kernel"}


# ---- the command line --------------------------------------------------------------------------------------------------------
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"


def test_stride_fmwalk_hybrid_and_kmerize_usage(api, tmp_path):
    from .test_fmwalk_host import FMWALK_USAGE

    run = lambda *args: subprocess.run([str(STRIDE), "fmwalk", *args], cwd=tmp_path, capture_output=True, text=True, input="")
    (tmp_path / "reads.fa").write_text(">r0/1\nACGTACGT\n>r0/2\nACGTACGT\n")
    for args, message in ((["--hybrid", "-a", "merge", "reads.fa"], "FMIndexWalk: -a is not given together with --hybrid"),
                          (["--hybrid", "--algorithm=hybrid", "reads.fa"], "FMIndexWalk: -a is not given together with --hybrid"),
                          (["-a", "kmerize", "--kmerize", "reads.fa"], "FMIndexWalk: -a is not given together with --kmerize"),
                          (["--hybrid", "--kmerize", "reads.fa"], "FMIndexWalk: --hybrid and --kmerize are two algorithms: give one"),
                          (["--hybrid", "--repeat-cutoff=-5", "reads.fa"], "FMIndexWalk: invalid repeat cutoff: -5"),
                          (["--hybrid"], "FMIndexWalk: missing arguments"),
                          (["--kmerize", "-k", "0", "reads.fa"], "FMIndexWalk: invalid kmer length: 0, must be greater than zero"),
                          # the refusals that test_fmwalk_host pins still hold
                          (["-a", "kmerize", "reads.fa"], "FMIndexWalk: -a kmerize is not built here"),
                          (["-a", "hybrid", "reads.fa"], "FMIndexWalk: -a hybrid is not built here"),
                          (["-a", "validate", "reads.fa"], "FMIndexWalk: -a validate is not built here"),
                          (["reads.fa"], "FMIndexWalk: without -a the reference runs its hybrid algorithm, which is not built here")):
        r = run(*args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert message in r.stderr and len([l for l in r.stderr.split("\n") if l.strip()]) == 1, (args, r.stderr)
        assert FMWALK_USAGE in r.stdout, (args, r.stdout, r.stderr)
        assert not list(tmp_path.glob("*.merge.fa")) and not list(tmp_path.glob("*.kmerized.fa")) and not list(tmp_path.glob("*.origin.fa"))
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith(FMWALK_USAGE) and r.stderr == ""
    usage = r.stdout.split("\n")
    assert len([l for l in usage if l.startswith("      --hybrid ")]) == 1 and len([l for l in usage if l.startswith("      --kmerize ")]) == 1
    assert "--repeat-cutoff=N" in r.stdout and "hybrid (default), merge, kmerize, or validate" in r.stdout
    for args in (["help"], []):                                   # the command lists are as they were
        r = subprocess.run([str(STRIDE), *args], cwd=tmp_path, capture_output=True, text=True, input="")
        lines = (r.stdout + r.stderr).split("\n")
        at = [i for i, l in enumerate(lines) if l.startswith("Commands:")]
        assert len(at) == 1 and lines[at[0]] == "Commands: index, merge, sai, grep, filter, correct, pbcorrect, kmerfreq, kmercheck"
        assert lines[at[0] + 1] == "          and fmwalk" and lines[at[0] + 2] == "          and overlap"


def plain_quartile2(counts) -> int:
    """q2 of KmerDistribution::computeKDAttributes (Util/KmerDistribution.cpp:84-106): the last frequency whose range of
    cumulative counts [before, after] holds total * 2 / 4"""
    from collections import Counter

    data = Counter(int(v) for v in counts)
    mid, before, after, q2 = len(counts) * 2 // 4, 0, 0, 0
    for freq in sorted(data):
        before, after = after, after + data[freq]
        if before <= mid <= after:
            q2 = freq
    return q2


def test_the_quartile_restatement():
    assert plain_quartile2([5] * 10) == 5 and plain_quartile2([1, 2, 3, 4]) == 3 and plain_quartile2([1, 1, 2, 2]) == 2 and plain_quartile2([7, 1, 9]) == 7
