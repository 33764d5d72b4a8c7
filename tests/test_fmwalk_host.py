"""The device FM-index walk (csrc/fm_fmwalk.h, fm_fmwalk.hip, capi_fmwalk.cpp) checked without a GPU.

1. The yardstick, plain_fmwalk_merge: FMIndexWalkProcess::MergePairedReads, trimRead and SAIntervalTree::mergeTwoReads restated in
   plain Python over strings, the count of a string taken from a dictionary of the substrings of the index's reads per length.  An
   interval is known by its string and by whether it is valid: "a valid interval within the terminal interval" is "s ends with e
   and that strand's count of s is above 0".  That reduction is held once against the same walk on literal suffix-array intervals
   (interval_walk, over naive_sa).  The named sets, each with an assertion that it holds what it is named for.
2. The per-lane and per-pair code that the kernel calls, compiled for the CPU (tests/host_tools/fmwalk_driver.cpp) and run in the
   kernel's order on images made by build_strand_image: every field equals the yardstick's on every set and on 300 seeded random
   pairs, for both layouts.  The driver again under AddressSanitizer and UBSan, as a stand-alone program.
3. The entry and its structs are declared, exported and bound, the ABI version is still 2; `stride fmwalk` refuses what it does
   not build with the usage text.
4. The kernels compile for gfx950 without scratch, spills or AGPRs, within the registers and the LDS their launch is sized for.

One thing strings cannot say: isTwoReadsOverlap's first case compares the root's interval with the terminal one whether they are
valid or not, and two different strings that both do not occur can end their searches on the same empty interval.  The yardstick
counts the walks in which both are invalid (BOTH_DEAD); interval_walk computes the case literally.
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

FW_DTYPE = np.dtype([("merged", "<u4"), ("length", "<u4"), ("status", "<i4", (2,)), ("max_used_leaves", "<u4", (2,)), ("coverage", "<u8", (2,)),
                     ("trimmed_length", "<u4", (2,))], align=True)
K, M_MIN, X, INSERT = 15, 21, 3, 160                             # -k 15 -m 21 -x 3 -I 160


def _const(name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", (REPO / "longreadselfcorrect_amd/csrc/fm_fmwalk.h").read_text())
    assert m, name
    return int(m.group(1))


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
class Counts:
    """single(w): the occurrences of w among the index's reads; both(w): plus those of its reverse complement"""

    def __init__(self, index_reads: list[str]):
        self.reads = index_reads
        self.longest = max(len(r) for r in index_reads)
        self.tables: dict = {}

    def single(self, w: str) -> int:
        n = len(w)
        if n > self.longest:
            return 0
        if n not in self.tables:
            self.tables[n] = Counter(r[i: i + n] for r in self.reads for i in range(len(r) - n + 1))
        return self.tables[n][w]

    def both(self, w: str) -> int:
        return self.single(w) + self.single(revcomp(w))


BOTH_DEAD: list = []                                             # (q, e) of the walks whose root and terminal intervals are both invalid


def plain_trim(c: Counts, read: str, k: int) -> str:
    """trimRead; the read has k bases or more"""
    def num_next(p: int, end: bool) -> int:
        kmer = read[p: p + k]
        return sum(1 for b in "ATCG" if c.both(kmer[1:] + b if end else b + kmer[:-1]) >= 1)

    head, tail = 0, len(read) - k
    if num_next(head, False) == 0:
        head += 1
        while head <= tail and num_next(head, False) < 2:
            head += 1
    if num_next(tail, True) == 0:
        tail -= 1
        while tail >= head and num_next(tail, True) < 2:
            tail -= 1
    return "" if head > tail else read[head: tail + k]


def plain_overlap(q: str, second: str, m: int, case1: bool):
    """isTwoReadsOverlap, its three cases as written -> the merged string or None"""
    if case1:
        return q + second[m:]
    left = second[:m]
    pos = q.find(left, len(q) - 200 if len(q) >= 200 else 0)
    if pos != -1 and q[pos:] == second[: len(q) - pos]:
        return q[:pos] + second
    pos = second.find(q[:m])
    if pos != -1 and pos <= 50 and second[pos:] == q[: len(second) - pos]:
        return second[pos:]
    return None


def plain_walk(c: Counts, q: str, second: str, m: int, max_overlap: int, insert: int, leaves_max: int, x: int, trace: list | None = None):
    """SAIntervalTree(q, m, max_overlap, insert, leaves_max, indices, second, x).mergeTwoReads -> (code, merged, maxUsedLeaves,
    kmerCoverage).  A leaf is (its string, is fwd valid, is rvc valid); the intervals are those of its last `kmer` bases.  trace
    collects (event, ...) tuples for the tests that ask how a result came about."""
    e, root = second[:m], q[len(q) - m:]
    root_valid, term_valid = c.single(root) > 0, c.single(e) > 0
    if not root_valid and not term_valid:
        BOTH_DEAD.append((q, e))
    merged = plain_overlap(q, second, m, (root_valid or term_valid) and root == e)
    if merged is not None:
        return 1, merged, 0, 0
    leaves = [(q, root_valid, c.single(revcomp(root)) > 0)]
    cur_len, kmer, max_used, results = len(q), m, 0, []

    def extend(kmer):
        new = []
        for t, f, r in leaves:
            s = t[len(t) - kmer:]
            for b in "ACGT":
                fs = c.single(s + b) if f else 0
                rs = c.single(revcomp(s + b)) if r else 0
                if fs + rs >= x:
                    new.append((t + b, fs > 0, rs > 0))
        return new

    def refine(ls):
        return [(t, c.single(t[-m:]) > 0, c.single(revcomp(t[-m:])) > 0) for t, _, _ in ls]

    while leaves and len(leaves) <= leaves_max and cur_len <= insert:
        new = extend(kmer)
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
            if trace is not None:
                trace.append(("refine", cur_len))
        max_used = max(max_used, len(leaves))
        results = [t for t, f, r in leaves if t[len(t) - kmer:].endswith(e) and (f or r)]
        if results:
            break
    if results:
        if trace is not None:
            trace.append(("results", len(results), len(leaves)))
        best, best_cov = "", 0
        for t in results:
            t = t + second[m:]
            cov = sum(c.both(t[i: i + m]) for i in range(0, len(t) - m + 1, m // 2))
            if trace is not None:
                trace.append(("cov", t, cov))
            if cov > best_cov:
                best, best_cov = t, cov
        return 1, best, max_used, best_cov
    code = -1 if not leaves else -2 if cur_len > insert else -3 if len(leaves) > leaves_max else -4
    return code, "", max_used, 0


def plain_fmwalk_merge(c: Counts, r1: str, r2: str, k: int = K, x: int = X, m: int = M_MIN, max_overlap: int = -1, insert: int = INSERT, leaves_max: int = 32,
                       trace: list | None = None, walk=plain_walk) -> dict:
    """MergePairedReads -> the fields of lrsc_fmwalk_result and the merged string"""
    out = dict(merged=0, length=0, seq="", status=[0, 0], max_used_leaves=[0, 0], coverage=[0, 0], trimmed_length=[0, 0])
    if len(r1) < k or len(r2) < k:                               # the reference throws; the trimmed length of a read it can trim is still given
        out["trimmed_length"] = [len(plain_trim(c, r, k)) if len(r) >= k else 0 for r in (r1, r2)]
        return out
    t1, t2 = plain_trim(c, r1, k), plain_trim(c, r2, k)
    out["trimmed_length"] = [len(t1), len(t2)]
    if len(t1) < m or len(t2) < m:
        return out
    a, b = t1[:m], t2[:m]
    mo = max_overlap if max_overlap != -1 else int(((len(r1) + len(r2)) // 2) * 0.9)
    w1 = walk(c, a, revcomp(b), m, mo, insert, leaves_max, x, trace)
    w2 = walk(c, b, revcomp(a), m, mo, insert, leaves_max, x, trace)
    out["status"], out["max_used_leaves"], out["coverage"] = [w1[0], w2[0]], [w1[2], w2[2]], [w1[3], w2[3]]
    s1, s2 = w1[1], w2[1]
    seq = s1 if s1 and not s2 else s2 if s2 and not s1 else (s1 if w1[3] > w2[3] else s2) if s1 and s2 and len(s1) == len(s2) else ""
    if seq:
        out.update(merged=1, length=len(seq), seq=seq)
    return out


# ---- the same walk on literal suffix-array intervals ---------------------------------------------------------------------------
class FmIndex:
    """the BWT of a string set with Occ by counting: findInterval and updateInterval as BWTAlgorithms has them, rows as [lo, hi1)"""

    def __init__(self, reads: list[str]):
        codes = naive_sa(reads)[0]
        self.occ = np.zeros((5, codes.size + 1), dtype=np.int64)
        for b in range(5):
            self.occ[b, 1:] = np.cumsum(codes == b)
        self.pred = np.concatenate([[0], np.cumsum(self.occ[:, -1])])

    def update(self, iv, ch: str):
        b = CODE[ch]
        return int(self.pred[b] + self.occ[b, iv[0]]), int(self.pred[b] + self.occ[b, iv[1]])

    def find(self, w: str):
        b = CODE[w[-1]]
        iv = (int(self.pred[b]), int(self.pred[b + 1]))
        for ch in reversed(w[:-1]):
            iv = self.update(iv, ch)
            if iv[0] >= iv[1]:
                break
        return iv


def interval_walk_over(bwt: FmIndex, rbwt: FmIndex):
    """plain_walk's twin: a leaf is (its string, fwd, rvc), the intervals literal"""
    valid = lambda iv: iv[0] < iv[1]
    size = lambda iv: iv[1] - iv[0] if valid(iv) else 0
    within = lambda iv, t: valid(iv) and iv[0] >= t[0] and iv[1] <= t[1]
    pair_of = lambda s: (rbwt.find(s[::-1]), bwt.find(revcomp(s)))
    comp = str.maketrans("ACGT", "TGCA")

    def walk(c: Counts, q, second, m, max_overlap, insert, leaves_max, x, trace=None):
        root_fwd, root_rvc = pair_of(q[len(q) - m:])
        term_fwd, term_rvc = pair_of(second[:m])
        merged = plain_overlap(q, second, m, root_fwd == term_fwd)
        if merged is not None:
            return 1, merged, 0, 0
        leaves = [(q, root_fwd, root_rvc)]
        cur_len, kmer, max_used, results = len(q), m, 0, []

        def extend():
            new = []
            for t, f, r in leaves:
                for b in "ACGT":
                    fp = rbwt.update(f, b) if valid(f) else f
                    rp = bwt.update(r, b.translate(comp)) if valid(r) else r
                    if size(fp) + size(rp) >= x:
                        new.append((t + b, fp, rp))
            return new

        refine = lambda ls: [(t, *pair_of(t[-m:])) for t, _, _ in ls]
        while leaves and len(leaves) <= leaves_max and cur_len <= insert:
            new = extend()
            if not new:
                leaves, kmer = refine(leaves), m
                new = extend()
            if new:
                kmer += 1
                cur_len += 1
            leaves = new
            if leaves and kmer >= max_overlap:
                leaves, kmer = refine(leaves), m
            max_used = max(max_used, len(leaves))
            results = [t for t, f, r in leaves if within(f, term_fwd) or within(r, term_rvc)]
            if results:
                break
        if results:
            best, best_cov = "", 0
            for t in results:
                t = t + second[m:]
                cov = sum(c.both(t[i: i + m]) for i in range(0, len(t) - m + 1, m // 2))
                if cov > best_cov:
                    best, best_cov = t, cov
            return 1, best, max_used, best_cov
        return (-1 if not leaves else -2 if cur_len > insert else -3 if len(leaves) > leaves_max else -4), "", max_used, 0

    return walk


# ---- the index of the sets: a 1.5 kb genome with a copied stretch, and a second haplotype --------------------------------------
_G0 = _rand(0xF3A1, 1500)
GENOME = _G0[:900] + _G0[300:360] + _G0[960:]                    # [300, 360) stands at [900, 960) too
SNP, SNP2 = 600, 1200                                            # the haplotypes differ here: at SNP both are tiled alike, at SNP2 the second one thinner
_alt = lambda ch, d: "ACGT"[("ACGT".index(ch) + d) % 4]
HAP2 = GENOME[:SNP] + _alt(GENOME[SNP], 1) + GENOME[SNP + 1: SNP2] + _alt(GENOME[SNP2], 1) + GENOME[SNP2 + 1:]


def _tile(g: str, lo: int, hi: int, step: int, off: int = 0) -> list[str]:
    reads = [g[s: s + 50] for s in range(lo + off, hi - 49, step)]
    return [revcomp(r) if i & 1 else r for i, r in enumerate(reads)]


_INDEX: dict = {}


def index_reads() -> list[str]:
    """50-base reads every 3 bases of the genome, alternate reads reverse-complemented; the second haplotype the same way where it
    can differ from the first, every 5 bases around SNP2"""
    return _tile(GENOME, 0, 1500, 3) + _tile(HAP2, 0, 900, 3, 1) + _tile(HAP2, 1050, 1350, 5, 2)


def index_case():
    """(reads of the index, their Counts, BWT codes of .bwt, of .rbwt), computed once"""
    if not _INDEX:
        reads = index_reads()
        _INDEX["v"] = (reads, Counts(reads), naive_sa(reads)[0], naive_sa([r[::-1] for r in reads])[0])
    return _INDEX["v"]


# ---- the sets: pairs and options --------------------------------------------------------------------------------------------------
def ends(g: str, start: int, n: int) -> tuple[str, str]:
    """the 50-base ends of the fragment g[start .. start + n)"""
    f = g[start: start + n]
    return f[:50], revcomp(f)[:50]


def wrong_first(read: str) -> str:
    return _alt(read[0], 2) + read[1:]


def _set(pairs, max_overlap=-1, insert=INSERT, leaves=32):
    return dict(pairs=list(pairs), k=K, x=X, m=M_MIN, max_overlap=max_overlap, insert=insert, leaves=leaves)


def _random_pairs(seed: int, n: int):
    """ends of 70 to 140-base fragments of either haplotype and strand, a quarter with one substituted base"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        size = int(rng.integers(70, 141))
        start = int(rng.integers(0, len(GENOME) - size + 1))
        r1, r2 = ends(HAP2 if rng.integers(2) else GENOME, start, size)
        if rng.integers(2):
            r1, r2 = r2, r1
        if i % 4 == 0:
            at, which = int(rng.integers(50)), int(rng.integers(2))
            r = [r1, r2][which]
            r = r[:at] + _alt(r[at], int(rng.integers(1, 4))) + r[at + 1:]
            r1, r2 = (r, r2) if which == 0 else (r1, r)
        pairs.append((r1, r2))
    return pairs


BUBBLE = [ends(GENOME, 540, 90), ends(HAP2, 540, 90), ends(GENOME, 1140, 90), ends(HAP2, 1140, 90)]
STRETCH = [ends(GENOME, 231, 130), ends(GENOME, 252, 70), ends(GENOME, 301, 70)]
FW_SETS = {
    "unique_path": lambda: _set([ends(GENOME, 100, 130), ends(GENOME, 1407, 70), ends(GENOME, 7, 70), ends(GENOME, 100, 100)]),
    "bubble_l32": lambda: _set(BUBBLE, max_overlap=30),
    "bubble_l1": lambda: _set(BUBBLE, max_overlap=30, leaves=1),
    "stretch_l32": lambda: _set(STRETCH),
    "stretch_l1": lambda: _set(STRETCH, leaves=1),
    "refine_m30": lambda: _set([ends(GENOME, 100, 100), ends(GENOME, 1000, 140)], max_overlap=30),
    "retry_m200": lambda: _set([ends(GENOME, 100, 100), ends(GENOME, 1000, 140)], max_overlap=200),
    "depth_i90": lambda: _set([ends(GENOME, 100, 130), ends(GENOME, 100, 90)], insert=90),
    "trims_to_nothing": lambda: _set([(wrong_first(ends(GENOME, 100, 100)[0]), ends(GENOME, 100, 100)[1]),
                                      (ends(GENOME, 100, 100)[0], wrong_first(ends(GENOME, 100, 100)[1]))]),
    "trims_at_the_site_and_merges": lambda: _set([(wrong_first(ends(GENOME, SNP - j, 100)[0]), ends(GENOME, SNP - j, 100)[1]) for j in (1, 3, 10)], max_overlap=30),
    "trims_below_m": lambda: _set([(wrong_first(ends(GENOME, SNP - 30, 100)[0]), ends(GENOME, SNP - 30, 100)[1])], max_overlap=30),
    "overlap_shortcut": lambda: _set([(GENOME[200:250], revcomp(GENOME[171:221]))]),
    "shorter_than_k": lambda: _set([(GENOME[100:114], ends(GENOME, 100, 100)[1]), (ends(GENOME, 100, 100)[0], "ACGT"), ("A", "C")]),
    "random_default": lambda: _set(_random_pairs(0xF00D, 100)),
    "random_m30": lambda: _set(_random_pairs(0xF00E, 100), max_overlap=30),
    "random_m30_l2": lambda: _set(_random_pairs(0xF00F, 100), max_overlap=30, leaves=2),
}
NAMED = [n for n in FW_SETS if not n.startswith("random")]
_FW: dict = {}


def set_options(s: dict) -> dict:
    return dict(k=s["k"], x=s["x"], m=s["m"], max_overlap=s["max_overlap"], insert=s["insert"], leaves_max=s["leaves"])


def fw_case(name: str):
    """(the set, [plain_fmwalk_merge's dict per pair], [its trace per pair]), computed once per set"""
    if name not in _FW:
        s = FW_SETS[name]()
        c = index_case()[1]
        traces = [[] for _ in s["pairs"]]
        _FW[name] = (s, [plain_fmwalk_merge(c, r1, r2, trace=t, **set_options(s)) for (r1, r2), t in zip(s["pairs"], traces)], traces)
    return _FW[name]


def test_the_sets_hold_what_they_are_named_for():
    c = index_case()[1]
    want = lambda name: fw_case(name)[1]
    events = lambda name, i, kind: [t for t in fw_case(name)[2][i] if t[0] == kind]
    status = lambda name: [tuple(w["status"]) for w in want(name)]
    assert GENOME[300:360] == GENOME[900:960] and sum(a != b for a, b in zip(GENOME, HAP2)) == 2 and GENOME[SNP] != HAP2[SNP] and GENOME[SNP2] != HAP2[SNP2]
    assert all(len(r) == 50 for r in index_case()[0]) and len(GENOME) == 1500
    # a unique path: both walks find, the lengths are equal, the coverage chooses (walk 1's only when it is greater)
    u = want("unique_path")
    assert status("unique_path") == [(1, 1)] * 4 and all(w["merged"] for w in u)
    assert [w["seq"] for w in u[:1]] == [revcomp(GENOME[100:230])] and u[0]["coverage"][0] <= u[0]["coverage"][1]
    assert u[1]["coverage"][0] > u[1]["coverage"][1] and u[1]["seq"] == GENOME[1407:1477]
    assert all(len(events("unique_path", i, "results")) == 2 and {t[1] for t in events("unique_path", i, "results")} == {1} for i in range(4))
    # the bubble: two results in one step.  At SNP they tie and the first in base order is taken; at SNP2 walk 2 takes its second
    b = want("bubble_l32")
    assert status("bubble_l32") == [(1, 1)] * 4 and all([t[1] for t in events("bubble_l32", i, "results")] == [2, 2] for i in range(4))
    covs = [[t[2] for t in events("bubble_l32", i, "cov")] for i in range(4)]
    assert all(cv[0] == cv[1] and cv[2] == cv[3] for cv in covs[:2]) and all(cv[0] > cv[1] and cv[2] < cv[3] for cv in covs[2:])
    strings = [[t[1] for t in events("bubble_l32", i, "cov")] for i in range(4)]
    assert all(st[0] < st[1] and st[2] < st[3] for st in strings), "a step's results stand in base order"
    # a walk's string: its first result on the tie, else the one with the greater coverage, which in walk 2 at SNP2 is the second
    bests = [(st[0], st[2]) for st in strings[:2]] + [(st[0], st[3]) for st in strings[2:]]
    assert [w["seq"] for w in b] == [w1 if w["coverage"][0] > w["coverage"][1] else w2 for w, (w1, w2) in zip(b, bests)]
    assert [w["coverage"] for w in b] == [[max(cv[:2]), max(cv[2:])] for cv in covs]
    assert all(revcomp(w["seq"]) == GENOME[1140:1230] for w in b[2:]), "the thicker haplotype wins by coverage, whichever pair asked"
    assert status("bubble_l1") == [(-3, -3)] * 4 and not any(w["merged"] for w in want("bubble_l1"))
    # the copied stretch: with one leaf only one of the walks finds; a result in a frontier above -L is still taken
    assert status("stretch_l32") == [(1, 1)] * 3
    assert status("stretch_l1") == [(1, -3), (1, -3), (-3, 1)] and all(w["merged"] for w in want("stretch_l1"))
    assert want("stretch_l1")[0]["max_used_leaves"][0] > 1 and want("stretch_l1")[0]["seq"] == GENOME[231:361]
    assert want("stretch_l1")[2]["seq"] == revcomp(GENOME[301:371])
    # -M 30: a refinement every nine steps; -M 200: the k-mer outgrows the reads, the frontier empties, the retry saves it
    assert status("refine_m30") == [(1, 1)] * 2 and [t[1] for t in events("refine_m30", 0, "refine")][:3] == [30, 39, 48]
    assert status("retry_m200") == [(1, 1)] * 2 and not events("retry_m200", 0, "refine")
    assert len(events("retry_m200", 1, "retry")) >= 4 and all(t[2] >= 1 for t in events("retry_m200", 1, "retry"))
    assert status("depth_i90") == [(-2, -2), (1, 1)] and [w["merged"] for w in want("depth_i90")] == [0, 1]
    # the trims
    assert [w["trimmed_length"] for w in want("trims_to_nothing")] == [[0, 50], [50, 0]] and status("trims_to_nothing") == [(0, 0)] * 2
    t = want("trims_at_the_site_and_merges")
    assert [w["trimmed_length"] for w in t] == [[48, 50], [46, 50], [39, 50]] and all(w["merged"] for w in t)
    assert [w["length"] for w in t] == [98, 96, 89]
    assert [w["trimmed_length"] for w in want("trims_below_m")] == [[19, 50]] and K <= 19 < M_MIN and status("trims_below_m") == [(0, 0)]
    o = want("overlap_shortcut")[0]
    a = GENOME[200:221]
    assert fw_case("overlap_shortcut")[0]["pairs"][0][1][:M_MIN] == revcomp(a)
    assert (o["merged"], o["seq"], o["status"], o["coverage"], o["max_used_leaves"]) == (1, revcomp(a), [1, 1], [0, 0], [0, 0])
    s = want("shorter_than_k")
    assert [w["trimmed_length"] for w in s] == [[0, 50], [50, 0], [0, 0]] and not any(w["merged"] for w in s) and status("shorter_than_k") == [(0, 0)] * 3
    # the random pairs: most merge, some do not, and a quarter carry a substitution
    merged = [w["merged"] for n in FW_SETS if n.startswith("random") for w in want(n)]
    assert len(merged) == 300 and 150 < sum(merged) < 300
    assert c.both(GENOME[700:721]) >= 2 * X
    assert not BOTH_DEAD, "no walk of the sets starts with both the root's and the terminal interval invalid"


def test_the_string_yardstick_equals_the_walk_on_literal_intervals():
    """the reduction "within the terminal interval" == "ends with e, and occurs" on every named set and a hundred random pairs"""
    reads, c, _, _ = index_case()
    walk = interval_walk_over(FmIndex(reads), FmIndex([r[::-1] for r in reads]))
    n = 0
    for name in NAMED + ["random_m30_l2"]:
        s, want, _ = fw_case(name)
        for (r1, r2), w in zip(s["pairs"], want):
            assert plain_fmwalk_merge(c, r1, r2, walk=walk, **set_options(s)) == w, (name, r1, r2)
            n += 1
    assert n > 130


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _build(exe: Path, *flags: str) -> str:
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/fmwalk_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def fmwalk_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fmwalk_driver") / "fmwalk_driver")


def pairs_input(pairs) -> tuple[np.ndarray, np.ndarray]:
    """(the ASCII bases of the pairs' reads back to back, their 2 n + 1 offsets)"""
    reads = [r for p in pairs for r in p]
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8), off


def result_dicts(res: np.ndarray, rows) -> list[dict]:
    """FW_DTYPE records and the merged rows (ASCII or codes as text) -> what plain_fmwalk_merge returns"""
    return [dict(merged=int(q["merged"]), length=int(q["length"]), seq=row[: int(q["length"])] if q["merged"] else "", status=q["status"].tolist(),
                 max_used_leaves=q["max_used_leaves"].tolist(), coverage=q["coverage"].tolist(), trimmed_length=q["trimmed_length"].tolist())
            for q, row in zip(res, rows)]


def run_fmwalk_driver(exe: str, name: str, wide: int):
    """-> [dict per pair], Occ queries, block loads"""
    s = fw_case(name)[0]
    _, _, bwt, rbwt = index_case()
    bases, off = pairs_input(s["pairs"])
    n = len(s["pairs"])
    blob = b"".join([_image_input(bwt), _image_input(rbwt),
                     np.array([s["k"], s["x"], s["m"], s["max_overlap"], s["insert"], s["leaves"]], dtype=np.int32).tobytes(),
                     np.array([n], dtype=np.uint64).tobytes(), off.tobytes(), bytes(CODE[chr(c)] - 1 for c in bases)])
    r = subprocess.run([exe, str(wide)], input=blob, capture_output=True)
    assert r.returncode == 0, (name, wide, r.returncode, r.stderr[-2000:])
    stride = max(s["insert"] + 1, s["m"])
    res = np.frombuffer(r.stdout, dtype=FW_DTYPE, count=n)
    p = n * FW_DTYPE.itemsize
    rows = np.frombuffer(r.stdout, dtype=np.uint8, count=n * stride, offset=p).reshape(n, stride)
    ranks, loads = np.frombuffer(r.stdout, dtype=np.uint64, count=2, offset=p + n * stride)
    assert p + n * stride + 16 == len(r.stdout)
    for q, row in zip(res, rows):                                 # nothing is written beyond the merged string
        assert (row[int(q["length"]) if q["merged"] else 0:] == 0xFF).all()
    text = ["".join("ACGT"[c & 3] for c in row) for row in rows]
    return result_dicts(res, text), int(ranks), int(loads)


def _run_sets(exe: str, wide: int, names) -> int:
    for name in names:
        got, ranks, loads = run_fmwalk_driver(exe, name, wide)
        want = fw_case(name)[1]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, wide, i)
        assert len(got) == len(want) and ranks // 2 <= loads <= ranks
    return len(names)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_field_equals_the_yardstick(fmwalk_driver, layout):
    assert FW_DTYPE.itemsize == 48
    assert _run_sets(fmwalk_driver, LAYOUTS[layout], list(FW_SETS)) == len(NAMED) + 3 >= 16


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: the named sets, both layouts; workspace, reads and merged string are allocations of their own"""
    exe = _build(tmp_path / "fmwalk_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        _run_sets(exe, wide, NAMED)


# ---- the ABI, the command line, the kernels -----------------------------------------------------------------------------------
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
FMWALK_USAGE = "Usage: StriDe FMIndexWalk [OPTION] ... READSFILE"


def test_fmwalk_entry_is_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    assert "lrsc_fmwalk_merge" in capi.declared_symbols() and " T lrsc_fmwalk_merge\n" in exported
    assert ("typedef struct lrsc_fmwalk_params { int32_t kmer_length, kmer_threshold, min_overlap, max_overlap /* -1: from the lengths */, max_insert, max_leaves; } "
            "lrsc_fmwalk_params;") in header
    assert ("typedef struct lrsc_fmwalk_result { uint32_t merged, length; int32_t status[2]; uint32_t max_used_leaves[2]; uint64_t coverage[2]; "
            "uint32_t trimmed_length[2]; } lrsc_fmwalk_result;") in header
    assert re.search(r"int lrsc_fmwalk_merge\(lrsc_ctx\* ctx, const char\* reads, const uint64_t\* read_off, uint32_t n_pairs", header)
    assert "FMIndexWalkProcess.cpp:153-226" in header and "SAIntervalTree.cpp" in header
    limits = {n: int(v) for n, v in re.findall(r"#define LRSC_FMWALK_MAX_(\w+) (\d+)", header)}
    assert limits == {"LEAVES": _const("kFwMaxLeaves"), "INSERT": _const("kFwMaxInsert"), "MIN_OVERLAP": _const("kFwMaxOverlap"), "KMER": _const("kFwMaxKmer")}
    assert limits["LEAVES"] >= 64 and limits["INSERT"] >= 2000 and limits["MIN_OVERLAP"] >= 255 and limits["KMER"] >= 255
    assert "#define LRSC_ABI_VERSION 2\n" in header and api.lib.lrsc_abi_version() == 2
    assert capi.FMWALK_DTYPE == FW_DTYPE and capi.FMWALK_DTYPE.itemsize == 48
    assert callable(capi.Ctx.fmwalk_merge)


def test_stride_fmwalk_usage(api, tmp_path):
    run = lambda *args: subprocess.run([str(STRIDE), "fmwalk", *args], cwd=tmp_path, capture_output=True, text=True, input="")
    (tmp_path / "reads.fa").write_text(">r0/1\nACGTACGT\n>r0/2\nACGTACGT\n")
    merge = ["-a", "merge"]
    for args, message in ((["-a", "kmerize", "reads.fa"], "FMIndexWalk: -a kmerize is not built here"),
                          (["-a", "validate", "reads.fa"], "FMIndexWalk: -a validate is not built here"),
                          (["--algorithm=hybrid", "reads.fa"], "FMIndexWalk: -a hybrid is not built here"),
                          (["reads.fa"], "FMIndexWalk: without -a the reference runs its hybrid algorithm, which is not built here"),
                          (["-a", "best", "reads.fa"], "FMIndexWalk: unrecognized -a,--algorithm parameter: best"),
                          (merge, "FMIndexWalk: missing arguments"),
                          (merge + ["reads.fa", "more.fa"], "FMIndexWalk: too many arguments"),
                          (merge + ["-k", "0", "reads.fa"], "FMIndexWalk: invalid kmer length: 0, must be greater than zero"),
                          (merge + ["-x", "-2", "reads.fa"], "FMIndexWalk: invalid kmer threshold: -2, must be greater than zero"),
                          (merge + ["-t", "0", "reads.fa"], "FMIndexWalk: invalid number of threads: 0"),
                          (merge + ["--frobnicate", "reads.fa"], "fmwalk: unrecognized option '--frobnicate'")):       # getopt's own line
        r = run(*args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert message in r.stderr and len([l for l in r.stderr.split("\n") if l.strip()]) == 1, (args, r.stderr)
        assert FMWALK_USAGE in r.stdout, (args, r.stdout, r.stderr)
        for option in ("--max-leaves=N", "--max-insertsize=N", "--min-overlap=N", "--max-overlap=N", "--device=N", "--build-index", "--load-on-device",
                       "hybrid (default), merge, kmerize, or validate"):
            assert option in r.stdout, (args, option)
        assert not list(tmp_path.glob("*.merge.fa"))
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith(FMWALK_USAGE) and r.stderr == ""
    # The two command lists.  test_kmer_correct_host pins the line that starts with `Commands:` word for word, so fmwalk stands
    # on the list's next line and that line stays as it was.
    for args in (["help"], []):
        r = subprocess.run([str(STRIDE), *args], cwd=tmp_path, capture_output=True, text=True, input="")
        lines = (r.stdout + r.stderr).split("\n")
        at = [i for i, l in enumerate(lines) if l.startswith("Commands:")]
        assert len(at) == 1 and " correct," in lines[at[0]] and lines[at[0] + 1] == "          and fmwalk", (args, r.stdout, r.stderr)


def test_fmwalk_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_fmwalk"), r"fmwalk_[a-z]+_kernel")
    assert {k: len(v) for k, v in seen.items()} == {"fmwalk_trim_kernel": 2, "fmwalk_walk_kernel": 2}, seen
    waves, threads = _const("kFwWavesPerSimd"), _const("kFwThreads")
    assert waves >= 4 and threads % 64 == 0
    for kernel in seen.values():
        for name, md in kernel:
            lds = md["group_segment_fixed_size"]
            assert md["max_flat_workgroup_size"] == threads
            # 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of LDS per CU for the workgroups of its four SIMDs
            assert md["vgpr_count"] <= 512 // waves // 8 * 8, (name, md)
            assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (name, md)
        assert {re.search(r"ILb([01])E", n).group(1) for n, _ in kernel} == {"0", "1"}
