"""The device overlap (csrc/fm_overlap.h, fm_overlap.hip, capi_overlap.cpp) checked without a GPU.

1. The yardstick, plain_overlap_exact: `stride overlap` in its exact, irreducible-only mode, the reference's code paths restated
   line by line over literal suffix-array intervals (inclusive [lower, upper], as BWTInterval holds them), the lists as Python
   lists, the sorts stable:
     OverlapAlgorithm::overlapReadExact, findOverlapBlocksExact, TrimOBLInterval, computeIrreducibleBlocks,
     _processIrreducibleBlocksExactIterative, updateOverlapBlockRangesRight   (Algorithm/OverlapAlgorithm.cpp)
     removeSubMaximalBlocks, resolveOverlap, removeContainmentBlocks, OverlapBlock::toOverlap   (Algorithm/OverlapBlock.cpp)
     OverlapProcess::process   (Concurrency/OverlapProcess.cpp);  HeaderRecord / VertexRecord / EdgeRecord ::write   (SQG/ASQG.cpp)
2. The same edges by definition, on the sets without substring reads and without a trim: every exact suffix-prefix overlap of
   min_overlap bases or more between two reads in either orientation by brute force, the transitive ones taken out.
3. The named sets, each with an assertion that it holds what it is named for.
4. The per-chain and per-read code that the kernels call, compiled for the CPU (tests/host_tools/overlap_driver.cpp) and run in
   the kernels' order on images made by build_strand_image: every field equals the yardstick's on every set, for both layouts.
   The driver again under AddressSanitizer and UBSan, as a stand-alone program.
5. The entry and its structs are declared, exported and bound, the ABI version is still 2; `stride overlap` refuses what it does
   not build with the usage text, and both command lists name it on a third line.
6. The kernels compile for gfx950 without scratch, spills or AGPRs, within the registers and the LDS their launch is sized for.

OverlapProcess::process returns on a substring read before it clears its block list, so with the reference the blocks of such a
read are written with the next read as their query.  Here a substring read writes no edges and leaves none behind.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_fmwalk_host import GENOME, HAP2, SNP
from .test_index_filter_host import LAYOUTS, _image_input, _kernel_notes, _kernels, _rand, revcomp
from .test_index_locate_host import naive_sa
from .test_index_merge_host import CODE

OVERLAP_READ_DTYPE = np.dtype([("is_substring", "<u4"), ("n_blocks", "<u4"), ("status", "<u4"), ("pad", "<u4"), ("first_block", "<u8")])
OVERLAP_BLOCK_DTYPE = np.dtype([("lower", "<i8"), ("upper", "<i8"), ("overlap_len", "<u4"), ("target_rev", "u1"), ("query_rev", "u1"), ("query_comp", "u1"),
                                ("contained", "u1")])
M = 20


def _const(name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", (REPO / "longreadselfcorrect_amd/csrc/fm_overlap.h").read_text())
    assert m, name
    return int(m.group(1))


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
RANK = {"$": 0, "A": 1, "C": 2, "G": 3, "T": 4}                  # RANK_ALPHABET
COMP = str.maketrans("ACGT", "TGCA")
# AlignFlags(queryRev, targetRev, queryComp)
SUF_PRE, PRE_PRE, SUF_SUF, PRE_SUF = (0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)


class Bwt:
    """one strand: getFullOcc, getPC"""

    def __init__(self, reads: list[str]):
        codes, sa = naive_sa(reads)
        self.occ = np.zeros((5, codes.size + 1), dtype=np.int64)
        for b in range(5):
            self.occ[b, 1:] = np.cumsum(codes == b)
        self.pred = [0] + [int(v) for v in np.cumsum(self.occ[:, -1])]
        self.order = [int(r) for r in sa["read"][sa["pos"] == 0]]    # the .sai: row of the '$' interval -> read

    def full(self, i: int) -> list[int]:
        return [int(v) for v in self.occ[:, i + 1]]


class Index:
    def __init__(self, reads: list[str]):
        self.bwt, self.rbwt = Bwt(reads), Bwt([r[::-1] for r in reads])


class Block:
    def __init__(self, ranges, overlap_len, flags):
        self.r = list(ranges)                                    # interval[0].lower, .upper, interval[1].lower, .upper
        self.len = overlap_len
        self.flags = flags

    def copy(self):
        return Block(self.r, self.len, self.flags)

    def key(self):
        return (self.r[0], self.r[1], self.len, *self.flags)


def init_pair(b: str, bwt: Bwt, rbwt: Bwt):
    out = []
    for s in (bwt, rbwt):
        lo = s.pred[RANK[b]]
        out += [lo, lo + s.full(int(s.occ.shape[1]) - 2)[RANK[b]] - 1]
    return out


def update_both_l(p, b: str, bwt: Bwt):
    l, u, k = bwt.full(p[0] - 1), bwt.full(p[1]), RANK[b]
    diff = [x - y for x, y in zip(u, l)]
    p[2] = p[2] + sum(diff[:k])
    p[3] = p[2] + diff[k] - 1
    p[0] = bwt.pred[k] + l[k]
    p[1] = bwt.pred[k] + u[k] - 1


def update_both_r(p, b: str, rbwt: Bwt):
    l, u, k = rbwt.full(p[2] - 1), rbwt.full(p[3]), RANK[b]
    diff = [x - y for x, y in zip(u, l)]
    p[0] = p[0] + sum(diff[:k])
    p[1] = p[0] + diff[k] - 1
    p[2] = rbwt.pred[k] + l[k]
    p[3] = rbwt.pred[k] + u[k] - 1


def ext_count(lower: int, upper: int, s: Bwt) -> list[int]:
    return [x - y for x, y in zip(s.full(upper), s.full(lower - 1))]


def pair_valid(p) -> bool:
    return p[0] <= p[1] and p[2] <= p[3]


def find_overlap_blocks_exact(w: str, bwt: Bwt, rbwt: Bwt, af, m: int, overlap_list: list, contain_list: list, result: dict):
    n = len(w)
    start = n - 1
    ranges = init_pair(w[start], bwt, rbwt)
    for i in range(start - 1, 0, -1):
        update_both_l(ranges, w[i], bwt)
        overlap_len = n - i
        if overlap_len >= m:
            probe = list(ranges)
            update_both_l(probe, "$", bwt)
            if probe[2] <= probe[3]:
                overlap_list.append(Block(probe, overlap_len, af))
    update_both_l(ranges, w[0], bwt)
    left, right = ext_count(ranges[0], ranges[1], bwt), ext_count(ranges[2], ranges[3], rbwt)
    if any(left[1:]) or any(right[1:]):
        result["is_substring"] = 1
    else:
        probe = list(ranges)
        update_both_l(probe, "$", bwt)
        if pair_valid(probe):
            update_both_r(probe, "$", rbwt)
            contain_list.append(Block(probe, n, af))


def trim_obl_interval(lst: list, read_length: int, trace: list):
    if not lst:                                                  # the reference decrements end() of an empty list; nothing to trim
        return
    lst.sort(key=lambda b: -b.len)
    interval = 0
    k = len(lst) - 1
    longest = lst[k].len
    while k != 0:
        interval += lst[k].r[3] - lst[k].r[2] + 1
        if interval >= 128 or (longest - lst[k].len >= read_length * 0.5):
            trace.append(("trim", [b.len for b in lst[: k + 1]], [b.len for b in lst[k + 1:]]))
            del lst[: k + 1]
            break
        k -= 1


def resolve_overlap(a: Block, b: Block) -> list:
    better, worse = (a, b) if a.len > b.len else (b, a)          # numDiff is 0 on both
    out = [better.copy()]
    dup = min(better.r[1], worse.r[1]) - max(better.r[0], worse.r[0]) + 1
    if better.r[1] - better.r[0] + 1 != dup:
        if better.r[0] < worse.r[0]:
            worse.r[0] += dup
        else:
            worse.r[1] -= dup
        if worse.r[0] <= worse.r[1]:
            out.append(worse.copy())
    out.sort(key=lambda x: x.r[0])
    return out


def remove_submaximal_blocks(lst: list, trace: list):
    lst.sort(key=lambda x: x.r[0])
    i = 0
    while i < len(lst):
        if i + 1 == len(lst):
            break
        a, b = lst[i], lst[i + 1]
        if not (b.r[0] > a.r[1] or a.r[0] > b.r[1]):
            resolved = resolve_overlap(a, b)
            trace.append(("submaximal", a.len, b.len, len(resolved)))
            del lst[i: i + 2]
            for x in resolved:                                   # list::merge: an element of the list stands before an equal one merged in
                at = 0
                while at < len(lst) and lst[at].r[0] <= x.r[0]:
                    at += 1
                lst.insert(at, x)
            i = 0
        else:
            i += 1


def canonical_ext_count(b: Block, bwt: Bwt, rbwt: Bwt) -> list[int]:
    out = ext_count(b.r[2], b.r[3], bwt if b.flags[1] else rbwt)
    if b.flags[2]:
        out = [out[0], out[4], out[3], out[2], out[1]]
    return out


def update_ranges_right(bwt: Bwt, rbwt: Bwt, lst: list, base: str):
    kept = []
    for b in lst:
        update_both_r(b.r, base.translate(COMP) if b.flags[2] else base, bwt if b.flags[1] else rbwt)
        if pair_valid(b.r):
            kept.append(b)
    lst[:] = kept


def compute_irreducible_blocks(bwt: Bwt, rbwt: Bwt, in_list: list, final: list, trace: list):
    in_list.sort(key=lambda b: -b.len)
    if not in_list:
        return
    groups = [[b.copy() for b in in_list]]
    while groups:
        incoming = []
        g = 0
        while g < len(groups):
            cur = groups[g]
            erase = False
            top = cur[0].len
            ext = [0] * 5
            at = 0
            while at < len(cur) and cur[at].len == top:
                ext = [x + y for x, y in zip(ext, canonical_ext_count(cur[at], bwt, rbwt))]
                at += 1
            extend = True
            if ext[0] > 0:
                extend = False
                t = 0
                while t < len(cur) and cur[t].len == top:
                    if canonical_ext_count(cur[t], bwt, rbwt)[0] == 0:
                        trace.append(("pop", t))
                        for _ in range(t):
                            final.pop()
                        extend = True                            # goto SARightExtension
                        break
                    branched = cur[t].copy()
                    update_both_r(branched.r, "$", bwt if branched.flags[1] else rbwt)
                    final.append(branched)
                    t += 1
                if not extend:
                    trace.append(("tlb", t))
                    erase = True
            if extend:
                while at < len(cur):
                    ext = [x + y for x, y in zip(ext, canonical_ext_count(cur[at], bwt, rbwt))]
                    at += 1
                if sum(1 for v in ext[1:] if v > 0) == 1:
                    update_ranges_right(bwt, rbwt, cur, "$ACGT"[[i for i in range(1, 5) if ext[i] > 0][0]])
                else:
                    bases = [b for b in "ACGT" if ext[RANK[b]] > 0]
                    trace.append(("split", len(bases)))
                    for b in bases:
                        branched = [x.copy() for x in cur]
                        update_ranges_right(bwt, rbwt, branched, b)
                        incoming.append(branched)
                        erase = True
            if erase:
                del groups[g]
            else:
                g += 1
        groups += incoming


def plain_overlap_exact(ix: Index, seq: str, m: int, trace: list | None = None) -> dict:
    """overlapRead -> is_substring and the final blocks, in the order of the output list"""
    trace = [] if trace is None else trace
    result = dict(is_substring=0, blocks=[])
    if len(seq) < m:
        return result
    bwt, rbwt = ix.bwt, ix.rbwt
    fwd_contain, rev_contain, suffix_fwd, suffix_rev, prefix_fwd, prefix_rev = [], [], [], [], [], []
    find_overlap_blocks_exact(seq, bwt, rbwt, SUF_PRE, m, suffix_fwd, fwd_contain, result)
    find_overlap_blocks_exact(seq.translate(COMP), rbwt, bwt, PRE_PRE, m, suffix_rev, rev_contain, result)
    find_overlap_blocks_exact(seq[::-1].translate(COMP), bwt, rbwt, SUF_SUF, m, prefix_fwd, fwd_contain, result)
    find_overlap_blocks_exact(seq[::-1], rbwt, bwt, PRE_SUF, m, prefix_rev, rev_contain, result)
    for lst in (suffix_fwd, suffix_rev, prefix_fwd, prefix_rev):
        trim_obl_interval(lst, len(seq), trace)
    suffix_fwd += [b.copy() for b in fwd_contain]
    prefix_fwd += [b.copy() for b in fwd_contain]
    suffix_rev += [b.copy() for b in rev_contain]
    prefix_rev += [b.copy() for b in rev_contain]
    for lst in (suffix_fwd, prefix_fwd, suffix_rev, prefix_rev):
        remove_submaximal_blocks(lst, trace)
    for lst in (suffix_fwd, prefix_fwd, suffix_rev, prefix_rev):
        lst[:] = [b for b in lst if b.len != len(seq)]
    suffix_fwd += suffix_rev
    prefix_fwd += prefix_rev
    final = fwd_contain + rev_contain
    compute_irreducible_blocks(bwt, rbwt, suffix_fwd, final, trace)
    compute_irreducible_blocks(bwt, rbwt, prefix_fwd, final, trace)
    result["blocks"] = [dict(lower=b.r[0], upper=b.r[1], overlap_len=b.len, target_rev=b.flags[1], query_rev=b.flags[0], query_comp=b.flags[2],
                             contained=int(b.len == len(seq))) for b in final]
    return result


def edge_lines(ix: Index, names: list[str], reads: list[str], q: int, res: dict) -> list[str]:
    """OverlapProcess::process of read q -> its ED lines"""
    out = []
    if res["is_substring"]:
        return out
    for b in res["blocks"]:
        for j in range(b["lower"], b["upper"] + 1):
            t = (ix.rbwt if b["target_rev"] else ix.bwt).order[j]
            if names[q] == names[t]:
                continue
            qn, tn, ol = len(reads[q]), len(reads[t]), b["overlap_len"]
            c1, c2 = [qn - ol, qn - 1], [0, ol - 1]
            if b["query_rev"]:
                c1 = [qn - c1[1] - 1, qn - c1[0] - 1]
            if b["target_rev"]:
                c2 = [tn - c2[1] - 1, tn - c2[0] - 1]
            contained = (c1[0] == 0 and c1[1] + 1 == qn) or (c2[0] == 0 and c2[1] + 1 == tn)
            if contained and b["query_rev"]:
                continue
            if names[q] < names[t]:
                continue
            out.append(f"ED\t{names[q]} {names[t]} {c1[0]} {c1[1]} {qn} {c2[0]} {c2[1]} {tn} {int(b['target_rev'] != b['query_rev'])} 0\n")
    return out


def plain_overlap_text(names: list[str], reads: list[str], m: int, in_file: str, results: list[dict], ix: Index) -> tuple[str, str]:
    """(the .asqg text, the -thread0.edges text) of `stride overlap -m m in_file`"""
    asqg = f"HT\tVN:i:1\tER:f:-1\tOL:i:{m}\tIN:Z:{in_file}\tCN:i:1\tTE:i:0\n"
    asqg += "".join(f"VT\t{n}\t{r}\tSS:i:{res['is_substring']}\n" for n, r, res in zip(names, reads, results))
    edges = "".join(line for q, res in enumerate(results) for line in edge_lines(ix, names, reads, q, res))
    return asqg, edges


# ---- the edges by definition ---------------------------------------------------------------------------------------------------
def brute_edge_lines(names: list[str], reads: list[str], m: int) -> set:
    """The ED lines of a set in which no read is a substring of another.  For a query x and one of its ends (the right end of x, or
    of its reverse complement for the left one) every other read z in either orientation overlaps with the longest L, m <= L <
    len(x), for which the last L bases of x are the first L of z; z's bases behind them are its extension.  x -> z is transitive
    when some x -> y at the same end has a longer overlap and its extension is a prefix of z's.  (Only the longest overlap of a
    pair at an end counts: removeSubMaximalBlocks takes a read out of the blocks of its shorter overlaps.  With a substring read
    the definition would need more: a read that ends first is dropped although no longer overlap's extension is a prefix of
    its own.)  Identical and reverse-complement identical reads are containments, written from the forward query.  A line is
    written from the query whose name is not below the target's."""
    lines = set()
    for q, x in enumerate(reads):
        n = len(x)
        if n < m:
            continue
        for end in (0, 1):
            xo = x if end == 0 else revcomp(x)
            found = []
            for t, z in enumerate(reads):
                if names[t] == names[q]:
                    continue
                for o in (0, 1):
                    zo = z if o == 0 else revcomp(z)
                    if end == 0 and zo == xo and names[q] >= names[t]:
                        lines.add(f"ED\t{names[q]} {names[t]} 0 {n - 1} {n} 0 {n - 1} {n} {o} 0\n")
                    for L in range(min(n - 1, len(zo)), m - 1, -1):
                        if xo[n - L:] == zo[:L]:
                            found.append((L, zo[L:], t, o))
                            break
            for L, ext, t, o in found:
                if any(L2 > L and ext.startswith(e2) for L2, e2, _, _ in found) or names[q] < names[t]:
                    continue
                tn = len(reads[t])
                c1 = (n - L, n - 1) if end == 0 else (0, L - 1)
                c2 = (0, L - 1) if o == 0 else (tn - L, tn - 1)
                lines.add(f"ED\t{names[q]} {names[t]} {c1[0]} {c1[1]} {n} {c2[0]} {c2[1]} {tn} {int(o != end)} 0\n")
    return lines


# ---- the sets ----------------------------------------------------------------------------------------------------------------
PATH = [GENOME[s: s + 50] for s in range(0, 260, 10)]            # 26 reads, each overlaps the next three by 40, 30 and 20
ALTERNATE = [revcomp(r) if i & 1 else r for i, r in enumerate(PATH)]
_UNIT = "ACGTT"
_Q_TRIM = _rand(0x0E11, 50)
_Q_SUB = _rand(0x0E12, 20) + _UNIT * 6


def _random_reads(seed: int, n: int) -> list[str]:
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = int(rng.integers(0, len(GENOME) - 49))
        r = (HAP2 if rng.integers(2) else GENOME)[s: s + 50]
        out.append(revcomp(r) if rng.integers(2) else r)
    return out


OV_SETS = {
    "unique_path": lambda: (PATH, M),
    "branch_at_the_snp": lambda: ([GENOME[s: s + 50] for s in range(500, 660, 10)] + [HAP2[s: s + 50] for s in range(560, 610, 10)], M),
    "both_strands": lambda: (ALTERNATE + [PATH[1]], M),
    "identical_reads": lambda: (PATH + [PATH[5]], M),
    "revcomp_identical_reads": lambda: (PATH + [revcomp(PATH[5])], M),
    "substring_read": lambda: (PATH + [GENOME[105:135]], M),
    "sa_right_extension_pop": lambda: ([GENOME[0:50], GENOME[10:60], revcomp(GENOME[10:65])] + [GENOME[s: s + 50] for s in range(20, 100, 10)], M),
    "trim": lambda: ([_Q_TRIM] + [_Q_TRIM[50 - L:] + _rand(0x7000 + 16 * L + i, 50 - L) for L in range(12, 31, 2) for i in range(16)], 10),
    "submaximal": lambda: (PATH + [_Q_SUB, _UNIT * 5 + _rand(0x0E13, 25)], M),
    "shorter_than_m": lambda: (PATH + ["ACGTTGCAAGGCTTA"], M),
    "m_equal_to_the_read_length": lambda: (PATH + [PATH[5]], 50),
    "random": lambda: (_random_reads(0x0E14, 200), M),
}
BY_DEFINITION = ["unique_path", "branch_at_the_snp", "both_strands", "identical_reads", "revcomp_identical_reads", "submaximal", "shorter_than_m",
                 "m_equal_to_the_read_length", "random"]
NAMED = [n for n in OV_SETS if n != "random"]
_OV: dict = {}


def ov_case(name: str) -> dict:
    """the set with its yardstick, computed once: names, reads, m, ix, results (plain_overlap_exact per read), traces, asqg, edges"""
    if name not in _OV:
        reads, m = OV_SETS[name]()
        names = [f"read{i}" for i in range(len(reads))]          # "read10" < "read9": the canonical filter compares strings
        ix = Index(reads)
        traces = [[] for _ in reads]
        results = [plain_overlap_exact(ix, r, m, t) for r, t in zip(reads, traces)]
        asqg, edges = plain_overlap_text(names, reads, m, f"{name}.fa", results, ix)
        _OV[name] = dict(names=names, reads=reads, m=m, ix=ix, results=results, traces=traces, asqg=asqg, edges=edges)
    return _OV[name]


def _events(name: str, read: int, kind: str) -> list:
    return [t for t in ov_case(name)["traces"][read] if t[0] == kind]


def _final(name: str, read: int) -> list:
    return [(b["overlap_len"], b["upper"] - b["lower"] + 1, b["target_rev"], b["query_rev"], b["contained"]) for b in ov_case(name)["results"][read]["blocks"]]


def test_the_sets_hold_what_they_are_named_for():
    assert len(GENOME) == 1500 and GENOME[SNP] != HAP2[SNP] and all(len(r) == 50 for r in PATH)
    # a unique path: one irreducible edge per end, to the neighbour, although three reads overlap at each end
    u = ov_case("unique_path")
    for i in range(3, 23):
        assert sorted(x for x in _final("unique_path", i) if not x[4]) == [(40, 1, 0, 0, 0), (40, 1, 1, 1, 0)], i
    assert [x for x in _final("unique_path", 0) if not x[4]] == [(40, 1, 0, 0, 0)] and u["edges"].count("ED\t") == 25 and not any(r["is_substring"] for r in u["results"])
    assert "ED\tread5 read4 0 39 50 10 49 50 0 0\n" in u["edges"] and "ED\tread9 read10 10 49 50 0 39 50 0 0\n" in u["edges"]
    # the branch: read 5 ends before the site, and its group splits in two there; both branches give an edge
    b = ov_case("branch_at_the_snp")
    assert b["reads"][5] == GENOME[550:600] and b["reads"][6][40] != b["reads"][16][40] and b["reads"][6][:40] == b["reads"][16][:40]
    assert ("split", 2) in _events("branch_at_the_snp", 5, "split")
    assert sorted(x for x in _final("branch_at_the_snp", 5) if not x[3] and not x[4]) == [(40, 1, 0, 0, 0), (40, 1, 0, 0, 0)]
    # both strands: the neighbour and its reverse complement are both reads, two top-length blocks end together and both go out
    assert ("tlb", 2) in _events("both_strands", 0, "tlb")
    assert sorted(x for x in _final("both_strands", 0) if not x[3] and not x[4]) == [(40, 1, 0, 0, 0), (40, 1, 1, 0, 0)]
    # identical reads, and reverse-complement identical ones: a containment block, one edge between the two
    i = ov_case("identical_reads")
    assert (50, 2, 0, 0, 1) in _final("identical_reads", 5) and (50, 2, 0, 0, 1) in _final("identical_reads", 26)
    assert "ED\tread5 read26 0 49 50 0 49 50 0 0\n" in i["edges"] and i["edges"].count("read26 read5 ") == 0
    r = ov_case("revcomp_identical_reads")
    assert (50, 1, 1, 0, 1) in _final("revcomp_identical_reads", 5) and "ED\tread5 read26 0 49 50 0 49 50 1 0\n" in r["edges"]
    # the substring read
    s = ov_case("substring_read")
    assert [q["is_substring"] for q in s["results"]] == [0] * 26 + [1] and "VT\tread26\t" + GENOME[105:135] + "\tSS:i:1\n" in s["asqg"]
    assert "read26" not in s["edges"] and s["asqg"].count("SS:i:0") == 26
    # the pop: read 1 ends while the longer read 2, of the same overlap with read 0, goes on: read 1's block is taken back
    p = ov_case("sa_right_extension_pop")
    assert _events("sa_right_extension_pop", 0, "pop") == [("pop", 1)] and p["results"][1]["is_substring"] == 1
    assert [x for x in _final("sa_right_extension_pop", 0) if not x[3] and not x[4]] == [(40, 1, 1, 0, 0)]
    # the trim: ten overlap lengths with sixteen reads each; the sum reaches 128 at the eighth from the back, which goes with the
    # two longer ones: the tails of the reads are random, so every read that is left ends up in a block of its own
    t = ov_case("trim")
    assert _events("trim", 0, "trim") == [("trim", [30, 28, 26], [24, 22, 20, 18, 16, 14, 12])]
    assert sorted(x for x in _final("trim", 0) if not x[3] and not x[4]) == sorted([(L, 1, 0, 0, 0) for L in range(12, 25, 2)] * 16) and t["m"] == 10
    # submaximal: one read starts with two suffixes of another, the blocks of both lengths hold it
    assert _events("submaximal", 26, "submaximal") == [("submaximal", 25, 20, 1)]
    assert [x for x in _final("submaximal", 26) if not x[3] and not x[4]] == [(25, 1, 0, 0, 0)]
    # a read shorter than m; m equal to the read length: containments only
    assert ov_case("shorter_than_m")["results"][26] == dict(is_substring=0, blocks=[])
    e = ov_case("m_equal_to_the_read_length")
    assert all(x[4] for i in range(27) for x in _final("m_equal_to_the_read_length", i)) and e["edges"] == "ED\tread5 read26 0 49 50 0 49 50 0 0\n"
    assert len(ov_case("random")["reads"]) == 200 and ov_case("random")["edges"].count("ED\t") > 200


def test_the_yardstick_gives_the_irreducible_overlaps_of_the_definition():
    with_edges = 0
    for name in BY_DEFINITION:
        c = ov_case(name)
        assert not any(r["is_substring"] for r in c["results"]) and not any(t[0] == "trim" for tr in c["traces"] for t in tr), name
        lines = c["edges"].splitlines(keepends=True)
        assert set(lines) == brute_edge_lines(c["names"], c["reads"], c["m"]), name
        # a pair of duplicates stands in one block: the yardstick writes a line once
        assert len(lines) == len(set(lines)), name
        with_edges += 1 if lines else 0
    assert with_edges >= 4


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _build(exe: Path, *flags: str) -> str:
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/overlap_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def overlap_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("overlap_driver") / "overlap_driver")


def reads_input(reads: list[str]) -> tuple[np.ndarray, np.ndarray]:
    """(the ASCII bases of the reads back to back, their n + 1 offsets)"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8), off


def result_dicts(per_read: np.ndarray, blocks: np.ndarray) -> list[dict]:
    """OVERLAP_READ_DTYPE and OVERLAP_BLOCK_DTYPE records -> what plain_overlap_exact returns"""
    out = []
    for q in per_read:
        assert q["status"] == 0 and q["pad"] == 0
        mine = blocks[int(q["first_block"]): int(q["first_block"]) + int(q["n_blocks"])]
        out.append(dict(is_substring=int(q["is_substring"]), blocks=[{k: int(b[k]) for k in OVERLAP_BLOCK_DTYPE.names} for b in mine]))
    return out


def run_overlap_driver(exe: str, name: str, wide: int):
    """-> [dict per read], Occ queries, block loads"""
    c = ov_case(name)
    bases, off = reads_input(c["reads"])
    n = len(c["reads"])
    blob = b"".join([_image_input(naive_sa(c["reads"])[0]), _image_input(naive_sa([r[::-1] for r in c["reads"]])[0]), np.array([c["m"]], dtype=np.int32).tobytes(),
                     np.array([n], dtype=np.uint64).tobytes(), off.tobytes(), bytes(CODE[chr(x)] - 1 for x in bases)])
    r = subprocess.run([exe, str(wide)], input=blob, capture_output=True)
    assert r.returncode == 0, (name, wide, r.returncode, r.stderr[-2000:])
    per_read = np.frombuffer(r.stdout, dtype=OVERLAP_READ_DTYPE, count=n)
    total = int(per_read["n_blocks"].sum())
    blocks = np.frombuffer(r.stdout, dtype=OVERLAP_BLOCK_DTYPE, count=total, offset=n * 24)
    ranks, loads = np.frombuffer(r.stdout, dtype=np.uint64, count=2, offset=n * 24 + total * 24)
    assert n * 24 + total * 24 + 16 == len(r.stdout)
    return result_dicts(per_read, blocks), int(ranks), int(loads)


def _run_sets(exe: str, wide: int, names) -> int:
    for name in names:
        got, ranks, loads = run_overlap_driver(exe, name, wide)
        want = ov_case(name)["results"]
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, wide, i)
        assert ranks // 2 <= loads <= ranks
    return len(names)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_field_equals_the_yardstick(overlap_driver, layout):
    assert OVERLAP_READ_DTYPE.itemsize == 24 and OVERLAP_BLOCK_DTYPE.itemsize == 24
    assert _run_sets(overlap_driver, LAYOUTS[layout], list(OV_SETS)) == 12


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: the named sets, both layouts; workspace, bases, chain blocks and output are allocations of their own"""
    exe = _build(tmp_path / "overlap_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        _run_sets(exe, wide, NAMED)


# ---- the ABI, the kernels ------------------------------------------------------------------------------------------------------
def test_overlap_entry_is_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    assert "lrsc_overlap_exact" in capi.declared_symbols() and " T lrsc_overlap_exact\n" in exported
    assert ("typedef struct lrsc_overlap_block { int64_t lower, upper; uint32_t overlap_len; uint8_t target_rev, query_rev, query_comp, contained; } "
            "lrsc_overlap_block;") in header
    assert "typedef struct lrsc_overlap_read { uint32_t is_substring, n_blocks, status, pad; uint64_t first_block; } lrsc_overlap_read;" in header
    assert ("int lrsc_overlap_exact(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap,\n"
            "                       lrsc_overlap_read* per_read, lrsc_overlap_block* blocks, uint64_t block_cap, uint64_t* n_blocks_out);") in header
    for cited in ("StriDe/overlap.cpp:126-413", "OverlapProcess.cpp:32-109", "OverlapAlgorithm.cpp:22-44, 270-389, 419-487, 1043-1193, 1423-1444", "OverlapBlock.cpp:",
                  "40-70, 128-160, 182-360", "updateBothL"):
        assert cited in header, cited
    limits = {n: int(v) for n, v in re.findall(r"#define LRSC_OVERLAP_MAX_(\w+) (\d+)", header)}
    assert limits == {"READ": _const("kOvMaxRead"), "MIN_OVERLAP": _const("kOvMaxMinOverlap")} and limits["READ"] >= 2000
    assert "#define LRSC_ABI_VERSION 2\n" in header and api.lib.lrsc_abi_version() == 2
    assert capi.OVERLAP_READ_DTYPE == OVERLAP_READ_DTYPE and capi.OVERLAP_BLOCK_DTYPE == OVERLAP_BLOCK_DTYPE and callable(capi.Ctx.overlap_exact)
    assert "isTargetSubstring" in (REPO / "longreadselfcorrect_amd/csrc/fm_overlap.h").read_text()


def test_overlap_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_overlap"), r"overlap_[a-z]+_kernel")
    assert {k: len(v) for k, v in seen.items()} == {"overlap_collect_kernel": 2, "overlap_reduce_kernel": 2}, seen
    waves, threads = _const("kOvWavesPerSimd"), _const("kOvThreads")
    assert waves >= 4 and threads % 64 == 0
    for kernel in seen.values():
        for name, md in kernel:
            lds = md["group_segment_fixed_size"]
            assert md["max_flat_workgroup_size"] == threads
            # 512 VGPRs per lane and SIMD, allocated in eights; 160 KiB of LDS per CU for the workgroups of its four SIMDs
            assert md["vgpr_count"] <= 512 // waves // 8 * 8, (name, md)
            assert 0 < lds and lds * (waves * 4 // (threads // 64)) <= 160 * 1024, (name, md)
        assert {re.search(r"ILb([01])E", n).group(1) for n, _ in kernel} == {"0", "1"}


# ---- the command line ------------------------------------------------------------------------------------------------------------
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
OVERLAP_USAGE = "Usage: StriDe overlap [OPTION] ... READSFILE"


def test_stride_overlap_usage(api, tmp_path):
    run = lambda *args: subprocess.run([str(STRIDE), "overlap", *args], cwd=tmp_path, capture_output=True, text=True, input="")
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n>r1\nACGTACGT\n")
    for args, message in ((["-e", "0.05", "reads.fa"], "overlap: -e is not built here"),
                          (["--error-rate=0.05", "reads.fa"], "overlap: -e is not built here"),
                          (["-a", "ADPF", "reads.fa"], "overlap: -a is not built here"),
                          (["-l", "3", "reads.fa"], "overlap: -l is not built here"),
                          (["-f", "other.fa", "reads.fa"], "overlap: -f is not built here"),
                          ([], "overlap: missing arguments"),
                          (["reads.fa", "more.fa"], "overlap: too many arguments"),
                          (["-t", "0", "reads.fa"], "overlap: invalid number of threads: 0"),
                          (["-d", "48", "reads.fa"], "overlap: invalid parameter to -d/--sample-rate, must be power of 2. got: 48"),
                          (["--frobnicate", "reads.fa"], "overlap: unrecognized option '--frobnicate'")):       # getopt's own line
        r = run(*args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert message in r.stderr and len([l for l in r.stderr.split("\n") if l.strip()]) == 1, (args, r.stderr)
        assert OVERLAP_USAGE in r.stdout, (args, r.stdout, r.stderr)
        for option in ("--min-overlap=LEN", "--exhaustive", "--exact", "--target-file=FILE", "--prefix=PREFIX", "--device=N", "--build-index", "--load-on-device"):
            assert option in r.stdout, (args, option)
        assert not list(tmp_path.glob("*.gz"))
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith(OVERLAP_USAGE) and r.stderr == ""
    # The two command lists: the lines that test_kmer_correct_host and test_fmwalk_host pin stay, overlap stands on a third.
    for args in (["help"], []):
        r = subprocess.run([str(STRIDE), *args], cwd=tmp_path, capture_output=True, text=True, input="")
        lines = (r.stdout + r.stderr).split("\n")
        at = [i for i, l in enumerate(lines) if l.startswith("Commands:")]
        assert len(at) == 1 and lines[at[0] + 1] == "          and fmwalk" and lines[at[0] + 2] == "          and overlap", (args, r.stdout, r.stderr)
