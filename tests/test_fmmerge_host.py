"""The device fm-merge (csrc/fm_fmmerge.h, fm_fmmerge.hip, capi_fmmerge.cpp) checked without a GPU.

1. The yardstick, plain_fmmerge: FMMergeProcess::process restated over a small bigraph, read by read in file order with the used
   set, the blocks being plain_overlap_exact's of test_overlap_host:
     FMMergeProcess::process, checkCandidate, addCandidates, FMMergePostProcess::process   (Algorithm/FMMergeProcess.cpp)
     Bigraph::sweepVertices, SGDuplicateVisitor, Bigraph::simplify, Bigraph::merge, Vertex::merge   (Bigraph/, StringGraph/SGVisitors.cpp)
   A vertex is named by its read (the reference names it by the read's row, which the lexicographic order maps to the read), and
   an edge keeps of its match coordinates the overlap length, which is all an exact overlap has.  The three decisions of lrsc.h:
   simplify visits the vertices in ascending read number (the reference: the order of a hash map), so a sequence reads on the
   forward strand of its lowest-numbered read and a cycle starts there and runs towards the sense end; a refused candidate
   stays red; where the reference asserts on a read that is its own candidate, the end has no link and the read is flagged.
2. The named sets, each with an assertion that it holds what it is named for.
3. The same sequences by definition: the unitigs of the graph of brute_edge_lines.
4. The invariant: every read that is not dropped stands at its offset in its sequence, the reads partition the set.
5. tests/host_tools/fmmerge_driver.cpp, fm_fmmerge.h compiled for the CPU and run in the kernels' order: every field equals the
   yardstick's on every set, for both layouts; again under AddressSanitizer and UBSan, as a stand-alone program.
6. The entry is declared, exported and bound; the kernels compile for gfx950 without scratch; `stride fm-merge --help`.
"""
from __future__ import annotations

import re
import subprocess
from collections import deque
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO
from .test_index_filter_host import LAYOUTS, _image_input, _kernel_notes, _kernels, _rand, revcomp
from .test_index_locate_host import naive_sa
from .test_index_merge_host import CODE
from .test_overlap_host import GENOME, HAP2, M, OV_SETS, PATH, STRIDE, Index, brute_edge_lines, plain_overlap_exact, reads_input

FMMERGE_READ_DTYPE = np.dtype([("seq", "<u4"), ("flags", "<u4"), ("offset", "<u8")])
FMMERGE_SEQ_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u8"), ("n_reads", "<u4"), ("root", "<u4"), ("circular", "<u4"), ("pad", "<u4")])
REVERSED, DROPPED, SELF_LINK = 1, 2, 4
SENSE, ANTISENSE = 0, 1
WHITE, RED, BLACK = 0, 1, 2


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
class Edge:
    def __init__(self, start, end, direction, comp, overlap):
        self.start, self.end, self.dir, self.comp, self.overlap = start, end, direction, comp, overlap
        self.twin = None
        self.color = WHITE

    def desc(self):
        return (self.end.id, self.dir, self.comp)


class Vertex:
    def __init__(self, vid: int, seq: str):
        self.id, self.seq, self.edges, self.color = vid, seq, [], WHITE
        self.members = [(vid, 0, 0)]                              # (read, offset, reversed) of what the sequence holds
        self.circular = 0

    def get_edges(self, direction):
        return [e for e in self.edges if e.dir == direction]


class Graph:
    def __init__(self):
        self.vertices = {}

    def add_vertex(self, v):
        self.vertices[v.id] = v

    def sweep_vertices(self, color):
        for v in [v for v in self.vertices.values() if v.color == color]:
            for e in v.edges:
                e.end.edges.remove(e.twin)
            del self.vertices[v.id]

    def remove_duplicate_edges(self):
        """SGDuplicateVisitor: Vertex::markDuplicateEdges, then sweepEdges"""
        for v in self.vertices.values():
            v.edges.sort(key=lambda e: -e.overlap)                # sortAdjListByLen
            for direction in (SENSE, ANTISENSE):
                for e in v.get_edges(direction):
                    if e.end.color == BLACK:
                        e.color = e.twin.color = RED
                    else:
                        e.end.color = BLACK
                for e in v.edges:
                    e.end.color = WHITE
        for v in self.vertices.values():
            v.edges = [e for e in v.edges if e.color != RED]

    def merge(self, v, edge):
        """Bigraph::merge with Vertex::merge"""
        w, twin = edge.end, edge.twin
        # Edge::getLabel: what the twin's match leaves of w, in v's strand
        label = w.seq[: len(w.seq) - edge.overlap] if twin.dir == SENSE else w.seq[edge.overlap:]
        if edge.comp:
            label = revcomp(label)
        moved = []
        for r, off, rev in w.members:
            n = len(self.reads[r])
            moved.append((r, len(w.seq) - off - n, rev ^ 1) if edge.comp else (r, off, rev))
        if edge.dir == SENSE:
            at = len(v.seq) - edge.overlap
            v.seq = v.seq + label
            v.members += [(r, at + off, rev) for r, off, rev in moved]
        else:
            v.seq = label + v.seq
            v.members = [(r, off, rev) for r, off, rev in moved] + [(r, off + len(label), rev) for r, off, rev in v.members]
        for t in w.get_edges(1 - twin.dir):                       # the edges opposite of the twin are v's now: Edge::join
            w.edges.remove(t)
            t.start, t.dir, t.comp = v, edge.dir, t.comp ^ edge.comp
            t.twin.end, t.twin.comp = v, t.comp
            v.edges.append(t)
        v.edges.remove(edge)
        w.edges.remove(twin)
        assert not w.edges
        del self.vertices[w.id]

    def simplify_from(self, v, direction):
        edges = v.get_edges(direction)
        while len(edges) == 1:
            single = edges[0]
            assert single.end is not v
            if len(single.end.get_edges(single.twin.dir)) != 1:
                break
            self.merge(v, single)
            edges = v.get_edges(direction)
            for e in [e for e in edges if e.end is v]:            # self edges of V->W->V
                if e in v.edges:
                    v.edges.remove(e)
                    v.edges.remove(e.twin)
                    v.circular = 1
            edges = v.get_edges(direction)

    def simplify(self):
        for vid in sorted(self.vertices):                         # the decision: ascending read number
            if vid in self.vertices:
                self.simplify_from(self.vertices[vid], SENSE)
                self.simplify_from(self.vertices[vid], ANTISENSE)


def final_blocks(c: dict, r: int) -> list[dict]:
    """overlapRead and removeContainmentBlocks of read r: (edge direction, target read, overlap, reverse complement, twin direction)"""
    out = []
    for b in c["results"][r]["blocks"]:
        if b["contained"]:
            continue
        assert b["lower"] == b["upper"], "a block of several rows: fm-merge requires `stride filter` first"
        t = (c["ix"].rbwt if b["target_rev"] else c["ix"].bwt).order[b["lower"]]
        out.append(dict(dir=ANTISENSE if b["query_rev"] else SENSE, target=t, overlap=b["overlap_len"], comp=int(b["target_rev"] != b["query_rev"]),
                        twin_dir=SENSE if b["target_rev"] else ANTISENSE))
    return out


def check_candidate(cand, blocks) -> bool:
    merge_dir = cand["edge"].twin.dir
    return sum(1 for b in blocks if b["dir"] == merge_dir) == 1


def add_candidates(c, g, x, edge_to_x, blocks, queue, self_link: set):
    count = {d: sum(1 for b in blocks if b["dir"] == d) for d in (SENSE, ANTISENSE)}
    for b in blocks:
        if count[b["dir"]] != 1:
            continue
        if edge_to_x is not None and edge_to_x.twin.dir == b["dir"]:
            continue
        if b["target"] == x.id:                                   # assert(vertexID != pX->getID()): the decision
            self_link.add(x.id)
            continue
        y = g.vertices.get(b["target"])
        if y is None:
            y = Vertex(b["target"], c["reads"][b["target"]])
            g.add_vertex(y)
        if (y.id, b["dir"], b["comp"]) in [e.desc() for e in x.edges]:
            continue
        xy, yx = Edge(x, y, b["dir"], b["comp"], b["overlap"]), Edge(y, x, b["twin_dir"], b["comp"], b["overlap"])
        xy.twin, yx.twin = yx, xy
        x.edges.append(xy)
        y.edges.append(yx)
        queue.append(dict(vertex=y, edge=xy))


def process(c, root: int, self_link: set):
    """FMMergeProcess::process of an unused read -> (the used reads, the vertices left)"""
    g = Graph()
    g.reads = c["reads"]
    v = Vertex(root, c["reads"][root])
    g.add_vertex(v)
    used, queue = [root], deque()
    add_candidates(c, g, v, None, final_blocks(c, root), queue, self_link)
    while queue:
        cand = queue.popleft()
        blocks = final_blocks(c, cand["vertex"].id)
        if check_candidate(cand, blocks):
            add_candidates(c, g, cand["vertex"], cand["edge"], blocks, queue, self_link)
            used.append(cand["vertex"].id)
        else:
            cand["vertex"].color = RED
    g.sweep_vertices(RED)
    g.remove_duplicate_edges()
    g.simplify()
    return sorted(set(used)), [g.vertices[k] for k in sorted(g.vertices)]


def plain_fmmerge(c: dict) -> dict:
    """-> per_read [(seq, flags, offset)], seqs [dict(bases, n_reads, root, circular)], the FASTA text"""
    n = len(c["reads"])
    marked, self_link = [False] * n, set()
    per_read, seqs = [None] * n, []
    for r in range(n):
        if marked[r]:
            continue
        used, left = process(c, r, self_link)
        assert used[0] == r and not any(marked[u] for u in used)
        for u in used:
            marked[u] = True
        first = len(seqs)
        for v in left:
            for read, off, rev in v.members:
                per_read[read] = [len(seqs), REVERSED if rev else 0, off]
            seqs.append(dict(bases=v.seq, n_reads=len(v.members), root=min(m[0] for m in v.members), circular=v.circular))
        for u in used:
            if per_read[u] is None:
                per_read[u] = [first, DROPPED, 0]
    for r in self_link:
        per_read[r][1] |= SELF_LINK
    fasta = "".join(f">merged-{i}\n{s['bases']}\n" for i, s in enumerate(seqs))
    return dict(per_read=[tuple(p) for p in per_read], seqs=seqs, fasta=fasta)


# ---- the sets ----------------------------------------------------------------------------------------------------------------
_CIRCLE = GENOME[700:900]
CYCLE = [(_CIRCLE * 2)[s: s + 50] for s in range(0, 200, 10)]
_TAIL = _rand(0x0F31, 10) + _CIRCLE[:40]
_PERIODIC = (_rand(0x0F32, 15) * 4)[:50]
_HALF = _rand(0x0F35, 10)
_PALINDROMIC = _rand(0x0F36, 30) + _HALF + revcomp(_HALF)         # its last 20 bases are their own reverse complement


def _shuffled(reads, seed):
    return [reads[i] for i in np.random.default_rng(seed).permutation(len(reads))]


def _random_set(seed: int, n: int) -> list[str]:
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        s = int(rng.integers(0, len(GENOME) - 49))
        r = (HAP2 if rng.integers(2) else GENOME)[s: s + 50]
        r = revcomp(r) if rng.integers(2) else r
        if r in seen or revcomp(r) in seen:
            continue
        seen.add(r)
        out.append(r)
    return out


FM_SETS = {
    "unique_path": lambda: (PATH, M),
    "alternate_strands": lambda: ([revcomp(r) if i & 1 else r for i, r in enumerate(PATH)], M),
    "root_on_reverse": lambda: ([revcomp(PATH[0])] + PATH[1:], M),
    "root_in_the_middle": lambda: (_shuffled(PATH, 0x0F33), M),
    "branch_at_the_snp": OV_SETS["branch_at_the_snp"],
    "revcomp_identical_reads": OV_SETS["revcomp_identical_reads"],
    "cycle": lambda: (CYCLE[7:] + CYCLE[:7], M),
    "lasso": lambda: (CYCLE[:5] + [_TAIL] + CYCLE[5:], M),
    "self_overlap": lambda: (PATH + [_PERIODIC], M),
    "self_palindrome": lambda: (PATH + [_PALINDROMIC], M),
    "shorter_than_m": OV_SETS["shorter_than_m"],
    "random": lambda: (_random_set(0x0F34, 200), M),
}
NAMED = [n for n in FM_SETS if n != "random"]
_FM: dict = {}


def fm_case(name: str) -> dict:
    """the set with both yardsticks, computed once and left unchanged"""
    if name not in _FM:
        reads, m = FM_SETS[name]()
        ix = Index(reads)
        c = dict(names=[f"read{i}" for i in range(len(reads))], reads=list(reads), m=m, ix=ix, results=[plain_overlap_exact(ix, r, m) for r in reads])
        c["merged"] = plain_fmmerge(c)
        _FM[name] = c
    return _FM[name]


def _bases(name):
    return [s["bases"] for s in fm_case(name)["merged"]["seqs"]]


def test_the_sets_hold_what_they_are_named_for():
    assert _bases("unique_path") == [GENOME[0:300]] and fm_case("unique_path")["merged"]["seqs"][0] == dict(bases=GENOME[0:300], n_reads=26, root=0, circular=0)
    assert fm_case("unique_path")["merged"]["per_read"][7] == (0, 0, 70)
    a = fm_case("alternate_strands")["merged"]
    assert [s["bases"] for s in a["seqs"]] == [GENOME[0:300]] and [p[1] for p in a["per_read"]] == [0, REVERSED] * 13
    r = fm_case("root_on_reverse")["merged"]
    assert [s["bases"] for s in r["seqs"]] == [revcomp(GENOME[0:300])] and r["per_read"][0] == (0, 0, 250) and r["per_read"][25] == (0, REVERSED, 0)
    mid = fm_case("root_in_the_middle")
    where = mid["reads"].index(PATH[0])
    assert 0 < where < 25 and mid["reads"][0] not in (PATH[0], PATH[25]) and _bases("root_in_the_middle") == [GENOME[0:300]]
    assert mid["merged"]["seqs"][0]["root"] == 0
    # the branch: the path before the site, the two alleles' paths, and the path behind it; no chain crosses the branch
    b = fm_case("branch_at_the_snp")["merged"]
    assert len(b["seqs"]) == 4 and sorted(s["n_reads"] for s in b["seqs"]) == [5, 5, 5, 6] and sum(len(s["bases"]) for s in b["seqs"]) > 21 * 10
    assert b["seqs"][0]["bases"] == GENOME[500:600] and all(not p[1] for p in b["per_read"])
    # reverse-complement identical reads: both stand as blocks on their neighbours' ends, which therefore have no link
    v = fm_case("revcomp_identical_reads")
    assert sum(1 for x in final_blocks(v, 4) if x["dir"] == SENSE) == 2 and sum(1 for x in final_blocks(v, 6) if x["dir"] == ANTISENSE) == 2
    assert [s["n_reads"] for s in v["merged"]["seqs"]] == [5, 1, 20, 1] and v["merged"]["per_read"][26][0] == 3
    # the cycle: once round from the lowest read towards its sense end, and the closing overlap
    c = fm_case("cycle")
    assert c["reads"][0] == CYCLE[7] and c["merged"]["seqs"] == [dict(bases=(_CIRCLE * 2)[70: 70 + 240], n_reads=20, root=0, circular=1)]
    # the lasso: read 0, where the tail enters the circle, is used by the first sequence and in none
    la = fm_case("lasso")
    assert la["reads"][0] == CYCLE[0] and sum(1 for x in final_blocks(la, 0) if x["dir"] == ANTISENSE) == 2 and la["reads"][5] == _TAIL
    assert la["merged"]["per_read"][0] == (0, DROPPED, 0) and [p[1] & DROPPED for p in la["merged"]["per_read"]].count(DROPPED) == 1
    assert la["merged"]["seqs"] == [dict(bases=(_CIRCLE * 2)[10:240], n_reads=19, root=1, circular=0), dict(bases=_TAIL, n_reads=1, root=5, circular=0)]
    # the periodic read overlaps itself by 35 and by 20 bases, but on its own strand its row is also the containment block's, and
    # removeSubMaximalBlocks keeps the longer block of a row: no block is left, no link, no flag
    s = fm_case("self_overlap")
    assert _PERIODIC[15:] == _PERIODIC[:35] and _PERIODIC[30:] == _PERIODIC[:20] and final_blocks(s, 26) == []
    assert s["merged"]["per_read"][26] == (1, 0, 0) and s["merged"]["seqs"][1] == dict(bases=_PERIODIC, n_reads=1, root=26, circular=0)
    # a read that ends in a reverse palindrome overlaps its own reverse complement; that block stands on the read's row of the
    # other strand, where the containment block of that strand's list absorbs it in the same way.  So no read is its own
    # candidate after overlapRead, the reference's assertion never fires, and LRSC_FMMERGE_SELF_LINK is never seen on these sets.
    pal = fm_case("self_palindrome")
    assert _PALINDROMIC[30:] == revcomp(_PALINDROMIC)[:20] and final_blocks(pal, 26) == []
    assert pal["merged"]["per_read"][26] == (1, 0, 0) and pal["merged"]["seqs"][1] == dict(bases=_PALINDROMIC, n_reads=1, root=26, circular=0)
    assert not any(p[1] & SELF_LINK for name in FM_SETS for p in fm_case(name)["merged"]["per_read"])
    assert fm_case("shorter_than_m")["merged"]["seqs"][1] == dict(bases="ACGTTGCAAGGCTTA", n_reads=1, root=26, circular=0)
    rnd = fm_case("random")
    assert len(rnd["reads"]) == 200 and len(set(rnd["reads"])) == 200 and 5 < len(rnd["merged"]["seqs"]) < 150
    assert any(p[1] & REVERSED for p in rnd["merged"]["per_read"]) and max(s["n_reads"] for s in rnd["merged"]["seqs"]) >= 4


# ---- the sequences by definition -------------------------------------------------------------------------------------------------
def unitigs(names: list[str], reads: list[str], m: int) -> list[tuple]:
    """The unitigs of the graph of brute_edge_lines: an end of a read with exactly one edge is joined to that edge's other end when
    that has exactly one edge too.  A walk, link by link, from the lowest read of every chain towards its sense end first:
    -> (bases on that read's forward strand, the chain's reads, circular), in the order of the lowest reads."""
    ends: dict = {}
    number = {n: i for i, n in enumerate(names)}
    for line in brute_edge_lines(names, reads, m):
        q, t, s1, e1, l1, s2, e2, l2, _rc, _ = line[3:].split()
        q, t, s1, e1, l1, s2, e2, l2 = number[q], number[t], int(s1), int(e1), int(l1), int(s2), int(e2), int(l2)
        if (s1 == 0 and e1 == l1 - 1) or (s2 == 0 and e2 == l2 - 1):
            continue
        a, b = (q, ANTISENSE if s1 == 0 else SENSE), (t, ANTISENSE if s2 == 0 else SENSE)
        ends.setdefault(a, []).append((b, e1 - s1 + 1))
        ends.setdefault(b, []).append((a, e1 - s1 + 1))

    def link(x):
        if len(ends.get(x, [])) != 1:
            return None
        y, ov = ends[x][0]
        return (y, ov) if len(ends[y]) == 1 and ends[y][0][0] == x and y[0] != x[0] else None

    seen, out = set(), []
    for r in range(len(reads)):
        if r in seen:
            continue
        # to the lowest read's antisense side first, to find where the chain starts
        chain, x, circular = [(r, 0)], (r, ANTISENSE), 0
        while link(x):
            (t, e), _ = link(x)
            if t == r:
                circular = 1
                break
            chain.insert(0, (t, int(e == ANTISENSE)))              # entered at its sense end: forward
            x = (t, 1 - e)
        if circular:
            chain = [(r, 0)]
        x = (r, SENSE)
        bases = None
        while link(x):
            (t, e), _ = link(x)
            if t == r:
                break
            chain.append((t, int(e == SENSE)))
            x = (t, 1 - e)
        for i, (t, rev) in enumerate(chain):
            s = revcomp(reads[t]) if rev else reads[t]
            if i == 0:
                bases = s
            else:
                p = chain[i - 1]
                bases += s[link((p[0], ANTISENSE if p[1] else SENSE))[1]:]      # behind the overlap at the end p is left by
        seen |= {t for t, _ in chain}
        out.append((bases, sorted(t for t, _ in chain), circular))
    return out


@pytest.mark.parametrize("name", list(FM_SETS))
def test_the_sequences_are_the_unitigs_of_the_definition(name):
    c = fm_case(name)
    want, got = unitigs(c["names"], c["reads"], c["m"]), c["merged"]["seqs"]
    if name == "lasso":                                           # the definition keeps the read that the reference drops
        assert len(want) == len(got) == 2 and want[1][0] == got[1]["bases"] and want[0][1] == list(range(5)) + list(range(6, 21))
        assert got[0]["bases"] in want[0][0] or revcomp(got[0]["bases"]) in want[0][0]
        return
    canonical = lambda s: min(s, revcomp(s))
    assert sorted(canonical(w[0]) for w in want) == sorted(canonical(g["bases"]) for g in got)
    # exactly, under the strand rule, in the order of the lowest reads; the cycle from its lowest read
    assert [w[0] for w in want] == [g["bases"] for g in got] and [w[2] for w in want] == [g["circular"] for g in got]
    assert [(w[1][0], len(w[1])) for w in want] == [(g["root"], g["n_reads"]) for g in got]


def check_invariant(reads: list[str], per_read, seqs: list[dict]):
    """per_read: (seq, flags, offset); seqs: dicts with bases and n_reads"""
    held = [0] * len(seqs)
    for r, (seq, flags, offset) in enumerate(per_read):
        assert 0 <= seq < len(seqs), r
        if flags & DROPPED:
            assert offset == 0
            continue
        held[seq] += 1
        me = revcomp(reads[r]) if flags & REVERSED else reads[r]
        assert seqs[seq]["bases"][offset: offset + len(me)] == me, r
    assert held == [s["n_reads"] for s in seqs] and all(h > 0 for h in held)
    for i, s in enumerate(seqs):                                  # every base of a sequence is some read's
        covered = np.zeros(len(s["bases"]), dtype=bool)
        for r, (seq, flags, offset) in enumerate(per_read):
            if seq == i and not flags & DROPPED:
                covered[offset: offset + len(reads[r])] = True
        assert covered.all(), i


@pytest.mark.parametrize("name", list(FM_SETS))
def test_every_read_stands_at_its_offset(name):
    c = fm_case(name)
    check_invariant(c["reads"], c["merged"]["per_read"], c["merged"]["seqs"])
    roots = [s["root"] for s in c["merged"]["seqs"]]
    assert all(c["merged"]["per_read"][r][1] & (REVERSED | DROPPED) == 0 for r in roots)
    assert c["merged"]["fasta"].count(">merged-") == len(roots) and c["merged"]["fasta"].startswith(">merged-0\n")


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _build(exe: Path, *flags: str) -> str:
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), str(REPO / "tests/host_tools/fmmerge_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def fmmerge_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fmmerge_driver") / "fmmerge_driver")


def driver_input(reads: list[str], m: int, ix: Index | None = None) -> bytes:
    ix = ix or Index(reads)
    bases, off = reads_input(reads)
    return b"".join([_image_input(naive_sa(reads)[0]), _image_input(naive_sa([r[::-1] for r in reads])[0]), np.array([m], dtype=np.int32).tobytes(),
                     np.array([len(reads)], dtype=np.uint64).tobytes(), off.tobytes(), bytes(CODE[chr(x)] - 1 for x in bases),
                     np.array(ix.bwt.order, dtype=np.uint32).tobytes(), np.array(ix.rbwt.order, dtype=np.uint32).tobytes()])


def merged_dicts(per_read: np.ndarray, seqs: np.ndarray, bases: bytes) -> dict:
    """FMMERGE_READ_DTYPE, FMMERGE_SEQ_DTYPE records and the bases -> what plain_fmmerge returns"""
    text = bases.decode()
    assert all(int(s["pad"]) == 0 for s in seqs)
    at = 0
    for s in seqs:                                                # back to back, in their order
        assert int(s["offset"]) == at
        at += int(s["length"])
    assert at == len(text)
    out = [dict(bases=text[int(s["offset"]): int(s["offset"]) + int(s["length"])], n_reads=int(s["n_reads"]), root=int(s["root"]), circular=int(s["circular"])) for s in seqs]
    return dict(per_read=[(int(p["seq"]), int(p["flags"]), int(p["offset"])) for p in per_read], seqs=out,
                fasta="".join(f">merged-{i}\n{s['bases']}\n" for i, s in enumerate(out)))


def run_fmmerge_driver(exe: str, reads: list[str], m: int, wide: int, ix: Index | None = None):
    """-> the refusal (kind, read), or the merged dicts"""
    r = subprocess.run([exe, str(wide)], input=driver_input(reads, m, ix), capture_output=True)
    assert r.returncode == 0, (wide, r.returncode, r.stderr[-2000:])
    assert re.fullmatch(rb"chain_ms \d+\.\d+\n", r.stderr) or len(r.stdout) == 8, r.stderr[-2000:]
    refusal = np.frombuffer(r.stdout, dtype=np.uint32, count=2)
    if refusal[0]:
        assert len(r.stdout) == 8
        return int(refusal[0]), int(refusal[1])
    n = len(reads)
    per_read = np.frombuffer(r.stdout, dtype=FMMERGE_READ_DTYPE, count=n, offset=8)
    n_seqs = int(np.frombuffer(r.stdout, dtype=np.uint64, count=1, offset=8 + 16 * n)[0])
    seqs = np.frombuffer(r.stdout, dtype=FMMERGE_SEQ_DTYPE, count=n_seqs, offset=16 + 16 * n)
    n_bases = int(np.frombuffer(r.stdout, dtype=np.uint64, count=1, offset=16 + 16 * n + 32 * n_seqs)[0])
    assert len(r.stdout) == 24 + 16 * n + 32 * n_seqs + n_bases
    return merged_dicts(per_read, seqs, r.stdout[24 + 16 * n + 32 * n_seqs:])


def _run_sets(exe: str, wide: int, names) -> int:
    for name in names:
        c = fm_case(name)
        got = run_fmmerge_driver(exe, c["reads"], c["m"], wide, c["ix"])
        assert got["seqs"] == c["merged"]["seqs"], (name, wide)
        assert got["per_read"] == c["merged"]["per_read"], (name, wide)
        assert got["fasta"] == c["merged"]["fasta"]
    return len(names)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_field_equals_the_yardstick(fmmerge_driver, layout):
    assert FMMERGE_READ_DTYPE.itemsize == 16 and FMMERGE_SEQ_DTYPE.itemsize == 32
    assert _run_sets(fmmerge_driver, LAYOUTS[layout], list(FM_SETS)) == 12


def _fan(n: int) -> list[str]:
    """read 0 and n reads that start with its last 20 bases and go on with 30 bases of their own: n irreducible blocks on its
    sense end"""
    tails, k = [], 0
    while len(tails) < n:
        t = _rand(0x0F50 + k, 30)
        k += 1
        if t not in tails:
            tails.append(t)
    return [GENOME[0:50]] + [GENOME[30:50] + t for t in tails]


REFUSED = {
    # (reads, the refusal's kind as fm_fmmerge.h numbers it + 1, the read it names)
    "identical_reads": (PATH + [PATH[5]], 2, 4),                  # read 4's block on its sense end holds reads 5 and 26
    "substring_read": (PATH + [GENOME[105:135]], 2, 26),
    # more final blocks than a read's output holds (kOvOutCap = 256): its overlap status is the overflow, it has no blocks, and
    # it must not become a singleton
    "overflow": (_fan(300), 1, 0),
}


def test_the_driver_refuses_what_the_entry_refuses(fmmerge_driver):
    for name, (reads, kind, read) in REFUSED.items():
        for wide in LAYOUTS.values():
            assert run_fmmerge_driver(fmmerge_driver, reads, M, wide) == (kind, read), name
    # the index of other reads: the orders lead elsewhere
    other = Index(PATH[::-1])
    assert run_fmmerge_driver(fmmerge_driver, PATH, M, 0, other)[0] == 3


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program, CPU only: the named sets, both layouts; every array of the state is an allocation of its own"""
    exe = _build(tmp_path / "fmmerge_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for wide in LAYOUTS.values():
        _run_sets(exe, wide, NAMED)


# ---- the ABI, the kernels, the command line --------------------------------------------------------------------------------------
def _const(name: str) -> int:
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", (REPO / "longreadselfcorrect_amd/csrc/fm_fmmerge.h").read_text())
    assert m, name
    return int(m.group(1))


def launches(n: int, chunk: int = 32768) -> int:
    """what lrsc.h states: 3 per chunk, 2 R + 9 with R = ceil(log2(2 n))"""
    return 3 * -(-n // chunk) + 2 * (2 * n - 1).bit_length() + 9


def test_fmmerge_entry_is_declared_exported_and_bound(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    header = (REPO / "include/lrsc.h").read_text()
    assert "lrsc_fmmerge" in capi.declared_symbols() and " T lrsc_fmmerge\n" in exported
    assert "typedef struct lrsc_fmmerge_read { uint32_t seq, flags; uint64_t offset; } lrsc_fmmerge_read;" in header
    assert "typedef struct lrsc_fmmerge_seq { uint64_t offset, length; uint32_t n_reads, root, circular, pad; } lrsc_fmmerge_seq;" in header
    assert ("int lrsc_fmmerge(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap, lrsc_fmmerge_read* per_read,\n"
            "                 lrsc_fmmerge_seq* seqs, uint32_t* n_seqs_out, char* bases, uint64_t bases_cap, uint64_t* n_bases_out);") in header
    for cited in ("StriDe/fm-merge.cpp", "FMMergeProcess.cpp:30-230", "checkCandidate", "Bigraph.cpp:162-220", "Vertex.cpp:30-75", "3 * chunks + 2 * R + 9",
                  "lowest-numbered", "LRSC_FMMERGE_DROPPED", "requires `stride filter`"):
        assert cited in header, cited
    assert "#define LRSC_ABI_VERSION 2\n" in header and api.lib.lrsc_abi_version() == 2
    assert capi.FMMERGE_READ_DTYPE == FMMERGE_READ_DTYPE and capi.FMMERGE_SEQ_DTYPE == FMMERGE_SEQ_DTYPE and callable(capi.Ctx.fmmerge)
    assert launches(26) == 3 + 2 * 6 + 9 and launches(40000) == 6 + 2 * 17 + 9 and launches(1) == 3 + 2 + 9
    design = (REPO / "DESIGN.md").read_text()
    assert "fm-merge" in design and "lowest-numbered" in design


def test_fmmerge_kernels_build_for_gfx950_without_scratch(tmp_path):
    seen = _kernels(_kernel_notes(tmp_path, "fm_fmmerge"), r"fmmerge_[a-z_]+_kernel")
    assert sorted(seen) == ["fmmerge_assemble_kernel", "fmmerge_cut_kernel", "fmmerge_finish_kernel", "fmmerge_init_kernel", "fmmerge_links_kernel", "fmmerge_place_kernel",
                            "fmmerge_round_kernel", "fmmerge_scan_apply_kernel", "fmmerge_scan_tiles_kernel", "fmmerge_scan_top_kernel"], seen
    waves, threads = _const("kFmmWavesPerSimd"), _const("kFmmThreads")
    assert waves >= 8 and threads % 64 == 0
    for kernel in seen.values():
        for name, md in kernel:
            assert md["max_flat_workgroup_size"] == threads
            assert md["vgpr_count"] <= 512 // waves // 8 * 8, (name, md)
            assert md["group_segment_fixed_size"] * (waves * 4 // (threads // 64)) <= 160 * 1024, (name, md)


FMMERGE_USAGE = "Usage: StriDe fm-merge [OPTION] ... READSFILE"


def test_stride_fm_merge_usage(api, tmp_path):
    run = lambda *args: subprocess.run([str(STRIDE), "fm-merge", *args], cwd=tmp_path, capture_output=True, text=True, input="")
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith(FMMERGE_USAGE) and r.stderr == ""
    for option in ("--min-overlap=LEN", "--prefix=PREFIX", "--outfile=FILE", "--threads=NUM", "--verbose", "--device=N", "--build-index", "--load-on-device"):
        assert option in r.stdout, option
    assert "Merge unambiguously sequences from the READSFILE using the FM-index." in r.stdout and "rmdup" in r.stdout
    r = run("--version")
    assert r.returncode == 0 and "fm-merge" in r.stdout
    for args, message in (([], "fm-merge: missing arguments"), (["a.fa", "b.fa"], "fm-merge: too many arguments"), (["-t", "0", "a.fa"], "fm-merge: invalid number of threads: 0")):
        r = run(*args)
        assert r.returncode == 1 and message in r.stderr and FMMERGE_USAGE in r.stdout, (args, r.stdout, r.stderr)
    r = subprocess.run([str(STRIDE), "help"], cwd=tmp_path, capture_output=True, text=True, input="")
    assert "fm-merge" in r.stdout + r.stderr
