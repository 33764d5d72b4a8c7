"""lrsc_fmmerge (fm_fmmerge.hip) and `stride fm-merge` against the plain restatement of test_fmmerge_host, and on one long chain
set whose sequences are known by construction.  Every comparison is exact.

What lrsc.h calls refused is of two kinds.  A wrong read count and the argument errors of lrsc_overlap_exact are seen before the
first launch: nothing is launched.  Duplicates, substring reads, an index of other reads and a read whose overlap status is the
overflow are seen in the reads' final blocks, so after the three launches of a chunk: the outputs are untouched, the call ends
with the first chunk that shows one, and no launch of the chain phase is made.
"""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from .test_fmmerge_host import (DROPPED, FM_SETS, FMMERGE_READ_DTYPE, FMMERGE_SEQ_DTYPE, REFUSED, REVERSED, check_invariant, fm_case, launches, merged_dicts)
from .test_index_filter_host import revcomp
from .test_overlap_host import M, PATH, STRIDE, reads_input

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG, LRSC_ERR_CAPACITY, LRSC_ERR_UNSUPPORTED, LRSC_ERR_LIMIT = -3, -6, -7, -8


def _force(monkeypatch, wide):
    """LRSC_FORCE_WIDE is read per call: set or unset before each index is made"""
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    else:
        monkeypatch.delenv("LRSC_FORCE_WIDE", raising=False)


def _context(api, reads):
    from oracle.oracle_py import pack_reads

    index = api.index_build(*pack_reads(reads), 0)
    return index, index.ctx(api.params_default(5, 90), 0)


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_every_set_equals_the_yardstick(api, monkeypatch, wide):
    from longreadselfcorrect_amd import capi

    assert capi.FMMERGE_READ_DTYPE == FMMERGE_READ_DTYPE and capi.FMMERGE_SEQ_DTYPE == FMMERGE_SEQ_DTYPE
    _force(monkeypatch, wide)
    for name in FM_SETS:
        c = fm_case(name)
        index, ctx = _context(api, c["reads"])
        assert index.info().block_symbols == (128 if wide else 192)
        got = merged_dicts(*ctx.fmmerge(*reads_input(c["reads"]), c["m"]))
        assert got["seqs"] == c["merged"]["seqs"], name
        assert got["per_read"] == c["merged"]["per_read"], name
        assert got["fasta"] == c["merged"]["fasta"], name
        assert ctx.stats(capi.K_FIND).launches == launches(len(c["reads"])), name
        ctx.close()
        index.close()


# ---- the long chains -------------------------------------------------------------------------------------------------------------
def _kmers(codes: np.ndarray, k: int) -> np.ndarray:
    v = np.zeros(codes.size - k + 1, dtype=np.uint64)
    for j in range(k):
        v = v * np.uint64(4) + codes[j: codes.size - k + 1 + j].astype(np.uint64)
    return v


def test_long_chains_across_the_chunks(api):
    """40 000 reads of 50 bases at step 10 over a random genome, each on a random strand, in shuffled file order, m = 30: a read
    overlaps its neighbour by 40 and the next but one by 30, so every read has one irreducible edge per end.  Where three
    consecutive reads are taken out, the reads on both sides share 10 bases and the chain ends.  The sequences are the genome's
    pieces, each on the strand of its lowest-numbered read, in the order of those reads."""
    from longreadselfcorrect_amd import capi

    rng = np.random.default_rng(0x0F40)
    n_pos, m = 40000, 30
    codes = rng.integers(0, 4, size=10 * (n_pos - 1) + 50, dtype=np.uint8)
    both = np.concatenate([_kmers(codes, m), _kmers((3 - codes)[::-1], m)])
    assert np.unique(both).size == both.size, "a 30-mer of the genome repeats"
    genome = "".join("ACGT"[c] for c in codes)
    holes = [137, 9000, 20001, 32766, 39000]                       # the first of three positions taken out
    gone = {h + i for h in holes for i in range(3)}
    kept = [p for p in range(n_pos) if p not in gone]
    pieces, start = [], 0
    for h in holes + [n_pos]:
        pieces.append((start, h - 1))                             # positions of the piece's first and last read
        start = h + 3
    order = rng.permutation(len(kept))
    flip = rng.integers(0, 2, size=len(kept))
    position = [kept[i] for i in order]
    reads = [revcomp(genome[10 * p: 10 * p + 50]) if f else genome[10 * p: 10 * p + 50] for p, f in zip(position, flip)]
    n = len(reads)
    assert n == n_pos - 15 and n > 32768
    number = {p: i for i, p in enumerate(position)}
    want = []
    for first, last in pieces:
        members = [number[p] for p in range(first, last + 1)]
        root = min(members)
        text = genome[10 * first: 10 * last + 50]
        want.append((root, dict(bases=revcomp(text) if flip[root] else text, n_reads=len(members), root=root, circular=0)))
    want = [w for _, w in sorted(want, key=lambda x: x[0])]
    assert max(w["n_reads"] for w in want) > 2 ** 13                # more than 13 rounds of doubling are needed

    index, ctx = _context(api, reads)
    got = merged_dicts(*ctx.fmmerge(*reads_input(reads), m))
    assert [(s["root"], s["n_reads"], len(s["bases"])) for s in got["seqs"]] == [(s["root"], s["n_reads"], len(s["bases"])) for s in want]
    assert got["seqs"] == want
    assert not any(f & DROPPED for _, f, _ in got["per_read"])
    for i, (seq, flags, offset) in enumerate(got["per_read"]):
        assert bool(flags & REVERSED) == (flip[i] != flip[want[seq]["root"]]), i
    check_invariant(reads, got["per_read"], got["seqs"])
    assert ctx.stats(capi.K_FIND).launches == launches(n) == 3 * 2 + 2 * 17 + 9
    ctx.close()
    index.close()
    # a duplicate in the first of the two chunks: refused after that chunk's three launches, the second is not run
    again = [reads[0], reads[0]] + reads[2:]
    index, ctx = _context(api, again)
    st, untouched, used, _ = _raw(api, ctx, again, m, 64)
    assert st == LRSC_ERR_ARG and untouched and used == 0x7E57 and "requires `stride filter` first" in api.lib.lrsc_last_error().decode()
    assert ctx.stats(capi.K_FIND).launches == 3
    ctx.close()
    index.close()


# ---- what is refused -------------------------------------------------------------------------------------------------------------
def _raw(api, ctx, reads, m, cap, n_reads=None):
    bases, off = reads_input(reads)
    per_read = np.full(len(reads) * 4, 0x5EED, dtype=np.uint32)
    seqs = np.full(len(reads) * 8, 0x5EED, dtype=np.uint32)
    out = np.full(max(cap, 1), 0x5A, dtype=np.uint8)
    counts = np.full(1, 0x7E57, dtype=np.uint32)
    used = np.full(1, 0x7E57, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = api.lib.lrsc_fmmerge(ctx.h, ptr(bases), ptr(off), len(reads) if n_reads is None else n_reads, m, ptr(per_read), ptr(seqs), ptr(counts), ptr(out), cap, ptr(used))
    untouched = bool((per_read == 0x5EED).all() and (seqs == 0x5EED).all() and (out == 0x5A).all() and counts[0] == 0x7E57)
    return st, untouched, int(used[0]), (per_read, seqs, out, int(counts[0]))


def test_refused_input_leaves_the_outputs_untouched(api):
    from longreadselfcorrect_amd import capi

    c = fm_case("unique_path")
    index, ctx = _context(api, c["reads"])
    good = list(c["reads"])
    swap = lambda i, r: good[:i] + [r] + good[i + 1:]
    refused = [(good, 1, LRSC_ERR_ARG), (good, 0, LRSC_ERR_ARG), (good, -5, LRSC_ERR_ARG), (swap(2, "ACGTNACGT" * 4), 20, LRSC_ERR_ARG), (swap(3, ""), 20, LRSC_ERR_ARG),
               (good, 2001, LRSC_ERR_UNSUPPORTED),
               (swap(25, "ACGT" * 501), 20, LRSC_ERR_UNSUPPORTED),
               # another number of reads than the index holds
               (good[:20], 20, LRSC_ERR_ARG), (good + [good[0]], 20, LRSC_ERR_ARG)]
    for reads, m, status in refused:
        st, untouched, used, _ = _raw(api, ctx, reads, m, 4096)
        assert st == status and untouched and used == 0x7E57, (m, len(reads), st)
    st, untouched, used, _ = _raw(api, ctx, good, 20, 4096, n_reads=0)
    assert st == LRSC_ERR_ARG and untouched and used == 0x7E57       # no reads, but the index holds 26
    assert ctx.stats(capi.K_FIND).launches == 0
    # an index of these reads in another order: a read's own row is not in its interval
    st, untouched, used, _ = _raw(api, ctx, good[::-1], 20, 4096)
    assert st == LRSC_ERR_ARG and untouched and used == 0x7E57 and ctx.stats(capi.K_FIND).launches == 3
    got = merged_dicts(*ctx.fmmerge(*reads_input(good), c["m"]))
    assert got["seqs"] == c["merged"]["seqs"] and got["per_read"] == c["merged"]["per_read"], "after the refused calls"
    ctx.close()
    index.close()
    # duplicates and substring reads: `stride filter` first; a read whose overlap overflowed: the limit; each with the first read
    # that shows it, after the three launches of the one chunk
    said = {1: (LRSC_ERR_LIMIT, "outgrow the kernel's workspace"), 2: (LRSC_ERR_ARG, "fm-merge requires `stride filter` first")}
    for name, (reads, kind, read) in REFUSED.items():
        index, ctx = _context(api, reads)
        st, untouched, used, _ = _raw(api, ctx, reads, M, 65536)
        assert st == said[kind][0] and untouched and used == 0x7E57, (name, st)
        message = api.lib.lrsc_last_error().decode()
        assert said[kind][1] in message and f"read {read} " in message, (name, message)
        assert ctx.stats(capi.K_FIND).launches == 3
        ctx.close()
        index.close()
    # n_reads == 0 is valid only for an index without reads, which index_build does not make: with these indexes it is the wrong
    # count above, and launches nothing either way


def test_a_bases_cap_that_is_too_small_says_what_is_needed(api):
    c = fm_case("branch_at_the_snp")
    index, ctx = _context(api, c["reads"])
    need = sum(len(s["bases"]) for s in c["merged"]["seqs"])
    for cap in (0, need - 1):
        st, untouched, used, _ = _raw(api, ctx, c["reads"], c["m"], cap)
        assert st == LRSC_ERR_CAPACITY and used == need and untouched
    st, untouched, used, (per_read, seqs, out, n_seqs) = _raw(api, ctx, c["reads"], c["m"], need)
    assert st == 0 and used == need and n_seqs == len(c["merged"]["seqs"])
    got = merged_dicts(per_read.view(FMMERGE_READ_DTYPE), seqs.view(FMMERGE_SEQ_DTYPE)[:n_seqs], out[:need].tobytes())
    assert got["seqs"] == c["merged"]["seqs"] and got["per_read"] == c["merged"]["per_read"]
    ctx.close()
    index.close()


# ---- `stride fm-merge` end to end ---------------------------------------------------------------------------------------------------
def _run(args, cwd, ok=True):
    r = subprocess.run([str(STRIDE)] + args, cwd=cwd, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _summary(c) -> str:
    seqs = c["merged"]["seqs"]
    total = sum(len(s["bases"]) for s in seqs)
    return ("[sga fm-merge] Merged %d reads into %d sequences\n[sga fm-merge] Reduction factor: %f\n[sga fm-merge] Mean merged size: %f\n"
            % (len(c["reads"]), len(seqs), len(c["reads"]) / len(seqs), total / len(seqs)))


@pytest.mark.parametrize("name", ["alternate_strands", "branch_at_the_snp", "cycle", "lasso", "random"])
def test_stride_fm_merge_writes_the_yardstick_s_fasta(api, tmp_path, name):
    """after `stride index` with -p, with --build-index, and with --load-on-device: the same file, byte for byte"""
    c = fm_case(name)
    (tmp_path / f"{name}.fa").write_text("".join(f">{n} extra words\n{r}\n" for n, r in zip(c["names"], c["reads"])))
    _run(["index", "-p", "idx", f"{name}.fa"], tmp_path)
    m = ["-m", str(c["m"])]
    r = _run(["fm-merge", *m, "-p", "idx", f"{name}.fa"], tmp_path)
    assert (tmp_path / "idx.merged.fa").read_text() == c["merged"]["fasta"] and r.stdout.endswith(_summary(c)), r.stdout
    assert "<Simplify>" not in r.stdout
    for extra in (["--build-index", "-t", "4"], ["--load-on-device", "-p", "idx", "--device=0", "-v"]):
        r = _run(["fm-merge", *m, *extra, "-o", "named.fa", f"{name}.fa"], tmp_path)
        assert (tmp_path / "named.fa").read_text() == c["merged"]["fasta"] and r.stdout.endswith(_summary(c))
        (tmp_path / "named.fa").unlink()


def test_stride_fm_merge_another_index_and_unfiltered_reads(api, tmp_path):
    c = fm_case("unique_path")
    (tmp_path / "clean.fa").write_text("".join(f">{n}\n{r}\n" for n, r in zip(c["names"], c["reads"])))
    _run(["index", "-p", "clean", "clean.fa"], tmp_path)
    (tmp_path / "fewer.fa").write_text("".join(f">{n}\n{r}\n" for n, r in list(zip(c["names"], c["reads"]))[:20]))
    r = _run(["fm-merge", "-m", str(c["m"]), "-p", "clean", "fewer.fa"], tmp_path, ok=False)
    assert r.returncode == 1 and "fm-merge: fewer.fa holds 20 reads, the index 26: the index is not that of these reads" in r.stderr
    assert not (tmp_path / "clean.merged.fa").exists()
    dup = PATH + [PATH[5]]
    (tmp_path / "dup.fa").write_text("".join(f">d{i}\n{r}\n" for i, r in enumerate(dup)))
    r = _run(["fm-merge", "-m", str(M), "--build-index", "dup.fa"], tmp_path, ok=False)
    assert r.returncode == 1 and "fm-merge requires `stride filter` first: read 4 " in r.stderr and not (tmp_path / "dup.merged.fa").exists()
