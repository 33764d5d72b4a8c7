"""lrsc_fmwalk_merge (fm_fmwalk.hip) and `stride fmwalk -a merge` against the plain restatement of test_fmwalk_host.
Every comparison is exact."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from .test_fmwalk_host import FW_DTYPE, FW_SETS, GENOME, INSERT, K, M_MIN, NAMED, X, ends, fw_case, index_case, index_reads, pairs_input, plain_fmwalk_merge, \
    result_dicts, set_options
from .test_gpu_index_build import STRIDE

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG, LRSC_ERR_UNSUPPORTED = -3, -7


def _force(monkeypatch, wide):
    """LRSC_FORCE_WIDE is read per call: set or unset before each index is made"""
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    else:
        monkeypatch.delenv("LRSC_FORCE_WIDE", raising=False)


def _merge(ctx, pairs, s) -> list[dict]:
    """-> what the yardstick gives, per pair"""
    bases, off = pairs_input(pairs)
    merged, res = ctx.fmwalk_merge(bases, off, s["k"], s["x"], s["m"], s["max_overlap"], s["insert"], s["leaves"])
    for q, row in zip(res, merged):                               # nothing is written beyond the merged string
        assert (row[int(q["length"]) if q["merged"] else 0:] == 0).all()
    return result_dicts(res, [row.tobytes().decode("latin-1") for row in merged])


def _context(api):
    from oracle.oracle_py import pack_reads

    index = api.index_build(*pack_reads(index_case()[0]), 0)
    return index, index.ctx(api.params_default(5, 90), 0)


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_every_set_equals_the_yardstick(api, monkeypatch, wide):
    from longreadselfcorrect_amd import capi

    assert capi.FMWALK_DTYPE == FW_DTYPE
    _force(monkeypatch, wide)
    index, ctx = _context(api)
    assert index.info().block_symbols == (128 if wide else 192)
    for name in FW_SETS:
        s, want, _ = fw_case(name)
        ctx.stats_reset()
        got = _merge(ctx, s["pairs"], s)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, i)
        stats = ctx.stats(capi.K_FIND)
        assert len(got) == len(want) and stats.launches == 2, name      # the trim and the walks
        assert stats.rank_queries > 0 and stats.rank_queries // 2 <= stats.block_loads <= stats.rank_queries, name
    ctx.close()
    index.close()


@pytest.fixture(scope="module")
def shuffled():
    """the pairs of every set with the default options, shuffled, and what the yardstick makes of them"""
    pairs, want, options = [], [], None
    for name in FW_SETS:
        s, w, _ = fw_case(name)
        if (s["max_overlap"], s["insert"], s["leaves"]) == (-1, INSERT, 32):
            pairs += s["pairs"]
            want += w
            options = s
    order = np.random.default_rng(11).permutation(len(pairs))
    assert len(pairs) >= 110
    return [pairs[i] for i in order], [want[i] for i in order], options


@pytest.mark.parametrize("size", [1, 7, 10 ** 6], ids=["batches_of_1", "batches_of_7", "one_batch"])
def test_shuffled_pairs_whatever_the_batches(api, shuffled, size):
    pairs, want, options = shuffled
    if size == 1:                                                 # a call a pair: a third of them says as much
        pairs, want = pairs[::3], want[::3]
    index, ctx = _context(api)
    got = []
    for i in range(0, len(pairs), size):
        got += _merge(ctx, pairs[i: i + size], options)
    assert got == want
    ctx.close()
    index.close()


def test_refused_arguments_leave_the_outputs_untouched(api):
    from longreadselfcorrect_amd import capi

    s, want, _ = fw_case("unique_path")
    index, ctx = _context(api)
    good = s["pairs"][:2]
    ok = (K, X, M_MIN, -1, INSERT, 32)

    def call(pairs, params, stride=INSERT + 1, n_pairs=None):
        bases, off = pairs_input(pairs)
        merged = np.full(len(pairs) * max(stride, 1), 0x5A, dtype=np.uint8)
        out = np.full(len(pairs) * 12, 0x5EED, dtype=np.uint32)
        p = np.array(params, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        st = api.lib.lrsc_fmwalk_merge(ctx.h, ptr(bases), ptr(off), len(pairs) if n_pairs is None else n_pairs, ptr(p), ptr(merged), stride, ptr(out))
        return st, merged, out

    replaced = lambda i, v: tuple(v if j == i else x for j, x in enumerate(ok))
    refused = [(good, replaced(i, v), INSERT + 1, LRSC_ERR_ARG) for i in range(6) for v in (0, -2)]
    refused += [(good, replaced(2, 1), INSERT + 1, LRSC_ERR_ARG), (good, ok, INSERT, LRSC_ERR_ARG), (good, replaced(4, 10), M_MIN - 1, LRSC_ERR_ARG),
                ([good[0], (good[1][0], "ACGTNACGT" * 4)], ok, INSERT + 1, LRSC_ERR_ARG), ([good[0], ("", good[1][1])], ok, INSERT + 1, LRSC_ERR_ARG),
                (good, replaced(5, 65), INSERT + 1, LRSC_ERR_UNSUPPORTED), (good, replaced(4, 2001), 2002, LRSC_ERR_UNSUPPORTED),
                (good, replaced(2, 256), INSERT + 1, LRSC_ERR_UNSUPPORTED), (good, replaced(0, 256), INSERT + 1, LRSC_ERR_UNSUPPORTED)]
    for pairs, params, stride, status in refused:
        st, merged, out = call(pairs, params, stride)
        assert st == status, (params, stride, st)
        assert (merged == 0x5A).all() and (out == 0x5EED).all()
    st, merged, out = call(good, ok, n_pairs=0)                  # a valid call that does nothing
    assert st == 0 and (merged == 0x5A).all() and (out == 0x5EED).all()
    assert ctx.stats(capi.K_FIND).launches == 0
    st, merged, out = call(good, replaced(3, 40))                # -M given: nothing of an unmerged pair's row is written
    assert st == 0 and not (out == 0x5EED).all()
    assert _merge(ctx, s["pairs"], s) == want, "after the refused calls"
    ctx.close()
    index.close()


# ---- `stride fmwalk -a merge` end to end ----------------------------------------------------------------------------------------
def _run(args, cwd, ok=True):
    r = subprocess.run([str(STRIDE)] + args, cwd=cwd, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _count_lines(stdout):
    return [l for l in stdout.split("\n") if l.startswith("Reads ")]


def _records(pairs, quals: bool) -> str:
    out = ""
    for i, (r1, r2) in enumerate(pairs):
        for j, r in enumerate((r1, r2)):
            out += f"@frag{i}/{j + 1}\n{r}\n+\n{'I' * len(r)}\n" if quals else f">frag{i}/{j + 1} extra\n{r}\n"
    return out


def _expected(pairs, c=None, **options):
    """the output file and the three count lines; c: the counts of another index than the sets'"""
    c = c or index_case()[1]
    text, merged = "", 0
    for i, (r1, r2) in enumerate(pairs):
        w = plain_fmwalk_merge(c, r1, r2, **options) if set(r1 + r2) <= set("ACGT") else dict(merged=0)
        if w["merged"]:
            text += f">frag{i}\n{w['seq']}\n"
            merged += 1
    return text, ["Reads are kmerized: 0", f"Reads are merged : {merged}", f"Reads failed to kmerize or merge: {2 * (len(pairs) - merged)}"]


@pytest.fixture(scope="module")
def fmwalk_dir(api, tmp_path_factory):
    """the index reads as reads.fa with their index by `stride index`; the pairs of the named sets with the default options as FASTA
    and as FASTQ"""
    d = tmp_path_factory.mktemp("fmwalk")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(index_reads())))
    _run(["index", "-p", "reads", "reads.fa"], d)
    pairs = [p for name in NAMED for p in fw_case(name)[0]["pairs"] if set_options(fw_case(name)[0]) == set_options(fw_case("unique_path")[0])]
    pairs = [p for p in pairs if p[0] and p[1]]
    assert len(pairs) >= 12
    (d / "pairs.fa").write_text(_records(pairs, False))
    (d / "pairs.fq").write_text(_records(pairs, True))
    return d, pairs


OPTIONS = ["-a", "merge", "-k", str(K), "-m", str(M_MIN), "-x", str(X), "-I", str(INSERT)]


@pytest.mark.parametrize("ext", ["fa", "fq"])
def test_stride_fmwalk_equals_the_yardstick_s_records(fmwalk_dir, ext):
    d, pairs = fmwalk_dir
    text, lines = _expected(pairs)
    assert text.count(">") >= 6 and lines[2] != "Reads failed to kmerize or merge: 0"
    r = _run(["fmwalk", *OPTIONS, "-p", "reads", "-o", f"plain_{ext}.out", f"pairs.{ext}"], d)
    assert (d / f"plain_{ext}.out").read_text() == text
    assert _count_lines(r.stdout) == lines
    assert "Median kmer frequency" not in r.stdout and not (d / "kmerized.fa").exists()


def test_stride_fmwalk_build_index_options_and_default_name(fmwalk_dir):
    d, pairs = fmwalk_dir
    sub = d / "built"
    sub.mkdir()
    # the index of the pairs' own reads is another index, where -x 1 finds paths: the walks are those of the yardstick over it
    from .test_fmwalk_host import Counts

    own = [p for p in pairs if len(p[0]) == 50 == len(p[1])] * 2
    (d / "own.fa").write_text(_records(own, False))
    text, lines = _expected(own, Counts([r for p in own for r in p]), x=1)
    r = _run(["fmwalk", "-a", "merge", "-k", str(K), "-m", str(M_MIN), "-x", "1", "-I", str(INSERT), "--build-index", "--device=0", "-t", "4", "../own.fa"], sub)
    assert (sub / "own.merge.fa").read_text() == text and _count_lines(r.stdout) == lines and lines[1] != "Reads are merged : 0"
    text, lines = _expected(pairs, max_overlap=30, leaves_max=2)
    r = _run(["fmwalk", *OPTIONS, "-L", "2", "--max-overlap", "30", "-p", "../reads", "../pairs.fa"], sub)
    assert (sub / "pairs.merge.fa").read_text() == text and _count_lines(r.stdout) == lines
    r = _run(["fmwalk", *OPTIONS, "-L", "2", "-M", "30", "--load-on-device", "-p", "../reads", "-o", "m.out", "../pairs.fa"], sub)
    assert (sub / "m.out").read_text() == text and _count_lines(r.stdout) == lines


def test_stride_fmwalk_odd_records_and_other_bases(fmwalk_dir):
    d, pairs = fmwalk_dir
    (d / "odd.fa").write_text(_records(pairs[:3], False) + f">last/1\n{pairs[3][0]}\n")
    r = _run(["fmwalk", *OPTIONS, "-p", "reads", "odd.fa"], d, ok=False)
    assert r.returncode == 1 and "FMIndexWalk: odd.fa holds an odd number of records" in r.stderr and not (d / "odd.merge.fa").exists()
    r1, r2 = ends(GENOME, 100, 100)
    with_n = [pairs[0], (r1[:25] + "N" + r1[26:], r2), pairs[1], (r1, r2)]
    (d / "with_n.fa").write_text(_records(with_n, False))
    text, lines = _expected(with_n)
    r = _run(["fmwalk", *OPTIONS, "-p", "reads", "with_n.fa"], d)
    assert (d / "with_n.merge.fa").read_text() == text and ">frag1\n" not in text and ">frag3\n" in text
    assert _count_lines(r.stdout) == lines and lines[2] == f"Reads failed to kmerize or merge: {2 * (4 - text.count('>'))}"
    assert r.stderr.count("Warning: pair") == 1
