"""wp_begin in two passes (`-m gpu`): pass 1 builds every walk's tables without the sort and lists the interval lists in which an
idmer code repeats, pass 2 (wp_begin_sort_kernel) runs the exact introsort for those alone.  The whole per-read path is held
against the CPU oracle on the bench-like set (few lists sort) and on the repeat-rich set (many more do), over both rank-block layouts;
the differential cases run one batch with `LRSC_WP_BEGIN_SORT=1` (every list sorted: the behaviour before) and by the default rule
and require identical corrected strings, per-read counters, and rank-query / block-load counts of the extension stage.
lrsc_extend_walks (walk_extend_kernel inlines the same Walk::begin_static) is held against the oracle walk by walk."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from longreadselfcorrect_amd.capi import K_EXTEND
from tests.test_gpu_fm import _fasta, _walk_descs

pytestmark = pytest.mark.gpu

NAMES = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
         "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")
N_REPEAT = 30            # reads of the repeat-rich set: some 250 FM walks and 150 DP answers; the oracle's DP stage sets the test's time


@pytest.fixture(scope="module")
def indexes(api, small_ds, repeat_ds):
    idx = {}
    idx["small"] = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    os.environ["LRSC_FORCE_WIDE"] = "1"
    try:
        idx["small-wide"] = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    finally:
        del os.environ["LRSC_FORCE_WIDE"]
    idx["repeat"] = api.index_open(repeat_ds.prefix + ".bwt", repeat_ds.prefix + ".rbwt")
    for i in idx.values():
        i.upload(0)
    assert idx["small"].info().block_symbols != 128 and idx["small-wide"].info().block_symbols == 128
    yield idx
    for i in idx.values():
        i.close()


def _batch(which, small_ds, repeat_ds):
    ds = repeat_ds if which == "repeat" else small_ds
    n = N_REPEAT if which == "repeat" else len(ds.off) - 1
    off = ds.off[: n + 1].copy()
    return ds, ds.bases[: int(off[-1])], off, ds.reads[:n]


@pytest.fixture(scope="module")
def wanted(api, oracle, small_ds, repeat_ds):
    """The oracle's answer per (set, nodp), computed once and shared: (correct.fa, discard.fa, counters)."""
    cache = {}

    def get(which, nodp):
        key = ("repeat" if which == "repeat" else "small", nodp)
        if key not in cache:
            ds, bases, off, _ = _batch(which, small_ds, repeat_ds)
            p = api.params_default(5, 90)
            p.no_dp = nodp
            ob, orb = oracle.bwt_load(ds.prefix + ".bwt"), oracle.bwt_load(ds.prefix + ".rbwt")
            w = oracle.correct_reads(ob, orb, p, bases, off)
            cache[key] = (w.correct_fa, w.discard_fa, np.array(w.counters, dtype=np.int64).copy())
            w.close(); ob.close(); orb.close()
        return cache[key]

    return get


def _run(api, index, which, nodp, small_ds, repeat_ds):
    _, bases, off, reads = _batch(which, small_ds, repeat_ds)
    p = api.params_default(5, 90)
    p.no_dp = nodp
    ctx = index.ctx(p, 0)
    ctx.stats_reset()
    results, pieces = ctx.correct_reads(bases, off)
    st = ctx.stats(K_EXTEND)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, reads, p.split)
    got = np.array([[getattr(r, n) for n in NAMES] for r in results], dtype=np.int64)
    return cfa, dfa, got, (int(st.launches), int(st.rank_queries), int(st.block_loads))


def _against_oracle(run, want, min_fm, min_dp):
    cfa, dfa, got, _ = run
    assert cfa == want[0]
    assert dfa == want[1]
    np.testing.assert_array_equal(got, want[2])
    assert got[:, 7].sum() > min_fm and (got[:, 4].sum() + got[:, 5].sum()) > 0      # many FM walks, some failures
    assert got[:, 8].sum() >= min_dp


@pytest.mark.parametrize("which", ["small", "small-wide"])
@pytest.mark.parametrize("nodp", [0, 1])
def test_small_set_whole_path(api, indexes, wanted, small_ds, repeat_ds, which, nodp, monkeypatch):
    monkeypatch.delenv("LRSC_WP_BEGIN_SORT", raising=False)
    _against_oracle(_run(api, indexes[which], which, nodp, small_ds, repeat_ds), wanted(which, nodp), 300, 0 if nodp else 20)


@pytest.mark.parametrize("nodp", [0, 1])
def test_repeat_set_whole_path(api, indexes, wanted, small_ds, repeat_ds, nodp, monkeypatch):
    """Repeat-rich reads (a 75-copy 60-bp unit, a 6-copy 350-bp segment): lists with and without a repeated code occur (test_both_classes_of_lists_occur)."""
    monkeypatch.delenv("LRSC_WP_BEGIN_SORT", raising=False)
    _against_oracle(_run(api, indexes["repeat"], "repeat", nodp, small_ds, repeat_ds), wanted("repeat", nodp), 100, 0 if nodp else 5)


def test_few_lanes_whole_path(api, indexes, wanted, small_ds, repeat_ds, monkeypatch):
    """LRSC_WP_LANES=256: the extension launches refill their lanes from the queue many times, and rounds >= 1 re-use the tables'
    arena for the re-queued walks."""
    monkeypatch.delenv("LRSC_WP_BEGIN_SORT", raising=False)
    monkeypatch.setenv("LRSC_WP_LANES", "256")
    _against_oracle(_run(api, indexes["small"], "small", 0, small_ds, repeat_ds), wanted("small", 0), 300, 20)


@pytest.mark.parametrize("which", ["small", "repeat"])
@pytest.mark.parametrize("nodp", [0, 1])
def test_sort_every_list_and_sort_by_rule_agree(api, indexes, small_ds, repeat_ds, which, nodp, monkeypatch):
    monkeypatch.setenv("LRSC_WP_BEGIN_SORT", "1")
    a = _run(api, indexes[which], which, nodp, small_ds, repeat_ds)
    monkeypatch.delenv("LRSC_WP_BEGIN_SORT")
    b = _run(api, indexes[which], which, nodp, small_ds, repeat_ds)
    assert a[0] == b[0] and a[1] == b[1]
    np.testing.assert_array_equal(a[2], b[2])
    assert a[3] == b[3] and a[3][1] > 0                      # launches, rank queries, block loads of LRSC_K_EXTEND


def test_both_classes_of_lists_occur(api, indexes, small_ds, repeat_ds, monkeypatch, capfd):
    """The decision itself, from the per-round profile line (LRSC_CORRECT_PROFILE): on the repeat-rich reads pass 1 finds lists with
    a repeated code (they go to pass 2) and lists without one (chained unsorted); with LRSC_WP_BEGIN_SORT=1 it looks for none."""
    monkeypatch.setenv("LRSC_CORRECT_PROFILE", "1")
    monkeypatch.delenv("LRSC_WP_BEGIN_SORT", raising=False)
    capfd.readouterr()
    _run(api, indexes["repeat"], "repeat", 1, small_ds, repeat_ds)
    err = capfd.readouterr().err
    m = re.search(r"round 0: wp_begin (\d+) interval lists, (\d+) with a repeated code .*entries (\d+) in the lists without one, (\d+) in those with one", err)
    assert m, err[-2000:]
    lists, rep, e_plain, e_rep = map(int, m.groups())
    assert 0 < rep < lists and e_plain > 0 and e_rep > 0
    monkeypatch.setenv("LRSC_WP_BEGIN_SORT", "1")
    _run(api, indexes["repeat"], "repeat", 1, small_ds, repeat_ds)
    err = capfd.readouterr().err
    m = re.search(r"round 0: wp_begin (\d+) interval lists, (\d+) entries, every list sorted", err)
    assert m and int(m.group(1)) == lists and int(m.group(2)) == e_plain + e_rep, err[-2000:]


def test_extend_walks_match_oracle(api, indexes, oracle, small_ds):
    """The 40-read walk set of test_gpu_fm.py through lrsc_extend_walks: return code, merged sequence and steps of every walk."""
    p = api.params_default(5, 90)
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    n_reads = 40
    off = small_ds.off[: n_reads + 1].copy()
    bases = small_ds.bases[: int(off[-1])]
    count, seeds, _ = oracle.find_seeds(ob, orb, p, bases, off)
    descs = _walk_descs(p, small_ds.reads[:n_reads], count, seeds)
    assert len(descs) > 100
    ctx = indexes["small"].ctx(p, 0)
    got = ctx.extend_walks(descs)
    ctx.close()
    codes = {}
    for d, (code, merged, steps) in zip(descs, got):
        wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
        assert (code, merged, steps) == (wcode, wmerged, wst[0]), d
        codes[wcode] = codes.get(wcode, 0) + 1
    ob.close(); orb.close()
    assert codes.get(1, 0) > len(descs) // 2 and codes.get(-1, 0) > 0
