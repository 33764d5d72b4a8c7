"""The bulk extension launch with extendLeaves dealt across the wavefront (wp_deal.hip, `LRSC_WP_DEAL`; `-m gpu`).

With `LRSC_WP_DEAL=1` (the default) the lane-per-walk launches of round 0 go through wp_extend_deal_kernel: the refines and the
extensions of all the walks a wavefront steps together run as (owner, leaf) tasks on whichever lane they fall.  The whole per-read
path is held against the CPU oracle, and the differential cases run one batch with `LRSC_WP_DEAL=0` (wp_extend_kernel, the serial
step) and `=1` and require identical corrected strings, per-read counters, and rank-query / block-load counts of the extension
stage.  `LRSC_WP_LANES=256` in the differential cases leaves four wavefronts, so that every lane refills from the queue many
times and ends while others of its wavefront still walk."""
from __future__ import annotations

import os

import numpy as np
import pytest

from longreadselfcorrect_amd.capi import K_EXTEND
from tests.test_gpu_fm import _check_whole_path, _fasta

pytestmark = pytest.mark.gpu

NAMES = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
         "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")


@pytest.fixture(autouse=True)
def deal_on(monkeypatch):
    monkeypatch.setenv("LRSC_WP_DEAL", "1")


@pytest.fixture(scope="module")
def indexes(api, small_ds, repeat_ds):
    idx = {"small": api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")}
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


@pytest.mark.parametrize("nodp,split,next_target", [(0, 1, 2), (1, 1, 2), (0, 0, 3), (1, 0, 3)])
def test_small_set_whole_path(api, indexes, oracle, small_ds, nodp, split, next_target):
    p = api.params_default(5, 90)
    p.no_dp, p.split, p.next_target = nodp, split, next_target
    _check_whole_path(api, indexes["small"], oracle, small_ds, p, min_fm=300, min_dp=0 if nodp else 20)


@pytest.mark.parametrize("nodp", [1, 0])
def test_small_set_wide_layout(api, indexes, oracle, small_ds, nodp):
    p = api.params_default(5, 90)
    p.no_dp = nodp
    _check_whole_path(api, indexes["small-wide"], oracle, small_ds, p, min_fm=300, min_dp=0 if nodp else 20)


@pytest.mark.parametrize("nodp", [1, 0])
def test_repeat_set_whole_path(api, indexes, oracle, repeat_ds, nodp):
    p = api.params_default(5, 90)
    p.no_dp = nodp
    # with the DP fallback the oracle's DP stage sets the test's time: 30 reads (some 250 FM walks, 150 DP answers)
    _check_whole_path(api, indexes["repeat"], oracle, repeat_ds, p, n_reads=120 if nodp else 30, min_fm=100, min_dp=0 if nodp else 5)


def test_four_leaves_whole_path(api, indexes, oracle, repeat_ds):
    """-l 4: frontiers overflow (the step's overflow branch ends those walks)."""
    p = api.params_default(5, 90)
    p.no_dp = 1
    p.max_leaves = 4
    got = _check_whole_path(api, indexes["repeat"], oracle, repeat_ds, p, n_reads=120, min_fm=50, fail_cols=(4, 5, 6))
    assert got[:, 6].sum() > 0, "no walk exceeded four leaves"


def _run(index, p, bases, off, reads, deal, monkeypatch):
    monkeypatch.setenv("LRSC_WP_DEAL", deal)
    ctx = index.ctx(p, 0)
    ctx.stats_reset()
    results, pieces = ctx.correct_reads(bases, off)
    st = ctx.stats(K_EXTEND)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, reads, p.split)
    got = np.array([[getattr(r, n) for n in NAMES] for r in results], dtype=np.int64)
    return cfa, dfa, got, (int(st.rank_queries), int(st.block_loads))


@pytest.mark.parametrize("which,max_leaves", [("small", 32), ("small-wide", 32), ("repeat", 32), ("repeat", 4)])
@pytest.mark.parametrize("nodp", [0, 1])
def test_serial_and_dealt_step_agree(api, indexes, small_ds, repeat_ds, which, max_leaves, nodp, monkeypatch):
    monkeypatch.setenv("LRSC_WP_LANES", "256")
    ds = repeat_ds if which == "repeat" else small_ds
    n = 120 if which == "repeat" else len(ds.off) - 1
    off = ds.off[: n + 1].copy()
    bases = ds.bases[: int(off[-1])]
    reads = ds.reads[:n]
    p = api.params_default(5, 90)
    p.no_dp = nodp
    p.max_leaves = max_leaves
    a = _run(indexes[which], p, bases, off, reads, "0", monkeypatch)
    b = _run(indexes[which], p, bases, off, reads, "1", monkeypatch)
    assert a[0] == b[0] and a[1] == b[1]
    np.testing.assert_array_equal(a[2], b[2])
    assert a[3] == b[3] and a[3][0] > 0
