"""The wavefront-cooperative extension kernel (wp_wave.hip, `-m gpu`).

`LRSC_WP_WAVE=2` sends every extension launch of the walk-parallel flow through wp_extend_wave_kernel (one walk per wavefront,
the frontier's leaves on the lanes), so that the whole per-read path -- default flow and --nodp -- runs every walk through it and
is held against the CPU oracle.  The differential cases run one batch under `LRSC_WP_WAVE=0` (lane 0 walks alone) and `=2` and
require identical corrected strings, per-read counters, and rank-query / block-load counts of the extension stage."""
from __future__ import annotations

import numpy as np
import pytest

from longreadselfcorrect_amd.capi import K_EXTEND
from tests.test_gpu_fm import _check_whole_path, _fasta
from tests.test_gpu_real_shape import GOLD, Shaped, _whole_path

pytestmark = pytest.mark.gpu

NAMES = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
         "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")


@pytest.fixture(autouse=True)
def wave_everywhere(monkeypatch):
    monkeypatch.setenv("LRSC_WP_WAVE", "2")


@pytest.fixture(scope="module")
def small_index(api, small_ds):
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def wide_small_index(api, small_ds):
    import os
    os.environ["LRSC_FORCE_WIDE"] = "1"
    try:
        idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    finally:
        del os.environ["LRSC_FORCE_WIDE"]
    idx.upload(0)
    assert idx.info().block_symbols == 128
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def repeat_index(api, repeat_ds):
    idx = api.index_open(repeat_ds.prefix + ".bwt", repeat_ds.prefix + ".rbwt")
    idx.upload(0)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def long_ds(api, oracle):
    assert GOLD is not None, "tests/golden/real_shape.json missing"
    ds = Shaped(api, oracle, GOLD["long"])
    yield ds
    ds.close()


@pytest.mark.parametrize("nodp,split,next_target", [(0, 0, 1), (0, 1, 1), (0, 0, 2), (1, 0, 1), (1, 1, 2), (1, 0, 3)])
def test_small_set_whole_path(api, small_index, oracle, small_ds, nodp, split, next_target):
    p = api.params_default(5, 90)
    p.no_dp, p.split, p.next_target = nodp, split, next_target
    _check_whole_path(api, small_index, oracle, small_ds, p, min_fm=300, min_dp=0 if nodp else 20)


@pytest.mark.parametrize("nodp", [1, 0])
def test_small_set_wide_layout(api, wide_small_index, oracle, small_ds, nodp, monkeypatch):
    monkeypatch.setenv("LRSC_WP_LANES", "256")
    p = api.params_default(5, 90)
    p.no_dp = nodp
    _check_whole_path(api, wide_small_index, oracle, small_ds, p, min_fm=300, min_dp=0 if nodp else 20)


@pytest.mark.parametrize("nodp", [1, 0])
def test_repeat_set_whole_path(api, repeat_index, oracle, repeat_ds, nodp):
    p = api.params_default(5, 90)
    p.no_dp = nodp
    _check_whole_path(api, repeat_index, oracle, repeat_ds, p, n_reads=120, min_fm=100, min_dp=0 if nodp else 5)


@pytest.mark.parametrize("nodp", [0, 1])
def test_10kb_set_whole_path(api, oracle, long_ds, nodp):
    g = GOLD["long"]["nodp" if nodp else "default"]
    _whole_path(api, oracle, long_ds, g["reads"], nodp, g)


def _run(index, p, bases, off, reads, wave, monkeypatch):
    monkeypatch.setenv("LRSC_WP_WAVE", wave)
    ctx = index.ctx(p, 0)
    ctx.stats_reset()
    results, pieces = ctx.correct_reads(bases, off)
    st = ctx.stats(K_EXTEND)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, reads, p.split)
    got = np.array([[getattr(r, n) for n in NAMES] for r in results], dtype=np.int64)
    return cfa, dfa, got, (int(st.rank_queries), int(st.block_loads))


@pytest.mark.parametrize("which", ["small", "small-wide", "repeat"])
@pytest.mark.parametrize("nodp", [0, 1])
def test_serial_and_wave_kernels_agree(api, small_index, wide_small_index, repeat_index, small_ds, repeat_ds, which, nodp, monkeypatch):
    """Few lanes (LRSC_WP_LANES): every wavefront refills from the queue many times."""
    monkeypatch.setenv("LRSC_WP_LANES", "256")
    index, ds = {"small": (small_index, small_ds), "small-wide": (wide_small_index, small_ds), "repeat": (repeat_index, repeat_ds)}[which]
    n = 120 if which == "repeat" else len(ds.off) - 1
    off = ds.off[: n + 1].copy()
    bases = ds.bases[: int(off[-1])]
    reads = ds.reads[:n]
    p = api.params_default(5, 90)
    p.no_dp = nodp
    a = _run(index, p, bases, off, reads, "0", monkeypatch)
    b = _run(index, p, bases, off, reads, "2", monkeypatch)
    assert a[0] == b[0] and a[1] == b[1]
    np.testing.assert_array_equal(a[2], b[2])
    assert a[3] == b[3] and a[3][0] > 0
