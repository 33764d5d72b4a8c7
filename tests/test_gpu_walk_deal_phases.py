"""The bulk extension launch with PrunedBySeedSupport and isTerminated's scans dealt across the wavefront too (wp_deal_step.h's
deal_prune and deal_term; `LRSC_WP_DEAL` 2 and 3; `-m gpu`).

The differential cases run one batch with `LRSC_WP_DEAL=0` (wp_extend_kernel, the serial step) and with 2 and 3
(wp_extend_deal_kernel at those levels) and require identical corrected strings, per-read counters, and rank-query / block-load
counts of the extension stage.  `LRSC_WP_LANES=256` leaves four wavefronts, so that every lane refills from the queue many times
and ends while others of its wavefront still walk.  The sets are those of tests/test_gpu_walk_deal.py: the small set, the same
in the forced-wide rank-block layout, the repeat-rich set, and the repeat-rich set with -l 4 (the overflow branch).  The serial
run of a set is made once and shared by the levels.

Level 3 is also held against the CPU oracle over the whole per-read path."""
from __future__ import annotations

import numpy as np
import pytest

from tests.test_gpu_fm import _check_whole_path
from tests.test_gpu_walk_deal import _run, indexes  # noqa: F401  (the module-scoped fixture of the predecessor's sets)

pytestmark = pytest.mark.gpu

_SERIAL = {}


@pytest.mark.parametrize("level", ["2", "3"])
@pytest.mark.parametrize("which,max_leaves", [("small", 32), ("small-wide", 32), ("repeat", 32), ("repeat", 4)])
@pytest.mark.parametrize("nodp", [0, 1])
def test_serial_step_and_dealt_phases_agree(api, indexes, small_ds, repeat_ds, which, max_leaves, nodp, level, monkeypatch):  # noqa: F811
    monkeypatch.setenv("LRSC_WP_LANES", "256")
    ds = repeat_ds if which == "repeat" else small_ds
    n = 120 if which == "repeat" else len(ds.off) - 1
    off = ds.off[: n + 1].copy()
    bases = ds.bases[: int(off[-1])]
    reads = ds.reads[:n]
    p = api.params_default(5, 90)
    p.no_dp = nodp
    p.max_leaves = max_leaves
    key = (which, max_leaves, nodp)
    if key not in _SERIAL:
        _SERIAL[key] = _run(indexes[which], p, bases, off, reads, "0", monkeypatch)
    a = _SERIAL[key]
    b = _run(indexes[which], p, bases, off, reads, level, monkeypatch)
    assert a[0] == b[0] and a[1] == b[1]
    np.testing.assert_array_equal(a[2], b[2])
    assert a[3] == b[3] and a[3][0] > 0


@pytest.fixture
def level3(monkeypatch):
    monkeypatch.setenv("LRSC_WP_DEAL", "3")


def test_small_set_whole_path(api, indexes, oracle, small_ds, level3):  # noqa: F811
    p = api.params_default(5, 90)
    _check_whole_path(api, indexes["small"], oracle, small_ds, p, min_fm=300, min_dp=20)


def test_small_set_wide_layout(api, indexes, oracle, small_ds, level3):  # noqa: F811
    p = api.params_default(5, 90)
    p.no_dp = 1
    _check_whole_path(api, indexes["small-wide"], oracle, small_ds, p, min_fm=300, min_dp=0)


def test_repeat_set_whole_path(api, indexes, oracle, repeat_ds, level3):  # noqa: F811
    p = api.params_default(5, 90)
    p.no_dp = 1
    _check_whole_path(api, indexes["repeat"], oracle, repeat_ds, p, n_reads=120, min_fm=100, min_dp=0)


def test_four_leaves_whole_path(api, indexes, oracle, repeat_ds, level3):  # noqa: F811
    """-l 4: frontiers overflow after a dealt prune (the overflow branch stays in the owner's lane)."""
    p = api.params_default(5, 90)
    p.no_dp = 1
    p.max_leaves = 4
    got = _check_whole_path(api, indexes["repeat"], oracle, repeat_ds, p, n_reads=120, min_fm=50, fail_cols=(4, 5, 6))
    assert got[:, 6].sum() > 0, "no walk exceeded four leaves"
