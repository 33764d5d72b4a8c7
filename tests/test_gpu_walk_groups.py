"""The serial general step's grouped loops on the device (walk_device.h: PrunedBySeedSupport, the commit, the isTerminated loop, the
trim, the extension loop's early load; `-m gpu`).

`LRSC_WP_WAVE=0` keeps every extension launch, rounds >= 1 included, in wp_extend_kernel -- a lane per walk, the serial general
step -- and `LRSC_WP_LANES=256` leaves so few lanes that every wavefront refills from the queue many times.  The whole per-read
path is held against the CPU oracle (corrected strings, per-read counters), and the extension stage's rank queries and block
loads against a run of the same reads through the wave kernel (`LRSC_WP_WAVE=2`), whose cross-leaf code this file's subject
does not share.  The sets are the smallest the suite has; tests/test_host_walk_groups.py records which step shapes they reach."""
from __future__ import annotations

import numpy as np
import pytest

from tests.test_gpu_fm import _check_whole_path
from tests.test_gpu_wave_walk import _run, repeat_index, small_index, wide_small_index  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def serial_everywhere(monkeypatch):
    monkeypatch.setenv("LRSC_WP_WAVE", "0")
    monkeypatch.setenv("LRSC_WP_LANES", "256")


@pytest.mark.parametrize("nodp,split,next_target", [(0, 0, 1), (0, 1, 2), (1, 0, 3), (1, 1, 2)])
def test_small_set_whole_path(api, small_index, oracle, small_ds, nodp, split, next_target):
    p = api.params_default(5, 90)
    p.no_dp, p.split, p.next_target = nodp, split, next_target
    _check_whole_path(api, small_index, oracle, small_ds, p, min_fm=300, min_dp=0 if nodp else 20)


@pytest.mark.parametrize("nodp", [1, 0])
def test_repeat_set_whole_path(api, repeat_index, oracle, repeat_ds, nodp):
    p = api.params_default(5, 90)
    p.no_dp = nodp
    _check_whole_path(api, repeat_index, oracle, repeat_ds, p, n_reads=40, min_fm=100, min_dp=0 if nodp else 5)


def test_small_set_wide_layout(api, wide_small_index, oracle, small_ds):
    p = api.params_default(5, 90)
    _check_whole_path(api, wide_small_index, oracle, small_ds, p, min_fm=300, min_dp=20)


def test_repeat_set_64_leaves(api, repeat_index, oracle, repeat_ds):
    """-l 64: walks that outgrow 32 leaves go on in the wide-frontier kernel; the ones that do not stay in the serial step."""
    p = api.params_default(5, 90)
    p.max_leaves = 64
    _check_whole_path(api, repeat_index, oracle, repeat_ds, p, n_reads=40, min_fm=100, min_dp=5)


@pytest.mark.parametrize("which", ["small", "small-wide", "repeat"])
def test_extension_counters_equal_the_wave_kernels(api, small_index, wide_small_index, repeat_index, small_ds, repeat_ds, which, monkeypatch):
    index, ds = {"small": (small_index, small_ds), "small-wide": (wide_small_index, small_ds), "repeat": (repeat_index, repeat_ds)}[which]
    n = 120 if which == "repeat" else len(ds.off) - 1
    off = ds.off[: n + 1].copy()
    bases = ds.bases[: int(off[-1])]
    reads = ds.reads[:n]
    p = api.params_default(5, 90)
    a = _run(index, p, bases, off, reads, "0", monkeypatch)
    b = _run(index, p, bases, off, reads, "2", monkeypatch)
    print(which, "rank queries / block loads of the extension stage: serial", a[3], "wave", b[3])
    assert a[0] == b[0] and a[1] == b[1]
    np.testing.assert_array_equal(a[2], b[2])
    assert a[3] == b[3] and a[3][0] > 0
