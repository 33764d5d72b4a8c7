"""The general step's grouped loops (csrc/walk_device.h: PrunedBySeedSupport, the commit, the isTerminated loop, the trim and the
extension loop's early load) on the CPU against the oracle, on inputs that are known to reach the shapes at which a group can go
wrong.

tests/host_walk_groups is tests/host_walk's harness compiled with the walk's trace hook (LRSC_WALK_TRACE): it counts, per general
step, the frontier's size, the children made, the threshold retries by leaf index and the SelectFreqsOfrange calls by leaf count.
The walks are those of tests/test_host_walk.py (same helpers, same comparison: return code, merged sequence and step count of
every walk equal the oracle's, through Walk::run and through the fast path with hand-over), and each case asserts what it reached.

The groups are 2 children (PrunedBySeedSupport, commit), 4 leaves (isTerminated, trim) and a look-ahead of one leaf (extension
loop), so G = 4 below.  What the cases reach (the hook sits outside the loops this change touches and every walk equals the
oracle's, so the parent commit's walk code reaches the same):

  repeat set, consecutive seeds, 60 reads (824 walks, about 3 s per layout):
      general steps with every frontier size from 1 to 28 and up to 32 leaves (1 ... 2G + 1 and 16 or more asserted);
      threshold retries on leaf 0 (4 930), leaf 1 (6 196), leaves 2, 3 (1 832, 958) and on up to leaf 27: the second of a pair,
      the second to fourth of a four, leaves of later groups;
      SelectFreqsOfrange over 1 ... 12 leaves (more than G asserted);
      up to 106 children in a step, 50 steps with more than 64 (the second word of the alive mask, children beyond the first
      group of 64).
  small set, seed i -> i + 4, 30 reads (75 walks): long walks, frontiers of every size 1 ... 10, result paths beyond 64 words.
  Both once more over the wide rank-block layout (64-bit positions: a leaf is 240 bytes, other field offsets, the same groups).

LRSC_WALK_ERR_CHILDREN is not reached, and cannot be through step(): a step starts with at most max_leaves = 32 leaves and a
leaf makes at most 4 children, 128 = kMaxChildren in all, and the error needs one more.  The hook's overflow count is asserted
to stay 0.  Its counter rule (nothing is counted for a leaf behind the child that raises it) holds by construction here: the
extension loop's look-ahead loads leaf i + 1's interval ends and nothing else -- no rank query is issued for a leaf before its
own turn, so there is no temporary count to hold back."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.host_walk import HostWalk
from tests.test_host_walk import _check, _units

HERE = Path(__file__).resolve().parent / "host_walk_groups"
SO = HERE / "_build" / "liblrsc_host_walk_groups.so"
G = 4
FIELDS = (("steps_by_leaves", 40), ("retries_by_leaf", 40), ("selects_by_leaves", 40), ("max_children", 1), ("steps_over_64_children", 1),
          ("children_overflows", 1))


class TracedHostWalk(HostWalk):
    """tests/host_walk's loader over the traced build of the same harness"""

    def __init__(self):
        r = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"building tests/host_walk_groups failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
        import tests.host_walk as plain
        so, build = plain.SO, plain.build
        plain.SO, plain.build = SO, lambda: None
        try:
            super().__init__()
        finally:
            plain.SO, plain.build = so, build
        self.lib.hw_trace_words.restype = C.c_uint32
        assert self.lib.hw_trace_words() == sum(n for _, n in FIELDS)

    def reset(self):
        self.lib.hw_trace_reset()

    def trace(self) -> dict:
        raw = np.zeros(sum(n for _, n in FIELDS), dtype=np.uint64)
        self.lib.hw_trace_get(raw.ctypes.data_as(C.c_void_p))
        out, k = {}, 0
        for name, n in FIELDS:
            out[name] = raw[k: k + n].copy() if n > 1 else int(raw[k])
            k += n
        return out


@pytest.fixture(scope="module")
def thw():
    return TracedHostWalk()


def _show(tag, t):
    print(tag, "steps by leaves", [int(x) for x in t["steps_by_leaves"]], "retries by leaf", [int(x) for x in t["retries_by_leaf"]],
          "selects by leaves", [int(x) for x in t["selects_by_leaves"]], "max children", t["max_children"],
          "steps over 64 children", t["steps_over_64_children"], "overflows", t["children_overflows"])


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_long_gap_walks(thw, api, oracle, small_ds, wide):
    """Seed i to seed i + 4 of the small set: walks of hundreds of steps, frontiers of every size up to 2G + 1."""
    thw.reset()
    tables = (5, 9) if wide else (5, 9, 11)
    n, codes, _, steps = _check(thw, api, oracle, small_ds, _units(small_ds), 5, 90, tables, wide, 30, skip=4)
    t = thw.trace()
    _show(f"[groups] small set skip 4 {'wide' if wide else 'narrow'}: {n} walks, codes {codes};", t)
    assert n >= 40 and steps > 20 * n
    by = t["steps_by_leaves"]
    assert all(by[k] > 0 for k in range(1, 2 * G + 2)), "a frontier of every size 1 ... 2G + 1"
    assert t["children_overflows"] == 0


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_repeat_walks_reach_every_group_shape(thw, api, oracle, repeat_ds, wide):
    """The repeat-rich set: wide frontiers, more than 64 children, the min_SA_threshold retry on leaves behind the first of a
    group, SelectFreqsOfrange over more than G leaves."""
    thw.reset()
    n, codes, _, _ = _check(thw, api, oracle, repeat_ds, _units(repeat_ds), 5, 90, (5, 9), wide, 60)
    t = thw.trace()
    _show(f"[groups] repeat set {'wide' if wide else 'narrow'}: {n} walks, codes {codes};", t)
    assert n > 100 and len(codes) >= 2
    by, re, se = t["steps_by_leaves"], t["retries_by_leaf"], t["selects_by_leaves"]
    assert all(by[k] > 0 for k in range(1, 2 * G + 2)), "a frontier of every size 1 ... 2G + 1"
    assert by[16:].sum() > 0, "a step with 16 or more leaves"
    assert t["steps_over_64_children"] > 0, "a step with more than 64 children"
    assert re[1::2].sum() > 0, "a retry on the second leaf of a pair"
    assert sum(re[k] for k in range(len(re)) if k % G) > 0, "a retry on a leaf that is not the first of a group of four"
    assert se[G + 1:].sum() > 0, "SelectFreqsOfrange over more than G leaves"
    assert t["children_overflows"] == 0
