"""-l above 32 on the CPU: the serial wide walk (Walk<WIDE, true> of csrc/walk_device.h, the source wp_wide.hip's kernels run with the
frontier over a wavefront) compiled for the host by tests/host_walk_wide and held walk by walk against the oracle's
LongReadSelfCorrectByOverlap with the same maxLeaves: return code, merged sequence and step count, through Walk::run and through
the single-leaf fast path with its hand-over, over the narrow and the wide rank-block layout.

The walks come from the repeat-rich dataset (a 75-copy interspersed repeat), where thousands of walks overflow 32 leaves; each
case first checks that the oracle's -l 32 and -l L walks differ there, i.e. that it covers what -l 32 cannot."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.host_walk_wide import HostWalkWide
from tests.test_gpu_fm import _walk_descs
from tests.test_host_walk import _units

N_READS = 48                     # read 46 holds a walk that -l 33 takes further than -l 32


@pytest.fixture(scope="module")
def hww():
    return HostWalkWide()


@pytest.fixture(scope="module")
def repeat_walks(api, oracle, repeat_ds):
    """The walks of the first reads of repeat_ds whose -l 32 oracle walk ends with its frontier overflowing (code -3)
    or that reach a frontier above 16, plus a sample of the others."""
    p = api.params_default(5, 90)
    ob, orb = oracle.bwt_load(repeat_ds.prefix + ".bwt"), oracle.bwt_load(repeat_ds.prefix + ".rbwt")
    off = repeat_ds.off[: N_READS + 1].copy()
    count, seeds, _ = oracle.find_seeds(ob, orb, p, repeat_ds.bases[: int(off[-1])], off)
    descs = _walk_descs(p, repeat_ds.reads[:N_READS], count, seeds)
    ob.close(); orb.close()
    return descs


def _params(api, max_leaves):
    p = api.params_default(5, 90)
    p.max_leaves = max_leaves
    return p


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("max_leaves", [33, 64, 128])
def test_wide_walk_matches_oracle(hww, api, oracle, repeat_ds, repeat_walks, max_leaves, wide):
    (u0, u1), n_sym = _units(repeat_ds)
    h = hww.index(u0, u1, n_sym, wide=wide, tables=(5, 9) if wide else (5, 9, 11))
    ob, orb = oracle.bwt_load(repeat_ds.prefix + ".bwt"), oracle.bwt_load(repeat_ds.prefix + ".rbwt")
    p32, pL = _params(api, 32), _params(api, max_leaves)
    n_diff, n_over, fronts = 0, 0, 0
    try:
        for d in repeat_walks:
            want = oracle.extend_walk(ob, orb, pL, *d)
            narrow = oracle.extend_walk(ob, orb, p32, *d)
            n_diff += (want[0], want[1], want[2][0]) != (narrow[0], narrow[1], narrow[2][0])
            n_over += narrow[0] == -3
            for mode in (0, 1):
                code, merged, steps, front = hww.extend_walk_wide(h, pL, *d, mode)
                assert (code, merged, steps) == (want[0], want[1], want[2][0]), (mode, d[3:])
                fronts = max(fronts, front)
    finally:
        hww.index_free(h)
        ob.close(); orb.close()
    # the data overflows 32 leaves, and -l L changes walks there (a walk that steps on where -l 32 stopped)
    assert n_over > 0 and n_diff > 0 and (fronts > 32 or max_leaves == 33), (n_over, fronts, n_diff)


def test_wide_walk_at_32_is_the_narrow_walk(hww, api, oracle, repeat_ds, repeat_walks):
    """With capacity 32 the wide walk is the 32-leaf walk: the same codes, sequences and steps as the oracle at -l 32."""
    (u0, u1), n_sym = _units(repeat_ds)
    h = hww.index(u0, u1, n_sym, wide=False, tables=(5, 9, 11))
    ob, orb = oracle.bwt_load(repeat_ds.prefix + ".bwt"), oracle.bwt_load(repeat_ds.prefix + ".rbwt")
    p = _params(api, 32)
    try:
        for d in repeat_walks[::3]:
            want = oracle.extend_walk(ob, orb, p, *d)
            code, merged, steps, _ = hww.extend_walk_wide(h, p, *d, 1)
            assert (code, merged, steps) == (want[0], want[1], want[2][0])
    finally:
        hww.index_free(h)
        ob.close(); orb.close()


@pytest.mark.parametrize("idmer,min_kmer", [(7, 13), (9, 15)], ids=["idmer7", "minkmer15"])
def test_wide_walk_with_options(hww, api, oracle, repeat_ds, repeat_walks, idmer, min_kmer):
    """-l 64 away from the default -i / -s: the wide walk builds its tables by the generic path (no k-mer table of 7; none of 15)."""
    from tests.test_host_walk import _in_domain

    p = _params(api, 64)
    p.idmer_len, p.min_kmer_len = idmer, min_kmer
    descs = [d for d in repeat_walks if _in_domain(p, d)]
    assert len(descs) >= 100
    (u0, u1), n_sym = _units(repeat_ds)
    h = hww.index(u0, u1, n_sym, wide=False, tables=(5, 9, 11))
    ob, orb = oracle.bwt_load(repeat_ds.prefix + ".bwt"), oracle.bwt_load(repeat_ds.prefix + ".rbwt")
    codes, fronts = set(), 0
    try:
        for d in descs:
            want = oracle.extend_walk(ob, orb, p, *d)
            codes.add(want[0])
            for mode in (0, 1):
                code, merged, steps, front = hww.extend_walk_wide(h, p, *d, mode)
                assert (code, merged, steps) == (want[0], want[1], want[2][0]), (mode, d[3:])
                fronts = max(fronts, front)
    finally:
        hww.index_free(h)
        ob.close(); orb.close()
    assert {1, -1} <= codes and fronts > 32, (codes, fronts)
