"""deal_prune and deal_term of wp_deal_step.h (LRSC_WP_DEAL 2 and 3) on the CPU, against Walk::step() and the oracle.

tests/host_walk_deal_phases/walk_host_deal_phases.hip is the stand-alone program of tests/test_host_walk_deal.py with a level in
its job: the 64-fibre wavefront, the kernel's loop, a twin per walk that steps through Walk::step(), and after every general
step the byte-for-byte comparison of leaves, rings, paths, results and scalars, and of the wavefront's rank-query and block-load
totals.  alive_lo / alive_hi / has_child are among the scalars: nothing after the prune writes them, so what the comparison sees
at the end of the step is what the prune left.  What each walk comes to must be the oracle's.

The shapes reached come from the trace kinds 4..11 of LRSC_DEAL_TRACE and, for the strand of a seed hit inside a prune task,
kind 12 of LRSC_WALK_TRACE.  Each case prints them and asserts the ones it is there for:

  deal_prune   tasks in a second or later pass; an owner whose children straddle a pass boundary with survivors on both sides (the
               alive bits carried across it); children with and without the seed-support search; hits on each strand; a parent
               with no surviving child.
  deal_term    tasks the filter rules out and tasks it lets through; hits that take a new result slot and hits on a leaf whose
               res_first is set; the overflow branch under max_leaves 4 (which stays in the owner's lane).

Not reached, and why:

A child pruned by currErrorRate > errorRate next to a surviving sibling.  No child of either set is pruned that way at all
(prune_dead_tasks is 0 in every case, in the twins' serial PrunedBySeedSupport as well, or the alive bits would differ): errorRate
is 0.25, and a lineage that loses its seed support is dropped long before its error rate gets there -- by attempToExtend's trim
(0.05 / 0.1 above the frontier's minimum) or because its k-mer has no extension left.  So a parent without a surviving child is,
in these sets, a parent without a child.  A pruned child goes the way of a lane without a task: no bit in the ballot, none in the
OR.  The count is asserted to be 0, so that a set which does prune gets the assertion turned round.

LRSC_WALK_ERR_RESULTS with later leaves of the same owner pending.  The error needs more than kMaxResults =
160 result slots in one walk; a slot is taken by a lineage's first hit, lineages are at most 32 at a time, and in these sets a
walk ends within a few steps of its first hits (the repeat set's largest count of result slots in a walk is far below the
bound).  The count is asserted to be 0 so that a set which does reach it gets the assertion turned round.

The same source under -fsanitize=address,undefined (walk_host_deal_phases_san, a program of its own: nothing of it is loaded into
Python) runs the first walks of the repeat set at level 3."""
from __future__ import annotations

import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.host_walk import _CODE
from tests.test_host_walk import _units
from tests.test_host_walk_deal import MAGIC, QUORUM, SHAPES as BASE_SHAPES, WAIT, _case

HERE = Path(__file__).resolve().parent / "host_walk_deal_phases"
BUILD = HERE / "_build"
SHAPES = BASE_SHAPES + (
    "prunes", "prunes_over_64_tasks", "prune_later_pass_tasks", "prune_straddling_owners", "prune_straddle_alive_both", "prune_need_tasks",
    "prune_noneed_tasks", "prune_fwd_hits", "prune_rvc_hits", "prune_dead_beside_alive", "prune_dead_tasks", "childless_parent_steps",
    "terms", "term_later_pass_tasks", "term_filtered_tasks", "term_scanned_tasks", "term_hits_new_slot", "term_hits_old_slot",
    "term_result_errors", "term_result_errors_pending")


@pytest.fixture(scope="module")
def programs():
    r = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building tests/host_walk_deal_phases failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return BUILD / "walk_host_deal_phases", BUILD / "walk_host_deal_phases_san"


def _run(program, tmp_path, units, n_sym, params, descs, wide, tables, n_lanes, level):
    """-> (return value, shapes, [(code, merged, steps)], first mismatch)"""
    u0, u1 = (np.ascontiguousarray(u, dtype=np.uint8) for u in units)
    ks = list(tables) + [0] * (5 - len(tables))
    recs, codes, off = [], [], 0
    for src, path, trg, dis, initk, max_overlap, min_sa in descs:
        q = (src[len(src) - initk:] + path + trg).encode()
        c = _CODE[np.frombuffer(q, dtype=np.uint8)]
        assert c.max(initial=0) < 4
        recs.append(struct.pack("<4Qq3Q", off, initk, len(path), len(trg), dis, max_overlap, min_sa, 0))
        codes.append(c)
        off += c.size
    head = struct.pack("<15Qd8Q", MAGIC, int(wide), len(tables), *ks, n_sym, u0.size, u1.size, params.idmer_len, params.min_kmer_len,
                       params.max_leaves, params.pb_coverage, params.error_rate, QUORUM, WAIT, n_lanes, len(descs), off, level, 0, 0)
    job, res = tmp_path / "job.bin", tmp_path / "result.bin"
    with open(job, "wb") as f:
        f.write(head)
        f.write(u0.tobytes()); f.write(u1.tobytes())
        f.write(b"".join(recs))
        f.write(np.concatenate(codes).tobytes() if codes else b"")
    r = subprocess.run([str(program), str(job), str(res)], capture_output=True, text=True)
    assert r.returncode in (0, 1, 2), f"{program.name} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    raw = res.read_bytes()
    rc, n, words = struct.unpack_from("<3Q", raw, 0)
    assert n == len(descs) and words == len(SHAPES)
    shapes = dict(zip(SHAPES, struct.unpack_from(f"<{words}Q", raw, 24)))
    k = 24 + 8 * words
    outs = [struct.unpack_from("<q3Q", raw, k + 32 * i) for i in range(n)]
    k += 32 * n
    walks = []
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for code, steps, out_len, _ in outs:
        walks.append((code, bytes(acgt[np.frombuffer(raw, dtype=np.uint8, count=out_len, offset=k)]).decode(), steps))
        k += out_len
    return rc, shapes, walks, raw[k:].decode() + r.stderr[-2000:]


def _check(program, tmp_path, api, oracle, ds, key, n_reads, skip, wide, n_lanes, level, max_leaves=None, first=None):
    p, descs, want = _case(api, oracle, ds, key, n_reads, skip, max_leaves)
    if first is not None:
        descs, want = descs[:first], want[:first]
    (u0, u1), n_sym = _units(ds)
    rc, sh, walks, msg = _run(program, tmp_path, (u0, u1), n_sym, p, descs, wide, (5, 9), n_lanes, level)
    print(f"[deal phases] {key} level {level} {'wide' if wide else 'narrow'} {program.name}: {len(descs)} walks on {n_lanes} lanes;",
          {k: v for k, v in sh.items() if k not in BASE_SHAPES or k in ("wave_steps", "compared_steps", "mismatches", "overflow_branches")})
    assert rc == 0 and sh["mismatches"] == 0, msg
    assert sh["compared_steps"] > 0 and sh["children_overflows"] == 0
    bad = [i for i, (w, g) in enumerate(zip(want, walks)) if w != g]
    assert not bad, f"walks {bad[:5]} differ from the oracle's: {want[bad[0]]} != {walks[bad[0]]}"
    return len(descs), sh


def _assert_prune_shapes(sh):
    assert sh["prunes"] > 0 and sh["prunes_over_64_tasks"] > 0 and sh["prune_later_pass_tasks"] > 0, "prune tasks in a second or later pass"
    assert sh["prune_straddling_owners"] > 0 and sh["prune_straddle_alive_both"] > 0, "alive bits on both sides of a pass boundary"
    assert sh["prune_need_tasks"] > 0 and sh["prune_noneed_tasks"] > 0, "children with and without the seed-support search"
    assert sh["prune_fwd_hits"] > 0 and sh["prune_rvc_hits"] > 0, "seed hits on each strand"
    assert sh["prune_dead_tasks"] == 0 and sh["prune_dead_beside_alive"] == 0, "a child pruned by its error rate: not reached by these sets (see above)"
    assert sh["childless_parent_steps"] > 0, "a parent with no surviving child"


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("level", [2, 3])
def test_repeat_walks_reach_every_phase_shape(programs, tmp_path, api, oracle, repeat_ds, wide, level):
    """The repeat-rich set on a full wavefront, at both levels and on both rank-block layouts."""
    n, sh = _check(programs[0], tmp_path, api, oracle, repeat_ds, "repeat", 60, 0, wide, 64, level)
    assert n > 100
    _assert_prune_shapes(sh)
    if level == 2:
        assert sh["terms"] == 0, "level 2 leaves isTerminated in the walk's own lane"
        return
    assert sh["terms"] > 0 and sh["term_filtered_tasks"] > 0 and sh["term_scanned_tasks"] > 0, "term tasks the filter rules out / lets through"
    assert sh["term_hits_new_slot"] > 0 and sh["term_hits_old_slot"] > 0, "hits with res_first == -1 and with res_first set"
    assert sh["term_result_errors"] == 0 and sh["term_result_errors_pending"] == 0, "LRSC_WALK_ERR_RESULTS: not reached by this set (see above)"


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("level", [2, 3])
def test_long_gap_walks_on_a_short_wavefront(programs, tmp_path, api, oracle, small_ds, wide, level):
    """Seed i to seed i + 4 of the small set on 40 lanes: 24 lanes never hold a walk and only run tasks."""
    n, sh = _check(programs[0], tmp_path, api, oracle, small_ds, "small-skip4", 30, 4, wide, 40, level)
    assert n >= 40
    assert sh["lanes_without_walk"] == 24 and sh["wave_steps"] > 100
    assert sh["prunes"] > 0 and sh["prune_need_tasks"] > 0 and sh["prune_noneed_tasks"] > 0
    if level == 3:
        assert sh["terms"] > 0 and sh["term_filtered_tasks"] > 0


@pytest.mark.parametrize("level", [2, 3])
def test_overflow_branch_with_four_leaves(programs, tmp_path, api, oracle, repeat_ds, level):
    """max_leaves 4: survivors > maxLeaves after a dealt prune; the branch and its terminated_leaf calls stay in the owner's lane."""
    n, sh = _check(programs[0], tmp_path, api, oracle, repeat_ds, "repeat-l4", 60, 0, False, 64, level, max_leaves=4)
    assert n > 100
    assert sh["overflow_branches"] > 0 and sh["max_leaves"] <= 4


def test_sanitized_program(programs, tmp_path, api, oracle, repeat_ds):
    """The stand-alone program under AddressSanitizer and UBSan (either ends the program with a code of its own), at level 3."""
    n, sh = _check(programs[1], tmp_path, api, oracle, repeat_ds, "repeat", 60, 0, False, 64, 3, first=160)
    assert n == 160 and sh["wave_steps"] > 0 and sh["prunes"] > 0 and sh["terms"] > 0
