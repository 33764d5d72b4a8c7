"""The dealt general step of wp_extend_deal_kernel (csrc/wp_deal_step.h, the source the kernel compiles) on the CPU: 64 walks per
emulated wavefront through the dealt step and through Walk::step(), compared after every step, and held against the oracle.

tests/host_walk_deal/walk_host_deal.hip is a stand-alone program.  It runs the kernel's loop -- persistent lanes over a queue,
refill and finish in the lane, step_fast for a one-leaf frontier, the quorum per wavefront -- with every lane a fibre: a
cross-lane operation (shuffle, ballot, wave_sync) is where a lane hands over to the next, so the lanes run one after the other from
one such operation to the next, which is a host loop over the 64 lanes per phase.  Every lane carries a twin of its walk that
takes the same steps through Walk::step(); after every general step the two walks' leaves, rings, paths, results and scalars
must be equal byte for byte, and the wavefront's rank-query and block-load totals equal the twins'.  What each walk comes to
(return code, merged sequence, steps) must be the oracle's, as in tests/test_host_walk.py.

Each case asserts the shapes it has reached.  Those of the serial reference come from the walk's trace hook (LRSC_WALK_TRACE)
while a twin is inside Walk::step(); those of the dealt code (a second or later pass of 64 tasks, an owner whose tasks straddle a
pass boundary, the count it carries over, the high-frequency sum of a later pass) from the hook of wp_deal_step.h.

  repeat set, consecutive seeds, 60 reads, 64 lanes: general steps of the wavefront with more than 64 leaves (several passes), an
      owner with more than 64 children, the level-1 and level-2 retries, the min_SA_threshold retry, the isInsufficientFreqs
      refine, a trim that removes a leaf, a further child with ring and path copies, siblings sharing a result slot, lanes that
      refill in the middle of the launch -- narrow and wide layout.
  small set, seed i -> i + 4, 30 reads, 40 lanes: a wavefront with fewer than 64 walks (24 lanes are workers only), long walks,
      refills.
  repeat set with max_leaves 4: the overflow branch (survivors > maxLeaves).

LRSC_WALK_ERR_CHILDREN is left out: it cannot be reached through step(), for the reason tests/test_host_walk_groups.py gives (at
most 32 leaves of four children, and nxt[] holds 128); the hook's overflow count is asserted to stay 0.

The same source built with -fsanitize=address,undefined (walk_host_deal_san, a program of its own: nothing of it is loaded into
Python) runs the first reads of the repeat set."""
from __future__ import annotations

import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.host_walk import _CODE
from tests.test_gpu_fm import _walk_descs
from tests.test_host_walk import _skip_descs, _units

HERE = Path(__file__).resolve().parent / "host_walk_deal"
BUILD = HERE / "_build"
MAGIC = 0x4C41454444574800
SHAPES = ("steps", "max_leaves", "max_children", "steps_over_64_children", "threshold_retries", "level1", "level2", "relax_refines",
          "trims", "trimmed_leaves", "further_children", "overflow_branches", "children_overflows", "shared_slot_steps",
          "wave_steps", "wave_steps_over_64_leaves", "max_wave_leaves", "lanes_without_walk", "refills_mid_launch",
          "attempts", "attempts_over_64_tasks", "max_attempt_tasks", "later_pass_tasks", "straddling_tasks", "carried_count_tasks",
          "later_pass_owner_sums", "later_pass_highfreq_sums", "refines_over_64_tasks", "compared_steps", "mismatches")
QUORUM, WAIT = 70, 6                       # the kernel's defaults (LRSC_WP_GEN_QUORUM, LRSC_WP_GEN_WAIT)


@pytest.fixture(scope="module")
def programs():
    r = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building tests/host_walk_deal failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return BUILD / "walk_host_deal", BUILD / "walk_host_deal_san"


def _run(program, tmp_path, units, n_sym, params, descs, wide, tables, n_lanes):
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
                       params.max_leaves, params.pb_coverage, params.error_rate, QUORUM, WAIT, n_lanes, len(descs), off, 0, 0, 0)
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


_WANT = {}


def _case(api, oracle, ds, key, n_reads, skip, max_leaves=None):
    """The walks of a case and what the oracle makes of each, computed once and shared by the layouts."""
    if key not in _WANT:
        p = api.params_default(5, 90)
        if max_leaves is not None:
            p.max_leaves = max_leaves
        ob, orb = oracle.bwt_load(ds.prefix + ".bwt"), oracle.bwt_load(ds.prefix + ".rbwt")
        off = ds.off[: n_reads + 1].copy()
        count, seeds, _ = oracle.find_seeds(ob, orb, p, ds.bases[: int(off[-1])], off)
        reads = ds.reads[:n_reads]
        descs = _skip_descs(p, reads, count, seeds, skip) if skip else _walk_descs(p, reads, count, seeds)
        want = []
        for d in descs:
            wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
            want.append((wcode, wmerged, wst[0]))
        ob.close(); orb.close()
        _WANT[key] = (p, descs, want)
    return _WANT[key]


def _check(program, tmp_path, api, oracle, ds, key, n_reads, skip, wide, n_lanes, max_leaves=None, first=None):
    p, descs, want = _case(api, oracle, ds, key, n_reads, skip, max_leaves)
    if first is not None:
        descs, want = descs[:first], want[:first]
    (u0, u1), n_sym = _units(ds)
    rc, sh, walks, msg = _run(program, tmp_path, (u0, u1), n_sym, p, descs, wide, (5, 9), n_lanes)
    print(f"[deal] {key} {'wide' if wide else 'narrow'} {program.name}: {len(descs)} walks on {n_lanes} lanes;", sh)
    assert rc == 0 and sh["mismatches"] == 0, msg
    assert sh["compared_steps"] > 0 and sh["children_overflows"] == 0
    bad = [i for i, (w, g) in enumerate(zip(want, walks)) if w != g]
    assert not bad, f"walks {bad[:5]} differ from the oracle's: {want[bad[0]]} != {walks[bad[0]]}"
    return len(descs), sh


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_repeat_walks_reach_every_dealt_shape(programs, tmp_path, api, oracle, repeat_ds, wide):
    """The repeat-rich set on a full wavefront: every shape of the list above but the two the next cases are for."""
    n, sh = _check(programs[0], tmp_path, api, oracle, repeat_ds, "repeat", 60, 0, wide, 64)
    assert n > 100
    # the serial reference
    assert sh["wave_steps_over_64_leaves"] > 0, "a wavefront step with more than 64 leaf tasks"
    assert sh["steps_over_64_children"] > 0 and sh["max_children"] > 64, "an owner with more than 64 children"
    assert sh["level1"] > 0 and sh["level2"] > 0, "the level-1 and level-2 retries"
    assert sh["threshold_retries"] > 0, "the count == 1 min_SA_threshold retry"
    assert sh["relax_refines"] > 0, "the isInsufficientFreqs refine"
    assert sh["trims"] > 0 and sh["trimmed_leaves"] > 0, "a trim that removes a leaf"
    assert sh["further_children"] > 0, "a further child that needs ring and path copies"
    assert sh["shared_slot_steps"] > 0, "siblings sharing a result slot"
    assert sh["refills_mid_launch"] > 0, "lanes that refill in the middle of a launch"
    # the dealt code
    assert sh["attempts_over_64_tasks"] > 0 and sh["later_pass_tasks"] > 0, "a second or later pass of deal_attempt"
    assert sh["straddling_tasks"] > 0, "an owner's tasks split across two passes (the prefix restarts at lane 0)"
    assert sh["carried_count_tasks"] > 0, "an owner's child count carried from one pass to the next"
    assert sh["later_pass_owner_sums"] > 0 and sh["later_pass_highfreq_sums"] > 0, "n_nxt and n_highfreq summed across passes"


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_long_gap_walks_on_a_short_wavefront(programs, tmp_path, api, oracle, small_ds, wide):
    """Seed i to seed i + 4 of the small set on 40 lanes: 24 lanes never hold a walk and only run tasks, the others refill."""
    n, sh = _check(programs[0], tmp_path, api, oracle, small_ds, "small-skip4", 30, 4, wide, 40)
    assert n >= 40
    assert sh["lanes_without_walk"] == 24, "a wavefront with fewer than 64 walks"
    assert sh["refills_mid_launch"] > 0, "lanes that refill in the middle of a launch"
    assert sh["wave_steps"] > 100 and sh["further_children"] > 0


def test_overflow_branch_with_four_leaves(programs, tmp_path, api, oracle, repeat_ds):
    """max_leaves 4: the frontier overflows (survivors > maxLeaves) and the walk ends as `too much repeats`."""
    n, sh = _check(programs[0], tmp_path, api, oracle, repeat_ds, "repeat-l4", 60, 0, False, 64, max_leaves=4)
    assert n > 100
    assert sh["overflow_branches"] > 0, "the overflow branch"
    assert sh["max_leaves"] <= 4


def test_sanitized_program(programs, tmp_path, api, oracle, repeat_ds):
    """The stand-alone program under AddressSanitizer and UBSan (either ends the program with a code of its own)."""
    n, sh = _check(programs[1], tmp_path, api, oracle, repeat_ds, "repeat", 60, 0, False, 64, first=160)
    assert n == 160 and sh["wave_steps"] > 0 and sh["refills_mid_launch"] > 0
