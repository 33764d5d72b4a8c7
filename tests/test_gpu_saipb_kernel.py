"""lrsc_saipb_merge on the device (`-m gpu`): the hash-guided seed-pair merge as kernels (csrc/saipb.hip, saipb_device.h) against the
oracle's restatement of SAIPBSelfCorrectTree and against the host class over the device's FM primitives (the path the call replaces):
every result field and both seed frequencies of every seed pair, in one call per set; batch independence; the error paths."""
from __future__ import annotations

import os

import pytest

from longreadselfcorrect_amd import LrscError
from longreadselfcorrect_amd.capi import K_SAIPB, saipb_pair_jobs, saipb_pair_results

from .test_host_saipb_kernel import wrong_target_pairs
from .test_saipb_host import build_driver, run_pairs
from .test_saipb_oracle import _pairs

pytestmark = pytest.mark.gpu


def _index(api, ds, wide=False, ktab=None):
    env = {"LRSC_FORCE_WIDE": "1"} if wide else {}
    if ktab is not None:
        env["LRSC_KTAB_K"] = str(ktab)
    os.environ.update(env)
    try:
        idx = api.index_open(ds.prefix + ".bwt", ds.prefix + ".rbwt")
        idx.upload(0)
    finally:
        for k in env:
            os.environ.pop(k, None)
    return idx


@pytest.fixture(scope="module")
def small(api, oracle, small_ds):
    ob, orb, _, raw = _pairs(oracle, api, small_ds, 60)
    pairs = [(s, b, t, d) for _, s, b, t, d in raw]
    want = {ml: [oracle.saipb_merge(ob, orb, s, b, t, d, ml) for s, b, t, d in pairs] for ml in (32, 8)}
    ob.close(); orb.close()
    idx = _index(api, small_ds)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    yield raw, pairs, want, ctx
    ctx.close(); idx.close()


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[3] == 0, ("status", i, g[3])
        assert (g[0], g[1], g[2]) == (w[0], w[1], w[2]), i


def test_one_call_over_all_pairs_matches_oracle(small):
    _, pairs, want, ctx = small
    assert len(pairs) == 672
    _same(ctx.saipb_merge_pairs(pairs), want[32])
    assert sum(w[0] == 1 for w in want[32]) > 250 and sum(w[2]["results"] > 1 for w in want[32]) >= 50


def test_eight_leaves_matches_oracle(small):
    _, pairs, want, ctx = small
    _same(ctx.saipb_merge_pairs(pairs, 8), want[8])
    assert sum(w[0] == -3 for w in want[8]) >= 10


def test_wrong_targets_match_oracle_with_search_depth_exceeded(api, oracle, small_ds, small):
    """Return code -2, which no seed-pair set reaches by itself (test_host_saipb_kernel's docstring)."""
    _, pairs, want, ctx = small
    wrong = wrong_target_pairs(pairs, [w[0] for w in want[32]])
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    expect = [oracle.saipb_merge(ob, orb, s, b, t, d, 32) for s, b, t, d in wrong]
    ob.close(); orb.close()
    assert len(wrong) == 240 and sum(w[0] == -2 for w in expect) >= 1
    _same(ctx.saipb_merge_pairs(wrong), expect)


def test_repeat_set_matches_oracle(api, oracle, repeat_ds):
    ob, orb, _, raw = _pairs(oracle, api, repeat_ds, 60)
    pairs = [(s, b, t, d) for _, s, b, t, d in raw if len(t) >= 17]
    assert len(pairs) == 736
    want = [oracle.saipb_merge(ob, orb, s, b, t, d) for s, b, t, d in pairs]
    ob.close(); orb.close()
    idx = _index(api, repeat_ds)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    _same(ctx.saipb_merge_pairs(pairs), want)
    assert sum(w[0] == -3 for w in want) > 0 and sum(w[2]["hash_entries"] == 0 for w in want) > 0
    ctx.close(); idx.close()


@pytest.mark.parametrize("wide,ktab", [(True, None), (False, 0)])
def test_wide_layout_and_no_tables(api, small_ds, small, wide, ktab):
    _, pairs, want, _ = small
    idx = _index(api, small_ds, wide=wide, ktab=ktab)
    if wide:
        assert idx.info().block_symbols == 128
    ctx = idx.ctx(api.params_default(5, 90), 0)
    _same(ctx.saipb_merge_pairs(pairs[:200]), want[32][:200])
    ctx.close(); idx.close()


def test_batch_independence_and_chunking(small, monkeypatch):
    _, pairs, want, ctx = small
    _same(ctx.saipb_merge_pairs(pairs[::-1]), want[32][::-1])
    before = ctx.stats(K_SAIPB).launches
    _same(ctx.saipb_merge_pairs(pairs), want[32])
    assert ctx.stats(K_SAIPB).launches == before + 1             # the default budget holds the whole set: one launch
    # a job's slice is over 150 KB (frontier, candidates, the alignment rows of a raw string of 77 bases or more), so 4 MiB hold
    # fewer than 30 of the 336 jobs of a call: more than ten launches per call
    monkeypatch.setenv("LRSC_SAIPB_CHUNK_MB", "4")
    half = len(pairs) // 2
    before = ctx.stats(K_SAIPB).launches
    _same(ctx.saipb_merge_pairs(pairs[:half]) + ctx.saipb_merge_pairs(pairs[half:]), want[32])
    assert ctx.stats(K_SAIPB).launches >= before + 2 * 10        # the budget was read


def test_equals_the_host_class_over_the_device_primitives(small, small_ds, tmp_path):
    raw, pairs, _, ctx = small
    exe = build_driver(tmp_path, False)
    host = run_pairs(exe, "device", small_ds, raw)
    got = ctx.saipb_merge_pairs(pairs)
    assert [(g[0], g[1]) for g in got] == host


def test_error_paths(small, monkeypatch):
    _, pairs, want, ctx = small
    some = pairs[:40]
    seq, seeds, jobs = saipb_pair_jobs(some)
    seeds[7].len = 16                                            # shorter than its large k-mer
    with pytest.raises(LrscError) as e:
        ctx.saipb_merge(seq, seeds, jobs)
    assert e.value.status == -3
    seq, seeds, jobs = saipb_pair_jobs(some)
    jobs[3].hash_kmer = 32
    with pytest.raises(LrscError) as e:
        ctx.saipb_merge(seq, seeds, jobs)
    assert e.value.status == -7
    jobs[3].hash_kmer, jobs[5].max_leaves = 15, 65
    with pytest.raises(LrscError) as e:
        ctx.saipb_merge(seq, seeds, jobs)
    assert e.value.status == -7
    # an arena one byte short: LRSC_ERR_CAPACITY with the needed size, then success with exactly that
    seq, seeds, jobs = saipb_pair_jobs(some)
    res, freq, arena = ctx.saipb_merge(seq, seeds, jobs)
    need = len(arena)
    assert need > 0
    with pytest.raises(LrscError) as e:
        ctx.saipb_merge(seq, seeds, jobs, arena_cap=need - 1)
    assert e.value.status == -6 and ctx.last_arena_used == need
    res, freq, arena = ctx.saipb_merge(seq, seeds, jobs, arena_cap=need)
    _same(saipb_pair_results(some, res, freq, arena), want[32][:40])


def test_job_over_the_per_job_capacity_gets_a_status(small, monkeypatch):
    _, pairs, want, ctx = small
    monkeypatch.setenv("LRSC_SAIPB_JOB_KB", "512")               # test hook: the long-gap pairs need more, the short ones less
    got = ctx.saipb_merge_pairs(pairs)
    limited = [i for i, g in enumerate(got) if g[3] != 0]
    assert 0 < len(limited) < len(pairs)
    for i, (g, w) in enumerate(zip(got, want[32])):
        if g[3] != 0:
            assert g[3] == 1 and g[0] == 0 and g[1] == "" and g[2]["steps"] == 0
        else:
            assert (g[0], g[1], g[2]["steps"], g[2]["max_leaves"], g[2]["results"], g[2]["hash_entries"]) == \
                   (w[0], w[1], w[2]["steps"], w[2]["max_leaves"], w[2]["results"], w[2]["hash_entries"]), i
