"""The pile-up kernel with several wavefronts per multiple alignment (csrc/dp_msa.hip, msa_pileup<GLOBAL, NW> with NW > 1; DESIGN.md
section 4b, "wide pile-ups") against the oracle's restatement of LongReadOverlap.cpp / multiple_alignment.cpp.

LRSC_MSA_WAVES=2 / 4 / 8 gives every launch that many wavefronts per workgroup, so the few-hundred- to two-thousand-column pile-ups
of the small set go through the code that the default keeps for pile-ups of thousands of columns.  The query lengths sit around
the multiples of 64 x NW columns, ops and bases, where a chunk of one wavefront ends and the next one's begins.  Then the whole
correction path in a fresh process per setting (the switch is read per call, the child makes that plain): 1 against 4 wavefronts
on the small and the repeat-rich set, and the default rule against the oracle."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.two_contexts_child import NAMES

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
LENGTHS = (250, 256, 260, 505, 512, 520, 760, 768, 1020, 1024, 1030, 1530, 1536, 1800, 2000)
PER_LENGTH = 24
COV = 90


@pytest.fixture(scope="module")
def queries(small_ds):
    reads = small_ds.reads
    rng = np.random.default_rng(20261021)
    qs = []
    for L in LENGTHS:
        for _ in range(PER_LENGTH):
            r = int(rng.integers(len(reads)))
            p = int(rng.integers(0, len(reads[r]) - L))
            k = int(rng.choice([13, 15]))
            qs.append((reads[r][p: p + L], k, L // 10, 0.65, 15))
    return qs


@pytest.fixture(scope="module")
def want(oracle, small_ds, queries):
    """The oracle's (rows, strings, consensus) per query, computed once; real pile-ups at every length, not only "too few rows"."""
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    w = [oracle.dp_consensus(ob, orb, q, k, mo, mi, COV, mc) for q, k, mo, mi, mc in queries]
    ob.close(); orb.close()
    multi = [sum(x[0] > 3 for x in w[i: i + PER_LENGTH]) for i in range(0, len(w), PER_LENGTH)]
    assert min(multi) >= 4 and sum(multi) >= 100, multi
    return w


@pytest.fixture(scope="module")
def gpu_index(api, small_ds):
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    yield idx
    idx.close()


def consensus(api, gpu_index, queries, monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("LRSC_MSA_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = gpu_index.ctx(api.params_default(5, COV), 0)
    got = ctx.dp_consensus(queries)
    walked = ctx.msa_rows_by_step_walk
    ctx.close()
    return got, walked


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_wide_workgroups_match_oracle(api, gpu_index, queries, want, monkeypatch, waves, force_global):
    env = {"LRSC_MSA_WAVES": str(waves)}
    if force_global:
        env["LRSC_MSA_FORCE_GLOBAL"] = "1"
    got, walked = consensus(api, gpu_index, queries, monkeypatch, env)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), [(i, len(queries[i][0]), got[i][:2], want[i][:2]) for i in bad[:5]])
    assert walked * 10 < sum(w[0] - 1 for w in want)           # the passes did the rows, not the step walk


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
@pytest.mark.parametrize("waves", [1, 4])
def test_step_walk_inside_a_wide_workgroup(api, gpu_index, queries, want, monkeypatch, waves, force_global):
    """LRSC_MSA_BATCH=0: every row through the step walk (msa_row_walk), which one wavefront of the four runs while the others wait,
    and which in a workgroup of one wavefront is the whole workgroup; in LDS and, with its wavefront-level synchronisation on
    workspace memory, in the global variant."""
    env = {"LRSC_MSA_WAVES": str(waves), "LRSC_MSA_BATCH": "0"}
    if force_global:
        env["LRSC_MSA_FORCE_GLOBAL"] = "1"
    got, walked = consensus(api, gpu_index, queries, monkeypatch, env)
    assert got == want
    assert walked == sum(w[0] - 1 for w in want)


@pytest.mark.parametrize("waves", [None, "4"], ids=["default", "waves4"])
def test_pile_ups_on_both_sides_of_a_bucket_ceiling(api, gpu_index, queries, want, monkeypatch, waves):
    """LRSC_MSA_LDS_MAX=12288: the short queries' pile-ups fit the LDS buckets, the long ones go to the global workspace."""
    env = {"LRSC_MSA_LDS_MAX": "12288"}
    if waves:
        env["LRSC_MSA_WAVES"] = waves
    got, _ = consensus(api, gpu_index, queries, monkeypatch, env)
    assert got == want


def test_default_rule_matches_oracle(api, gpu_index, queries, want, monkeypatch):
    got, _ = consensus(api, gpu_index, queries, monkeypatch, {})
    assert got == want


# ---- rows that open several hundred new columns: the wide global variant keeps them on the passes (kMaxInsGlobal) --------------------
LONG_LENGTHS = (2600, 3000, 3500)


@pytest.fixture(scope="module")
def long_ds(api, oracle, tmp_path_factory):
    """6 kb templates at 90x over a 7 kb genome: queries of several kilobases.  With 9 % insertions per read base and 4.5 % deletions,
    a row shows about 0.13 x L bases where the query has none: 330 and more new columns in the first row of a 2600-base query."""
    from tests.conftest import Dataset

    return Dataset(api, oracle, tmp_path_factory.mktemp("long_ds"), 7000, 105, 6000, seed=0x5EED0101)


@pytest.fixture(scope="module")
def long_index(api, long_ds):
    idx = api.index_open(long_ds.prefix + ".bwt", long_ds.prefix + ".rbwt")
    idx.upload(0)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def long_cases(oracle, long_ds):
    """(queries, the oracle's results): draws of 2600 to 3500 bases, of which the first four with a real pile-up are kept -- a 15-mer
    of a read with 15 % errors has few exact copies, so many draws retrieve one or two strings only."""
    reads = long_ds.reads
    rng = np.random.default_rng(20261022)
    ob, orb = oracle.bwt_load(long_ds.prefix + ".bwt"), oracle.bwt_load(long_ds.prefix + ".rbwt")
    qs, want = [], []
    for t in range(60):
        L = LONG_LENGTHS[t % len(LONG_LENGTHS)]
        r = int(rng.integers(len(reads)))
        if len(reads[r]) <= L:
            continue
        p = int(rng.integers(0, len(reads[r]) - L))
        q = (reads[r][p: p + L], 15, L // 10, 0.65, 15)
        w = oracle.dp_consensus(ob, orb, q[0], q[1], q[2], q[3], COV, q[4])
        if w[0] > 3:
            qs.append(q); want.append(w)
        if len(qs) == 4:
            break
    ob.close(); orb.close()
    assert len(qs) == 4
    return qs, want


@pytest.fixture(scope="module")
def long_queries(long_cases):
    return long_cases[0]


@pytest.fixture(scope="module")
def long_want(long_cases):
    return long_cases[1]


@pytest.fixture(scope="module")
def long_walked_by_one_wavefront(api, long_index, long_queries, long_want):
    """The one-wavefront kernel (256 new columns per row at most on the passes): how many rows it sends to the step walk."""
    mp = pytest.MonkeyPatch()
    try:
        got, walked = consensus(api, long_index, long_queries, mp, {"LRSC_MSA_WAVES": "1", "LRSC_MSA_FORCE_GLOBAL": "1"})
    finally:
        mp.undo()
    assert got == long_want
    return walked


@pytest.mark.parametrize("waves", ["2", "4", "8", None], ids=["waves2", "waves4", "waves8", "default"])
def test_rows_of_several_hundred_new_columns_stay_on_the_passes(api, long_index, long_queries, long_want, long_walked_by_one_wavefront,
                                                                monkeypatch, waves):
    """Multi-kilobase queries in the global workspace.  A row that the one-wavefront kernel walks and a wide workgroup does not is a row
    of 257-4096 new columns.  A row that spans 2000 bases of its query opens that many (the fixture's arithmetic), but a row may
    overlap a tenth of the query only, so what is asserted is that such rows exist and that the wide workgroups walk a tenth of the
    rows at most; the counts are printed (37 rows; one wavefront walks 10 of them, 2 / 4 / 8 wavefronts none).  By the default rule
    pile-ups of this size fit the LDS bucket of one workgroup per CU, which keeps one wavefront and the 256 ceiling."""
    env = {"LRSC_MSA_FORCE_GLOBAL": "1", "LRSC_MSA_WAVES": waves} if waves else {}
    got, walked = consensus(api, long_index, long_queries, monkeypatch, env)
    rows = sum(w[0] - 1 for w in long_want)
    print(f"rows {rows}, by the step walk: one wavefront {long_walked_by_one_wavefront}, {waves or 'default'} {walked}")
    assert got == long_want
    if waves:
        assert long_walked_by_one_wavefront - walked >= 1
        assert walked * 10 < rows
    else:                                                      # the default rule: whichever launch a pile-up falls to, never more walks
        assert walked <= long_walked_by_one_wavefront


# ---- the whole correction path, a fresh process per setting ------------------------------------------------------------------------
_runs: dict[tuple, dict] = {}


def whole_path(ds, tag, bases, off, waves, tmp_path_factory):
    key = (tag, waves)
    if key not in _runs:
        tmp = tmp_path_factory.mktemp(f"msa_wide_{tag}_{waves}")
        np.savez(tmp / "reads.npz", bases=bases, off=off)
        env = {k: v for k, v in os.environ.items() if not k.startswith("LRSC_MSA_")}
        if waves:
            env["LRSC_MSA_WAVES"] = waves
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "two_contexts_child.py"), ds.prefix, str(tmp / "reads.npz"), str(tmp / "out.json")],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{key}: child exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        _runs[key] = json.loads((tmp / "out.json").read_text())
    return _runs[key]


def read_set(tag, small_ds, repeat_ds):
    ds, n = (small_ds, small_ds.n_reads) if tag == "small" else (repeat_ds, 120)      # the oracle's time: 120 reads of the repeat set
    off = ds.off[: n + 1].copy()
    return ds, ds.bases[: int(off[-1])], off


@pytest.mark.parametrize("tag", ["small", "repeat"])
def test_whole_path_one_wavefront_against_four(small_ds, repeat_ds, tag, tmp_path_factory):
    ds, bases, off = read_set(tag, small_ds, repeat_ds)
    one, four = (whole_path(ds, tag, bases, off, w, tmp_path_factory) for w in ("1", "4"))
    assert four == one, "strings or per-read counters change with the wavefronts per pile-up"
    assert sum(row["c"][NAMES.index("dp_num")] for row in one["one"]) >= 5     # the DP stage really ran


@pytest.mark.parametrize("tag", ["small", "repeat"])
def test_whole_path_default_against_oracle(api, oracle, small_ds, repeat_ds, tag, tmp_path_factory):
    ds, bases, off = read_set(tag, small_ds, repeat_ds)
    dflt = whole_path(ds, tag, bases, off, None, tmp_path_factory)
    params = api.params_default(5, 90)
    params.no_dp = 0
    ob, orb = oracle.bwt_load(ds.prefix + ".bwt"), oracle.bwt_load(ds.prefix + ".rbwt")
    w = oracle.correct_reads(ob, orb, params, bases, off)
    want_fa, want_counters = w.correct_fa, np.array(w.counters, dtype=np.int64)
    w.close(); ob.close(); orb.close()
    assert dflt["two"] == dflt["one"]
    rows = dflt["one"]
    assert all(row["c"][NAMES.index("status")] == 0 for row in rows)
    got_fa = "".join(f">r{r}\n{piece}\n" for r, row in enumerate(rows) if row["c"][NAMES.index("merge")] for piece in row["p"])
    assert got_fa == want_fa
    np.testing.assert_array_equal(np.array([row["c"][:11] for row in rows], dtype=np.int64), want_counters)
    assert want_counters[:, 8].sum() >= 5                      # the DP stage really ran
