"""The general-step counters of the bulk extension launch (`LRSC_CORRECT_PROFILE=1`, WpArgs::gen_stats, wp_gen_count in wp_walk.h; `-m gpu`).

At every general step a lane-per-walk wavefront of round 0's bulk launch takes, the first lane taking part adds: 1, the lanes taking
part, the sum and the maximum of their frontiers (n_cur), the same of their children after extendLeaves (n_nxt), maximum x lanes
for both, and the passes of 64 lanes the leaves / children would fill.  The sums come from ballots over bit planes; this file holds
them to what any such step satisfies, and the run with the counters on to the results and the rank-query counts of the run without."""
from __future__ import annotations

import re

import numpy as np
import pytest

from longreadselfcorrect_amd.capi import K_EXTEND
from tests.test_gpu_fm import _fasta

pytestmark = pytest.mark.gpu

NAMES = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
         "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")


@pytest.fixture(scope="module")
def index(api, small_ds):
    i = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    i.upload(0)
    yield i
    i.close()


def _run(api, index, small_ds):
    p = api.params_default(5, 90)
    p.no_dp = 1
    ctx = index.ctx(p, 0)
    ctx.stats_reset()
    results, pieces = ctx.correct_reads(small_ds.bases, small_ds.off)
    st = ctx.stats(K_EXTEND)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, small_ds.reads, p.split)
    got = np.array([[getattr(r, n) for n in NAMES] for r in results], dtype=np.int64)
    return cfa, dfa, got, (int(st.launches), int(st.rank_queries), int(st.block_loads))


def test_counters_of_the_bulk_launch(api, index, small_ds, monkeypatch, capfd):
    monkeypatch.delenv("LRSC_CORRECT_PROFILE", raising=False)
    plain = _run(api, index, small_ds)
    monkeypatch.setenv("LRSC_CORRECT_PROFILE", "1")
    capfd.readouterr()
    prof = _run(api, index, small_ds)
    err = capfd.readouterr().err
    # counting changes nothing
    assert plain[0] == prof[0] and plain[1] == prof[1]
    np.testing.assert_array_equal(plain[2], prof[2])
    assert plain[3] == prof[3] and plain[3][1] > 0
    m = re.search(r"wp bulk launches, general steps of a wavefront: .*counters ((?:\d+ ?){10})", err)
    assert m, err[-2000:]
    steps, lanes, s_cur, mx_cur, s_nxt, mx_nxt, pay_cur, pay_nxt, pass_cur, pass_nxt = map(int, m.group(1).split())
    print(m.group(0))
    assert steps > 0 and steps <= lanes <= 64 * steps
    assert lanes > steps, "no step with company: the quorum never gathered two lanes on this set"
    # a lane taking part has a frontier of at least one leaf; a wavefront's widest frontier is one of them
    assert lanes <= s_cur and steps <= mx_cur <= s_cur
    assert mx_cur < s_cur, "every step had one lane"
    assert s_cur <= pay_cur <= 64 * mx_cur and mx_cur <= pay_cur
    assert steps <= pass_cur <= mx_cur                       # sum <= 64 x maximum
    # children: a step may end with none
    assert mx_nxt <= s_nxt <= pay_nxt <= 64 * mx_nxt
    assert pass_nxt <= mx_nxt and 64 * pass_nxt >= s_nxt
    assert s_nxt > 0
