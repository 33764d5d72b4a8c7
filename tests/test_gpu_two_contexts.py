"""Two contexts on one device, each correcting half of the small read set from its own host thread (the way bench.py runs the two
parts of a step), must give what one context gives and what the oracle gives: corrected strings, discarded reads and every counter.
While one context is in its DP stage the other one's extension kernels are in flight, so this is where the streams' hardware queues
and the MSA launches' LDS budget ("A part's DP stage beside the other part's kernels") can go wrong.

Each case is a fresh process (tests/two_contexts_child.py): the runtime reads GPU_MAX_HW_QUEUES when it starts.  Cases: 4 hardware
queues (21 streams used to share them) and 16; LRSC_MSA_LDS_MAX=12288, which puts the small set's pile-ups on both sides of the
MSA launches' LDS ceiling, and LRSC_MSA_LDS_MAX=1, which sends every pile-up to the global-workspace variant."""
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
CASES = {"queues4": {"GPU_MAX_HW_QUEUES": "4"}, "queues16": {"GPU_MAX_HW_QUEUES": "16"},
         "lds_max_12288": {"GPU_MAX_HW_QUEUES": "4", "LRSC_MSA_LDS_MAX": "12288"},
         "lds_max_1": {"GPU_MAX_HW_QUEUES": "4", "LRSC_MSA_LDS_MAX": "1"}}


@pytest.fixture(scope="module")
def want(api, oracle, small_ds):
    """The oracle's run over the whole small set, default flow (DP fallback on): computed once for every case."""
    p = api.params_default(5, 90)
    p.no_dp = 0
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    w = oracle.correct_reads(ob, orb, p, small_ds.bases, small_ds.off)
    got = (w.correct_fa, w.discard_fa, np.array(w.counters, dtype=np.int64))
    w.close(); ob.close(); orb.close()
    return got


@pytest.fixture(scope="module")
def reads_npz(small_ds, tmp_path_factory):
    path = tmp_path_factory.mktemp("two_ctx") / "reads.npz"
    np.savez(path, bases=small_ds.bases, off=small_ds.off)
    return path


_runs: dict[str, dict] = {}


def run_case(name, small_ds, reads_npz, tmp_path_factory):
    if name not in _runs:
        out = tmp_path_factory.mktemp("two_ctx_" + name) / "out.json"
        env = {k: v for k, v in os.environ.items() if not k.startswith("LRSC_MSA_")}
        env.update(CASES[name])
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "two_contexts_child.py"), small_ds.prefix, str(reads_npz), str(out)],
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"{name}: child exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        _runs[name] = json.loads(out.read_text())
    return _runs[name]


def fasta_and_counters(rows, reads):
    correct, discard = [], []
    for r, row in enumerate(rows):
        if row["c"][NAMES.index("merge")]:
            correct += [f">r{r}\n{p}\n" for p in row["p"]]
        else:
            discard.append(f">r{r}\n{reads[r]}\n")
    return "".join(correct), "".join(discard), np.array([row["c"][:11] for row in rows], dtype=np.int64)


@pytest.mark.parametrize("name", list(CASES))
def test_two_contexts_equal_one_context_and_oracle(name, want, small_ds, reads_npz, tmp_path_factory):
    got = run_case(name, small_ds, reads_npz, tmp_path_factory)
    assert len(got["one"]) == len(got["two"]) == small_ds.n_reads
    assert all(row["c"][NAMES.index("status")] == 0 for row in got["one"] + got["two"])
    assert got["two"] == got["one"], "two contexts at once differ from one context"
    cfa, dfa, counters = fasta_and_counters(got["two"], small_ds.reads)
    assert cfa == want[0] and dfa == want[1]
    np.testing.assert_array_equal(counters, want[2])
    assert counters[:, 8].sum() >= 20                      # the DP stage (and with it the MSA launches) really ran
    if name != "queues4":                                  # the switches change where a pile-up's state lives, never the output
        assert got == run_case("queues4", small_ds, reads_npz, tmp_path_factory)
