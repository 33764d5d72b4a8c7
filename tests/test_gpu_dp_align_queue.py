"""The align launches hand their alignments to the wavefronts from a queue: per staging-size class a list of job indices
(csrc/dp_order.h), a wavefront's first ticket its block index, every further one drawn from the launch's head word
(dp_align_kernel).  Results must not depend on who ran what: dp_align_kernel against the oracle's extend_match, field for field and
cigar for cigar, with LRSC_DP_ALIGN_WAVES capping the wavefronts of every launch at 1, 2 and 7 (every wavefront draws many tickets), at
one class's job count and one below it (where the static first tickets and the first drawn ticket meet), and unset.

The pairs: the three LDS classes interleaved so that no class's jobs are contiguous, one pair beyond 64 KB of staging (a class with
exactly one job, the global-workspace launch), short alignments among long ones, and one pair with an empty s2.  extendMatch
itself does not admit an empty sequence (the oracle asserts on it), so that pair is held to the record the entry point documents for
an alignment it does not run; it is here because it leaves the kernel's job loop early and must still draw the next ticket.

The whole DP path: correct_reads with the DP fallback on small_ds, LRSC_DP_ALIGN_WAVES=3 with LRSC_DP_CHUNK_MB=1 (several chunks: the
lists are built from chunk-relative job indices of requests with begin > 0), against the oracle and against a run with neither set."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PAIRS = 150
CLASS_LEN = [(30, 1500), (2300, 6000), (8500, 11000)]          # 4 KB, 16 KB, 64 KB of staging for s1 and an s2 of about its length
EMPTY = dict(m0s=0, m0e=-1, m1s=0, m1e=-1, score=-1, edit=-1, cols=-1, cigar="")
ERRORS = [(0.01, 0.03, 0.02), (0.015, 0.09, 0.045), (0.05, 0.15, 0.1)]


def _rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def _mutate(rng, s, sub, ins, dele):
    out = []
    for c in s:
        u = rng.random()
        if u < dele:
            continue
        if u < dele + sub:
            c = "ACGT"[rng.integers(4)]
        out.append(c)
        while rng.random() < ins:
            out.append("ACGT"[rng.integers(4)])
    return "".join(out)


def _stage_class(s1, s2):
    """dp_align_class(dp_align_stage_bytes(..)) of csrc/dp_order.h."""
    sb = ((len(s1) + 2 + 3) & ~3) + 264 + ((len(s2) + 3) & ~3) + 16
    return sum(sb > cap for cap in (4096, 16384, 65536))


@pytest.fixture(scope="module")
def gpu_ctx(api, small_ds):
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    yield ctx
    ctx.close()
    idx.close()


@pytest.fixture(scope="module")
def workload(oracle):
    """(pairs, expected results, jobs per class); computed once and left unchanged."""
    rng = np.random.default_rng(4711)
    pairs = []
    for t in range(N_PAIRS - 2):
        lo, hi = CLASS_LEN[t % 3]
        L = int(rng.integers(lo, hi))
        if t % 5 == 0:
            L = lo + 100 * (t % 3)                                # the shortest of its class
        s1 = _rand_seq(rng, L)
        s2 = _mutate(rng, s1 + _rand_seq(rng, int(rng.integers(0, 60))), *ERRORS[t % 3]) or "A"
        if t % 4 == 0:
            pairs.append((s1, s2, 0, 0))
        elif t % 4 == 1:
            pairs.append((s1, s2[: max(1, len(s2) // 2)], 0, 0))  # truncated s2: a short alignment in a long class
        else:
            pairs.append((s1, s2, L // 2, min(L // 2, len(s2) - 1)))
    s1 = _rand_seq(rng, 34000)
    pairs.insert(77, (s1, _mutate(rng, s1, 0.01, 0.03, 0.02), 0, 0))            # 68 kB of staging: the global-workspace variant
    pairs.insert(20, (_rand_seq(rng, 900), "", 0, 0))
    assert len(pairs) == N_PAIRS
    classes = [_stage_class(a, b) for a, b, _, _ in pairs]
    counts = [classes.count(k) for k in range(4)]
    assert min(counts[:3]) > 25 and counts[3] == 1, counts
    # interleaved: every class from one end of the call to the other, never three neighbours of one class
    assert all(classes.index(k) < 10 and classes[::-1].index(k) < 10 for k in range(3)), classes
    assert not any(classes[i] == classes[i + 1] == classes[i + 2] for i in range(N_PAIRS - 2)), classes
    want = [EMPTY if not s2 else oracle.extend_match(s1, s2, a, b, bandwidth=200, scores=(1, -1, -8)) for s1, s2, a, b in pairs]
    return pairs, want, counts


@pytest.mark.parametrize("waves", [None, 1, 2, 7, "class", "class - 1"])
def test_results_do_not_depend_on_who_draws(gpu_ctx, workload, monkeypatch, waves):
    pairs, want, counts = workload
    if waves is None:
        monkeypatch.delenv("LRSC_DP_ALIGN_WAVES", raising=False)
    else:
        cap = waves if isinstance(waves, int) else counts[2] - (waves != "class")
        monkeypatch.setenv("LRSC_DP_ALIGN_WAVES", str(cap))
    got = gpu_ctx.dp_align(pairs, band_width=200, scores=(1, -1, -8))
    assert len(got) == len(pairs)
    for i, ((s1, s2, a, b), g, w) in enumerate(zip(pairs, got, want)):
        assert g == w, (waves, i, len(s1), len(s2), a, b, s1[:200], s2[:200])


NAMES = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
         "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")


def test_whole_dp_path_with_few_wavefronts_and_small_chunks(api, oracle, small_ds, monkeypatch):
    p = api.params_default(5, 90)
    p.no_dp = 0
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    want = oracle.correct_reads(ob, orb, p, small_ds.bases, small_ds.off)
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    reads = small_ds.reads
    runs = []
    for env in ({"LRSC_DP_ALIGN_WAVES": "3", "LRSC_DP_CHUNK_MB": "1"}, {}):
        for name in ("LRSC_DP_ALIGN_WAVES", "LRSC_DP_CHUNK_MB"):
            if name in env:
                monkeypatch.setenv(name, env[name])
            else:
                monkeypatch.delenv(name, raising=False)
        ctx = idx.ctx(p, 0)
        results, pieces = ctx.correct_reads(small_ds.bases, small_ds.off)
        ctx.close()
        cfa = "".join(f">r{r}\n{ps[0]}\n" for r, (res, ps) in enumerate(zip(results, pieces)) if res.merge)
        dfa = "".join(f">r{r}\n{reads[r]}\n" for r, res in enumerate(results) if not res.merge)
        got = np.array([[getattr(r, f) for f in NAMES] for r in results], dtype=np.int64)
        assert cfa == want.correct_fa and dfa == want.discard_fa, env
        np.testing.assert_array_equal(got, want.counters)
        runs.append((cfa, dfa, got))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])
    assert runs[0][2][:, 8].sum() > 20                            # walks that went through the DP fallback
    idx.close()
    want.close(); ob.close(); orb.close()
