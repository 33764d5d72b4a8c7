"""dp_align_kernel (the device extendMatch) against the oracle's extend_match where the traceback takes a run of M steps per trip: every
SequenceOverlap field and the cigar, bit for bit, none skipped or tolerated.

A trip of the traceback evaluates the 16 columns of its trace window at once, takes the run of M steps from the current column downward
and the I or D step behind it, and cuts the run where the serial walk would have refreshed something: at the window's first column, at
the first row of the 64-row window of s2, at the next flush of 64 ops, at ti == 0 or tj == 0.  The pairs are the smallest at which one
of these can go wrong: a single run across every one of the edges (identical strings without equal neighbours, every length 1 .. 40 and
around 64, 128 and 256); one indel and one substitution at every position of a 40- and a 70-letter string, which gives runs of every
length that end at every offset of the windows (under the scores (2, -3, -5) the run passes over the substitution and edit_distance
counts it, under (1, -1, -8) it ends there); runs that end on the matrix edge (one string a prefix of the other, or about 300 longer,
the seed at the start and at the end); runs of 1 - 6 equal letters, where the homopolymer tests change the table entry inside a run; a
junk prefix on either string, which moves the path into each quarter of the band's rows (the four lanes of a column); band widths 2 and
3; one pair beyond the LDS stage (the global variant's windows); and a few hundred seeded pairs at 2 %, 10 % and 30 % mutations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCORES = ((1, -1, -8), (2, -3, -5))
EDGE_LENGTHS = tuple(range(1, 41)) + tuple(range(62, 68)) + tuple(range(126, 132)) + tuple(range(254, 260))


@pytest.fixture(scope="module")
def gpu_ctx(api, small_ds):
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    yield ctx
    ctx.close()
    idx.close()


def _plain(rng, n, letters="ACGT"):
    """n letters, no two neighbours equal (one letter: as it is)."""
    out = []
    while len(out) < n:
        c = letters[rng.integers(len(letters))]
        if len(letters) == 1 or not out or out[-1] != c:
            out.append(c)
    return "".join(out)


def _runs(rng, n, letters, longest=6):
    out = []
    while len(out) < n:
        out.extend(letters[rng.integers(len(letters))] * int(rng.integers(1, longest + 1)))
    return "".join(out[:n])


def _mutate(rng, s, rate):
    out = []
    for c in s:
        u = rng.random()
        if u < rate:
            continue
        if u < 2 * rate:
            c = "ACGT"[rng.integers(4)]
        out.append(c)
        if rng.random() < rate:
            out.append("ACGT"[rng.integers(4)])
    return "".join(out) or "A"


def _both_seeds(s1, s2):
    k = min(17, len(s1), len(s2))
    return [(s1, s2, 0, 0), (s1, s2, len(s1) - k, len(s2) - k)]


def _other(c):
    return "ACGT"[("ACGT".index(c) + 2) % 4]


def _edge_pairs():
    """One run across every window edge; one indel, one substitution at every position; runs of equal letters."""
    rng = np.random.default_rng(372412)
    single, indel, subst, homo = [], [], [], []
    for L in EDGE_LENGTHS:
        s = _plain(rng, L)
        single.append((s, s, 0, 0))
    for L in (40, 70):
        s = _plain(rng, L)
        for p in range(L):
            shorter = s[:p] + s[p + 1:] or "A"
            indel += [(shorter, s, 0, 0), (s, shorter, 0, 0)]
            subst.append((s, s[:p] + _other(s[p]) + s[p + 1:], 0, 0))
    for letters in ("A", "AC", "ACGT"):
        for L in EDGE_LENGTHS:
            s = _runs(rng, L, letters)
            homo.append((s, s, 0, 0))
            homo.append((s, _mutate(rng, s, 0.04), 0, 0))
    return single, indel, subst, homo


@pytest.fixture(scope="module")
def edge_pairs():
    return _edge_pairs()


@pytest.fixture(scope="module")
def matrix_edge_pairs():
    """The run is cut by ti == 0 or tj == 0: one string a prefix of the other, one about 300 longer, the seed at either end."""
    rng = np.random.default_rng(4120)
    pairs = []
    for L in (5, 16, 40, 70, 130):
        s = _plain(rng, L)
        for extra in (1, 17, 300):
            longer = s + _plain(rng, extra)
            pairs += _both_seeds(s, longer) + _both_seeds(longer, s)
            longer = _plain(rng, extra) + s
            pairs += _both_seeds(s, longer) + _both_seeds(longer, s)
    return pairs


@pytest.fixture(scope="module")
def quarter_pairs():
    """A junk prefix on one string, the seed at (0, 0): the path runs that many band rows off the centre diagonal."""
    rng = np.random.default_rng(64128192)
    pairs = []
    for junk in (30, 60, 90, 95, 120):
        for body in (_plain(rng, 150), _runs(rng, 150, "ACGT", 4)):
            other = _mutate(rng, body, 0.03)
            pre = _plain(rng, junk, "AC")
            pairs += [(body, pre + other, 0, 0), (pre + body, other, 0, 0)]
    return pairs


@pytest.fixture(scope="module")
def long_pair():
    """Beyond the LDS stage (more than 66 kB of staging) with a handful of indels."""
    rng = np.random.default_rng(66001)
    s1 = _plain(rng, 34000)
    s2 = s1
    for p in sorted(rng.integers(100, 33900, size=6), reverse=True):
        s2 = s2[:p] + s2[p + 1:] if p & 1 else s2[:p] + "ACGT"[p % 4] + s2[p:]
    assert len(s1) + len(s2) > 66000
    return [(s1, s2, 0, 0)]


@pytest.fixture(scope="module")
def fuzz_pairs():
    rng = np.random.default_rng(210300)
    pairs = []
    for t in range(300):
        s = _runs(rng, int(rng.integers(1, 301)), "ACGT", 3)
        pairs.append((s, _mutate(rng, s, (0.02, 0.10, 0.30)[t % 3])[:300], 0, 0))
    return pairs


def _check(gpu_ctx, oracle, pairs, bw, scores):
    got = gpu_ctx.dp_align(pairs, band_width=bw, scores=scores)
    assert len(got) == len(pairs)
    for (s1, s2, a, b), g in zip(pairs, got):
        want = oracle.extend_match(s1, s2, a, b, bandwidth=bw, scores=scores)
        assert g == want, (bw, scores, len(s1), len(s2), a, b, s1[:400], s2[:400])
    return got


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("bw", (2, 3, 200, 254))
def test_runs_across_window_edges(gpu_ctx, oracle, edge_pairs, bw, scores):
    single, indel, subst, homo = edge_pairs
    got = _check(gpu_ctx, oracle, single, bw, scores)
    assert [g["cigar"] for g in got] == [f"{len(s)}M" for s, _, _, _ in single]
    got = _check(gpu_ctx, oracle, indel, bw, scores)
    assert sum("I" in g["cigar"] for g in got) > 60 and sum("D" in g["cigar"] for g in got) > 60
    got = _check(gpu_ctx, oracle, subst, bw, scores)
    if scores == SCORES[1]:                                    # the run passes over the mismatch
        assert sum(g["cigar"] == f"{len(s1)}M" and g["edit"] == 1 for g, (s1, _, _, _) in zip(got, subst)) > 80
    else:                                                      # a gap on either side is cheaper than the mismatch
        assert sum(g["edit"] == 2 for g in got) > 80
    _check(gpu_ctx, oracle, homo, bw, scores)


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("bw", (200, 254))
def test_runs_to_the_matrix_edge_and_in_every_band_quarter(gpu_ctx, oracle, matrix_edge_pairs, quarter_pairs, bw, scores):
    _check(gpu_ctx, oracle, matrix_edge_pairs, bw, scores)
    got = _check(gpu_ctx, oracle, quarter_pairs, bw, scores)
    assert sum(g["cols"] > 100 for g in got) > len(got) // 2


@pytest.mark.parametrize("scores", SCORES)
def test_pair_beyond_the_lds_stage(gpu_ctx, oracle, long_pair, scores):
    got = _check(gpu_ctx, oracle, long_pair, 200, scores)
    assert got[0]["cols"] > 33000 and "I" in got[0]["cigar"] and "D" in got[0]["cigar"]


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("bw", (3, 200))
def test_seeded_fuzz(gpu_ctx, oracle, fuzz_pairs, bw, scores):
    _check(gpu_ctx, oracle, fuzz_pairs, bw, scores)
