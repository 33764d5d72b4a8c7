"""dp_align_kernel (the device extendMatch) against the oracle's extend_match where the traceback's choice is decided by ties and by the
sequence tests: every SequenceOverlap field and the cigar, bit for bit, none skipped or tolerated.

The fill stores two score comparisons per cell and the traceback finishes the reference's decision tree from the two homopolymer tests
and the mismatch test, which it takes from windows of the sequences (s1: the 16 columns of a trace fetch; s2: 64 rows across the
lanes).  The pairs are chosen so that the three score comparisons tie and those tests sit on the windows' and the strings' edges:
alphabets of one and two letters at every (L1, L2) in 1..9 x 1..9, homopolymer runs that end exactly where s1 and s2 end (the sentinel
compares), every L1 mod 4 and the lengths around 16, 32, 64, 128 and 256, s2 about 300 longer than s1 and the reverse (the traceback
starts on the last column / on the last row), each with the seed at the start and at the end, band widths 2, 3, 200, 254 and both
score sets of the fuzz test; and one pair of runs of 1-6 equal letters beyond the LDS stage (the global variant's character windows)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BANDS = (2, 3, 200, 254)
SCORES = ((1, -1, -8), (2, -3, -5))
EDGE_LENGTHS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257)


@pytest.fixture(scope="module")
def gpu_ctx(api, small_ds):
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    yield ctx
    ctx.close()
    idx.close()


def _seq(rng, n, letters):
    return "".join(letters[c] for c in rng.integers(0, len(letters), size=n))


def _runs(rng, n, letters="ACGT", longest=6):
    """n characters in runs of 1 .. longest equal letters."""
    out = []
    while len(out) < n:
        out.extend(letters[rng.integers(len(letters))] * int(rng.integers(1, longest + 1)))
    return "".join(out[:n])


def _mutate(rng, s, rate, letters):
    out = []
    for c in s:
        u = rng.random()
        if u < rate:
            continue
        if u < 2 * rate:
            c = letters[rng.integers(len(letters))]
        out.append(c)
        if rng.random() < rate:
            out.append(letters[rng.integers(len(letters))])
    return "".join(out) or letters[0]


def _both_seeds(s1, s2):
    """The seed at the start of both strings and at their end, as the forward and the backward extension pass it."""
    k = min(17, len(s1), len(s2))
    return [(s1, s2, 0, 0), (s1, s2, len(s1) - k, len(s2) - k)]


def _tie_pairs():
    rng = np.random.default_rng(604661)
    pairs = []
    for L1 in range(1, 10):                                    # one and two letters, every small shape
        for L2 in range(1, 10):
            pairs += _both_seeds("A" * L1, "A" * L2)
            for _ in range(2):
                pairs += _both_seeds(_seq(rng, L1, "AC"), _seq(rng, L2, "AC"))
    for k1 in range(0, 6):                                     # runs that end exactly at the end of s1 and / or of s2
        for k2 in range(0, 6):
            body = _runs(rng, int(rng.integers(20, 90)), "ACG")
            pairs += _both_seeds(body + "T" * k1, _mutate(rng, body, 0.05, "ACG") + "T" * k2)
    for L in EDGE_LENGTHS:                                     # the 16-column and 64-lane windows, every L1 mod 4
        s = _runs(rng, L, "AC", 4)
        pairs += _both_seeds(s, s)
        pairs += _both_seeds(s, _mutate(rng, s, 0.08, "AC"))
        pairs += _both_seeds(_mutate(rng, s, 0.08, "AC"), s)
        pairs += _both_seeds(_runs(rng, L, "ACGT"), _runs(rng, L + int(rng.integers(-2, 3)), "ACGT"))
    for L in (40, 257, 700):                                   # the traceback starts on the last column / on the last row
        s = _runs(rng, L, "ACGT")
        longer = _mutate(rng, s, 0.04, "ACGT") + _runs(rng, 300, "ACGT")
        pairs += _both_seeds(s, longer) + _both_seeds(longer, s)
        longer = _runs(rng, 300, "AC") + _mutate(rng, s, 0.04, "ACGT")
        pairs += _both_seeds(s, longer) + _both_seeds(longer, s)
    return pairs


@pytest.fixture(scope="module")
def tie_pairs():
    return _tie_pairs()


@pytest.fixture(scope="module")
def long_pair():
    """Beyond the LDS stage (more than 66 kB of staging): runs of 1-6 equal letters, so the homopolymer tests hold at every few cells of a
    traceback that crosses hundreds of windows of each string."""
    rng = np.random.default_rng(66000)
    s1 = _runs(rng, 34000)
    s2 = _mutate(rng, s1, 0.02, "ACGT")
    assert len(s1) + len(s2) > 66000
    return [(s1, s2, 0, 0)]


def _check(gpu_ctx, oracle, pairs, bw, scores):
    got = gpu_ctx.dp_align(pairs, band_width=bw, scores=scores)
    assert len(got) == len(pairs)
    for (s1, s2, a, b), g in zip(pairs, got):
        want = oracle.extend_match(s1, s2, a, b, bandwidth=bw, scores=scores)
        assert g == want, (bw, scores, len(s1), len(s2), a, b, s1[:400], s2[:400])
    return got


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("bw", BANDS)
def test_ties_and_window_edges(gpu_ctx, oracle, tie_pairs, bw, scores):
    got = _check(gpu_ctx, oracle, tie_pairs, bw, scores)
    assert sum("I" in g["cigar"] for g in got) > 20 and sum("D" in g["cigar"] for g in got) > 20


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("bw", BANDS)
def test_pair_beyond_the_lds_stage(gpu_ctx, oracle, long_pair, bw, scores):
    _check(gpu_ctx, oracle, long_pair, bw, scores)
