"""dp_align_kernel (the device extendMatch) against the oracle's extend_match on a few thousand seeded pairs: every SequenceOverlap field
and the cigar, bit for bit, none skipped or tolerated.

The pairs cover what the fill's column classes and the host's staging-size launches distinguish: lengths 1 .. 3000 (and up to the
global-workspace variant in the mixed batch), error profiles from identical to unrelated, homopolymer runs, truncated s2, seed
positions anywhere in the two strings (the band is then cut by the first row, by the last row, by both, or leaves the matrix
after a few columns), band widths 2, 3, 11, 64, 200, 254 and two score sets.  Seed positions stay inside their strings, as
extendMatch's callers pass them: the band's centre diagonal then crosses the matrix and ends on its last row or column."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BANDS = (2, 3, 11, 64, 200, 254)
SCORES = ((1, -1, -8), (2, -3, -5))          # the product's (LongReadOverlap.cpp:635-643) and another


@pytest.fixture(scope="module")
def gpu_ctx(api, small_ds):
    idx = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    idx.upload(0)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    yield ctx
    ctx.close()
    idx.close()


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


ERRORS = [(0, 0, 0), (0.01, 0.03, 0.02), (0.015, 0.09, 0.045), (0.05, 0.15, 0.1), (0.3, 0.3, 0.3)]


def _pair(rng, t, max_len):
    """One (s1, s2, start1, start2); t picks the kind."""
    kind = t % 11
    if kind == 0:                                             # very short strings: one-column / one-row matrices
        L = int(rng.integers(1, 6))
    elif kind in (1, 2):
        L = int(rng.integers(6, 120))
    else:
        L = int(rng.integers(120, max_len + 1))
    s1 = _rand_seq(rng, L)
    if kind in (3, 4):                                        # homopolymer-rich
        s1 = "".join(c * int(rng.integers(1, 6)) for c in s1)[:L]
    if kind == 5:                                             # unrelated
        s2 = _rand_seq(rng, int(rng.integers(1, max_len + 1)))
    else:
        s2 = _mutate(rng, s1 + _rand_seq(rng, int(rng.integers(0, 80))), *ERRORS[t % 5]) or "A"
        if kind == 6:                                         # truncated (the LF-walk hit a '$')
            s2 = s2[: int(rng.integers(1, len(s2) + 1))]
        elif kind == 7:                                       # s2 starts before s1
            s2 = _rand_seq(rng, int(rng.integers(1, 300))) + s2
        elif kind == 8:                                       # s2 is a piece from the middle of s1
            a = int(rng.integers(0, len(s2)))
            s2 = s2[a: a + int(rng.integers(1, len(s2) - a + 1))]
    if not s2:
        s2 = "A"
    L1, L2 = len(s1), len(s2)
    mode = int(rng.integers(0, 4))
    if mode == 0:                                             # forward extension: the shared k-mer starts both strings
        a, b = 0, 0
    elif mode == 1:                                           # backward extension: it ends them
        k = min(17, L1, L2)
        a, b = L1 - k, L2 - k
    elif mode == 2:                                           # a seed somewhere on a nearby diagonal
        a = int(rng.integers(0, L1))
        b = int(np.clip(a + rng.integers(-130, 131), 0, L2 - 1))
    else:                                                     # anywhere: the band crosses a corner of the matrix
        a, b = int(rng.integers(0, L1)), int(rng.integers(0, L2))
    return s1, s2, a, b


def _check(gpu_ctx, oracle, pairs, bw, scores):
    got = gpu_ctx.dp_align(pairs, band_width=bw, scores=scores)
    assert len(got) == len(pairs)
    for (s1, s2, a, b), g in zip(pairs, got):
        want = oracle.extend_match(s1, s2, a, b, bandwidth=bw, scores=scores)
        assert g == want, (bw, scores, len(s1), len(s2), a, b, s1[:400], s2[:400])
    return got


def test_product_band_and_scores(gpu_ctx, oracle):
    rng = np.random.default_rng(20240)
    pairs = [_pair(rng, t, 3000) for t in range(1100)]
    got = _check(gpu_ctx, oracle, pairs, 200, SCORES[0])
    assert sum(("I" in g["cigar"]) or ("D" in g["cigar"]) for g in got) > 300
    assert sum(g["cols"] > 1000 for g in got) > 100


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("bw", BANDS)
def test_band_widths_and_scores(gpu_ctx, oracle, bw, scores):
    rng = np.random.default_rng(1000 * bw + scores[0])
    _check(gpu_ctx, oracle, [_pair(rng, t, 1500) for t in range(165)], bw, scores)


def test_every_staging_class_in_one_call(gpu_ctx, oracle):
    """Pairs of every staging-size class (4 KB, 16 KB, 64 KB of LDS) and one beyond the LDS stage, interleaved in one call: each LDS
    launch and the global-workspace variant run, and each must leave the others' results alone."""
    rng = np.random.default_rng(777)
    pairs = []
    for t in range(60):
        lo, hi = [(30, 1500), (2500, 7000), (9000, 30000)][t % 3]
        L = int(rng.integers(lo, hi))
        s1 = _rand_seq(rng, L)
        s2 = _mutate(rng, s1 + _rand_seq(rng, 40), *ERRORS[1 + t % 3])
        if t % 4 == 0:
            pairs.append((s1, s2, 0, 0))
        else:
            k = 17
            pairs.append((s1, s2, L - k, len(s2) - k) if s2[-k:] == s1[-k:] else (s1, s2, L // 2, min(L // 2, len(s2) - 1)))
    s1 = _rand_seq(rng, 34000)
    pairs.insert(31, (s1, _mutate(rng, s1, 0.01, 0.03, 0.02), 0, 0))            # 68 kB of staging: the global-workspace variant
    pairs.insert(7, ("ACGT", "ACGA", 0, 0))
    sizes = [len(a) + len(b) for a, b, _, _ in pairs]
    assert min(sizes) < 3500 and any(4500 < s < 15000 for s in sizes) and any(17000 < s < 64000 for s in sizes) and max(sizes) > 66000
    _check(gpu_ctx, oracle, pairs, 200, SCORES[0])
