"""The product's seed-to-seed walk (csrc/walk_device.h: the source wp_extend_kernel and walk_extend_kernel compile for gfx950),
compiled for the host by tests/host_walk and run on the CPU against the oracle: return code, merged sequence and step count of
every walk -- through Walk::run (general step only) and through the single-leaf fast path with its hand-over to the general step
(the loop of wp_extend_kernel), over the narrow and the wide rank-block layout, with and without k-mer tables.
The GPU parity tests run the same source on the device."""
from __future__ import annotations

import numpy as np
import pytest

from tests.host_walk import HostWalk
from tests.test_gpu_fm import _walk_descs


@pytest.fixture(scope="module")
def hw():
    return HostWalk()


def _units(ds):
    u = [np.fromfile(f"{ds.prefix}.{ext}", dtype=np.uint8)[30:] for ext in ("bwt", "rbwt")]
    return u, int(ds.off[-1]) + ds.n_reads


@pytest.fixture(scope="module")
def ds_units(small_ds):
    return _units(small_ds)


def _skip_descs(params, reads, count, seeds, skip):
    """Walks from seed i to seed i + skip (the seeds in between ignored): gaps of several hundred bases to more than a kilobase,
    most of them beyond what the walk can bridge -- the wide-frontier, failing, many-step walks."""
    descs, k = [], 0
    for r, n in enumerate(count):
        ss = seeds[k: k + n]
        k += n
        read = reads[r]
        for i in range(0, max(int(n) - skip, 0), skip):
            s, t = ss[i], ss[i + skip]
            if s[3] or t[3]:
                continue
            s_start, s_len, t_start, t_len = int(s[0]), int(s[1]), int(t[0]), int(t[1])
            s_end = s_start + s_len - 1
            interval = t_start - s_end - 1
            ext = min(int(s[5]), int(t[4])) - 2
            if interval < 0 or ext > s_len:
                continue
            min_sa = (params.pb_coverage // 60) * 3 if params.pb_coverage > 60 else 3
            descs.append((read[s_start: s_start + s_len][s_len - ext:], read[s_end + 1: s_end + 1 + interval], read[t_start: t_start + t_len],
                          interval, ext, ext + 2, min_sa))
    return descs


def _in_domain(params, desc):
    """The walks the reference itself can take with these params: source, target and start k-mer at least as long as the k-mers it
    cuts from them (it throws from substr on shorter ones)."""
    src, _, trg, _, initk = desc[:5]
    return min(len(src), len(trg), initk) >= max(params.min_kmer_len, params.idmer_len)


def _check(hw, api, oracle, small_ds, ds_units, genome, cov, tables, wide, n_reads, modes=(0, 1), skip=0):
    (u0, u1), n_sym = ds_units
    h = hw.index(u0, u1, n_sym, wide=wide, tables=tables)
    p = api.params_default(genome, cov)
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    off = small_ds.off[: n_reads + 1].copy()
    bases = small_ds.bases[: int(off[-1])]
    count, seeds, _ = oracle.find_seeds(ob, orb, p, bases, off)
    descs = _skip_descs(p, small_ds.reads[:n_reads], count, seeds, skip) if skip else _walk_descs(p, small_ds.reads[:n_reads], count, seeds)
    codes, fast, steps = {}, 0, 0
    for d in descs:
        wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
        for mode in modes:
            code, merged, st, nf = hw.extend_walk(h, p, *d, mode)
            assert (code, merged, st) == (wcode, wmerged, wst[0]), (mode, d)
            if mode == 1:
                fast += nf; steps += st
        codes[wcode] = codes.get(wcode, 0) + 1
    hw.index_free(h)
    ob.close(); orb.close()
    return len(descs), codes, fast, steps


def test_host_walk_matches_oracle(hw, api, oracle, small_ds, ds_units):
    n, codes, fast, steps = _check(hw, api, oracle, small_ds, ds_units, 5, 90, (5, 9, 11), False, 40)
    assert n > 100 and codes.get(1, 0) > n // 2 and codes.get(-1, 0) > 0
    assert fast > steps // 2                                  # the fast path carries most steps, the hand-over the rest


def test_host_walk_without_tables_and_wide_layout(hw, api, oracle, small_ds, ds_units):
    _check(hw, api, oracle, small_ds, ds_units, 10, 90, (), False, 12)
    _check(hw, api, oracle, small_ds, ds_units, 5, 90, (5, 9), True, 12)


def test_host_walk_long_gaps(hw, api, oracle, small_ds, ds_units):
    """Seed i to seed i + 4: result paths beyond 64 words, frontiers of many leaves, walks that fail after hundreds of steps."""
    n, codes, fast, steps = _check(hw, api, oracle, small_ds, ds_units, 5, 90, (5, 9, 11), False, 30, skip=4)
    assert n >= 40 and steps > 20 * n and sum(v for c, v in codes.items() if c <= 0) > 0


def test_host_walk_repeat_dataset(hw, api, oracle, repeat_ds):
    """Repeat-rich reads: repeat-to-unique walks on the reverse strand, the isInsufficientFreqs / SelectFreqsOfrange branch."""
    n, codes, fast, steps = _check(hw, api, oracle, repeat_ds, _units(repeat_ds), 5, 90, (5, 9), False, 60)
    assert n > 100 and len(codes) >= 2


# ---- -i / -s / -e / -c away from their defaults ---------------------------------------------------------------------------------
# (idmer_len, min_kmer_len, error_rate, coverage); the default setting is the yardstick of the histogram check
DEFAULT_SETTING = (9, 13, .15, 90)
OPTION_SETTINGS = [(7, 13, .15, 90), (5, 13, .15, 90), (12, 13, .15, 90), (13, 13, .15, 90), (16, 17, .15, 90),
                   (9, 11, .15, 90), (9, 9, .15, 90), (9, 17, .15, 90),
                   (9, 13, .05, 90), (9, 13, .30, 90), (9, 13, .15, 30), (11, 15, .10, 60)]
MUST_DIFFER = [(5, 13, .15, 90), (9, 13, .30, 90), (9, 13, .15, 30)]      # settings whose oracle code histogram must not be the default's
OPTION_CASES = [(s, t) for s in OPTION_SETTINGS for t in ((5, 9, 11), ())] + [((7, 13, .15, 90), (5, 7, 13))]
N_OPTION_READS = 15
_OPTION_WANT = {}


def _option_params(api, setting):
    idmer, mink, err, cov = setting
    p = api.params_default(5, cov)
    p.idmer_len, p.min_kmer_len, p.error_rate = idmer, mink, err
    return p


def _option_want(api, oracle, ds, setting):
    """The walks of a setting (consecutive seeds plus seed i to seed i + 3, inside the reference's domain) and what the oracle makes
    of each, computed once per setting and shared by its table configurations."""
    if setting not in _OPTION_WANT:
        p = _option_params(api, setting)
        ob, orb = oracle.bwt_load(ds.prefix + ".bwt"), oracle.bwt_load(ds.prefix + ".rbwt")
        off = ds.off[: N_OPTION_READS + 1].copy()
        count, seeds, _ = oracle.find_seeds(ob, orb, p, ds.bases[: int(off[-1])], off)
        reads = ds.reads[:N_OPTION_READS]
        descs = [d for d in _walk_descs(p, reads, count, seeds) + _skip_descs(p, reads, count, seeds, 3) if _in_domain(p, d)]
        want = []
        for d in descs:
            wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
            want.append((wcode, wmerged, wst[0]))
        ob.close(); orb.close()
        _OPTION_WANT[setting] = (descs, want)
    return _OPTION_WANT[setting]


def _histogram(want):
    h = {}
    for code, _, _ in want:
        h[code] = h.get(code, 0) + 1
    return h


@pytest.mark.parametrize("setting,tables", OPTION_CASES, ids=lambda v: "-".join(str(x) for x in v) or "notab")
def test_host_walk_options(hw, api, oracle, small_ds, ds_units, setting, tables):
    """Walk::run and the wp_extend_kernel loop under non-default idmer_len / min_kmer_len / error_rate / coverage: with tables of
    5 / 9 / 11 (the fast table path only where the setting's sizes are among them), without tables (the generic path), and for
    idmer_len 7 with tables of 5 / 7 / 13 (the fast table path with a 7-base seed)."""
    descs, want = _option_want(api, oracle, small_ds, setting)
    hist = _histogram(want)
    assert len(descs) >= 100 and hist.get(1, 0) > 0 and hist.get(-1, 0) > 0, hist
    if setting in MUST_DIFFER:
        assert hist != _histogram(_option_want(api, oracle, small_ds, DEFAULT_SETTING)[1])
    (u0, u1), n_sym = ds_units
    h = hw.index(u0, u1, n_sym, wide=False, tables=tables)
    p = _option_params(api, setting)
    try:
        for d, w in zip(descs, want):
            for mode in (0, 1):
                code, merged, st, _ = hw.extend_walk(h, p, *d, mode)
                assert (code, merged, st) == w, (mode, d)
    finally:
        hw.index_free(h)
