"""`stride pbcorrect`'s -e / -i / -s / -k -u -r / -m / -c / -l on the device (`-m gpu`), every one against the CPU oracle with the
same lrsc_params: correct.fa, discard.fa and all eleven per-read counters of the whole path; return code, merged sequence and step
count of explicit walks.  Every comparison is exact.

The option sets (SETS) override params_default(5, 90).  Away from the defaults the per-walk tables leave the fast table path
(k-mer tables exist for 5 / 9 / 11 only on the small index), the seed codes and masks change width, the static k-mer sizes move
the seed slab, and -l below 32 trims the frontier.  Each whole-path case first checks that the oracle's own counters differ from
the oracle's at the defaults, so a device that ignored the option would fail.  The variants of the flow (per-walk rounds, the
serial and the wavefront kernel, the Block64 layout, no k-mer tables) are each held against the oracle, not against one another."""
from __future__ import annotations

import types

import numpy as np
import pytest

from longreadselfcorrect_amd.capi import K_DP, K_EXTEND, K_EXTEND_WIDE, K_MSA, K_SEEDS, LrscError
from tests.test_gpu_fm import _check_whole_path, _fasta, _walk_descs
from tests.test_gpu_wide_walk import N_READS as WIDE_N_READS
from tests.test_host_walk import _in_domain, _skip_descs

pytestmark = pytest.mark.gpu

NAMES = ("total_reads_len", "corrected_len", "total_seed_num", "total_walk_num", "high_error_num", "exceed_depth_num",
         "exceed_leave_num", "fm_num", "dp_num", "seed_dis", "merge")
FM, DP = NAMES.index("fm_num"), NAMES.index("dp_num")

SETS = {
    "E05": dict(error_rate=0.05), "E25": dict(error_rate=0.25),
    "I5": dict(idmer_len=5), "I7": dict(idmer_len=7), "I13": dict(idmer_len=13),
    "S9": dict(min_kmer_len=9), "S15": dict(min_kmer_len=15),
    "I11S11": dict(idmer_len=11, min_kmer_len=11),            # min_kmer_len <= idmer_len: the table path's early exit
    "C30": dict(coverage=30),                                   # more seeds, exceed_depth_num > 0, min_sa 3
    "K21": dict(start_kmer_len=21, offset=(0, 2, -4)),          # -k 21 -u 2 -r -4
    "K15": dict(start_kmer_len=15, offset=(0, 4, -2)),          # the smallest static k-mer drops to 13; differs on repeat_ds only
    "M0": dict(manual=1, mode=0),                               # -m 0
    "L4": dict(max_leaves=4), "L1": dict(max_leaves=1),
    "I16S17": dict(idmer_len=16, min_kmer_len=17),              # upper edge of the accepted range; direct walks only
}
SMALL_SETS = [s for s in SETS if s not in ("K15", "I16S17")]
REPEAT_SETS = [s for s in SETS if s != "I16S17"]
VARIANT_SETS = ["I7", "S15", "E25", "L4", "K21"]
WALK_SETS = ["I5", "I7", "I13", "S9", "S15", "I11S11", "E05", "E25", "C30", "I16S17"]
N_SMALL, N_REPEAT, N_REPEAT_DP, N_WALK_READS = 40, 60, 20, 15


def make_params(api, name, no_dp=0):
    o = dict(SETS[name]) if name != "default" else {}
    p = api.params_default(5, o.pop("coverage", 90))
    for k, v in o.items():
        if k == "offset":
            p.offset[0], p.offset[1], p.offset[2] = v
        else:
            setattr(p, k, v)
    p.no_dp = no_dp
    return p


# ---- indexes (module scope; the switches that act when an index is opened are set around open + upload only) ---------------
def _open(api, ds, **env):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        idx = api.index_open(ds.prefix + ".bwt", ds.prefix + ".rbwt")
        idx.upload(0)
    return idx


@pytest.fixture(scope="module")
def small_index(api, small_ds):
    idx = _open(api, small_ds)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def small_index_b64(api, small_ds):
    idx = _open(api, small_ds, LRSC_FORCE_WIDE="1")
    assert idx.info().block_symbols == 128
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def small_index_notab(api, small_ds):
    idx = _open(api, small_ds, LRSC_KTAB_K="0")
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def repeat_index(api, repeat_ds):
    idx = _open(api, repeat_ds)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def datasets(small_ds, repeat_ds):
    return {"small": small_ds, "repeat": repeat_ds}


# ---- the oracle, once per (dataset, reads, set, no_dp) -----------------------------------------------------------------------
_ORACLE_RUNS = {}


def _oracle_run(api, oracle, datasets, which, n_reads, name, no_dp):
    key = (which, n_reads, name, no_dp)
    if key not in _ORACLE_RUNS:
        ds = datasets[which]
        off = ds.off[: n_reads + 1].copy()
        ob, orb = oracle.bwt_load(ds.prefix + ".bwt"), oracle.bwt_load(ds.prefix + ".rbwt")
        run = oracle.correct_reads(ob, orb, make_params(api, name, no_dp), ds.bases[: int(off[-1])], off)
        _ORACLE_RUNS[key] = types.SimpleNamespace(correct_fa=run.correct_fa, discard_fa=run.discard_fa, counters=run.counters.copy())
        run.close(); ob.close(); orb.close()
    return _ORACLE_RUNS[key]


# What _check_whole_path asks of a run besides parity: more FM-corrected walks than a floor, some failed walks, and -- with the DP
# fallback -- walks that went through it.  The floors are ones the oracle itself clears on these reads (checked before the device
# runs): most sets correct 400..900 walks; K21 finds half the seeds, -l 1 gives up on most walks.
FM_FLOOR = {"small": 300, "repeat": 300, "repeat-dp": 100}
FM_FLOOR_OF_SET = {("small", "K21"): 150, ("small", "L1"): 40, ("repeat", "K21"): 150, ("repeat", "L1"): 150}
DP_FLOOR = 10
FAIL_COLS = tuple(NAMES.index(n) for n in ("high_error_num", "exceed_depth_num"))
FAIL_COLS_L1 = FAIL_COLS + (NAMES.index("exceed_leave_num"),)           # at -l 1 the walks that fail do so by their leaves


def _whole_path(api, oracle, datasets, index, which, n_reads, name, no_dp):
    """Device against oracle under option set `name`, after checking that the set is no no-op for the oracle on these reads."""
    want = _oracle_run(api, oracle, datasets, which, n_reads, name, no_dp)
    dflt = _oracle_run(api, oracle, datasets, which, n_reads, "default", no_dp)
    assert want.counters.shape != dflt.counters.shape or (want.counters != dflt.counters).any(), f"{name} changes nothing on this data"
    min_fm = FM_FLOOR_OF_SET.get((which, name), FM_FLOOR[which if no_dp or which == "small" else which + "-dp"])
    min_dp = 0 if no_dp else DP_FLOOR
    fail_cols = FAIL_COLS_L1 if name == "L1" else FAIL_COLS
    assert want.counters[:, FM].sum() > min_fm and want.counters[:, DP].sum() >= min_dp and want.counters[:, list(fail_cols)].sum() > 0
    return _check_whole_path(api, index, oracle, datasets[which], make_params(api, name, no_dp), n_reads=n_reads, min_fm=min_fm, min_dp=min_dp,
                             want=want, fail_cols=fail_cols)


# ---- a. whole path, small_ds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_dp", [1, 0])
@pytest.mark.parametrize("name", SMALL_SETS)
def test_small_set_whole_path(api, oracle, datasets, small_index, name, no_dp):
    _whole_path(api, oracle, datasets, small_index, "small", N_SMALL, name, no_dp)


# ---- b. whole path, repeat_ds: repeat seeds, repeat-to-unique walks (trg_len = k meets min_overlap) ------------------------
@pytest.mark.parametrize("name", REPEAT_SETS)
def test_repeat_set_whole_path_nodp(api, oracle, datasets, repeat_index, name):
    _whole_path(api, oracle, datasets, repeat_index, "repeat", N_REPEAT, name, 1)


@pytest.mark.parametrize("name", ["I7", "S15", "E25", "L4"])
def test_repeat_set_whole_path_dp_fallback(api, oracle, datasets, repeat_index, name):
    _whole_path(api, oracle, datasets, repeat_index, "repeat", N_REPEAT_DP, name, 0)


# ---- c. the other implementations of the same flow --------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANT_SETS)
def test_rounds_mode(api, oracle, datasets, small_index, name, monkeypatch):
    """Per-walk launches through extend.hip, stitched on the host (--nodp only)."""
    monkeypatch.setenv("LRSC_CORRECT_MODE", "rounds")
    _whole_path(api, oracle, datasets, small_index, "small", N_SMALL, name, 1)


@pytest.mark.parametrize("no_dp", [1, 0])
@pytest.mark.parametrize("wave", ["0", "2"])
@pytest.mark.parametrize("name", VARIANT_SETS)
def test_serial_and_wave_kernels(api, oracle, datasets, small_index, name, wave, no_dp, monkeypatch):
    """Every extension launch through the serial kernel (0) or the wavefront kernel (2), few lanes: many refills per wavefront."""
    monkeypatch.setenv("LRSC_WP_WAVE", wave)
    monkeypatch.setenv("LRSC_WP_LANES", "256")
    _whole_path(api, oracle, datasets, small_index, "small", N_SMALL, name, no_dp)


@pytest.mark.parametrize("no_dp", [1, 0])
@pytest.mark.parametrize("name", VARIANT_SETS)
def test_block64_layout(api, oracle, datasets, small_index_b64, name, no_dp):
    _whole_path(api, oracle, datasets, small_index_b64, "small", N_SMALL, name, no_dp)


@pytest.mark.parametrize("no_dp", [1, 0])
@pytest.mark.parametrize("name", VARIANT_SETS)
def test_without_kmer_tables(api, oracle, datasets, small_index_notab, name, no_dp):
    _whole_path(api, oracle, datasets, small_index_notab, "small", N_SMALL, name, no_dp)


# ---- d. -l above 32 together with a non-default table path ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["I7", "S15"])
def test_wide_walks_with_option(api, oracle, repeat_ds, repeat_index, name):
    p = make_params(api, name, 1)
    p.max_leaves = 64
    off = repeat_ds.off[: WIDE_N_READS + 1].copy()
    bases = repeat_ds.bases[: int(off[-1])]
    ob, orb = oracle.bwt_load(repeat_ds.prefix + ".bwt"), oracle.bwt_load(repeat_ds.prefix + ".rbwt")
    want = oracle.correct_reads(ob, orb, p, bases, off)
    ctx = repeat_index.ctx(p, 0)
    results, pieces = ctx.correct_reads(bases, off)
    wide = ctx.stats(K_EXTEND_WIDE)
    ctx.close()
    cfa, dfa = _fasta(results, pieces, repeat_ds.reads[:WIDE_N_READS], 0)
    assert cfa == want.correct_fa
    assert dfa == want.discard_fa
    np.testing.assert_array_equal(np.array([[getattr(r, n) for n in NAMES] for r in results], dtype=np.int64), want.counters)
    assert wide.launches > 0
    want.close(); ob.close(); orb.close()


# ---- e. lrsc_extend_walks directly ------------------------------------------------------------------------------------------
def _option_descs(oracle, ds, p, ob, orb, n_reads):
    """Consecutive-seed walks plus seed i to seed i + 3, inside the reference's domain for these params."""
    off = ds.off[: n_reads + 1].copy()
    count, seeds, _ = oracle.find_seeds(ob, orb, p, ds.bases[: int(off[-1])], off)
    reads = ds.reads[:n_reads]
    descs = _walk_descs(p, reads, count, seeds) + _skip_descs(p, reads, count, seeds, 3)
    return [d for d in descs if _in_domain(p, d)]


@pytest.mark.parametrize("name", WALK_SETS)
def test_extend_walks(api, oracle, small_ds, small_index, name):
    p = make_params(api, name)
    ob, orb = oracle.bwt_load(small_ds.prefix + ".bwt"), oracle.bwt_load(small_ds.prefix + ".rbwt")
    descs = _option_descs(oracle, small_ds, p, ob, orb, N_WALK_READS)
    assert len(descs) >= 100
    ctx = small_index.ctx(p, 0)
    got = ctx.extend_walks(descs)
    ctx.close()
    codes = set()
    for d, (code, merged, steps) in zip(descs, got):
        wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
        assert (code, merged, steps) == (wcode, wmerged, wst[0]), d
        codes.add(wcode)
    ob.close(); orb.close()
    assert {1, -1} <= codes


# ---- f. rejections ---------------------------------------------------------------------------------------------------------
def _launches(ctx):
    return sum(ctx.stats(k).launches for k in (K_SEEDS, K_EXTEND, K_EXTEND_WIDE, K_DP, K_MSA))


@pytest.mark.parametrize("overrides,msg", [
    (dict(idmer_len=4), "idmer_len must be 5..16"),
    (dict(idmer_len=17), "idmer_len must be 5..16"),
    (dict(idmer_len=9, min_kmer_len=8), "min_kmer_len out of range"),
    (dict(min_kmer_len=63), "min_kmer_len out of range"),
    (dict(max_leaves=0), "max_leaves must be 1..256"),
], ids=["idmer4", "idmer17", "minkmer-below-idmer", "minkmer63", "leaves0"])
def test_unsupported_params_are_rejected(api, oracle, small_ds, small_index, overrides, msg):
    """check_walk_params: both entry points refuse, launch nothing, and the same context then serves a default call."""
    off = small_ds.off[:4].copy()
    bases = small_ds.bases[: int(off[-1])]
    read = small_ds.reads[0]
    desc = (read[100:119], read[119:160], read[160:180], 41, 17, 19, 3)
    p = api.params_default(5, 90)
    for k, v in overrides.items():
        setattr(p, k, v)
    ctx = small_index.ctx(p, 0)
    ctx.stats_reset()
    for call in (lambda: ctx.extend_walks([desc]), lambda: ctx.correct_reads(bases, off)):
        with pytest.raises(LrscError) as e:
            call()
        assert e.value.status == -7 and msg in e.value.detail            # LRSC_ERR_UNSUPPORTED
    assert _launches(ctx) == 0
    ctx.close()
    _follow_up_default_call(api, oracle, small_ds, small_index)


def _follow_up_default_call(api, oracle, ds, index, ctx=None):
    p = api.params_default(5, 90)
    ob, orb = oracle.bwt_load(ds.prefix + ".bwt"), oracle.bwt_load(ds.prefix + ".rbwt")
    descs = _option_descs(oracle, ds, p, ob, orb, 2)
    own = ctx is None
    if own:
        ctx = index.ctx(p, 0)
    got = ctx.extend_walks(descs)
    if own:
        ctx.close()
    assert len(descs) > 5
    for d, (code, merged, steps) in zip(descs, got):
        wcode, wmerged, wst = oracle.extend_walk(ob, orb, p, *d)
        assert (code, merged, steps) == (wcode, wmerged, wst[0]), d
    ob.close(); orb.close()


def test_walks_outside_the_params_are_rejected(api, oracle, small_ds, small_index):
    """A target seed shorter than min_kmer_len, an init k-mer shorter than idmer_len: LRSC_ERR_ARG, nothing launched, and the next
    call on the same context is served."""
    read = small_ds.reads[0]
    p = api.params_default(5, 90)
    ctx = small_index.ctx(p, 0)
    ctx.stats_reset()
    good = (read[100:119], read[119:160], read[160:180], 41, 17, 19, 3)
    short_target = (read[100:119], read[119:160], read[160:160 + p.min_kmer_len - 1], 41, 17, 19, 3)
    short_init = (read[100:119], read[119:160], read[160:180], 41, p.idmer_len - 1, p.idmer_len + 1, 3)
    for bad, msg in ((short_target, "target seed shorter than min_kmer_len"), (short_init, "idmer_len <= init_kmer")):
        with pytest.raises(LrscError) as e:
            ctx.extend_walks([good, bad])
        assert e.value.status == -3 and msg in e.value.detail             # LRSC_ERR_ARG
    assert _launches(ctx) == 0
    _follow_up_default_call(api, oracle, small_ds, small_index, ctx)
    assert ctx.stats(K_EXTEND).launches > 0
    ctx.close()
