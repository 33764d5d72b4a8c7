"""lrsc_index_build (reads -> both strands' index, sorted and packed on the device, no files) against the host builder on the
same reads: lrsc_index_open of the fixture's files, or lrsc_index_from_units of lrsc_build_bwt's units.  Equality is exact:
the index's info, every BWT symbol, rank at every position for every base (which pins the blocks' counts, both bit planes, the
'$' flag, list and directory), k-mer intervals (the k-mer tables) and whole corrections."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from .conftest import REPO, write_fasta

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
LRSC_ERR_ARG = -3


def _info(index):
    i = index.info()
    return {"num_strings": i.num_strings, "num_symbols": i.num_symbols, "num_runs": list(i.num_runs),
            "pred_count": [list(r) for r in i.pred_count], "block_bytes": i.block_bytes, "block_symbols": i.block_symbols,
            "device_bytes": i.device_bytes}


def _assert_same_index(api, built, want, *, device=0):
    """info, bwt_chars at every position, rank for every idx in [-1, N) x ACGT, both strands -> the two contexts"""
    ib, iw = _info(built), _info(want)
    assert ib["num_runs"] == [0, 0] and min(iw["num_runs"]) > 0
    ib.pop("num_runs"); iw.pop("num_runs")
    assert ib == iw
    n = ib["num_symbols"]
    p = api.params_default(5, 90)
    cb, cw = built.ctx(p, device), want.ctx(p, device)
    pos = np.arange(n, dtype=np.uint64)
    idx = np.tile(np.arange(-1, n, dtype=np.int64), 4)
    base = np.repeat(ACGT, n + 1)
    for strand in (0, 1):
        np.testing.assert_array_equal(cb.bwt_chars(strand, pos), cw.bwt_chars(strand, pos))
        np.testing.assert_array_equal(cb.rank(base, idx, strand), cw.rank(base, idx, strand))
    return cb, cw


def _assert_same_answers(cb, cw, bases, off, n_correct):
    rng = np.random.default_rng(77)
    for k in (5, 13, 19):
        starts = rng.integers(0, bases.size - k, size=12000)
        inside = np.array([not np.any((off > s) & (off < s + k)) for s in starts])
        kmers = np.stack([bases[s:s + k] for s in starts[inside][:10000]]).astype(np.uint8).reshape(-1)
        assert kmers.size == 10000 * k
        got, want = cb.find_kmers(kmers, k), cw.find_kmers(kmers, k)
        assert got.tobytes() == want.tobytes(), f"find_kmers differs at k={k}"
    c_off = off[: n_correct + 1].copy()
    c_bases = bases[: int(c_off[-1])]
    res_b, pieces_b = cb.correct_reads(c_bases, c_off)
    res_w, pieces_w = cw.correct_reads(c_bases, c_off)
    assert [bytes(r) for r in res_b] == [bytes(r) for r in res_w]        # every lrsc_read_result field, piece ranges included
    assert pieces_b == pieces_w
    assert sum(r.n_pieces for r in res_b) > 0


def _built_vs_opened(api, ds, n_correct):
    built = api.index_build(ds.bases, ds.off, 0)
    opened = api.index_open(ds.prefix + ".bwt", ds.prefix + ".rbwt")
    opened.upload(0)
    cb, cw = _assert_same_index(api, built, opened)
    _assert_same_answers(cb, cw, ds.bases, ds.off, n_correct)
    for x in (cb, cw, built, opened):
        x.close()


def test_built_index_equals_opened_index(api, small_ds):
    _built_vs_opened(api, small_ds, small_ds.n_reads)


def test_built_index_equals_opened_index_block64(api, small_ds, monkeypatch):
    monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    _built_vs_opened(api, small_ds, small_ds.n_reads)


def test_built_index_equals_opened_index_grouped_jobs_64bit_positions(api, small_ds, monkeypatch):
    monkeypatch.setenv("LRSC_BWT_JOB", "20000")
    monkeypatch.setenv("LRSC_BWT_WIDE_POS", "1")
    _built_vs_opened(api, small_ds, 32)


def _pathological():
    rng = np.random.default_rng(3)
    base = "".join(rng.choice(list("ACGT"), size=300))
    return [base, base, base[:150], base[150:], "A" * 200, "A" * 199, "A", "C", base[::-1], base, "ACGT" * 40, "T"]


def _filler(reads, multiple, extra):
    """reads + one random read sized so that the symbol count is a multiple of `multiple`, plus `extra`"""
    n = sum(len(r) for r in reads) + len(reads) + 1             # with the filler's own '$'
    fill = (-n) % multiple or multiple
    rng = np.random.default_rng(9)
    return reads + ["".join(rng.choice(list("ACGT"), size=fill + extra))]


def _short_reads():
    rng = np.random.default_rng(21)
    return ["".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 3)))) for _ in range(3000)]


EDGE_SETS = {
    "pathological": _pathological,
    "multiple_of_384": lambda: _filler(_pathological(), 384, 0),
    "multiple_of_384_plus_1": lambda: _filler(_pathological(), 384, 1),
    "dollar_dense": _short_reads,
    "one_base": lambda: ["G"],
}


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
@pytest.mark.parametrize("name", list(EDGE_SETS))
def test_edge_read_sets_equal_index_from_units(api, monkeypatch, name, wide):
    from oracle.oracle_py import pack_reads

    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    reads = EDGE_SETS[name]()
    bases, off = pack_reads(reads)
    n_sym = int(off[-1]) + len(reads)
    if name == "multiple_of_384":
        assert n_sym % 384 == 0
    if name == "multiple_of_384_plus_1":
        assert n_sym % 384 == 1
    if name == "dollar_dense":
        assert n_sym // 192 + 1 > 3 * 8 and len(reads) / (n_sym / 1024) > 24      # several groups, dozens of '$' rows in each
    units = [api.build_bwt(bases, off, rev, 0) for rev in (False, True)]
    want = api.index_from_units(units[0], units[1], len(reads), n_sym)
    want.upload(0)
    built = api.index_build(bases, off, 0)
    assert built.info().block_symbols == (128 if wide else 192)
    cb, cw = _assert_same_index(api, built, want)
    for x in (cb, cw, built, want):
        x.close()


def _hip():
    return C.CDLL("libamdhip64.so")


def _grid_table_loads(ctx, ds):
    """k-mer table look-ups of the resident batch's k-mer grid over the first reads (the compact grid is the kernel that starts
    its searches from the tables), and the seeds found from it"""
    off = ds.off[:9].copy()
    ctx.stats_reset()
    b = ctx.batch(ds.bases[: int(off[-1])], off)
    b.kmer_grid()
    loads = ctx.stats(2).table_loads                         # LRSC_K_GRID
    b.find_seeds()
    count, seeds, _ = b.seeds(want_attribute=False)
    b.close()
    return (count, seeds), loads


def test_built_index_is_resident_on_its_device(api, small_ds, monkeypatch):
    """The packed image and its k-mer tables are device 0's copy, and upload(0) leaves them alone: with the tables switched off
    for new copies, an upload that made one would give a context whose k-mer grid looks nothing up in a table -- as the opened
    index uploaded under the same setting shows."""
    built = api.index_build(small_ds.bases, small_ds.off, 0)
    p = api.params_default(5, 90)
    c0 = built.ctx(p, 0)                                    # needs a copy on device 0: there without an upload
    seeds0, loads0 = _grid_table_loads(c0, small_ds)
    assert loads0 > 0, "the build leaves the k-mer tables on its device"
    monkeypatch.setenv("LRSC_KTAB_K", "0")
    built.upload(0)
    c1 = built.ctx(p, 0)
    seeds1, loads1 = _grid_table_loads(c1, small_ds)
    assert loads1 == loads0
    opened = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    opened.upload(0)                                        # a real upload under LRSC_KTAB_K=0: no tables
    c2 = opened.ctx(p, 0)
    seeds2, loads2 = _grid_table_loads(c2, small_ds)
    assert loads2 == 0
    for got in (seeds1, seeds2):
        assert got[0].tobytes() == seeds0[0].tobytes() and got[1].tobytes() == seeds0[1].tobytes()
    assert seeds0[0].sum() > 0
    for x in (c0, c1, c2, built, opened):
        x.close()


def test_built_index_uploads_to_a_second_device(api, small_ds):
    hip = _hip()
    n_dev = C.c_int()
    assert hip.hipGetDeviceCount(C.byref(n_dev)) == 0
    if n_dev.value < 2:
        pytest.skip("one device visible")
    built = api.index_build(small_ds.bases, small_ds.off, 0)
    built.upload(1)
    p = api.params_default(5, 90)
    c0, c1 = built.ctx(p, 0), built.ctx(p, 1)
    n = built.info().num_symbols
    rng = np.random.default_rng(4)
    idx = rng.integers(-1, n, size=100000)
    base = rng.choice(ACGT, size=idx.size)
    for strand in (0, 1):
        np.testing.assert_array_equal(c1.rank(base, idx, strand), c0.rank(base, idx, strand))
    for x in (c0, c1, built):
        x.close()


def test_errors_leave_the_device_usable(api, small_ds):
    from longreadselfcorrect_amd.capi import LrscError
    from oracle.oracle_py import pack_reads

    good_bases, good_off = pack_reads(["ACGTTGCA", "GATTACA"])

    def good():
        ix = api.index_build(good_bases, good_off, 0)
        assert ix.info().num_symbols == 17
        ix.close()

    bases, off = pack_reads(["ACGT", "ACNT", "GG"])
    with pytest.raises(LrscError) as e:
        api.index_build(bases, off, 0)
    assert e.value.status == LRSC_ERR_ARG and "sequence contains a base other than A,C,G,T" in e.value.detail
    with pytest.raises(LrscError) as e2:
        api.build_bwt(bases, off, False, 0)
    assert e2.value.status == e.value.status and e2.value.detail == e.value.detail
    good()
    with pytest.raises(LrscError) as e:
        api.index_build(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 0)
    assert e.value.status == LRSC_ERR_ARG
    good()


def test_stride_pbcorrect_build_index_end_to_end(api, small_ds, tmp_path):
    """`stride pbcorrect --build-index` against `stride index` + `stride pbcorrect -p`: same FASTA files and statistics, and no
    index file anywhere under the run's working directory."""
    stride = str(STRIDE)
    work_a, work_b = tmp_path / "a", tmp_path / "b"
    work_a.mkdir(); work_b.mkdir()
    for w in (work_a, work_b):
        write_fasta(w / "reads.fa", small_ds.reads)
    common = ["-c", "90", "-g", "5", "--batch", "70"]
    ra = subprocess.run([stride, "pbcorrect", "--build-index", "-o", "A"] + common + ["reads.fa"], cwd=work_a, capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr
    subprocess.run([stride, "index", "-p", "P", "reads.fa"], cwd=work_b, check=True, capture_output=True)
    rb = subprocess.run([stride, "pbcorrect", "-p", "P", "-o", "B"] + common + ["reads.fa"], cwd=work_b, capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr
    for name in ("correct.fa", "discard.fa", "threshold-table"):
        assert (work_a / "A" / name).read_bytes() == (work_b / "B" / name).read_bytes(), name
    assert (work_a / "A" / "correct.fa").stat().st_size > 0

    def stats(text):                                        # the statistics block without its three wall-clock lines
        return [l for l in text.split("\n") if not l.startswith("Time")]

    assert stats(ra.stdout) == stats(rb.stdout) and len(stats(ra.stdout)) > 3
    assert not [p for p in work_a.rglob("*") if p.suffix in (".bwt", ".rbwt", ".sai", ".rsai")]
    assert "Loading BWT" not in ra.stderr

    r = subprocess.run([stride, "pbcorrect", "--build-index", "-p", "x", "-o", str(tmp_path / "o"), "reads.fa"], cwd=work_a,
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "--build-index reads no index files: give either it or -p" in r.stderr and "Usage: StriDe PacBioSelfCorrection" in r.stderr
