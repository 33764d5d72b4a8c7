"""lrsc_index_open_device / lrsc_index_from_units_device (RL units decoded and packed on the device, fm_unrle.hip) against the
host route on the same files or units: lrsc_index_open / lrsc_index_from_units + lrsc_index_upload.  Equality is exact: the
index's info, every BWT symbol, rank at every position for every base (which pins the blocks' counts, both bit planes, the '$'
flag, list and directory), the RL units encoded back from the resident copy, k-mer intervals (the k-mer tables) and whole
corrections."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from .conftest import write_fasta
from .test_gpu_index_build import ACGT, STRIDE, _assert_same_answers, _grid_table_loads, _hip, _info
from .test_index_unrle_host import CORRUPT, EXCEED, SHORT, decode, encode, patterns, tiles

pytestmark = pytest.mark.gpu

LRSC_ERR_IO, LRSC_ERR_FORMAT = -1, -2
DOLLARS = "number of '$' rows differs from the number of strings in the header"


def _assert_same_index(api, dev, want, *, device=0):
    """info, bwt_chars at every position, rank for every idx in [-1, N) x ACGT, the units of both strands -> the two contexts"""
    i_d, i_w = _info(dev), _info(want)
    assert i_d == i_w and min(i_d["num_runs"]) > 0
    n = i_d["num_symbols"]
    p = api.params_default(5, 90)
    cd, cw = dev.ctx(p, device), want.ctx(p, device)
    pos = np.arange(n, dtype=np.uint64)
    idx = np.tile(np.arange(-1, n, dtype=np.int64), 4)
    base = np.repeat(ACGT, n + 1)
    for strand in (0, 1):
        np.testing.assert_array_equal(cd.bwt_chars(strand, pos), cw.bwt_chars(strand, pos))
        np.testing.assert_array_equal(cd.rank(base, idx, strand), cw.rank(base, idx, strand))
        np.testing.assert_array_equal(dev.units(strand, device), want.units(strand, device))
    return cd, cw


def _opened_on_device_vs_host(api, ds):
    files = ds.prefix + ".bwt", ds.prefix + ".rbwt"
    dev = api.index_open_device(*files, 0)
    want = api.index_open(*files)
    want.upload(0)
    cd, cw = _assert_same_index(api, dev, want)
    for strand, f in enumerate(files):
        payload = np.fromfile(f, dtype=np.uint8)[30:]
        np.testing.assert_array_equal(dev.units(strand, 0), payload)
        assert dev.info().num_runs[strand] == payload.size
    _assert_same_answers(cd, cw, ds.bases, ds.off, 32)
    for x in (cd, cw, dev, want):
        x.close()


def test_index_opened_on_the_device_equals_opened_index(api, small_ds):
    _opened_on_device_vs_host(api, small_ds)


def test_index_opened_on_the_device_equals_opened_index_block64(api, small_ds, monkeypatch):
    monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    _opened_on_device_vs_host(api, small_ds)


def test_index_opened_on_the_device_is_resident_there(api, small_ds, monkeypatch):
    """As for a built index: the packed image and its k-mer tables are device 0's copy, and upload(0) leaves them alone."""
    files = small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt"
    dev = api.index_open_device(*files, 0)
    p = api.params_default(5, 90)
    c0 = dev.ctx(p, 0)                                      # needs a copy on device 0: there without an upload
    seeds0, loads0 = _grid_table_loads(c0, small_ds)
    assert loads0 > 0, "the open leaves the k-mer tables on its device"
    monkeypatch.setenv("LRSC_KTAB_K", "0")
    dev.upload(0)
    c1 = dev.ctx(p, 0)
    seeds1, loads1 = _grid_table_loads(c1, small_ds)
    assert loads1 == loads0
    opened = api.index_open(*files)
    opened.upload(0)                                        # a real upload under LRSC_KTAB_K=0: no tables
    c2 = opened.ctx(p, 0)
    seeds2, loads2 = _grid_table_loads(c2, small_ds)
    assert loads2 == 0
    for got in (seeds1, seeds2):
        assert got[0].tobytes() == seeds0[0].tobytes() and got[1].tobytes() == seeds0[1].tobytes()
    assert seeds0[0].sum() > 0
    for x in (c0, c1, c2, dev, opened):
        x.close()


# (pattern of test_index_unrle_host.patterns, N as a function of the symbol tile)
STREAMS = {
    "all_runs_31": ("all_runs_31", lambda t: 3 * t + 7),
    "all_runs_1": ("all_runs_1", lambda t: 3 * t + 7),
    "non_canonical": ("non_canonical", lambda t: 384 * 200),
    "dollar_dense": ("dollar_dense", lambda t: 3 * t + 7),
    "dollar_dense_multiple_of_384": ("dollar_dense", lambda t: 384 * 200),
    "dollar_unit_tile": ("dollar_unit_tile", lambda t: 3 * t + 7),
    "across_unit_tile_edges": ("across_unit_tile_edges", lambda t: 384 * 200 + 1),
}


def _stream(name, wide):
    ksyms, t, u = tiles(0, int(wide))
    pat, n_of = STREAMS[name]
    n = n_of(t)
    assert n <= 100000
    units = patterns(n, ksyms, t, u, seed=5, every_phase=False)[pat].copy()
    units[0] &= 0x1F                                        # at least one '$' row
    return units, n, int((units[(units >> 5) == 0] & 31).sum())


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
@pytest.mark.parametrize("name", list(STREAMS))
def test_unit_streams_equal_index_from_units(api, monkeypatch, name, wide):
    monkeypatch.setenv("LRSC_KTAB_K", "0")                  # the streams are no BWT of anything: nothing may search them
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    units, n, n_strings = _stream(name, wide)
    other = units[::-1].copy()                              # the second strand: the same '$' rows elsewhere
    if name == "non_canonical":
        assert not np.array_equal(encode(decode(units)), units)
    dev = api.index_from_units_device(units, other, n_strings, n, 0)
    want = api.index_from_units(units, other, n_strings, n)
    want.upload(0)
    assert dev.info().block_symbols == (128 if wide else 192)
    assert list(dev.info().num_runs) == [units.size, units.size]
    cd, cw = _assert_same_index(api, dev, want)
    for strand, u in enumerate((units, other)):
        np.testing.assert_array_equal(dev.units(strand, 0), encode(decode(u)))
    for x in (cd, cw, dev, want):
        x.close()


def test_errors_are_the_host_route_s_and_leave_the_device_usable(api, small_ds, tmp_path, monkeypatch):
    from longreadselfcorrect_amd.capi import LrscError

    monkeypatch.setenv("LRSC_KTAB_K", "0")
    good, n, n_strings = _stream("dollar_dense", False)

    def works():
        ix = api.index_from_units_device(good, good, n_strings, n, 0)
        assert ix.info().num_symbols == n and list(ix.info().num_runs) == [good.size, good.size]
        ix.close()

    corrupt = good.copy()
    corrupt[good.size // 2] |= 0xE0
    run0 = good.copy()
    run0[good.size - 1] &= 0xE0
    cases = [(corrupt, good, n, n_strings, CORRUPT), (good, run0, n, n_strings, CORRUPT),
             (np.append(good, np.uint8(1 << 5 | 1)), good, n, n_strings, EXCEED), (good, good[:-1], n, n_strings, SHORT),
             (good, good, n, n_strings + 1, DOLLARS)]
    works()
    for a, b, n_sym, n_str, text in cases:
        with pytest.raises(LrscError) as e_dev:
            api.index_from_units_device(a, b, n_str, n_sym, 0)
        with pytest.raises(LrscError) as e_host:
            api.index_from_units(a, b, n_str, n_sym)
        assert e_dev.value.status == e_host.value.status == LRSC_ERR_FORMAT, text
        assert e_dev.value.detail == e_host.value.detail and text in e_dev.value.detail
        works()
    # the same through files
    bad = tmp_path / "bad.bwt"
    api.write_bwt_file(bad, corrupt, n_strings, n)
    ok = tmp_path / "ok.bwt"
    api.write_bwt_file(ok, good, n_strings, n)
    with pytest.raises(LrscError) as e:
        api.index_open_device(ok, bad, 0)
    assert e.value.status == LRSC_ERR_FORMAT and CORRUPT in e.value.detail
    with pytest.raises(LrscError) as e:
        api.index_open_device(ok, tmp_path / "missing.rbwt", 0)
    assert e.value.status == LRSC_ERR_IO
    with pytest.raises(LrscError) as e_host:
        api.index_open(ok, tmp_path / "missing.rbwt")
    assert e.value.detail == e_host.value.detail
    ix = api.index_open_device(ok, ok, 0)
    assert ix.info().num_symbols == n
    ix.close()


def test_index_opened_on_the_device_uploads_to_a_second_device(api, small_ds):
    hip = _hip()
    n_dev = C.c_int()
    assert hip.hipGetDeviceCount(C.byref(n_dev)) == 0
    if n_dev.value < 2:
        pytest.skip("one device visible")
    dev = api.index_open_device(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt", 0)
    dev.upload(1)
    p = api.params_default(5, 90)
    c0, c1 = dev.ctx(p, 0), dev.ctx(p, 1)
    n = dev.info().num_symbols
    rng = np.random.default_rng(4)
    idx = rng.integers(-1, n, size=100000)
    base = rng.choice(ACGT, size=idx.size)
    for strand in (0, 1):
        np.testing.assert_array_equal(c1.rank(base, idx, strand), c0.rank(base, idx, strand))
    for x in (c0, c1, dev):
        x.close()


def test_stride_pbcorrect_load_on_device_end_to_end(api, small_ds, tmp_path):
    """`stride pbcorrect -p Q --load-on-device` against `stride pbcorrect -p Q`: same FASTA files and statistics."""
    stride = str(STRIDE)
    write_fasta(tmp_path / "reads.fa", small_ds.reads)
    common = ["-p", small_ds.prefix, "-c", "90", "-g", "5", "--batch", "70"]
    ra = subprocess.run([stride, "pbcorrect", "--load-on-device", "-o", "A"] + common + ["reads.fa"], cwd=tmp_path, capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr
    rb = subprocess.run([stride, "pbcorrect", "-o", "B"] + common + ["reads.fa"], cwd=tmp_path, capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr
    for name in ("correct.fa", "discard.fa", "threshold-table"):
        assert (tmp_path / "A" / name).read_bytes() == (tmp_path / "B" / name).read_bytes(), name
    assert (tmp_path / "A" / "correct.fa").stat().st_size > 0

    def stats(text):                                        # the statistics block without its three wall-clock lines
        return [l for l in text.split("\n") if not l.startswith("Time")]

    assert stats(ra.stdout) == stats(rb.stdout) and len(stats(ra.stdout)) > 3
