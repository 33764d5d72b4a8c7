"""The device RL encoder (csrc/fm_rle.hip) behind lrsc_index_units / lrsc_index_write / lrsc_build_bwt, on the GPU.

The units of an index, encoded from the rank blocks of its device copy, must be the payload of the oracle's .bwt/.rbwt files (and
the written files those files) for an opened and for a built index, on both block layouts; on edge read sets the three routes --
rank blocks of a built index, the byte-per-symbol BWT inside lrsc_build_bwt, and lrsc_build_bwt's host loop
(LRSC_BWT_HOST_RLE=1) -- must agree byte for byte."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO, write_fasta

pytestmark = pytest.mark.gpu

STRIDE = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
LRSC_ERR_ARG, LRSC_ERR_IO, LRSC_ERR_DEVICE = -3, -1, -5
LAYOUTS = pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])


def _payload(path) -> bytes:
    return Path(path).read_bytes()[30:]


def _info(index):
    i = index.info()
    return {"num_strings": i.num_strings, "num_symbols": i.num_symbols, "num_runs": list(i.num_runs),
            "pred_count": [list(r) for r in i.pred_count], "block_bytes": i.block_bytes, "block_symbols": i.block_symbols,
            "device_bytes": i.device_bytes}


def _units_and_files_equal_the_oracles(index, ds, tmp_path, wide):
    assert index.info().block_symbols == (128 if wide else 192)
    for s, ext in ((0, ".bwt"), (1, ".rbwt")):
        assert index.units(s, 0).tobytes() == _payload(ds.prefix + ext), ext
    index.write(tmp_path / "w.bwt", tmp_path / "w.rbwt", 0)
    for ext in (".bwt", ".rbwt"):
        assert (tmp_path / ("w" + ext)).read_bytes() == Path(ds.prefix + ext).read_bytes(), ext


@LAYOUTS
def test_opened_index_gives_back_its_files(api, small_ds, tmp_path, monkeypatch, wide):
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    index = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    index.upload(0)
    _units_and_files_equal_the_oracles(index, small_ds, tmp_path, wide)
    index.close()


@LAYOUTS
def test_built_index_gives_the_oracles_files(api, small_ds, tmp_path, monkeypatch, wide):
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    index = api.index_build(small_ds.bases, small_ds.off, 0)
    _units_and_files_equal_the_oracles(index, small_ds, tmp_path, wide)
    assert list(index.info().num_runs) == [0, 0]
    index.close()


def _pathological():
    rng = np.random.default_rng(3)
    base = "".join(rng.choice(list("ACGT"), size=300))
    return [base, base, base[:150], base[150:], "A" * 200, "A" * 199, "A", "C", base[::-1], base, "ACGT" * 40, "T"]


def _short_reads():
    rng = np.random.default_rng(21)
    return ["".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 3)))) for _ in range(3000)]


EDGE_SETS = {
    "pathological": _pathological,
    "dollar_dense": _short_reads,                    # long '$' runs in flagged blocks
    "one_base": lambda: ["G"],
    "one_long_run": lambda: ["A" * 2000] * 200,      # one A run of 400 k symbols: the carry passes through single-run tiles
}


@LAYOUTS
@pytest.mark.parametrize("name", list(EDGE_SETS))
def test_edge_read_sets_three_routes_agree(api, monkeypatch, name, wide):
    from oracle.oracle_py import pack_reads

    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    reads = EDGE_SETS[name]()
    bases, off = pack_reads(reads)
    assert int(off[-1]) + len(reads) <= 500_000
    monkeypatch.setenv("LRSC_BWT_HOST_RLE", "1")
    host = [api.build_bwt(bases, off, rev, 0).tobytes() for rev in (False, True)]
    monkeypatch.delenv("LRSC_BWT_HOST_RLE")
    from_bytes = [api.build_bwt(bases, off, rev, 0).tobytes() for rev in (False, True)]
    built = api.index_build(bases, off, 0)
    from_blocks = [built.units(s, 0).tobytes() for s in (0, 1)]
    built.close()
    if name == "one_long_run":                       # 400 000 A = 12903 units of 31 and one of 7, then the 200 '$'
        assert host[0][:12903] == bytes([(1 << 5) | 31]) * 12903 and host[0][12903] == (1 << 5) | 7
    for s in (0, 1):
        assert from_bytes[s] == host[s], f"strand {s}: encoder on the byte BWT differs from the host loop"
        assert from_blocks[s] == host[s], f"strand {s}: encoder on the rank blocks differs from the host loop"


def test_grouped_builder_path_is_unchanged(api, small_ds, monkeypatch):
    monkeypatch.setenv("LRSC_BWT_JOB", "20000")
    monkeypatch.setenv("LRSC_BWT_WIDE_POS", "1")
    for rev, ext in ((False, ".bwt"), (True, ".rbwt")):
        assert api.build_bwt(small_ds.bases, small_ds.off, rev, 0).tobytes() == _payload(small_ds.prefix + ext), ext


def test_written_index_opens_as_the_oracles(api, small_ds, tmp_path):
    built = api.index_build(small_ds.bases, small_ds.off, 0)
    built.write(tmp_path / "b.bwt", tmp_path / "b.rbwt", 0)
    built.close()
    again = api.index_open(str(tmp_path / "b.bwt"), str(tmp_path / "b.rbwt"))
    want = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    ia, iw = _info(again), _info(want)
    assert min(ia["num_runs"]) > 0
    assert ia == iw
    again.close(); want.close()


def test_error_paths(api, small_ds, tmp_path):
    from longreadselfcorrect_amd.capi import LrscError

    index = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")
    with pytest.raises(LrscError) as e:
        index.units(0, 0)
    assert e.value.status == LRSC_ERR_DEVICE and "index not uploaded to this device" in e.value.detail
    index.upload(0)
    for strand in (2, -1):
        with pytest.raises(LrscError) as e:
            index.units(strand, 0)
        assert e.value.status == LRSC_ERR_ARG
    with pytest.raises(LrscError) as e:
        index.write(tmp_path / "no_such_dir" / "x.bwt", tmp_path / "x.rbwt", 0)
    assert e.value.status == LRSC_ERR_IO
    assert index.units(1, 0).tobytes() == _payload(small_ds.prefix + ".rbwt")     # and the index still works
    index.close()


def test_stride_pbcorrect_save_index_end_to_end(api, small_ds, tmp_path):
    """`stride pbcorrect --build-index --save-index P` against `stride index -p Q` + `stride pbcorrect -p Q`: the four index files
    pairwise byte-identical, the same FASTA files and statistics."""
    stride = str(STRIDE)
    work_a, work_b = tmp_path / "a", tmp_path / "b"
    work_a.mkdir(); work_b.mkdir()
    for w in (work_a, work_b):
        write_fasta(w / "reads.fa", small_ds.reads)
    common = ["-c", "90", "-g", "5", "--batch", "70"]
    ra = subprocess.run([stride, "pbcorrect", "--build-index", "--save-index", "P", "-o", "A"] + common + ["reads.fa"], cwd=work_a,
                        capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr
    subprocess.run([stride, "index", "-p", "Q", "reads.fa"], cwd=work_b, check=True, capture_output=True)
    rb = subprocess.run([stride, "pbcorrect", "-p", "Q", "-o", "B"] + common + ["reads.fa"], cwd=work_b, capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr
    for ext in (".bwt", ".rbwt", ".sai", ".rsai"):
        a, b = (work_a / ("P" + ext)).read_bytes(), (work_b / ("Q" + ext)).read_bytes()
        assert a == b and len(a) > 30, ext
    assert (work_a / "P.bwt").read_bytes() == Path(small_ds.prefix + ".bwt").read_bytes()
    for name in ("correct.fa", "discard.fa", "threshold-table"):
        assert (work_a / "A" / name).read_bytes() == (work_b / "B" / name).read_bytes(), name
    assert (work_a / "A" / "correct.fa").stat().st_size > 0

    def stats(text):                                        # the statistics block without its three wall-clock lines
        return [l for l in text.split("\n") if not l.startswith("Time")]

    assert stats(ra.stdout) == stats(rb.stdout) and len(stats(ra.stdout)) > 3
