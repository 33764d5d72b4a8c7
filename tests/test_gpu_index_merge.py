"""lrsc_index_merge (two resident indexes -> the index of A's reads followed by B's, fm_merge.hip) against lrsc_index_build of
the concatenated reads.  Equality is exact: the index's info, every BWT symbol, rank at every position for every base, the RL
units encoded back from the resident copy, k-mer intervals (the k-mer tables) and whole corrections; `stride merge` and
`stride pbcorrect --merge-index` against `stride index` of the concatenated FASTA, file for file."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from .conftest import write_fasta
from .test_gpu_index_build import ACGT, STRIDE, _assert_same_answers, _grid_table_loads, _info
from .test_index_merge_host import CASES, kernel_tile, sorted_case

pytestmark = pytest.mark.gpu

LRSC_ERR_DEVICE = -5


def _split(ds, at):
    """(bases, off) of the reads before `at` and of those from `at` on"""
    cut = int(ds.off[at])
    return (ds.bases[:cut], ds.off[: at + 1].copy()), (ds.bases[cut:], (ds.off[at:] - ds.off[at]).astype(np.uint64))


def _assert_same_index(api, got, want, *, device=0):
    """info, bwt_chars at every position, rank for every idx in [-1, N) x ACGT, the units of both strands -> the two contexts"""
    ig, iw = _info(got), _info(want)
    assert ig == iw and ig["num_runs"] == [0, 0]
    n = ig["num_symbols"]
    p = api.params_default(5, 90)
    cg, cw = got.ctx(p, device), want.ctx(p, device)
    pos = np.arange(n, dtype=np.uint64)
    idx = np.tile(np.arange(-1, n, dtype=np.int64), 4)
    base = np.repeat(ACGT, n + 1)
    for strand in (0, 1):
        np.testing.assert_array_equal(cg.bwt_chars(strand, pos), cw.bwt_chars(strand, pos))
        np.testing.assert_array_equal(cg.rank(base, idx, strand), cw.rank(base, idx, strand))
        np.testing.assert_array_equal(got.units(strand, device), want.units(strand, device))
    return cg, cw


def _merged_vs_built(api, ds, monkeypatch, wide_a, wide_b, wide_union, n_correct=32):
    """LRSC_FORCE_WIDE is read per call: set or unset before each index is made"""
    (bases_a, off_a), (bases_b, off_b) = _split(ds, 120)

    def force(wide):
        if wide:
            monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
        else:
            monkeypatch.delenv("LRSC_FORCE_WIDE", raising=False)

    force(wide_a)
    a = api.index_build(bases_a, off_a, 0)
    force(wide_b)
    b = api.index_build(bases_b, off_b, 0)
    syms = lambda wide: 128 if wide else 192
    assert (a.info().block_symbols, b.info().block_symbols) == (syms(wide_a), syms(wide_b))
    units_before = [x.units(s, 0) for x in (a, b) for s in (0, 1)]
    force(wide_union)
    merged = api.index_merge(a, b, 0)
    union = api.index_build(ds.bases, ds.off, 0)
    assert merged.info().block_symbols == syms(wide_union)
    assert merged.info().num_strings == ds.n_reads and merged.info().num_symbols == a.info().num_symbols + b.info().num_symbols
    cm, cu = _assert_same_index(api, merged, union)
    _assert_same_answers(cm, cu, ds.bases, ds.off, n_correct)
    # a and b answer as before
    for before, after in zip(units_before, [x.units(s, 0) for x in (a, b) for s in (0, 1)]):
        np.testing.assert_array_equal(before, after)
    force(wide_a)
    a2 = api.index_build(bases_a, off_a, 0)
    ca, ca2 = _assert_same_index(api, a, a2)
    for x in (cm, cu, ca, ca2, a, a2, b, merged, union):
        x.close()


def test_merged_index_equals_built_union(api, small_ds, monkeypatch):
    _merged_vs_built(api, small_ds, monkeypatch, False, False, False)


@pytest.mark.parametrize("wide_a,wide_b,wide_union", [(True, True, True), (True, False, False), (False, True, True)],
                         ids=["all_block64", "a64_b32_to_32", "a32_b64_to_64"])
def test_merged_index_equals_built_union_layouts(api, small_ds, monkeypatch, wide_a, wide_b, wide_union):
    _merged_vs_built(api, small_ds, monkeypatch, wide_a, wide_b, wide_union)


def test_merged_index_is_resident_on_its_device(api, small_ds, monkeypatch):
    """As for a built index: the packed image and its k-mer tables are device 0's copy, and upload(0) leaves them alone."""
    (bases_a, off_a), (bases_b, off_b) = _split(small_ds, 120)
    a, b = api.index_build(bases_a, off_a, 0), api.index_build(bases_b, off_b, 0)
    merged = api.index_merge(a, b, 0)
    p = api.params_default(5, 90)
    c0 = merged.ctx(p, 0)                                   # needs a copy on device 0: there without an upload
    seeds0, loads0 = _grid_table_loads(c0, small_ds)
    assert loads0 > 0, "the merge leaves the k-mer tables on its device"
    monkeypatch.setenv("LRSC_KTAB_K", "0")
    merged.upload(0)
    c1 = merged.ctx(p, 0)
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
    for x in (c0, c1, c2, a, b, merged, opened):
        x.close()


T = kernel_tile()
EDGE = ["pathological-split1", "pathological-split6", "pathological-split11", "multiple_of_384-split6", "multiple_of_384_plus_1-split6",
        "multiple_of_384_minus_1", "dollar_dense-split1500", "dollar_dense-split2999", "one_base-twice", "a_equals_b", "a_equals_b-dollar_dense",
        "b_all_A", "b_all_T", "a_all_A", "duplicates_across", f"total{T - 1}", f"total{T}", f"total{T + 1}", f"total{3 * T + 7}"]


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
@pytest.mark.parametrize("name", EDGE)
def test_edge_read_sets_equal_build_bwt_of_the_concatenation(api, monkeypatch, name, wide):
    from oracle.oracle_py import pack_reads

    monkeypatch.setenv("LRSC_KTAB_K", "0")                  # nothing searches these indexes
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    reads_a, reads_b = CASES[name]()
    same = reads_a == reads_b
    a = api.index_build(*pack_reads(reads_a), 0)
    b = a if same else api.index_build(*pack_reads(reads_b), 0)      # a == b: the same object twice
    merged, origin = api.index_merge(a, b, 0, want_origin=True)
    bases, off = pack_reads(reads_a + reads_b)
    info = merged.info()
    assert (info.num_strings, info.num_symbols, info.block_symbols) == (len(reads_a) + len(reads_b), int(off[-1]) + len(off) - 1, 128 if wide else 192)
    for strand in (0, 1):
        np.testing.assert_array_equal(merged.units(strand, 0), api.build_bwt(bases, off, bool(strand), 0), err_msg=f"strand {strand}")
        np.testing.assert_array_equal(origin[strand], sorted_case(name)[strand][4], err_msg=f"dollar_origin of strand {strand}")
    for x in {a, b, merged}:
        x.close()


# ---- through files and the command line --------------------------------------------------------------------------------
def _run(args, cwd):
    r = subprocess.run([str(STRIDE)] + args, cwd=cwd, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r


@pytest.fixture(scope="module")
def parts(api, small_ds, tmp_path_factory):
    """small_ds in three parts, each indexed by `stride index`, and the indexes of the first two and of all three together"""
    d = tmp_path_factory.mktemp("merge_parts")
    reads = small_ds.reads
    sets = {"P0": reads[:100], "P1": reads[100:150], "P2": reads[150:], "U01": reads[:150], "U012": reads}
    for name, rs in sets.items():
        write_fasta(d / f"{name}.fa", rs)
        _run(["index", "-p", name, f"{name}.fa"], d)
    return d


def _same_files(d, got, want):
    for ext in (".bwt", ".rbwt", ".sai", ".rsai"):
        assert (d / (got + ext)).read_bytes() == (d / (want + ext)).read_bytes(), (got, want, ext)
        assert (d / (got + ext)).stat().st_size > 0


def test_indexes_opened_on_the_device_merge_to_the_built_union(api, small_ds, parts):
    """a merge does not depend on how its inputs became resident"""
    a = api.index_open_device(parts / "P0.bwt", parts / "P0.rbwt", 0)
    b = api.index_open_device(parts / "P1.bwt", parts / "P1.rbwt", 0)
    assert min(a.info().num_runs) > 0
    merged = api.index_merge(a, b, 0)
    (bases, off), _ = _split(small_ds, 150)
    union = api.index_build(bases, off, 0)
    cm, cu = _assert_same_index(api, merged, union)
    for strand, ext in enumerate(("bwt", "rbwt")):
        np.testing.assert_array_equal(merged.units(strand, 0), np.fromfile(parts / f"U01.{ext}", dtype=np.uint8)[30:])
    for x in (cm, cu, a, b, merged, union):
        x.close()


def test_input_without_a_device_copy_is_refused_and_leaves_the_device_usable(api, small_ds, parts):
    from longreadselfcorrect_amd.capi import LrscError

    host_only = api.index_open(parts / "P1.bwt", parts / "P1.rbwt")             # never uploaded
    a = api.index_open_device(parts / "P0.bwt", parts / "P0.rbwt", 0)
    for x, y in ((a, host_only), (host_only, a)):
        with pytest.raises(LrscError) as e:
            api.index_merge(x, y, 0)
        assert e.value.status == LRSC_ERR_DEVICE and "not uploaded" in e.value.detail
        out = C.c_void_p(0x5EED)
        assert api.lib.lrsc_index_merge(x.h, y.h, 0, C.byref(out), None) == LRSC_ERR_DEVICE and out.value == 0x5EED
    host_only.upload(0)
    merged = api.index_merge(a, host_only, 0)
    for strand, ext in enumerate(("bwt", "rbwt")):
        np.testing.assert_array_equal(merged.units(strand, 0), np.fromfile(parts / f"U01.{ext}", dtype=np.uint8)[30:])
    for x in (a, host_only, merged):
        x.close()


def test_stride_merge_equals_stride_index_of_the_concatenation(api, parts):
    _run(["merge", "-p", "M01", "P0", "P1"], parts)
    _same_files(parts, "M01", "U01")
    _run(["merge", "--prefix=M012", "--device=0", "P0", "P1", "P2"], parts)
    _same_files(parts, "M012", "U012")


def test_stride_pbcorrect_merge_index_end_to_end(api, parts):
    """`stride pbcorrect --build-index --merge-index=U01 P2.fa` against `stride pbcorrect -p U012 P2.fa`: same FASTA files and
    statistics, and --save-index writes the union's four files."""
    common = ["-c", "90", "-g", "5", "--batch", "70"]
    ra = _run(["pbcorrect", "--build-index", "--merge-index=U01", "--save-index=S", "-o", "X"] + common + ["P2.fa"], parts)
    rb = _run(["pbcorrect", "-p", "U012", "-o", "Y"] + common + ["P2.fa"], parts)
    for name in ("correct.fa", "discard.fa", "threshold-table"):
        assert (parts / "X" / name).read_bytes() == (parts / "Y" / name).read_bytes(), name
    assert (parts / "X" / "correct.fa").stat().st_size > 0

    def stats(text):                                        # the statistics block without its three wall-clock lines
        return [l for l in text.split("\n") if not l.startswith("Time")]

    assert stats(ra.stdout) == stats(rb.stdout) and len(stats(ra.stdout)) > 3
    _same_files(parts, "S", "U012")
