"""Locate on the device (fm_locate.hip: lrsc_index_locate_prepare, lrsc_index_lexico_order, lrsc_locate) and the command-line
pieces on top of it.  On the edge read sets everything is held against the naive suffix sort of test_index_locate_host; on
small_ds the located pairs of all rows are shown to be the one suffix array without sorting: they are a bijection onto the
(read, position) pairs and consecutive rows are strictly ordered.  `stride sai`, the merges without .sai files and `stride grep`
are compared byte for byte with the host route and with a restatement of the reference's grep."""
from __future__ import annotations

import ctypes as C
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from .conftest import write_fasta
from .test_gpu_index_build import STRIDE
from .test_gpu_index_merge import _split
from .test_index_locate_host import LOCATE_SETS, SA_DTYPE, expected, sorted_set

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG, LRSC_ERR_DEVICE = -3, -5
COMP = str.maketrans("ACGT", "TGCA")


def _all_rows(index):
    return np.arange(index.info().num_symbols, dtype=np.uint64)


# ---- the edge sets against the suffix sort -----------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
@pytest.mark.parametrize("name", list(LOCATE_SETS))
def test_edge_read_sets_equal_the_suffix_sort(api, monkeypatch, name, wide):
    from oracle.oracle_py import pack_reads

    monkeypatch.setenv("LRSC_KTAB_K", "0")                  # nothing searches these indexes
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    bases, off = pack_reads(LOCATE_SETS[name]())
    n_reads, strands = sorted_set(name)
    for rate in (0, 7, 16):
        index = api.index_build(bases, off, 0)
        assert index.info().block_symbols == (128 if wide else 192)
        units = [index.units(s, 0) for s in (0, 1)]
        index.locate_prepare(rate, 0)
        ctx = index.ctx(None, 0)
        for strand, (_, sa) in enumerate(strands):
            want_order, want_len, _ = expected(sa, n_reads, rate)
            order, read_len = index.lexico_order(strand, 0, want_len=True)
            what = f"{name} rate {rate} strand {strand}"
            np.testing.assert_array_equal(order, want_order, err_msg=f"{what}: order[]")
            np.testing.assert_array_equal(read_len, want_len, err_msg=f"{what}: read_len[]")
            np.testing.assert_array_equal(ctx.locate(strand, _all_rows(index)), sa, err_msg=f"{what}: located (read, pos)")
            np.testing.assert_array_equal(index.units(strand, 0), units[strand], err_msg=f"{what}: the units after prepare")
        ctx.close()
        index.close()


# ---- small_ds: the one suffix array, without a sort --------------------------------------------------------------------
@pytest.fixture(scope="module")
def located(api, small_ds):
    """per rate: the built index with its tables, a context, the located pairs of all rows of both strands and the LF steps"""
    from longreadselfcorrect_amd.capi import K_LOCATE

    out = {}
    for rate in (0, 16):
        index = api.index_build(small_ds.bases, small_ds.off, 0)
        index.locate_prepare(rate, 0)
        ctx = index.ctx(api.params_default(5, 90), 0)
        ctx.stats_reset()
        sa = [ctx.locate(strand, _all_rows(index)) for strand in (0, 1)]
        st = ctx.stats(K_LOCATE)
        assert st.launches == 2 and st.total_ms > 0
        out[rate] = SimpleNamespace(index=index, ctx=ctx, sa=sa, steps=int(st.rank_queries))
    yield out
    for x in out.values():
        x.ctx.close()
        x.index.close()


def _text(reads):
    """the reads as codes 1..4, each followed by a 0; where each starts"""
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    text = np.zeros(int((lens + 1).sum()), dtype=np.uint8)
    lut = np.zeros(256, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = [1, 2, 3, 4]
    for s, r in zip(start, reads):
        text[s: s + len(r)] = lut[np.frombuffer(r.encode(), dtype=np.uint8)]
    return text, start, lens


def _assert_the_suffix_array(reads, sa):
    text, start, lens = _text(reads)
    read, pos = sa["read"].astype(np.int64), sa["pos"].astype(np.int64)
    assert sa.size == text.size and (read < len(reads)).all() and (pos <= lens[np.minimum(read, len(reads) - 1)]).all()
    p = start[read] + pos
    assert np.array_equal(np.sort(p), np.arange(text.size)), "the located pairs are no bijection onto the (read, position) pairs"
    # consecutive rows: the suffix ('$' lowest, so a proper prefix first), then the read
    a, b = p[:-1].copy(), p[1:].copy()
    active = np.arange(a.size)
    while active.size:
        ca, cb = text[a[active]], text[b[active]]
        assert not (ca > cb).any(), "two consecutive rows out of order"
        ends = (ca == 0) & (cb == 0)
        assert (read[:-1][active][ends] < read[1:][active][ends]).all(), "equal suffixes out of input order"
        active = active[(ca == cb) & ~ends]
        a[active] += 1
        b[active] += 1


@pytest.mark.parametrize("rate", [0, 16])
@pytest.mark.parametrize("strand", [0, 1], ids=["bwt", "rbwt"])
def test_located_rows_are_the_suffix_array(small_ds, located, strand, rate):
    reads = small_ds.reads if strand == 0 else [r[::-1] for r in small_ds.reads]
    _assert_the_suffix_array(reads, located[rate].sa[strand])


def test_both_rates_locate_alike_and_sampling_takes_a_quarter_of_the_steps(located):
    for strand in (0, 1):
        np.testing.assert_array_equal(located[0].sa[strand], located[16].sa[strand])
    # rate 0: every row walks to its read's '$' row
    assert located[0].steps == sum(int(sa["pos"].astype(np.int64).sum()) for sa in located[0].sa)
    print(f"LF steps of all rows of both strands: {located[0].steps} at rate 0, {located[16].steps} at rate 16")
    assert 0 < 4 * located[16].steps <= located[0].steps


def test_rows_of_a_kmer_interval_are_its_occurrences(small_ds, located):
    reads = small_ds.reads
    for rate in (0, 16):
        for kmer in (reads[3][700:717], reads[90][5:22], reads[11][-17:]):
            want = sorted((i, k) for i, r in enumerate(reads) for k in range(len(r) - 16) if r.startswith(kmer, k))
            iv = located[rate].ctx.find_kmers(np.frombuffer(kmer[::-1].translate(COMP).encode(), dtype=np.uint8), 17)[0]
            rows = np.arange(iv["rvc_lower"], iv["rvc_upper"] + 1, dtype=np.uint64)
            got = located[rate].ctx.locate(0, rows)
            assert len(want) >= 1 and sorted(map(tuple, got.tolist())) == want, (rate, kmer)


# ---- other index sources ---------------------------------------------------------------------------------------------
def test_opened_and_merged_indexes_locate_as_the_built_one(api, small_ds, located):
    opened = api.index_open_device(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt", 0)
    (bases_a, off_a), (bases_b, off_b) = _split(small_ds, 120)
    a, b = api.index_build(bases_a, off_a, 0), api.index_build(bases_b, off_b, 0)
    merged = api.index_merge(a, b, 0)
    for index in (opened, merged):
        index.locate_prepare(16, 0)
        ctx = index.ctx(None, 0)
        for strand in (0, 1):
            np.testing.assert_array_equal(ctx.locate(strand, _all_rows(index)), located[16].sa[strand])
            np.testing.assert_array_equal(index.lexico_order(strand, 0), located[16].index.lexico_order(strand, 0))
        ctx.close()
    for x in (opened, a, b, merged):
        x.close()


# ---- statuses --------------------------------------------------------------------------------------------------------
def test_statuses(api, small_ds):
    from longreadselfcorrect_amd.capi import LrscError

    index = api.index_open_device(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt", 0)
    ctx = index.ctx(None, 0)
    n = index.info().num_symbols
    rows = np.array([0, n // 2, n - 1], dtype=np.uint64)
    with pytest.raises(LrscError) as e:
        ctx.locate(0, rows)
    assert e.value.status == LRSC_ERR_DEVICE and "lrsc_index_locate_prepare" in e.value.detail
    index.locate_prepare(16, 0)
    want = ctx.locate(0, rows)
    index.locate_prepare(16, 0)                                  # the same rate again: nothing happens
    with pytest.raises(LrscError) as e:
        index.locate_prepare(32, 0)
    assert e.value.status == LRSC_ERR_ARG and "already prepared with rate 16" in e.value.detail
    with pytest.raises(LrscError) as e:
        index.locate_prepare(0, 0)
    assert e.value.status == LRSC_ERR_ARG
    np.testing.assert_array_equal(ctx.locate(0, rows), want)     # the tables still answer
    assert want["read"][0] == 0 and want["pos"][0] == index.lexico_order(0, 0, want_len=True)[1][0]     # row 0: read 0's sentinel
    for strand in (0, 1):
        with pytest.raises(LrscError) as e:
            ctx.locate(strand, np.array([0, n], dtype=np.uint64))
        assert e.value.status == LRSC_ERR_ARG and "out of range" in e.value.detail
    with pytest.raises(LrscError) as e:
        ctx.locate(2, rows)
    assert e.value.status == LRSC_ERR_ARG
    assert ctx.locate(1, np.zeros(0, dtype=np.uint64)).size == 0

    host_only = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")          # never uploaded
    with pytest.raises(LrscError) as e:
        host_only.locate_prepare(16, 0)
    assert e.value.status == LRSC_ERR_DEVICE and "not uploaded" in e.value.detail
    order = np.full(small_ds.n_reads, 0x5EED, dtype=np.uint32)
    assert api.lib.lrsc_index_lexico_order(host_only.h, 0, 0, order.ctypes.data_as(C.c_void_p), None) == LRSC_ERR_DEVICE
    assert (order == 0x5EED).all()                               # untouched, as *out of the neighbouring entries
    host_only.upload(0)
    np.testing.assert_array_equal(host_only.lexico_order(0, 0), index.lexico_order(0, 0))    # prepares with rate 0 by itself
    c2 = host_only.ctx(None, 0)
    np.testing.assert_array_equal(c2.locate(0, rows), want)
    for x in (ctx, c2, index, host_only):
        x.close()


# ---- through files and the command line --------------------------------------------------------------------------------
def _run(args, cwd, stdin=""):
    r = subprocess.run([str(STRIDE)] + args, cwd=cwd, capture_output=True, text=True, input=stdin)
    assert r.returncode == 0, (args, r.stderr)
    return r


@pytest.fixture(scope="module")
def parts(api, small_ds, tmp_path_factory):
    """small_ds in three parts and whole, each indexed by `stride index`; Q0 and Q1 are P0 and P1 without .sai/.rsai"""
    d = tmp_path_factory.mktemp("locate_parts")
    reads = small_ds.reads
    for name, rs in {"P0": reads[:100], "P1": reads[100:150], "P2": reads[150:], "U": reads}.items():
        write_fasta(d / f"{name}.fa", rs)
        _run(["index", "-p", name, f"{name}.fa"], d)
    for src, dst in (("P0", "Q0"), ("P1", "Q1")):
        for ext in (".bwt", ".rbwt"):
            shutil.copy(d / (src + ext), d / (dst + ext))
    return d


def _same_files(d, got, want):
    for ext in (".bwt", ".rbwt", ".sai", ".rsai"):
        assert (d / (got + ext)).read_bytes() == (d / (want + ext)).read_bytes(), (got, want, ext)
        assert (d / (got + ext)).stat().st_size > 0


def _read_sai(path):
    lines = path.read_text().split("\n")
    assert lines[0] == "51914" and lines[1] == lines[2] and lines[-1] == ""
    body = [l.split(" ") for l in lines[3:-1]]
    assert len(body) == int(lines[1]) and all(len(b) == 2 and b[1] == "0" for b in body)
    return np.array([int(b[0]) for b in body], dtype=np.uint32)


def test_lexico_order_equals_the_sai_files_of_stride_index(located, parts):
    for rate in (0, 16):
        for strand, ext in enumerate((".sai", ".rsai")):
            np.testing.assert_array_equal(located[rate].index.lexico_order(strand, 0), _read_sai(parts / ("U" + ext)))


def test_stride_sai_reproduces_the_files_of_stride_index(api, parts):
    for ext in (".bwt", ".rbwt"):
        shutil.copy(parts / ("P0" + ext), parts / ("C" + ext))
    assert not (parts / "C.sai").exists()
    _run(["sai", "--device=0", "-p", "C"], parts)
    _same_files(parts, "C", "P0")
    _run(["sai", "--prefix=Q1"], parts)
    try:
        _same_files(parts, "Q1", "P1")
    finally:
        (parts / "Q1.sai").unlink(missing_ok=True)
        (parts / "Q1.rsai").unlink(missing_ok=True)


def test_stride_merge_without_sai_files_writes_the_same_index(api, parts):
    _run(["merge", "-p", "M", "P0", "P1"], parts)
    assert not (parts / "Q1.sai").exists() and not (parts / "Q0.rsai").exists()
    _run(["merge", "-p", "M1", "P0", "Q1"], parts)
    _same_files(parts, "M1", "M")
    _run(["merge", "-p", "M2", "Q0", "P1"], parts)
    _same_files(parts, "M2", "M")


def test_stride_pbcorrect_merge_index_without_sai_files_saves_the_same_index(api, parts):
    common = ["-c", "90", "-g", "5", "--batch", "70"]
    _run(["pbcorrect", "--build-index", "--merge-index=P0", "--save-index=S", "-o", "X"] + common + ["P2.fa"], parts)
    _run(["pbcorrect", "--build-index", "--merge-index=Q0", "--save-index=T", "-o", "Y"] + common + ["P2.fa"], parts)
    _same_files(parts, "T", "S")
    assert (parts / "X" / "correct.fa").read_bytes() == (parts / "Y" / "correct.fa").read_bytes()


def _grep(reads, queries):
    """StriDe/grep.cpp:56-138 restated: the rows of a query's interval are its occurrences in suffix order, the suffix running to
    the end of its read ('$' lowest: a proper prefix first), equal ones in read order"""
    out, seen = [], []
    for q in queries:
        out.append("--\n")
        if q and set(q) <= set("ACGT"):
            hits = sorted((r[k:], i) for i, r in enumerate(reads) for k in range(len(r) - len(q) + 1) if r.startswith(q, k))
            for _, i in hits:
                at = reads[i].find(q)
                out.append(f"r{i}\n{reads[i][:at]}\033[33m{q}\033[0m{reads[i][at + len(q):]}\n")
                if i not in seen:
                    seen.append(i)
        out.append("--\n")
    out += [f">r{i}\n{reads[i]}\n" for i in seen]
    return "".join(out)


def test_stride_grep_equals_the_reference_s_grep(api, small_ds, parts):
    reads = small_ds.reads
    count = lambda q: sum(r.count(q) > 0 for r in reads)
    mers = [reads[7][s: s + 17] for s in range(0, len(reads[7]) - 17, 3)]
    many = max(mers, key=count)
    once = next(m for m in mers if count(m) == 1 and sum(r.count(m) for r in reads) == 1)
    rng = np.random.default_rng(12)
    absent = next(m for m in ("".join(rng.choice(list("ACGT"), size=17)) for _ in range(100)) if count(m) == 0)
    with_n = many[:8] + "N" + many[9:]
    short = many[2:14]                                           # another length: in every read that holds `many`, and more
    assert count(many) >= 5 and count(short) >= count(many)
    queries = [many, once, absent, with_n, short, once]
    want = _grep(reads, queries)
    assert want.count("\033[33m") >= count(many) + count(short) + 2
    stdin = f"{many} {once}\n{absent}\t{with_n}\n\n{short}\n{once}"
    for args in (["grep", "-p", "U", "U.fa"], ["grep", "U.fa"], ["grep", "--sample-rate=0", "--device=0", "--prefix=U", "U.fa"], ["grep", "--sample-rate=1", "U.fa"]):
        got = subprocess.run([str(STRIDE)] + args, cwd=parts, capture_output=True, input=stdin.encode())
        assert got.returncode == 0, (args, got.stderr)
        assert got.stdout == want.encode(), args
    assert _run(["grep", "U.fa"], parts, stdin="").stdout == ""
