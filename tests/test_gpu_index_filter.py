"""lrsc_dupcheck_reads (fm_dup.hip) against the plain definition of test_index_filter_host, lrsc_index_remove (fm_remove.hip)
against lrsc_index_build of the kept reads, and `stride filter` against both and against `stride index` of its pass file.
Every comparison is exact."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from .test_gpu_index_build import STRIDE, _assert_same_answers
from .test_gpu_index_merge import _assert_same_index
from .test_index_filter_host import (ABSENT, DUP_SETS, FULL_LENGTH, REMOVE_SETS, SUBSTRING, UNIQUE, assert_same_dup, dup_case, plain_dupcheck,
                                     remove_case, revcomp)

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG, LRSC_ERR_DEVICE = -3, -5


def _force(monkeypatch, wide):
    """LRSC_FORCE_WIDE is read per call: set or unset before each index is made"""
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    else:
        monkeypatch.delenv("LRSC_FORCE_WIDE", raising=False)


def _session_calls(api, index, calls):
    """the calls of one lrsc_dupcheck on a fresh context of the index -> one DUP_DTYPE array per call, K_FIND's statistics"""
    from longreadselfcorrect_amd import capi
    from oracle.oracle_py import pack_reads

    ctx = index.ctx(api.params_default(5, 90), 0)
    session = ctx.dupcheck()
    got = [session.reads(*pack_reads(call)) for call in calls]
    stats = ctx.stats(capi.K_FIND)
    session.close()
    ctx.close()
    return got, stats


# ---- the duplicate check ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_dup_sets_equal_the_plain_definition(api, monkeypatch, wide):
    from oracle.oracle_py import pack_reads

    monkeypatch.setenv("LRSC_KTAB_K", "0")                  # the check starts no search from a table
    _force(monkeypatch, wide)
    for name in DUP_SETS:
        reads, calls, _, want = dup_case(name)
        index = api.index_build(*pack_reads(reads), 0)
        assert index.info().block_symbols == (128 if wide else 192)
        got, stats = _session_calls(api, index, calls)
        for k, (g, w) in enumerate(zip(got, want)):
            assert_same_dup(g, w, f"{name} call {k}")
        assert stats.launches == len(calls) and stats.rank_queries // 2 <= stats.block_loads <= stats.rank_queries
        index.close()


@pytest.fixture(scope="module")
def planted(small_ds):
    """small_ds's reads with copies, reverse complements and substrings of some of them planted among them, and what the plain
    definition makes of them, taken in one call"""
    reads = small_ds.reads
    plants = [reads[3], revcomp(reads[5]), reads[7][100:900], revcomp(reads[9][:700]), reads[11][-500:], reads[3], reads[13][1:]]
    out = list(reads)
    for k, p in enumerate(plants):
        out.insert(20 * k + 10, p)
    want = plain_dupcheck(out, [out])[0]
    counts = np.bincount(want["cls"], minlength=4)
    assert counts[SUBSTRING] >= 4 and counts[FULL_LENGTH] >= 3 and counts[UNIQUE] >= 150 and counts[ABSENT] == 0
    return out, want


def _batches(reads, size):
    return [reads[i: i + size] for i in range(0, len(reads), size)]


def _assert_planted(api, index, planted, size):
    reads, want = planted
    got, stats = _session_calls(api, index, _batches(reads, size))
    assert_same_dup(np.concatenate(got), want, f"batches of {size}")
    return stats


@pytest.mark.parametrize("size", [1, 7, 10 ** 6], ids=["batches_of_1", "batches_of_7", "one_batch"])
def test_planted_duplicates_in_a_built_index_whatever_the_batches(api, planted, size):
    from oracle.oracle_py import pack_reads

    index = api.index_build(*pack_reads(planted[0]), 0)
    stats = _assert_planted(api, index, planted, size)
    # a step of a chain is two Occ queries; a read of L bases takes at most 4 (L - 1) steps
    assert 0 < stats.rank_queries <= 8 * sum(len(r) - 1 for r in planted[0])
    index.close()


@pytest.mark.parametrize("config", ["opened_on_device", "block64", "no_kmer_tables", "opened_block64"])
def test_planted_duplicates_in_other_indexes_of_the_same_reads(api, planted, monkeypatch, tmp_path, config):
    from oracle.oracle_py import pack_reads

    if config == "no_kmer_tables":
        monkeypatch.setenv("LRSC_KTAB_K", "0")
    built = api.index_build(*pack_reads(planted[0]), 0)
    index = built
    if config.startswith("opened"):
        built.write(tmp_path / "p.bwt", tmp_path / "p.rbwt", 0)
        _force(monkeypatch, config == "opened_block64")
        index = api.index_open_device(tmp_path / "p.bwt", tmp_path / "p.rbwt", 0)
        assert min(index.info().num_runs) > 0
    elif config == "block64":
        _force(monkeypatch, True)
        index = api.index_build(*pack_reads(planted[0]), 0)
    assert index.info().block_symbols == (128 if config.endswith("block64") else 192)
    _assert_planted(api, index, planted, 64)
    for x in {built, index}:
        x.close()


def test_dupcheck_refuses_empty_reads_and_other_bases_and_keeps_its_bits(api):
    from longreadselfcorrect_amd.capi import LrscError
    from oracle.oracle_py import pack_reads

    reads, calls, _, want = dup_case("three_copies")
    index = api.index_build(*pack_reads(reads), 0)
    ctx = index.ctx(api.params_default(5, 90), 0)
    session = ctx.dupcheck()
    for bad in ([reads[0], "", reads[1]], [reads[0], "ACGNT"]):
        with pytest.raises(LrscError) as e:
            session.reads(*pack_reads(bad))
        assert e.value.status == LRSC_ERR_ARG
    assert_same_dup(session.reads(*pack_reads(calls[0])), want[0], "after the refused calls")
    session.close()
    ctx.close()
    index.close()


# ---- the removal ----------------------------------------------------------------------------------------------------------
def _kept(reads, drop):
    from oracle.oracle_py import pack_reads

    return pack_reads([r for r, d in zip(reads, drop) if not d])


@pytest.mark.parametrize("wide_in,wide_out", [(False, False), (True, True), (True, False), (False, True)], ids=["32_to_32", "64_to_64", "64_to_32", "32_to_64"])
def test_removed_index_equals_built_index_of_the_kept_reads(api, small_ds, monkeypatch, wide_in, wide_out):
    reads = small_ds.reads
    drop = np.array([int(i % 5 == 2 or i >= 170) for i in range(len(reads))], dtype=np.uint8)
    _force(monkeypatch, wide_in)
    index = api.index_build(small_ds.bases, small_ds.off, 0)
    units_before = [index.units(s, 0) for s in (0, 1)]
    _force(monkeypatch, wide_out)
    removed = index.remove(drop, 0)
    bases, off = _kept(reads, drop)
    want = api.index_build(bases, off, 0)
    syms = lambda wide: 128 if wide else 192
    assert (index.info().block_symbols, removed.info().block_symbols) == (syms(wide_in), syms(wide_out))
    assert removed.info().num_strings == len(reads) - int(drop.sum()) == off.size - 1
    cr, cw = _assert_same_index(api, removed, want)
    _assert_same_answers(cr, cw, bases, off, 32)
    for before, s in zip(units_before, (0, 1)):             # the input answers as before
        np.testing.assert_array_equal(before, index.units(s, 0))
    for x in (cr, cw, index, removed, want):
        x.close()


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
@pytest.mark.parametrize("name", list(REMOVE_SETS))
def test_edge_drops_equal_build_bwt_of_the_kept_reads(api, monkeypatch, name, wide):
    from oracle.oracle_py import pack_reads

    monkeypatch.setenv("LRSC_KTAB_K", "0")                  # nothing searches these indexes
    _force(monkeypatch, wide)
    reads, drop, _ = remove_case(name)
    index = api.index_build(*pack_reads(reads), 0)
    removed = index.remove(drop, 0)
    bases, off = _kept(reads, drop)
    info = removed.info()
    assert (info.num_strings, info.num_symbols, info.block_symbols, list(info.num_runs)) == (off.size - 1, int(off[-1]) + off.size - 1, 128 if wide else 192, [0, 0])
    for strand in (0, 1):
        np.testing.assert_array_equal(removed.units(strand, 0), api.build_bwt(bases, off, bool(strand), 0), err_msg=f"strand {strand}")
    index.close()
    removed.close()


def test_remove_refuses_what_it_must_and_leaves_the_device_usable(api, small_ds):
    from longreadselfcorrect_amd.capi import LrscError

    n = small_ds.n_reads
    drop = np.zeros(n, dtype=np.uint8)
    drop[::2] = 1
    host_only = api.index_open(small_ds.prefix + ".bwt", small_ds.prefix + ".rbwt")           # never uploaded
    with pytest.raises(LrscError) as e:
        host_only.remove(drop, 0)
    assert e.value.status == LRSC_ERR_DEVICE and "not uploaded" in e.value.detail
    host_only.upload(0)
    for bad, why in ((drop[:-1], "entries"), (np.ones(n, dtype=np.uint8), "nothing is kept")):
        with pytest.raises(LrscError) as e:
            host_only.remove(bad, 0)
        assert e.value.status == LRSC_ERR_ARG and why in e.value.detail
        out = C.c_void_p(0x5EED)
        assert api.lib.lrsc_index_remove(host_only.h, bad.ctypes.data_as(C.c_void_p), bad.size, 0, C.byref(out)) == LRSC_ERR_ARG and out.value == 0x5EED
    removed = host_only.remove(drop, 0)
    bases, off = _kept(small_ds.reads, drop)
    for strand in (0, 1):
        np.testing.assert_array_equal(removed.units(strand, 0), api.build_bwt(bases, off, bool(strand), 0))
    host_only.close()
    removed.close()


def test_merge_of_a_removed_index_equals_the_built_index(api, small_ds):
    """X = A + B; merge(remove(X, B's reads), B') == build(A + B')"""
    from oracle.oracle_py import pack_reads

    reads = small_ds.reads
    a, b2 = reads[:120], [revcomp(r) for r in reads[150:]]
    x = api.index_build(small_ds.bases, small_ds.off, 0)
    only_a = x.remove(np.array([0] * 120 + [1] * (len(reads) - 120), dtype=np.uint8), 0)
    other = api.index_build(*pack_reads(b2), 0)
    merged = api.index_merge(only_a, other, 0)
    want = api.index_build(*pack_reads(a + b2), 0)
    cm, cw = _assert_same_index(api, merged, want)
    for v in (cm, cw, x, only_a, other, merged, want):
        v.close()


# ---- `stride filter` end to end ------------------------------------------------------------------------------------------
def _run(args, cwd, ok=True):
    r = subprocess.run([str(STRIDE)] + args, cwd=cwd, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _fasta(reads, ids, suffix=lambda i: ""):
    return "".join(f">r{i}{suffix(i)}\n{reads[i]}\n" for i in ids)


def _counts(kept, discarded, dup=None, hp=0, degen=0):
    dup = discarded - hp - degen if dup is None else dup
    return [f"Reads kept: {kept}", f"Reads discarded: {discarded}", "Reads failed kmer check: 0", f"Reads failed duplicate check: {dup}",
            f"Reads failed homopolymer check: {hp}", f"Reads failed degenerate check: {degen}"]


def _count_lines(stdout):
    return [l for l in stdout.split("\n") if l.startswith("Reads ")]


def _same_index_files(d, got, want):
    for ext in (".bwt", ".rbwt", ".sai", ".rsai"):
        assert (d / (got + ext)).read_bytes() == (d / (want + ext)).read_bytes(), (got, want, ext)
        assert (d / (got + ext)).stat().st_size > 0


@pytest.fixture(scope="module")
def filter_dir(api, tmp_path_factory):
    """about 300 reads of 200 to 2000 bases off one genome, with copies, reverse complements and substrings planted; their index
    by `stride index`; the classes by the plain definition"""
    d = tmp_path_factory.mktemp("filter")
    rng = np.random.default_rng(0xF117E4)
    genome = "".join(rng.choice(list("ACGT"), size=400000))     # one-fold coverage: few reads lie inside another by chance
    reads = []
    for _ in range(280):
        n = int(rng.integers(200, 2001))
        s = int(rng.integers(0, len(genome) - n))
        reads.append(genome[s: s + n] if rng.random() < 0.5 else revcomp(genome[s: s + n]))
    plants = [reads[4], revcomp(reads[8]), reads[15][50:450], revcomp(reads[16][:300]), reads[23][-250:], reads[4], reads[42][1:], revcomp(reads[8]),
              reads[60][:-1], reads[77]]
    for k, p in enumerate(plants):
        reads.insert(25 * k + 12, p)
    want = plain_dupcheck(reads, [reads])[0]["cls"]
    counts = np.bincount(want, minlength=4)
    assert 200 <= min(map(len, reads)) and max(map(len, reads)) <= 2000 and counts[FULL_LENGTH] >= 5 and counts[SUBSTRING] >= 5 and counts[ABSENT] == 0
    (d / "reads.fa").write_text(_fasta(reads, range(len(reads))))
    _run(["index", "-p", "reads", "reads.fa"], d)
    return d, reads, want


def _assert_filtered(d, reads, passed, stdout, pass_file, discard_file, index_prefix):
    ids = range(len(reads))
    assert (d / pass_file).read_text() == _fasta(reads, [i for i in ids if passed[i]])
    assert (d / discard_file).read_text() == _fasta(reads, [i for i in ids if not passed[i]], lambda i: f",seqrank={i}")
    kept = int(np.sum(passed))
    assert _count_lines(stdout) == _counts(kept, len(reads) - kept)
    want = "want_" + index_prefix.replace(".", "_")
    _run(["index", "-p", want, pass_file], d)
    _same_index_files(d, index_prefix, want)


def test_stride_filter_equals_the_plain_definition_and_stride_index_of_the_pass_file(api, filter_dir):
    d, reads, want = filter_dir
    r = _run(["filter", "reads.fa"], d)
    _assert_filtered(d, reads, want == UNIQUE, r.stdout, "reads.filter.pass.fa", "reads.discard.fa", "reads.filter.pass")


def test_stride_filter_build_index_and_outfile(api, filter_dir):
    d, reads, want = filter_dir
    r = _run(["filter", "--build-index", "--device=0", "-t", "4", "-o", "kept.fa", "reads.fa"], d)
    _assert_filtered(d, reads, want == UNIQUE, r.stdout, "kept.fa", "kept.discard.fa", "kept")


def test_stride_filter_substring_only(api, filter_dir):
    d, reads, want = filter_dir
    r = _run(["filter", "--substring-only", "-p", "reads", "--outfile=nosub.fa", "reads.fa"], d)
    _assert_filtered(d, reads, want != SUBSTRING, r.stdout, "nosub.fa", "nosub.discard.fa", "nosub")


def test_stride_filter_without_the_duplicate_check_keeps_every_read_and_the_index(api, filter_dir):
    d, reads, _ = filter_dir
    r = _run(["filter", "--no-duplicate-check", "--no-kmer-check", "-o", "all.fa", "reads.fa"], d)
    assert (d / "all.fa").read_text() == (d / "reads.fa").read_text() and (d / "all.discard.fa").read_text() == ""
    assert _count_lines(r.stdout) == _counts(len(reads), 0)
    _same_index_files(d, "all", "reads")


def test_stride_filter_refuses_a_reads_file_that_is_not_the_index_s(api, filter_dir):
    d, reads, _ = filter_dir
    swapped = list(reads)
    swapped[30], swapped[200] = swapped[200], swapped[30]
    assert swapped[30] != reads[30]
    (d / "swapped.fa").write_text(_fasta(swapped, range(len(swapped))))
    r = _run(["filter", "-p", "reads", "swapped.fa"], d, ok=False)
    assert "filter: read 30 of swapped.fa is not read 30 of the index reads" in r.stderr and "no index written" in r.stderr
    assert not any((d / ("swapped.filter.pass" + ext)).exists() for ext in (".bwt", ".rbwt", ".sai", ".rsai"))
    (d / "short.fa").write_text(_fasta(reads, range(len(reads) - 1)))
    r = _run(["filter", "-p", "reads", "short.fa"], d, ok=False)
    assert f"short.fa holds {len(reads) - 1} reads, the index reads {len(reads)}" in r.stderr
    assert not (d / "short.filter.pass.bwt").exists()


def test_stride_filter_homopolymer_and_low_complexity_checks(api, tmp_path):
    """eleven reads share a 58-mer with a run of eight A, a twelfth has it with seven: its covering 51-mer is seen once, the one
    with the run a base longer eleven times, so it fails the homopolymer check; a read of 19 A in 20 fails the degenerate check"""
    rng = np.random.default_rng(51)

    def flank(n):                                           # no run of six or more
        while True:
            s = "".join(rng.choice(list("ACGT"), size=n))
            if max(len(m) for m in re.findall(r"A+|C+|G+|T+", s)) < 6:
                return s

    left, right = flank(25), flank(25)
    left, right = left[:-1] + "C", "G" + right[1:]
    reads = [flank(100) + "C" + left + "A" * 8 + right + "G" + flank(100) for _ in range(11)]
    reads.append(flank(100) + "C" + left + "A" * 7 + right + "G" + flank(100))
    reads.append(("A" * 19 + "C") * 4)
    assert (plain_dupcheck(reads, [reads])[0]["cls"] == UNIQUE).all()
    (tmp_path / "hp.fa").write_text(_fasta(reads, range(len(reads))))
    r = _run(["filter", "--build-index", "--homopolymer-check", "--low-complexity-check", "hp.fa"], tmp_path)
    assert _count_lines(r.stdout) == _counts(11, 2, dup=0, hp=1, degen=1)
    assert (tmp_path / "hp.discard.fa").read_text() == _fasta(reads, [11, 12], lambda i: f",seqrank={i}")
    _run(["index", "-p", "want", "hp.filter.pass.fa"], tmp_path)
    _same_index_files(tmp_path, "hp.filter.pass", "want")
    r = _run(["filter", "--build-index", "hp.fa"], tmp_path)      # neither check unless asked for
    assert _count_lines(r.stdout) == _counts(13, 0)
