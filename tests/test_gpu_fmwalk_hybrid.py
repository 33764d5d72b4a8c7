"""lrsc_fmwalk_hybrid, lrsc_fmwalk_kmerize and lrsc_kmer_sample_counts (fm_kmerize.hip) against the plain restatement of
test_fmwalk_hybrid_host.  Every comparison is exact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from .test_fmwalk_host import INSERT, K, M_MIN, X, Counts, fw_case, index_case, index_reads, pairs_input
from .test_fmwalk_hybrid_host import HYBRID_DTYPE, HYBRID_SETS, KMERIZE_SETS, PIECE_DTYPE, READ_DTYPE, check_unwritten, hy_case, hy_options, hybrid_dicts, km_case, \
    piece_slots, plain_kmerize, plain_merge_and_kmerize, plain_quartile2, plain_sample_count, read_record, reads_input, sample_rows
from .test_gpu_fmwalk import _count_lines, _records, _run

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG, LRSC_ERR_UNSUPPORTED = -3, -7


def _force(monkeypatch, wide):
    """LRSC_FORCE_WIDE is read per call: set or unset before each index is made"""
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    else:
        monkeypatch.delenv("LRSC_FORCE_WIDE", raising=False)


def _context(api):
    from oracle.oracle_py import pack_reads

    index = api.index_build(*pack_reads(index_case()[0]), 0)
    return index, index.ctx(api.params_default(5, 90), 0)


def _kmerize(ctx, reads, k, x) -> list[dict]:
    bases, off = reads_input(reads)
    res, pieces, slots = ctx.fmwalk_kmerize(bases, off, k, x)
    assert slots.tolist() == piece_slots(reads, k).tolist()
    check_unwritten(pieces[: int(slots[-1])], slots, [int(q["n_pieces"]) for q in res], 0)
    return [read_record(q, pieces, int(slots[i]), reads[i], 0) for i, q in enumerate(res)]


def _hybrid(ctx, pairs, s) -> list[dict]:
    bases, off = pairs_input(pairs)
    merged, res, pieces, slots = ctx.fmwalk_hybrid(bases, off, s["repeat"], s["k"], s["x"], s["m"], s["max_overlap"], s["insert"], s["leaves"])
    for q, row in zip(res, merged):                               # nothing is written beyond the merged string
        assert (row[int(q["walk"]["length"]) if q["walk"]["merged"] else 0:] == 0).all()
    return hybrid_dicts(res, [row.tobytes().decode("latin-1") for row in merged], pieces[: int(slots[-1])], slots, pairs, 0)


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_every_set_equals_the_yardstick(api, monkeypatch, wide):
    from longreadselfcorrect_amd import capi

    assert capi.FMWALK_HYBRID_DTYPE == HYBRID_DTYPE and capi.FMWALK_READ_DTYPE == READ_DTYPE and capi.FMWALK_PIECE_DTYPE == PIECE_DTYPE
    _force(monkeypatch, wide)
    index, ctx = _context(api)
    assert index.info().block_symbols == (128 if wide else 192)
    for name in KMERIZE_SETS:
        (reads, k, x), want = km_case(name)
        ctx.stats_reset()
        assert _kmerize(ctx, reads, k, x) == want, name
        stats = ctx.stats(capi.K_FIND)
        assert stats.launches == 1 and stats.rank_queries > 0 and stats.rank_queries // 2 <= stats.block_loads <= stats.rank_queries, name
    for name in HYBRID_SETS:
        s, want = hy_case(name)
        ctx.stats_reset()
        got = _hybrid(ctx, s["pairs"], s)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, i)
        stats = ctx.stats(capi.K_FIND)
        split = any(rd["pieces"] for w in want for rd in w["reads"])
        assert len(got) == len(want) and stats.launches == 2 + (1 if split else 0), name      # the gate, the walks, the splits
        assert stats.rank_queries > 0 and stats.rank_queries // 2 <= stats.block_loads <= stats.rank_queries, name
    ctx.close()
    index.close()


@pytest.fixture(scope="module")
def shuffled():
    """the pairs of every hybrid set with the default options and the reads of every kmerize set with them, shuffled, and what the
    yardstick makes of them"""
    pairs, want, options = [], [], None
    for name in HYBRID_SETS:
        s, w = hy_case(name)
        if hy_options(s) == hy_options(hy_case("merges_as_merge_does")[0]) and s["repeat"] == hy_case("merges_as_merge_does")[0]["repeat"]:
            pairs += s["pairs"]
            want += w
            options = s
    reads, rwant = [], []
    for name in KMERIZE_SETS:
        (r, k, x), w = km_case(name)
        if (k, x) == (K, X):
            reads += r
            rwant += w
    order, rorder = np.random.default_rng(12).permutation(len(pairs)), np.random.default_rng(13).permutation(len(reads))
    assert len(pairs) >= 16 and len(reads) >= 12
    return [pairs[i] for i in order], [want[i] for i in order], options, [reads[i] for i in rorder], [rwant[i] for i in rorder]


@pytest.mark.parametrize("size", [1, 7, 10 ** 6], ids=["batches_of_1", "batches_of_7", "one_batch"])
def test_shuffled_reads_whatever_the_batches(api, shuffled, size):
    pairs, want, options, reads, rwant = shuffled
    index, ctx = _context(api)
    got = []
    for i in range(0, len(pairs), size):
        got += _hybrid(ctx, pairs[i: i + size], options)
    assert got == want
    got = []
    for i in range(0, len(reads), size):
        got += _kmerize(ctx, reads[i: i + size], K, X)
    assert got == rwant
    ctx.close()
    index.close()


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_sample_counts_of_every_row(api, monkeypatch, wide):
    from longreadselfcorrect_amd import capi

    _force(monkeypatch, wide)
    index, ctx = _context(api)
    reads, c, _, _ = index_case()
    rows, lengths = sample_rows()
    for length in lengths:
        ctx.stats_reset()
        got = ctx.kmer_sample_counts(rows, length)
        assert got.tolist() == [plain_sample_count(c, reads, int(r), length) for r in rows], length
        assert ctx.stats(capi.K_FIND).launches == 1
    again = np.concatenate([rows[::-1], rows[:5], rows[:5]])      # any order, repeats
    assert ctx.kmer_sample_counts(again, M_MIN).tolist() == [plain_sample_count(c, reads, int(r), M_MIN) for r in again]
    ctx.close()
    index.close()


def test_refused_arguments_leave_the_outputs_untouched(api):
    from longreadselfcorrect_amd import capi

    s, want = hy_case("merges_as_merge_does")
    index, ctx = _context(api)
    good = s["pairs"][:2]
    ok = (K, X, M_MIN, -1, INSERT, 32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def hybrid(pairs, params, stride=INSERT + 1, n_pairs=None, slots=None):
        bases, off = pairs_input(pairs)
        merged = np.full(len(pairs) * max(stride, 1), 0x5A, dtype=np.uint8)
        out = np.full(len(pairs) * 24, 0x5EED, dtype=np.uint32)
        need = int(piece_slots([r for p in pairs for r in p], max(params[0], 1))[-1])
        pieces = np.full(3 * max(need, 1), 0x5EED, dtype=np.uint32)
        p = np.array(params, dtype=np.int32)
        st = api.lib.lrsc_fmwalk_hybrid(ctx.h, ptr(bases), ptr(off), len(pairs) if n_pairs is None else n_pairs, ptr(p), 10 ** 6, ptr(merged), stride, ptr(out),
                                        ptr(pieces), need if slots is None else slots)
        return st, (merged == 0x5A).all() and (out == 0x5EED).all() and (pieces == 0x5EED).all()

    def kmerize(reads, k, x, n_reads=None, slots=None):
        bases, off = reads_input(reads)
        out = np.full(len(reads) * 6, 0x5EED, dtype=np.uint32)
        need = int(piece_slots(reads, max(k, 1))[-1])
        pieces = np.full(3 * max(need, 1), 0x5EED, dtype=np.uint32)
        st = api.lib.lrsc_fmwalk_kmerize(ctx.h, ptr(bases), ptr(off), len(reads) if n_reads is None else n_reads, k, x, ptr(out), ptr(pieces),
                                         need if slots is None else slots)
        return st, (out == 0x5EED).all() and (pieces == 0x5EED).all()

    def sample(rows, length, n=None):
        rows = np.array(rows, dtype=np.uint64)
        counts = np.full(max(rows.size, 1), 0x5EED, dtype=np.uint32)
        st = api.lib.lrsc_kmer_sample_counts(ctx.h, ptr(rows), rows.size if n is None else n, length, ptr(counts))
        return st, (counts == 0x5EED).all()

    replaced = lambda i, v: tuple(v if j == i else x for j, x in enumerate(ok))
    refused = [(good, replaced(i, v), INSERT + 1, None, LRSC_ERR_ARG) for i in range(6) for v in (0, -2)]
    refused += [(good, replaced(2, 1), INSERT + 1, None, LRSC_ERR_ARG), (good, ok, INSERT, None, LRSC_ERR_ARG), (good, ok, INSERT + 1, 143, LRSC_ERR_ARG),
                ([good[0], (good[1][0], "ACGTNACGT" * 4)], ok, INSERT + 1, None, LRSC_ERR_ARG), ([good[0], ("", good[1][1])], ok, INSERT + 1, None, LRSC_ERR_ARG),
                (good, replaced(5, 65), INSERT + 1, None, LRSC_ERR_UNSUPPORTED), (good, replaced(4, 2001), 2002, None, LRSC_ERR_UNSUPPORTED),
                (good, replaced(2, 256), INSERT + 1, None, LRSC_ERR_UNSUPPORTED), (good, replaced(0, 256), INSERT + 1, None, LRSC_ERR_UNSUPPORTED)]
    assert int(piece_slots([r for p in good for r in p], K)[-1]) == 144
    for pairs, params, stride, slots, status in refused:
        st, untouched = hybrid(pairs, params, stride, slots=slots)
        assert st == status and untouched, (params, stride, slots, st)
    reads = [good[0][0], good[1][1], "ACGT"]
    for args, status in (((reads, 0, X), LRSC_ERR_ARG), ((reads, -1, X), LRSC_ERR_ARG), ((reads, K, 0), LRSC_ERR_ARG), ((reads, 256, X), LRSC_ERR_UNSUPPORTED),
                         ((reads + ["ACGNT" * 5], K, X), LRSC_ERR_ARG), ((reads + [""] + reads, K, X), LRSC_ERR_ARG)):
        st, untouched = kmerize(*args)
        assert st == status and untouched, (args[1:], st)
    st, untouched = kmerize(reads, K, X, slots=71)
    assert st == LRSC_ERR_ARG and untouched
    n = len(index_case()[0])
    for rows, length, status in (([0, 1], 0, LRSC_ERR_ARG), ([0, n], 5, LRSC_ERR_ARG), ([2 ** 40], 5, LRSC_ERR_ARG), ([0, 1], 4097, LRSC_ERR_UNSUPPORTED)):
        st, untouched = sample(rows, length)
        assert st == status and untouched, (rows, length, st)
    # valid calls that do nothing
    assert hybrid(good, ok, n_pairs=0) == (0, True) and kmerize(reads, K, X, n_reads=0) == (0, True) and sample([0, 1], 5, n=0) == (0, True)
    assert ctx.stats(capi.K_FIND).launches == 0
    st, untouched = kmerize(["ACGT", "A"], K, X)                  # no read reaches k: the records are written, nothing is launched
    assert st == 0 and not untouched and ctx.stats(capi.K_FIND).launches == 0
    assert _hybrid(ctx, s["pairs"], s) == want, "after the refused calls"
    ctx.close()
    index.close()


def test_merge_mode_is_as_it_was(api):
    """lrsc_fmwalk_merge between two hybrid calls on the same context, which share its buffers"""
    from .test_gpu_fmwalk import _merge

    index, ctx = _context(api)
    s, want = hy_case("bubble")
    assert _hybrid(ctx, s["pairs"], s) == want
    for name in ("unique_path", "bubble_l32", "stretch_l1", "trims_at_the_site_and_merges"):
        fs, fwant, _ = fw_case(name)
        assert _merge(ctx, fs["pairs"], fs) == fwant, name
    assert _hybrid(ctx, s["pairs"], s) == want
    ctx.close()
    index.close()


# ---- `stride fmwalk --hybrid` and `--kmerize` end to end ------------------------------------------------------------------------
def _cli_pairs():
    """the pairs of the hybrid sets with the default options, without those that hold an empty read"""
    default = hy_options(hy_case("merges_as_merge_does")[0])
    pairs = [p for name in HYBRID_SETS for p in hy_case(name)[0]["pairs"] if hy_options(hy_case(name)[0]) == default]
    return [p for p in pairs if p[0] and p[1]]


def _record(rid: str, read: str, seq: str, quals: bool) -> str:
    """SeqRecord::write: FASTQ with the read's own quality string when it has one"""
    return f"@{rid}\n{seq}\n+\n{'I' * len(read)}\n" if quals else f">{rid}\n{seq}\n"


def _kmerized_text(rid: str, read: str, rd: dict, quals: bool) -> str:
    text = _record(rid, read, rd["correct"], quals) if rd["correct"] else ""
    return text + "".join(f">{rid}:{i}\n{s}\n" for i, s in enumerate(rd["kmerized"]))


def _lines(kmerized, merged, failed):
    return [f"Reads are kmerized: {kmerized}", f"Reads are merged : {merged}", f"Reads failed to kmerize or merge: {failed}"]


def expected_hybrid(pairs, quals: bool, repeat: int, c=None, **options):
    """(the merge file, the kmerized file, the three count lines)"""
    c = c or index_case()[1]
    merge_text, km_text, kmerized, merged, failed = "", "", 0, 0, 0
    for i, (r1, r2) in enumerate(pairs):
        if not set(r1 + r2) <= set("ACGT"):
            failed += 2
            continue
        w = plain_merge_and_kmerize(c, r1, r2, repeat, **options)
        if w["walk"]["merged"]:
            merge_text += f">frag{i}\n{w['walk']['seq']}\n"
            merged += 1
            continue
        flags = [rd["kmerize"] for rd in w["reads"]]
        kmerized += sum(flags) if any(flags) else 0
        failed += 2 - sum(flags) if any(flags) else 2
        for j, (r, rd) in enumerate(zip((r1, r2), w["reads"])):
            km_text += _kmerized_text(f"frag{i}/{j + 1}", r, rd, quals)
    return merge_text, km_text, _lines(kmerized, merged, failed)


def expected_kmerize(reads, quals: bool, c=None, k=K, x=X):
    c = c or index_case()[1]
    text, kmerized, failed = "", 0, 0
    for i, r in enumerate(reads):
        rd = plain_kmerize(c, r, k, x) if set(r) <= set("ACGT") else dict(kmerize=0)
        if not rd["kmerize"]:
            failed += 1
            continue
        kmerized += 1
        text += _kmerized_text(f"read{i}", r, rd, quals)
    return text, _lines(kmerized, 0, failed)


def _single_records(reads, quals: bool) -> str:
    return "".join(f"@read{i} extra\n{r}\n+\n{'I' * len(r)}\n" if quals else f">read{i} extra\n{r}\n" for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def hybrid_dir(api, tmp_path_factory):
    """the index reads as reads.fa with their index by `stride index`; the pairs and the single reads as FASTA and as FASTQ"""
    d = tmp_path_factory.mktemp("fmwalk_hybrid")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(index_reads())))
    _run(["index", "-p", "reads", "reads.fa"], d)
    pairs = _cli_pairs()
    reads = [r for name in KMERIZE_SETS for r in km_case(name)[0][0]]
    assert len(pairs) >= 20 and len(reads) >= 15
    for ext, quals in (("fa", False), ("fq", True)):
        (d / f"pairs.{ext}").write_text(_records(pairs, quals))
        (d / f"singles.{ext}").write_text(_single_records(reads, quals))
    return d, pairs, reads


CLI_OPTIONS = ["-k", str(K), "-m", str(M_MIN), "-x", str(X), "-I", str(INSERT)]


@pytest.mark.parametrize("ext", ["fa", "fq"])
def test_stride_fmwalk_hybrid_equals_the_yardstick_s_files(hybrid_dir, ext):
    d, pairs, _ = hybrid_dir
    merge_text, km_text, lines = expected_hybrid(pairs, ext == "fq", 21)
    assert merge_text.count(">") >= 6 and km_text.count(":") >= 2 and "0" not in {l.split(": ")[1] for l in lines}
    r = _run(["fmwalk", "--hybrid", "--repeat-cutoff=21", *CLI_OPTIONS, "-p", "reads", f"pairs.{ext}"], d)
    assert (d / "pairs.merge.fa").read_text() == merge_text and (d / "pairs.kmerized.fa").read_text() == km_text
    assert _count_lines(r.stdout) == lines and "Median kmer frequency" not in r.stdout
    if ext == "fq":
        assert "\n+\n" in km_text
    # -o names the merge file; the kmerized file keeps the input's prefix.  A cutoff of 0 lets no pair walk.
    merge_text, km_text, lines = expected_hybrid(pairs, ext == "fq", 0)
    r = _run(["fmwalk", "--hybrid", "--repeat-cutoff", "0", *CLI_OPTIONS, "--load-on-device", "-p", "reads", "-o", f"zero_{ext}.out", f"pairs.{ext}"], d)
    assert merge_text == "" and km_text.count(":") >= 20 and (d / f"zero_{ext}.out").read_text() == "" and (d / "pairs.kmerized.fa").read_text() == km_text and _count_lines(r.stdout) == lines


@pytest.mark.parametrize("ext", ["fa", "fq"])
def test_stride_fmwalk_kmerize_equals_the_yardstick_s_files(hybrid_dir, ext):
    d, _, reads = hybrid_dir
    text, lines = expected_kmerize(reads, ext == "fq")
    assert text.count(":") >= 50 and lines[2] != "Reads failed to kmerize or merge: 0"
    r = _run(["fmwalk", "--kmerize", *CLI_OPTIONS, "-p", "reads", f"singles.{ext}"], d)
    assert (d / "singles.kmerized.fa").read_text() == text and (d / "singles.origin.fa").read_text() == "" and _count_lines(r.stdout) == lines
    assert "Median kmer frequency" not in r.stdout


def test_stride_fmwalk_hybrid_build_index_other_bases_and_odd_records(hybrid_dir):
    d, pairs, reads = hybrid_dir
    sub = d / "built"
    sub.mkdir()
    own = [p for p in pairs if len(p[0]) == 50 == len(p[1])][:12] * 2
    (d / "own.fa").write_text(_records(own, False))
    c = Counts([r for p in own for r in p])
    merge_text, km_text, lines = expected_hybrid(own, False, 50, c, x=1)
    r = _run(["fmwalk", "--hybrid", "--repeat-cutoff=50", "-k", str(K), "-m", str(M_MIN), "-x", "1", "-I", str(INSERT), "--build-index", "--device=0", "../own.fa"], sub)
    assert (sub / "own.merge.fa").read_text() == merge_text and (sub / "own.kmerized.fa").read_text() == km_text and _count_lines(r.stdout) == lines
    own_reads = [r for p in own[:6] for r in p]
    (d / "own_singles.fa").write_text(_single_records(own_reads, False))
    text, lines = expected_kmerize(own_reads, False, Counts(own_reads), x=1)
    r = _run(["fmwalk", "--kmerize", "-k", str(K), "-x", "1", "--build-index", "../own_singles.fa"], sub)
    assert (sub / "own_singles.kmerized.fa").read_text() == text and _count_lines(r.stdout) == lines
    # a pair and a read that hold N: counted as failed, one warning
    r1, r2 = pairs[0]
    with_n = [pairs[0], (r1[:25] + "N" + r1[26:], r2), pairs[1]]
    (d / "with_n.fa").write_text(_records(with_n, False))
    merge_text, km_text, lines = expected_hybrid(with_n, False, 21)
    r = _run(["fmwalk", "--hybrid", "--repeat-cutoff=21", *CLI_OPTIONS, "-p", "reads", "with_n.fa"], d)
    assert (d / "with_n.merge.fa").read_text() == merge_text and (d / "with_n.kmerized.fa").read_text() == km_text and _count_lines(r.stdout) == lines
    assert r.stderr.count("Warning: pair") == 1 and "frag1" not in merge_text + km_text
    (d / "n_singles.fa").write_text(_single_records([reads[0], "ACGTN" * 6, reads[1]], False))
    text, lines = expected_kmerize([reads[0], "ACGTN" * 6, reads[1]], False)
    r = _run(["fmwalk", "--kmerize", *CLI_OPTIONS, "-p", "reads", "n_singles.fa"], d)
    assert (d / "n_singles.kmerized.fa").read_text() == text and _count_lines(r.stdout) == lines and r.stderr.count("Warning: read") == 1
    # an odd record count: hybrid refuses and leaves no file; kmerize takes every record
    (d / "odd.fa").write_text(_records(pairs[:3], False) + f">last/1\n{pairs[3][0]}\n")
    r = _run(["fmwalk", "--hybrid", "--repeat-cutoff=21", *CLI_OPTIONS, "-p", "reads", "odd.fa"], d, ok=False)
    assert r.returncode == 1 and "FMIndexWalk: odd.fa holds an odd number of records" in r.stderr
    assert not (d / "odd.merge.fa").exists() and not (d / "odd.kmerized.fa").exists()
    (d / "odd_singles.fa").write_text(_single_records(reads[:3], False))
    text, lines = expected_kmerize(reads[:3], False)
    r = _run(["fmwalk", "--kmerize", *CLI_OPTIONS, "-p", "reads", "odd_singles.fa"], d)
    assert (d / "odd_singles.kmerized.fa").read_text() == text and _count_lines(r.stdout) == lines


def test_stride_fmwalk_hybrid_samples_as_the_reference_does(hybrid_dir):
    """without --repeat-cutoff: the Median line's q2 is the quartile of the counts at the rows that an unseeded rand() gives"""
    import re
    import subprocess
    import sys

    d, pairs, _ = hybrid_dir
    reads, c, _, _ = index_case()
    child = ("import ctypes, ctypes.util; libc = ctypes.CDLL(ctypes.util.find_library('c')); libc.rand.restype = ctypes.c_int; "
             f"print(' '.join(str(libc.rand() % {len(reads)}) for _ in range(100000)))")
    rows = [int(v) for v in subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, check=True).stdout.split()]
    per_row = {row: plain_sample_count(c, reads, row, M_MIN) for row in set(rows)}
    q2 = plain_quartile2([per_row[row] for row in rows])
    assert len(rows) == 100000 and q2 > 0
    r = _run(["fmwalk", "--hybrid", *CLI_OPTIONS, "-p", "reads", "pairs.fa"], d)
    m = re.search(r"^Median kmer frequency: (\d+)\t Std: (\S+)\t 95% kmer frequency: (\d+)\t Repeat frequency cutoff: (\d+)$", r.stdout, flags=re.M)
    assert m, r.stdout
    assert int(m.group(1)) == q2 and int(m.group(4)) == int(q2 * 1.3) and float(m.group(2)) > 0
    ordered = sorted(per_row[row] for row in rows)
    assert int(m.group(3)) == next(v for i, v in enumerate(ordered) if (i + 1) / len(ordered) > 0.95 and (i + 1 == len(ordered) or ordered[i + 1] != v))
    merge_text, km_text, lines = expected_hybrid(pairs, False, int(q2 * 1.3))
    assert (d / "pairs.merge.fa").read_text() == merge_text and (d / "pairs.kmerized.fa").read_text() == km_text and _count_lines(r.stdout) == lines


def test_stride_fmwalk_merge_mode_is_as_it_was(hybrid_dir):
    from .test_gpu_fmwalk import OPTIONS, _expected

    d, pairs, _ = hybrid_dir
    text, lines = _expected(pairs)
    r = _run(["fmwalk", *OPTIONS, "-p", "reads", "-o", "merge_mode.out", "pairs.fa"], d)
    assert (d / "merge_mode.out").read_text() == text and _count_lines(r.stdout) == lines and text.count(">") >= 6
    assert "Median kmer frequency" not in r.stdout and not (d / "merge_mode.kmerized.fa").exists()
