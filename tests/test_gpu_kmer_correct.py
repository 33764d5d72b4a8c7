"""lrsc_kmer_correct (fm_kcorrect.hip) and `stride correct -a kmer` against the plain restatement of test_kmer_correct_host.
Every comparison is exact."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from .test_gpu_index_build import STRIDE
from .test_kmer_correct_host import CUTOFF, KC_SETS, index_case, kc_case, kmer_counter, phred_of, plain_kmer_correct

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG = -3


def _force(monkeypatch, wide):
    """LRSC_FORCE_WIDE is read per call: set or unset before each index is made"""
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    else:
        monkeypatch.delenv("LRSC_FORCE_WIDE", raising=False)


def _correct(ctx, reads, quals, k, x, rounds):
    """-> [(corrected, kmer_qc, n_changed, passes) per read], as the yardstick gives them"""
    from oracle.oracle_py import pack_reads

    bases, off = pack_reads(reads)
    corrected, res = ctx.kmer_correct(bases, off, phred_of(quals), k, x, rounds, CUTOFF)
    text = corrected.tobytes().decode()
    return [(text[int(a): int(b)], bool(r["kmer_qc"]), int(r["n_changed"]), int(r["passes"])) for a, b, r in zip(off[:-1], off[1:], res)]


@pytest.mark.parametrize("tables", ["no_kmer_tables", "default_tables"])
@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_every_set_equals_the_yardstick(api, monkeypatch, wide, tables):
    from longreadselfcorrect_amd import capi
    from oracle.oracle_py import pack_reads

    if tables == "no_kmer_tables":
        monkeypatch.setenv("LRSC_KTAB_K", "0")
    else:
        monkeypatch.delenv("LRSC_KTAB_K", raising=False)
    _force(monkeypatch, wide)
    made: dict = {}
    for name in KC_SETS:
        s, want = kc_case(name)
        if s["index"] not in made:
            index = api.index_build(*pack_reads(index_case(s["index"])[0]), 0)
            assert index.info().block_symbols == (128 if wide else 192)
            made[s["index"]] = (index, index.ctx(api.params_default(5, 90), 0))
        ctx = made[s["index"]][1]
        ctx.stats_reset()
        assert _correct(ctx, s["reads"], s["quals"], s["k"], s["x"], s["rounds"]) == want, name
        stats = ctx.stats(capi.K_FIND)
        assert stats.launches == 1, name
        if max(len(r) for r in s["reads"]) > s["k"] > 1:
            assert stats.rank_queries > 0 and stats.rank_queries // 2 <= stats.block_loads <= stats.rank_queries, name
    for index, ctx in made.values():
        ctx.close()
        index.close()


@pytest.fixture(scope="module")
def shuffled():
    """the reads of every FASTA set over the tiling index with k = 21, -x 3, -i 10, shuffled, and what the yardstick makes of them"""
    reads, want = [], []
    for name in KC_SETS:
        s, w = kc_case(name)
        if (s["index"], s["k"], s["x"], s["rounds"], s["quals"]) == ("tiling", 21, 3, 10, None):
            reads += s["reads"]
            want += w
    order = np.random.default_rng(7).permutation(len(reads))
    assert len(reads) >= 25
    return [reads[i] for i in order], [want[i] for i in order]


@pytest.mark.parametrize("size", [1, 7, 10 ** 6], ids=["batches_of_1", "batches_of_7", "one_batch"])
def test_shuffled_reads_whatever_the_batches(api, shuffled, size):
    from longreadselfcorrect_amd import capi
    from oracle.oracle_py import pack_reads

    reads, want = shuffled
    index = api.index_build(*pack_reads(index_case("tiling")[0]), 0)
    ctx = index.ctx(api.params_default(5, 90), 0)
    got = []
    for i in range(0, len(reads), size):
        got += _correct(ctx, reads[i: i + size], None, 21, 3, 10)
    assert got == want
    stats = ctx.stats(capi.K_FIND)
    assert stats.launches == -(-len(reads) // size) > 0 and stats.rank_queries > 0
    ctx.close()
    index.close()


def test_refused_arguments_leave_the_outputs_untouched(api):
    from longreadselfcorrect_amd import capi
    from oracle.oracle_py import pack_reads

    s, want = kc_case("one_error_k21")
    index = api.index_build(*pack_reads(index_case("tiling")[0]), 0)
    ctx = index.ctx(api.params_default(5, 90), 0)
    good = s["reads"][:2]

    def call(reads, params, n_reads=None):
        bases, off = pack_reads(reads)
        corrected = np.full(max(bases.size, 1), 0x5A, dtype=np.uint8)
        out = np.full(max(off.size - 1, 1) * 4, 0x5EED, dtype=np.uint32)
        p = np.array(params, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        st = api.lib.lrsc_kmer_correct(ctx.h, ptr(bases), ptr(off), off.size - 1 if n_reads is None else n_reads, None, ptr(p), ptr(corrected), ptr(out))
        return st, corrected, out

    for reads, params in ((good, (0, 3, 10, 20)), (good, (-5, 3, 10, 20)), (good, (21, 0, 10, 20)), (good, (21, 3, 0, 20)), (good, (21, 3, -1, 20)),
                          ([good[0], "ACGTNACGT" * 4, good[1]], (21, 3, 10, 20)), ([good[0], "", good[1]], (21, 3, 10, 20))):
        st, corrected, out = call(reads, params)
        assert st == LRSC_ERR_ARG, (reads[1][:10], params, st)
        assert (corrected == 0x5A).all() and (out == 0x5EED).all()
    st, corrected, out = call(good, (21, 3, 10, 20), n_reads=0)          # a valid call that does nothing
    assert st == 0 and (corrected == 0x5A).all() and (out == 0x5EED).all()
    assert ctx.stats(capi.K_FIND).launches == 0
    assert _correct(ctx, s["reads"], None, 21, 3, 10) == want, "after the refused calls"
    ctx.close()
    index.close()


# ---- `stride correct -a kmer` end to end ----------------------------------------------------------------------------------
def _run(args, cwd, ok=True):
    r = subprocess.run([str(STRIDE)] + args, cwd=cwd, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _count_lines(stdout):
    return [l for l in stdout.split("\n") if l.startswith("Reads ")]


@pytest.fixture(scope="module")
def correct_dir(api, tmp_path_factory):
    """the tiling reads, every fifth with one or two errors, some with more than -i 10 allows, one shorter than k; as FASTA and, with
    qualities, as FASTQ; their own index by `stride index`; what the yardstick makes of both files with k = 21"""
    from .test_kmer_correct_host import _sub, count_lines, fastx

    d = tmp_path_factory.mktemp("correct")
    rng = np.random.default_rng(0xEC)
    reads = list(index_case("tiling")[0])
    for i in range(0, len(reads), 5):
        reads[i] = _sub(reads[i], *rng.choice(np.arange(2, 98, 5), size=1 + i // 5 % 2, replace=False).tolist())
    for i in (101, 333):
        reads[i] = _sub(reads[i], *range(30, 95, 5))
    reads[200] = reads[200][:15]
    quals = ["".join(rng.choice(list("I5#4"), size=len(r), p=[0.7, 0.1, 0.1, 0.1])) for r in reads]
    count = kmer_counter(reads, 21)
    records = {}
    for ext, qs in (("fa", [""] * len(reads)), ("fq", quals)):
        records[ext] = [(f"r{i}", r, q) + plain_kmer_correct(count, r, q or None, 21, 3, 10)[:2] for i, (r, q) in enumerate(zip(reads, qs))]
        (d / f"reads.{ext}").write_text(fastx(records[ext], corrected=False))
        failed = sum(1 for r in records[ext] if not r[4])
        changed = sum(1 for r in records[ext] if r[4] and r[1] != r[3])
        assert 3 <= failed <= 40 and changed >= 100, (ext, failed, changed)
    assert [r[3:] for r in records["fa"]] != [r[3:] for r in records["fq"]], "the qualities change what is corrected"
    _run(["index", "-p", "reads", "reads.fa"], d)
    return d, records, fastx, count_lines


@pytest.mark.parametrize("ext", ["fa", "fq"])
def test_stride_correct_equals_the_yardstick_s_records(correct_dir, ext):
    d, records, fastx, count_lines = correct_dir
    r = _run(["correct", "-a", "kmer", "-k", "21", "-p", "reads", "-o", f"plain_{ext}.out", f"reads.{ext}"], d)
    assert (d / f"plain_{ext}.out").read_text() == fastx(records[ext])
    assert _count_lines(r.stdout) == count_lines(records[ext])
    assert not (d / "reads.discard.fa").exists()


@pytest.mark.parametrize("ext", ["fa", "fq"])
def test_stride_correct_discard_and_build_index(correct_dir, ext):
    d, records, fastx, count_lines = correct_dir
    sub = d / f"discard_{ext}"
    sub.mkdir()
    r = _run(["correct", "-a", "kmer", "-k", "21", "--discard", "--build-index", "--device=0", f"../reads.{ext}"], sub)
    assert (sub / "reads.ec.fa").read_text() == fastx(records[ext], lambda qc: qc)           # the default name, beside the working directory
    assert (sub / "reads.discard.fa").read_text() == fastx(records[ext], lambda qc: not qc)
    assert _count_lines(r.stdout) == count_lines(records[ext])
    r = _run(["correct", "-a", "kmer", "-k", "21", "--discard", "-p", "../reads", "-o", "with_p.out", f"../reads.{ext}"], sub)
    assert (sub / "with_p.out").read_text() == fastx(records[ext], lambda qc: qc)
    assert _count_lines(r.stdout) == count_lines(records[ext])


def test_stride_correct_metrics_file(correct_dir):
    from .test_kmer_correct_host import plain_metrics

    d, records, _, count_lines = correct_dir
    r = _run(["correct", "-a", "kmer", "-k", "21", "-p", "reads", "-o", "m.out", "--metrics=m.txt", "reads.fq"], d)
    want, summary = plain_metrics(records["fq"])
    assert (d / "m.txt").read_text() == want
    lines = r.stdout.strip().split("\n")
    assert lines[-5:] == summary + count_lines(records["fq"])


def test_stride_correct_other_bases_and_bad_qualities(correct_dir):
    d, records, fastx, count_lines = correct_dir
    some = records["fa"][:12]
    with_n = some[:4] + [("n1", some[4][1][:50] + "N" + some[4][1][51:], "", None, False)] + some[5:9] + [("n2", "ACGTNNNNacgt", "", None, False)] + some[9:]
    (d / "with_n.fa").write_text(fastx(with_n, corrected=False))
    want = [rec if rec[3] is not None else rec[:3] + (rec[1].upper(), False) for rec in with_n]
    r = _run(["correct", "-a", "kmer", "-k", "21", "-p", "reads", "--discard", "with_n.fa"], d)
    assert (d / "with_n.ec.fa").read_text() == fastx(want, lambda qc: qc)
    assert (d / "with_n.discard.fa").read_text() == fastx(want, lambda qc: not qc) and ">n1\n" in (d / "with_n.discard.fa").read_text()
    assert _count_lines(r.stdout) == count_lines(want)
    assert r.stderr.count("Warning: read") == 1 and "Warning: read n1 holds a base other than A, C, G, T" in r.stderr
    rid, seq = some[0][0], some[0][1]
    for name, qual in (("short", "I" * (len(seq) - 1)), ("low", "I" * 10 + " " + "I" * (len(seq) - 11))):
        (d / f"{name}.fq").write_text(f"@{some[1][0]}\n{some[1][1]}\n+\n{'I' * len(some[1][1])}\n@{rid}\n{seq}\n+\n{qual}\n")
        r = _run(["correct", "-a", "kmer", "-k", "21", "-p", "reads", f"{name}.fq"], d, ok=False)
        assert r.returncode == 1 and f"correct: read {rid} of {name}.fq has a quality string" in r.stderr
