"""lrsc_fmwalk_validate (fm_validate.hip) and `stride fmwalk --validate` against the plain restatement of
test_fmwalk_validate_host.  Every comparison is exact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from .test_fmwalk_host import GENOME, K, M_MIN, X, Counts, index_case, index_reads
from .test_fmwalk_hybrid_host import piece_slots, reads_input
from .test_fmwalk_validate_host import DEFAULT_SETS, ENTRY_SETS, NINE_TENTHS, VALIDATE_DTYPE, _sub, default_stride, plain_validate, summary_lines, validate_dicts, \
    vd_case, written_files
from .test_gpu_fmwalk import _count_lines, _run
from .test_index_filter_host import revcomp
from .test_gpu_fmwalk_hybrid import _context, _force

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG, LRSC_ERR_UNSUPPORTED = -3, -7
MAX_INSERT = 2000                                                 # LRSC_FMWALK_MAX_INSERT


def _validate(ctx, reads, s, stride=None) -> list[dict]:
    bases, off = reads_input(reads)
    merged, res, pieces, slots = ctx.fmwalk_validate(bases, off, s["k"], s["x"], s["m"], s["max_overlap"], s["leaves"], stride)
    assert merged.shape[1] == (stride or default_stride(reads)) and slots.tolist() == piece_slots(reads, s["k"]).tolist()
    for q, row in zip(res, merged):                               # a row is untouched beyond the sequence
        assert (row[int(q["length"]) if q["merged"] else 0:] == 0).all()
    return validate_dicts(res, [row.tobytes().decode("latin-1") for row in merged], pieces[: int(slots[-1])], slots, reads, 0)


def launches(reads, want, m) -> int:
    """one for the walks when a read is longer than m, one more when a read is split"""
    return (1 if any(len(r) > m for r in reads) else 0) + (1 if any(w["read"]["pieces"] for w in want) else 0)


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_every_set_equals_the_yardstick(api, monkeypatch, wide):
    from longreadselfcorrect_amd import capi

    assert capi.FMWALK_VALIDATE_DTYPE == VALIDATE_DTYPE
    _force(monkeypatch, wide)
    index, ctx = _context(api)
    assert index.info().block_symbols == (128 if wide else 192)
    seen = set()
    for name in ENTRY_SETS:
        s, want, _ = vd_case(name)
        ctx.stats_reset()
        got = _validate(ctx, s["reads"], s)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, i)
        stats = ctx.stats(capi.K_FIND)
        assert len(got) == len(want) and stats.launches == launches(s["reads"], want, s["m"]), name
        seen.add(stats.launches)
        if stats.launches:
            assert stats.rank_queries > 0 and stats.rank_queries // 2 <= stats.block_loads <= stats.rank_queries, name
    assert seen == {0, 1, 2}
    ctx.close()
    index.close()


@pytest.fixture(scope="module")
def shuffled():
    """the reads of every set with the default options, shuffled, and what the yardstick makes of them"""
    reads = [r for name in DEFAULT_SETS for r in vd_case(name)[0]["reads"]]
    want = [w for name in DEFAULT_SETS for w in vd_case(name)[1]]
    order = np.random.default_rng(14).permutation(len(reads))
    assert len(reads) >= 25
    return [reads[i] for i in order], [want[i] for i in order], vd_case("both_walks_agree")[0]


@pytest.mark.parametrize("size", [1, 7, 10 ** 6], ids=["batches_of_1", "batches_of_7", "one_batch"])
def test_shuffled_reads_whatever_the_batches(api, shuffled, size):
    reads, want, options = shuffled
    index, ctx = _context(api)
    got = []
    for i in range(0, len(reads), size):
        got += _validate(ctx, reads[i: i + size], options)
    assert got == want
    # a stride above the least one: the rows are as far apart, and as untouched
    assert _validate(ctx, reads, options, stride=default_stride(reads) + 37) == want
    ctx.close()
    index.close()


def test_refused_arguments_leave_the_outputs_untouched(api):
    from longreadselfcorrect_amd import capi

    s, want, _ = vd_case("bad_first_end_splits")
    index, ctx = _context(api)
    good = s["reads"]
    ok = (K, X, M_MIN, -1, 0, 32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def validate(reads, params, stride=None, n_reads=None, slots=None):
        bases, off = reads_input(reads)
        stride = default_stride(reads) if stride is None else stride
        merged = np.full(len(reads) * max(stride, 1), 0x5A, dtype=np.uint8)
        out = np.full(len(reads) * 20, 0x5EED, dtype=np.uint32)
        need = int(piece_slots(reads, max(params[0], 1))[-1])
        pieces = np.full(3 * max(need, 1), 0x5EED, dtype=np.uint32)
        p = np.array(params, dtype=np.int32)
        st = api.lib.lrsc_fmwalk_validate(ctx.h, ptr(bases), ptr(off), len(reads) if n_reads is None else n_reads, ptr(p), ptr(merged), stride, ptr(out), ptr(pieces),
                                          need if slots is None else slots)
        return st, bool((merged == 0x5A).all() and (out == 0x5EED).all() and (pieces == 0x5EED).all())

    replaced = lambda i, v: tuple(v if j == i else x for j, x in enumerate(ok))
    refused = [(good, replaced(i, v), None, None, LRSC_ERR_ARG) for i in (0, 1, 2, 3, 5) for v in (0, -2)]
    refused += [(good, replaced(2, 1), None, None, LRSC_ERR_ARG), (good, ok, default_stride(good) - 1, None, LRSC_ERR_ARG),
                (good, ok, None, int(piece_slots(good, K)[-1]) - 1, LRSC_ERR_ARG), (good + ["ACGTNACGT" * 4], ok, None, None, LRSC_ERR_ARG),
                ([good[0], "", good[1]], ok, None, None, LRSC_ERR_ARG),
                (good, replaced(5, 65), None, None, LRSC_ERR_UNSUPPORTED), (good, replaced(2, 256), None, None, LRSC_ERR_UNSUPPORTED),
                (good, replaced(0, 256), None, None, LRSC_ERR_UNSUPPORTED)]
    for reads, params, stride, slots, status in refused:
        st, untouched = validate(reads, params, stride, slots=slots)
        assert st == status and untouched, (params, stride, slots, st)
    # max_insert is ignored, whatever it holds
    for v in (-5, 0, 10 ** 6):
        st, untouched = validate(good, replaced(4, v))
        assert st == 0 and not untouched
    # the longest read: a walk's string has at most (size_t)(n * 1.1) + 1 bases, which LRSC_FMWALK_MAX_INSERT bounds
    assert int(1818 * 1.1) + 1 == MAX_INSERT and int(1819 * 1.1) + 1 == MAX_INSERT + 1
    long_read = (GENOME + GENOME)[:1819]
    st, untouched = validate([good[0], long_read], ok)
    assert st == LRSC_ERR_UNSUPPORTED and untouched and "read 1 has 1819 bases" in api.lib.lrsc_last_error().decode()
    ctx.stats_reset()
    st, untouched = validate([good[0], long_read[:1818]], ok)
    assert st == 0 and not untouched
    # valid calls that do nothing, or launch nothing
    ctx.stats_reset()
    assert validate(good, ok, n_reads=0) == (0, True) and ctx.stats(capi.K_FIND).launches == 0
    st, untouched = validate(["ACGT", NINE_TENTHS], ok)
    assert st == 0 and not untouched and ctx.stats(capi.K_FIND).launches == 0
    assert _validate(ctx, good, s) == want, "after the refused calls"
    ctx.close()
    index.close()


def test_the_longest_read_the_entry_takes(api):
    """1818 bases: the depth limit is 1999 and the workspace the largest there is.  The read is most of the genome and a stretch of its
    other strand: neither walk meets its terminal and both run to the depth limit, the deepest tree there is; its record equals the
    yardstick's."""
    index, ctx = _context(api)
    s = vd_case("both_walks_agree")[0]
    read = GENOME[100:1480] + revcomp(GENOME[100:538])
    want = plain_validate(index_case()[1], read)
    assert int(len(read) * 1.1) == MAX_INSERT - 1 and not want["merged"] and want["read"]["kmerize"] and want["status"] == [-2, -2]
    assert len(read) == 1818 and want["max_used_leaves"][0] >= 2 and len(want["read"]["pieces"]) > 1
    assert _validate(ctx, [read, s["reads"][0]], s) == [want, vd_case("both_walks_agree")[1][0]]
    ctx.close()
    index.close()


def test_the_other_algorithms_are_as_they_were(api):
    """merge and hybrid calls between two validate calls on the same context, which share its buffers"""
    from .test_fmwalk_host import fw_case
    from .test_fmwalk_hybrid_host import hy_case, km_case
    from .test_gpu_fmwalk import _merge
    from .test_gpu_fmwalk_hybrid import _hybrid, _kmerize

    index, ctx = _context(api)
    s, want, _ = vd_case("split_with_restart")
    assert _validate(ctx, s["reads"], s) == want
    fs, fwant, _ = fw_case("overlap_shortcut")
    assert _merge(ctx, fs["pairs"], fs) == fwant
    hs, hwant = hy_case("substitutions")
    assert _hybrid(ctx, hs["pairs"], hs) == hwant
    (reads, k, x), kwant = km_case("substitutions")
    assert _kmerize(ctx, reads, k, x) == kwant
    assert _validate(ctx, s["reads"], s) == want
    ctx.close()
    index.close()


# ---- `stride fmwalk --validate` end to end --------------------------------------------------------------------------------------
def _single_records(reads, quals: bool) -> str:
    return "".join(f"@read{i} extra\n{r}\n+\n{'I' * len(r)}\n" if quals else f">read{i} extra\n{r}\n" for i, r in enumerate(reads))


@pytest.mark.parametrize("ext", ["fa", "fq"])
def test_stride_fmwalk_validate_build_index_equals_the_yardstick_s_files(api, tmp_path, ext):
    """the reads are their own index: a third of the index reads of the sets, some of them with a wrong base, and three short reads"""
    own = index_reads()[::3]
    own = [_sub(r, 25) if i % 10 == 3 else _sub(r, 3) if i % 10 == 7 else r for i, r in enumerate(own)] + [NINE_TENTHS, "A" * 20, own[0][:M_MIN]]
    c = Counts(own)
    quals = ext == "fq"
    (tmp_path / f"own.{ext}").write_text(_single_records(own, quals))
    wants = [plain_validate(c, r) for r in own]
    records = [(f"read{i}", r, w) for i, (r, w) in enumerate(zip(own, wants))]
    origin, kmerized, low = written_files(records, quals)
    assert origin.count(">") >= 100 and kmerized.count(":") >= 20 and low.count("read") >= 1
    r = _run(["fmwalk", "--validate", "-k", str(K), "-m", str(M_MIN), "-x", str(X), "--build-index", f"own.{ext}"], tmp_path)
    assert (tmp_path / "own.origin.fa").read_text() == origin and (tmp_path / "own.kmerized.fa").read_text() == kmerized
    assert (tmp_path / "LowComplexityReads.fa").read_text() == low
    assert _count_lines(r.stdout) == summary_lines([w for _, _, w in records])
    if quals:
        assert "\n+\n" in kmerized and "\n+\n" in low and "+" not in origin
        return
    # -o names the file of the merged reads; the other two keep their names
    r = _run(["fmwalk", "--validate", "-k", str(K), "-m", str(M_MIN), "-x", str(X), "--build-index", "-o", "named.out", "own.fa"], tmp_path)
    assert (tmp_path / "named.out").read_text() == origin and (tmp_path / "own.kmerized.fa").read_text() == kmerized
    # a read above the limit ends the run with one line that names it
    (tmp_path / "long.fa").write_text(_single_records(own[:3] + [(GENOME + GENOME)[:1819]], False))
    r = _run(["fmwalk", "--validate", "-k", str(K), "-m", str(M_MIN), "--build-index", "long.fa"], tmp_path, ok=False)
    lines = [l for l in r.stderr.split("\n") if l.strip()]
    assert r.returncode == 1 and len(lines) == 1 and lines[0].startswith("FMIndexWalk: read read3 has 1819 bases")
