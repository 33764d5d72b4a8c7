"""lrsc_overlap_exact (fm_overlap.hip) and `stride overlap` against the plain restatement of test_overlap_host.  Every comparison
is exact."""
from __future__ import annotations

import ctypes as C
import gzip
import subprocess

import numpy as np
import pytest

from .test_overlap_host import NAMED, OV_SETS, OVERLAP_BLOCK_DTYPE, OVERLAP_READ_DTYPE, STRIDE, ov_case, plain_overlap_exact, plain_overlap_text, reads_input, result_dicts

pytestmark = pytest.mark.gpu

LRSC_ERR_ARG, LRSC_ERR_CAPACITY, LRSC_ERR_UNSUPPORTED = -3, -6, -7


def _force(monkeypatch, wide):
    """LRSC_FORCE_WIDE is read per call: set or unset before each index is made"""
    if wide:
        monkeypatch.setenv("LRSC_FORCE_WIDE", "1")
    else:
        monkeypatch.delenv("LRSC_FORCE_WIDE", raising=False)


def _context(api, reads):
    from oracle.oracle_py import pack_reads

    index = api.index_build(*pack_reads(reads), 0)
    return index, index.ctx(api.params_default(5, 90), 0)


def _overlap(ctx, reads, m) -> list[dict]:
    """-> what the yardstick gives, per read; one call, with room for every block a read can have"""
    return result_dicts(*ctx.overlap_exact(*reads_input(reads), m, block_cap=256 * len(reads)))


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_every_set_equals_the_yardstick(api, monkeypatch, wide):
    from longreadselfcorrect_amd import capi

    assert capi.OVERLAP_READ_DTYPE == OVERLAP_READ_DTYPE and capi.OVERLAP_BLOCK_DTYPE == OVERLAP_BLOCK_DTYPE
    _force(monkeypatch, wide)
    for name in OV_SETS:
        c = ov_case(name)
        index, ctx = _context(api, c["reads"])
        assert index.info().block_symbols == (128 if wide else 192)
        got = _overlap(ctx, c["reads"], c["m"])
        assert len(got) == len(c["results"])
        for i, (g, w) in enumerate(zip(got, c["results"])):
            assert g == w, (name, i)
        stats = ctx.stats(capi.K_FIND)
        # the collect and the reduce of the one workspace chunk
        assert stats.launches == 2, name
        assert stats.rank_queries > 0 and stats.rank_queries // 2 <= stats.block_loads <= stats.rank_queries, name
        ctx.close()
        index.close()


@pytest.mark.parametrize("size", [1, 7, 10 ** 6], ids=["batches_of_1", "batches_of_7", "one_batch"])
def test_shuffled_reads_whatever_the_batches(api, size):
    from longreadselfcorrect_amd import capi

    c = ov_case("random")
    index, ctx = _context(api, c["reads"])
    order = np.random.default_rng(12).permutation(len(c["reads"]))
    if size == 1:                                                 # a call a read: a quarter of them says as much
        order = order[::4]
    reads, want = [c["reads"][i] for i in order], [c["results"][i] for i in order]
    got, calls = [], 0
    for i in range(0, len(reads), size):
        got += _overlap(ctx, reads[i: i + size], c["m"])
        calls += 1
    assert got == want and ctx.stats(capi.K_FIND).launches == 2 * calls
    ctx.close()
    index.close()


def _raw(api, ctx, reads, m, cap, n_reads=None):
    bases, off = reads_input(reads)
    per_read = np.full(len(reads) * 6, 0x5EED, dtype=np.uint32)
    blocks = np.full(max(cap, 1) * 24, 0x5A, dtype=np.uint8)
    used = np.full(1, 0x7E57, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = api.lib.lrsc_overlap_exact(ctx.h, ptr(bases), ptr(off), len(reads) if n_reads is None else n_reads, m, ptr(per_read), ptr(blocks), cap, ptr(used))
    return st, per_read, blocks, int(used[0])


def test_refused_arguments_leave_the_outputs_untouched(api):
    from longreadselfcorrect_amd import capi

    c = ov_case("unique_path")
    index, ctx = _context(api, c["reads"])
    good = c["reads"][:4]
    refused = [(good, 1, LRSC_ERR_ARG), (good, 0, LRSC_ERR_ARG), (good, -5, LRSC_ERR_ARG), (good[:2] + ["ACGTNACGT" * 4], 20, LRSC_ERR_ARG), (good[:2] + [""] + good[2:], 20, LRSC_ERR_ARG),
               (good, 2001, LRSC_ERR_UNSUPPORTED), (good + ["ACGT" * 501], 20, LRSC_ERR_UNSUPPORTED)]
    for reads, m, status in refused:
        st, per_read, blocks, used = _raw(api, ctx, reads, m, 64)
        assert st == status, (m, st)
        assert (per_read == 0x5EED).all() and (blocks == 0x5A).all() and used == 0x7E57
    assert ctx.stats(capi.K_FIND).launches == 0
    st, per_read, blocks, used = _raw(api, ctx, good, 20, 64, n_reads=0)     # a valid call that launches nothing
    assert st == 0 and (per_read == 0x5EED).all() and (blocks == 0x5A).all() and used == 0 and ctx.stats(capi.K_FIND).launches == 0
    assert _overlap(ctx, c["reads"], c["m"]) == c["results"], "after the refused calls"
    ctx.close()
    index.close()


def test_a_block_cap_that_is_too_small_says_what_is_needed(api):
    c = ov_case("unique_path")
    index, ctx = _context(api, c["reads"])
    need = sum(len(r["blocks"]) for r in c["results"])
    assert need > 26
    for cap in (0, need - 1):
        st, per_read, blocks, used = _raw(api, ctx, c["reads"], c["m"], cap)
        assert st == LRSC_ERR_CAPACITY and used == need and (per_read == 0x5EED).all() and (blocks == 0x5A).all()
    st, per_read, blocks, used = _raw(api, ctx, c["reads"], c["m"], need)
    assert st == 0 and used == need
    got = result_dicts(per_read.view(OVERLAP_READ_DTYPE), blocks.view(OVERLAP_BLOCK_DTYPE)[:need])
    assert got == c["results"]
    per_read, blocks = ctx.overlap_exact(*reads_input(c["reads"]), c["m"], block_cap=None)       # the binding asks again by itself
    assert result_dicts(per_read, blocks) == c["results"]
    ctx.close()
    index.close()


# ---- `stride overlap` end to end ------------------------------------------------------------------------------------------------
def _run(args, cwd, ok=True):
    r = subprocess.run([str(STRIDE)] + args, cwd=cwd, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _gz(path) -> str:
    return gzip.decompress(path.read_bytes()).decode()


def _fasta(c) -> str:
    return "".join(f">{n} extra words\n{r}\n" for n, r in zip(c["names"], c["reads"]))


BANNER = "StriDe overlap computation using min overlap: {m}\nError Rate: -1\nMax Indel: 0\nTransitive reduction: 1\nAlgorithm: LSSF\n"


@pytest.mark.parametrize("name", NAMED)
def test_stride_overlap_writes_the_yardstick_s_files(api, tmp_path, name):
    """after `stride index` with -p, with --build-index, and with --load-on-device: the same two files, byte for byte"""
    c = ov_case(name)
    (tmp_path / f"{name}.fa").write_text(_fasta(c))
    _run(["index", "-p", "idx", f"{name}.fa"], tmp_path)
    m = ["-m", str(c["m"])]
    r = _run(["overlap", *m, "-p", "idx", f"{name}.fa"], tmp_path)
    assert BANNER.format(m=c["m"]) in r.stdout
    assert _gz(tmp_path / f"{name}.asqg.gz") == c["asqg"] and _gz(tmp_path / f"{name}-thread0.edges.gz") == c["edges"]
    for extra in (["--build-index", "-x", "-t", "4"], ["--load-on-device", "-p", "idx", "--exact", "--device=0", "-v"]):
        (tmp_path / f"{name}-thread0.edges.gz").unlink()
        _run(["overlap", *m, *extra, "-o", "named.asqg.gz", f"{name}.fa"], tmp_path)
        assert _gz(tmp_path / "named.asqg.gz") == c["asqg"] and _gz(tmp_path / f"{name}-thread0.edges.gz") == c["edges"]
    if name == "substring_read":
        assert c["asqg"].count("SS:i:1") == 1


def test_stride_overlap_other_bases_and_another_index(api, tmp_path):
    c = ov_case("unique_path")
    (tmp_path / "clean.fa").write_text(_fasta(c))
    _run(["index", "-p", "clean", "clean.fa"], tmp_path)
    reads = list(c["reads"])
    reads[7] = reads[7][:25] + "N" + reads[7][26:]
    reads[9] = "N" + reads[9][1:]
    (tmp_path / "with_n.fa").write_text("".join(f">{n}\n{r}\n" for n, r in zip(c["names"], reads)))
    results = [plain_overlap_exact(c["ix"], r, c["m"]) if set(r) <= set("ACGT") else dict(is_substring=0, blocks=[]) for r in reads]
    asqg, edges = plain_overlap_text(c["names"], reads, c["m"], "with_n.fa", results, c["ix"])
    r = _run(["overlap", "-m", str(c["m"]), "-p", "clean", "with_n.fa"], tmp_path)
    assert _gz(tmp_path / "with_n.asqg.gz") == asqg and _gz(tmp_path / "with_n-thread0.edges.gz") == edges
    assert r.stderr.count("Warning: read") == 1 and "read7 " in r.stderr and edges.count("ED\t") > 10 and "ED\tread7 " not in edges and "ED\tread9 " not in edges
    # an index of another number of reads
    (tmp_path / "fewer.fa").write_text("".join(f">{n}\n{r}\n" for n, r in list(zip(c["names"], c["reads"]))[:20]))
    r = _run(["overlap", "-m", str(c["m"]), "-p", "clean", "fewer.fa"], tmp_path, ok=False)
    assert r.returncode == 1 and "overlap: fewer.fa holds 20 reads, the index 26" in r.stderr
