"""lrsc_fmmerge (fm_fmmerge.hip, capi_fmmerge.cpp) and `stride fm-merge` on the sets of test_overlap_shapes_host: reads of 40 to 400
bases in one call, whose sequences are the genome's pieces by construction; long chains that end in a 2000-base read, which
overlap_plan cuts into two chunks below its cap; the boundary of a read's overlap output.  Every comparison is exact."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from .test_fmmerge_host import launches, merged_dicts, plain_fmmerge
from .test_overlap_host import M, STRIDE, reads_input
from .test_overlap_shapes_host import FAN_FITS, MERGE_SETS, check_merged, merge_case, plan_chunk, shape_case

pytestmark = pytest.mark.gpu

LRSC_ERR_LIMIT = -8


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


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_every_set_equals_the_yardstick_and_the_construction(api, monkeypatch, wide):
    from longreadselfcorrect_amd import capi

    _force(monkeypatch, wide)
    for name in MERGE_SETS:
        c = merge_case(name)
        index, ctx = _context(api, c["reads"])
        assert index.info().block_symbols == (128 if wide else 192)
        check_merged(c, merged_dicts(*ctx.fmmerge(*reads_input(c["reads"]), c["m"])))
        n, chunk = len(c["reads"]), plan_chunk(max(len(r) for r in c["reads"]), c["m"])
        assert ctx.stats(capi.K_FIND).launches == launches(n, chunk), name
        if name == "two_chunks_by_length":
            assert chunk < n and launches(n, chunk) == 3 * 2 + 2 * 11 + 9 == launches(n) + 3
        else:
            assert launches(n, chunk) == launches(n)
        ctx.close()
        index.close()


def test_the_boundary_of_a_read_s_overlap_output(api):
    """256 final blocks of read 0 are taken: it has 254 blocks on one end, no link, and every read is a sequence of its own; with
    257 the read's overlap status is the overflow and the call is refused for it, after the three launches of the one chunk"""
    from longreadselfcorrect_amd import capi

    fits = shape_case("out_cap_fits")
    index, ctx = _context(api, fits["reads"])
    got, want = merged_dicts(*ctx.fmmerge(*reads_input(fits["reads"]), M)), plain_fmmerge(fits)
    assert got == want and [s["n_reads"] for s in got["seqs"]] == [1] * (FAN_FITS + 1)
    ctx.close()
    index.close()
    over = shape_case("out_cap_overflows")
    index, ctx = _context(api, over["reads"])
    bases, off = reads_input(over["reads"])
    n = len(over["reads"])
    per_read, seqs, out = np.full(n * 4, 0x5EED, dtype=np.uint32), np.full(n * 8, 0x5EED, dtype=np.uint32), np.full(bases.size, 0x5A, dtype=np.uint8)
    counts, used = np.full(1, 0x7E57, dtype=np.uint32), np.full(1, 0x7E57, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = api.lib.lrsc_fmmerge(ctx.h, ptr(bases), ptr(off), n, M, ptr(per_read), ptr(seqs), ptr(counts), ptr(out), out.size, ptr(used))
    message = api.lib.lrsc_last_error().decode()
    assert st == LRSC_ERR_LIMIT and "outgrow the kernel's workspace" in message and "read 0 " in message
    assert (per_read == 0x5EED).all() and (seqs == 0x5EED).all() and (out == 0x5A).all() and counts[0] == 0x7E57 and used[0] == 0x7E57
    assert ctx.stats(capi.K_FIND).launches == 3
    ctx.close()
    index.close()


def test_stride_fm_merge_writes_the_pieces_of_the_genome(api, tmp_path):
    c = merge_case("monotone_mixed_lengths_with_holes")
    (tmp_path / "mixed.fa").write_text("".join(f">{n} extra words\n{r}\n" for n, r in zip(c["names"], c["reads"])))
    r = subprocess.run([str(STRIDE), "fm-merge", "-m", str(c["m"]), "--build-index", "-o", "pieces.fa", "mixed.fa"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert (tmp_path / "pieces.fa").read_text() == c["merged"]["fasta"] == "".join(f">merged-{i}\n{w['bases']}\n" for i, w in enumerate(c["want"]))
    assert "Merged %d reads into 3 sequences" % len(c["reads"]) in r.stdout
