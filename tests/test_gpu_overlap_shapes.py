"""lrsc_overlap_exact (fm_overlap.hip, capi_overlap.cpp) and `stride overlap` on the sets of test_overlap_shapes_host: chains of more
than one 64-lane tile, reads of unequal length in one call, reads and m at the limits, a read's output at its boundary and past
it, and one call that overlap_plan cuts into two chunks because of its longest read.  Every comparison is exact, against the
plain restatement of test_overlap_host."""
from __future__ import annotations

import gzip
import subprocess

import numpy as np
import pytest

from .test_overlap_host import STRIDE, reads_input
from .test_overlap_shapes_host import FAN_OVERFLOWS, LRSC_OVERLAP_OVERFLOW, SHAPE_SETS, expected_status, plan_chunk, shape_case, status_dicts

pytestmark = pytest.mark.gpu


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
    """one call, which returns LRSC_OK or raises, with room for every block a read can have -> per read the yardstick's dict and
    the status"""
    return status_dicts(*ctx.overlap_exact(*reads_input(reads), m, block_cap=256 * len(reads)))


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
@pytest.mark.parametrize("name", list(SHAPE_SETS))
def test_the_set_equals_the_yardstick(api, monkeypatch, name, wide):
    from longreadselfcorrect_amd import capi

    _force(monkeypatch, wide)
    c = shape_case(name)
    index, ctx = _context(api, c["reads"])
    assert index.info().block_symbols == (128 if wide else 192)
    got, want = _overlap(ctx, c["reads"], c["m"]), expected_status(name)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i
    if name == "out_cap_overflows":                               # the call is LRSC_OK, the one read says that it overflowed
        assert got[0] == dict(is_substring=0, blocks=[], status=LRSC_OVERLAP_OVERFLOW) and all(g["status"] == 0 and g["blocks"] for g in got[1:]) and len(got) == FAN_OVERFLOWS + 1
    else:
        assert all(g["status"] == 0 for g in got)
    chunk = plan_chunk(max(len(r) for r in c["reads"]), c["m"])
    assert len(c["reads"]) <= chunk and ctx.stats(capi.K_FIND).launches == 2     # one chunk: its collect and its reduce
    ctx.close()
    index.close()


def _two_chunk_order(n_index: int) -> list[int]:
    """800 query reads: the `random` set's 200 four times over, a 2000-base read in the first chunk, one behind read 704, one last"""
    order = list(range(n_index - 3)) * 4
    order[5], order[710], order[799] = n_index - 3, n_index - 2, n_index - 1
    return order


@pytest.mark.parametrize("wide", [False, True], ids=["block32", "block64"])
def test_two_chunks_by_length(api, monkeypatch, wide):
    """overlap_plan's chunk follows the call's longest read: 704 reads with one of 2000 bases.  lrsc_overlap_exact's chunk loop runs
    twice: the second chunk's reads are found at their own offsets, every chunk's pool is put back in read order, and first_block
    goes on across the border (status_dicts asserts that it is contiguous and ascending)."""
    from longreadselfcorrect_amd import capi

    _force(monkeypatch, wide)
    c = shape_case("random_and_the_long_reads")
    want_of = expected_status("random_and_the_long_reads")
    index, ctx = _context(api, c["reads"])
    order = _two_chunk_order(len(c["reads"]))
    chunk = plan_chunk(2000, c["m"])
    assert len(order) == 800 >= 720 and chunk < len(order) and order.index(len(c["reads"]) - 3) < chunk <= order.index(len(c["reads"]) - 2)
    launches = 0
    for queries in (order, [order[i] for i in np.random.default_rng(0x1E10).permutation(len(order))]):
        got = _overlap(ctx, [c["reads"][i] for i in queries], c["m"])
        assert len(got) == len(queries)
        for at, (g, i) in enumerate(zip(got, queries)):
            assert g == want_of[i], (at, i)
        launches += 2 * -(-len(queries) // chunk)
        assert ctx.stats(capi.K_FIND).launches == launches and launches % 4 == 0
    # the same number of reads without a long one: the chunk is the cap again, one collect and one reduce
    short = [c["reads"][i] for i in order if len(c["reads"][i]) == 50]
    assert len(short) == 797 and plan_chunk(50, c["m"]) > len(short)
    got = _overlap(ctx, short, c["m"])
    assert got == [want_of[i] for i in order if len(c["reads"][i]) == 50] and ctx.stats(capi.K_FIND).launches == launches + 2
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


@pytest.mark.parametrize("name", ["monotone_mixed_lengths", "at_the_limits", "at_the_limits_m_2000"])
def test_stride_overlap_writes_the_yardstick_s_files(api, tmp_path, name):
    c = shape_case(name)
    (tmp_path / f"{name}.fa").write_text(_fasta(c))
    _run(["overlap", "-m", str(c["m"]), "--build-index", f"{name}.fa"], tmp_path)
    assert _gz(tmp_path / f"{name}.asqg.gz") == c["asqg"] and _gz(tmp_path / f"{name}-thread0.edges.gz") == c["edges"]
    assert c["edges"].count("ED\t") >= 1


def test_stride_overlap_says_which_read_outgrows_the_workspace(api, tmp_path):
    c = shape_case("out_cap_overflows")
    (tmp_path / "fan.fa").write_text(_fasta(c))
    r = _run(["overlap", "-m", str(c["m"]), "--build-index", "fan.fa"], tmp_path, ok=False)
    assert r.returncode != 0 and "overlap: the overlap blocks of read read0 outgrow the device's workspace" in r.stderr
