"""The device RL encoder (csrc/fm_rle.h, fm_rle.hip) checked without a GPU.

1. The per-lane functions that the kernels call, compiled for the CPU (tests/host_tools/rle_driver.cpp) and run in the kernels'
   order, against the sequential rule of lrsc_build_bwt on the same codes, byte for byte: with the kernels' tile and with a tile
   of one Block32, so that the paths over several tiles run on short inputs as well.
2. unpack_block gives back what pack_block was given, both layouts, every n_valid, the '$' patterns of test_index_pack_host.py.
3. lrsc_index_units / lrsc_index_write are declared and exported, the ABI version is still 2, the binding has the methods.
4. The encoder's kernels compile for gfx950 without scratch or spills.
5. `stride pbcorrect --save-index` without --build-index is an argument error.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO

LLVM = Path("/opt/rocm/lib/llvm/bin")
HDR = (REPO / "longreadselfcorrect_amd/csrc/fm_rle.h").read_text()
TILES = {"kernel_tile": 0, "one_block_tile": 1}                  # the driver's <small> argument
RUNS = [30, 31, 32, 61, 62, 63, 93]


def tile_size(small: int) -> int:
    """the kernels' tile as fm_rle.h names it, or the driver's small one (12 lanes x 16 symbols)"""
    if small:
        return 192
    c = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (kRleLanes|kRleChunks) = (\d+);", HDR)}
    assert re.search(r"kRleTile = kRleLanes \* kRleChunks \* 16;", HDR)
    t = c["kRleLanes"] * c["kRleChunks"] * 16
    assert t % 192 == 0 and t % 128 == 0
    return t


def sizes(t: int) -> list[int]:
    m = -(-t // 31) * 31                                          # the multiple of 31 next to the tile's end
    s = {1, t - 1, t, t + 1, 3 * t + 7, 30, 31, 32, 61, 62, 63, 92, 93, 94, m - 31 - 1, m - 31, m - 31 + 1, m - 1, m, m + 1,
         2 * 31 * 7 - 1, 2 * 31 * 7, 2 * 31 * 7 + 1}
    return sorted(x for x in s if x >= 1)


def _runs_of(n: int, lengths, symbols) -> np.ndarray:
    out, i = [], 0
    while sum(len(x) for x in out) < n:
        out.append(np.full(lengths[i % len(lengths)], symbols[i % len(symbols)], dtype=np.uint8))
        i += 1
    return np.concatenate(out)[:n]


def _put(c: np.ndarray, start: int, length: int, sym: int):
    """a run of `sym` at [start, start + length), clipped; its neighbours made different so that it is exactly that run"""
    n = c.size
    a, b = max(start, 0), min(start + length, n)
    if a >= b:
        return
    c[a:b] = sym
    other = 1 + sym % 4
    if a > 0:
        c[a - 1] = other
    if b < n:
        c[b] = other


def patterns(n: int, t: int, seed: int) -> dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    rnd = lambda: rng.integers(1, 5, size=n, dtype=np.uint8)     # runs mostly of length 1
    p = {"random": rnd()}
    for k, r in enumerate(RUNS):                                  # runs of exactly r, all through, at every phase against the tile
        p[f"runs_{r}"] = _runs_of(n, [r], [1, 2, 3, 4])
        p[f"dollar_runs_{r}"] = _runs_of(n, [r], [0, 3])
    p["runs_mixed"] = _runs_of(n, RUNS, [2, 4, 1])
    p["dollar_runs_mixed"] = _runs_of(n, RUNS + [1, 2], [0, 1, 0, 4])
    c = rnd()
    for e in range(t, n + t, t):                                  # runs longer than 31 across every tile edge
        _put(c, e - 17 - 9 * ((e // t) % 3), 40 + 31 * ((e // t) % 3), 3)
    p["straddle"] = c
    c = rnd()
    for e in range(t, n + t, t):                                  # a run that begins on a tile's last symbol
        _put(c, e - 1, RUNS[(e // t) % len(RUNS)], 2)
    p["begins_on_last"] = c
    c = rnd()
    for e in range(t, n + t, t):                                  # a run that ends on a tile's first symbol
        r = RUNS[(e // t) % len(RUNS)]
        _put(c, e + 1 - r, r, 4)
    p["ends_on_first"] = c
    for sym, name in ((1, "two_tiles"), (0, "dollar_two_tiles")):  # two whole tiles and parts of both neighbours
        c = rnd()
        _put(c, t - 5, 2 * t + 9, sym)
        p[name] = c
    p["one_run"] = np.full(n, 1, dtype=np.uint8)
    p["one_dollar_run"] = np.zeros(n, dtype=np.uint8)
    for at in (t - 1, t, t + 1, 45):                              # A..A C A..A: the run after the C starts from nothing
        c = np.full(n, 1, dtype=np.uint8)
        if at < n:
            c[at] = 2
        p[f"reset_at_{at}"] = c
    return p


def cases():
    """(name, small, codes) of every input of the encoder test; also what a sanitizer build of the driver is run over"""
    for name, small in TILES.items():
        t = tile_size(small)
        for n in sizes(t):
            for pat, codes in patterns(n, t, seed=7 * n + small).items():
                assert codes.size == n and codes.dtype == np.uint8 and codes.max(initial=0) <= 4
                yield f"{name}-N{n}-{pat}", small, codes


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rle_driver") / "rle_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(REPO / "tests/host_tools/rle_driver.cpp")],
                   check=True)
    return str(exe)


def _units(blob: bytes):
    out, p = [], 0
    for _ in range(2):
        n = int(np.frombuffer(blob, dtype=np.uint64, count=1, offset=p)[0])
        out.append(blob[p + 8: p + 8 + n])
        p += 8 + n
    assert p == len(blob)
    return out


def _sequential(codes: np.ndarray) -> bytes:
    out, prev, run = bytearray(), -1, 0
    for c in codes.tolist():
        if c == prev and run < 31:
            run += 1
            out[-1] = (c << 5) | run
        else:
            prev, run = c, 1
            out.append((c << 5) | 1)
    return bytes(out)


@pytest.mark.parametrize("tile", list(TILES))
def test_tiled_encoder_equals_the_sequential_rule(driver, tile):
    n_cases = 0
    for name, small, codes in cases():
        if small != TILES[tile]:
            continue
        r = subprocess.run([driver, "encode", str(small)], input=codes.tobytes(), capture_output=True)
        assert r.returncode == 0, (name, r.stderr)
        got, want = _units(r.stdout)
        assert got == want, name
        if codes.size <= 400:                                     # and the driver's restatement of the rule is the rule
            assert want == _sequential(codes), name
        n_cases += 1
    assert n_cases > 400


def test_the_cases_hold_what_they_are_named_for():
    t = tile_size(0)
    p = patterns(3 * t + 7, t, 1)
    assert (p["two_tiles"][t - 5: 3 * t + 4] == 1).all() and p["two_tiles"][t - 6] != 1 and p["two_tiles"][3 * t + 4] != 1
    assert (p["begins_on_last"][t - 1: t + 29] == 2).all() and p["begins_on_last"][t - 2] != 2
    assert p["ends_on_first"][t] == 4 and p["ends_on_first"][t + 1] != 4 and p["ends_on_first"][t - 1] == 4
    assert (p["straddle"][t - 26: t + 45] == 3).all()
    assert (np.diff(np.flatnonzero(np.diff(p["runs_93"]))) == 93).all()
    assert p["reset_at_%d" % t][t] == 2 and (np.delete(p["reset_at_%d" % t], t) == 1).all()


@pytest.mark.parametrize("wide", [0, 1], ids=["block32", "block64"])
@pytest.mark.parametrize("pattern", ["none", "first", "last", "boundaries", "whole_block", "third"])
def test_unpack_block_inverts_pack_block(driver, wide, pattern):
    from .test_index_pack_host import _codes

    ksyms = 128 if wide else 192
    codes = _codes(ksyms, pattern, ksyms // 4 if pattern == "boundaries" else ksyms, seed=31 + wide)
    if pattern == "boundaries":
        assert (codes == 0).sum() >= 6
    r = subprocess.run([driver, "decode", str(wide)], input=codes.tobytes(), capture_output=True, check=True)
    got = np.frombuffer(r.stdout, dtype=np.uint8).reshape(ksyms + 1, ksyms)
    for nv in range(ksyms + 1):
        want = codes.copy()
        want[nv:] = 0
        np.testing.assert_array_equal(got[nv], want, err_msg=f"n_valid={nv}")


def test_units_and_write_are_declared_and_exported(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    for name in ("lrsc_index_units", "lrsc_index_write"):
        assert name in capi.declared_symbols()
        assert f" T {name}\n" in exported
    assert api.lib.lrsc_abi_version() == 2
    assert callable(capi.Index.units) and callable(capi.Index.write)


def test_encoder_kernels_build_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as g

    g.build()
    obj = REPO / "longreadselfcorrect_amd" / "_build" / "obj" / "fm_rle.hip.o"
    assert obj.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp_path / "fm_rle.fatbin", tmp_path / "fm_rle.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    seen = {}
    for b in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(_ZN4lrsc\d+(rle_summary_kernel|rle_count_kernel|rle_emit_kernel)\S*)\s", b + "\n")
        if not m or m.group(1).endswith(".kd"):
            continue
        md = {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
        seen.setdefault(m.group(2), []).append(md)
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, (m.group(1), md)
        # registers must not hold fewer wavefronts than LDS does: 160 KiB of LDS per CU, four wavefronts per workgroup, four SIMDs
        # per CU with 512 VGPRs per lane each, at most eight wavefronts per SIMD
        lds = md["group_segment_fixed_size"]
        assert 0 < lds <= 64 * 1024
        per_simd = min(8, (160 * 1024 // lds) * 4 // 4)
        assert md["vgpr_count"] <= 512 // per_simd // 8 * 8 and md.get("agpr_count", 0) == 0, (m.group(1), per_simd, md)
    # every kernel for the byte BWT and for both block layouts
    assert {k: len(v) for k, v in seen.items()} == {"rle_summary_kernel": 3, "rle_count_kernel": 3, "rle_emit_kernel": 3}, seen


def test_save_index_needs_build_index(api, tmp_path):
    stride = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n")
    r = subprocess.run([str(stride), "pbcorrect", "--save-index", "x", "-o", "o", "reads.fa"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0
    assert "--save-index" in r.stderr and "Usage: StriDe PacBioSelfCorrection" in r.stderr
    assert not [p for p in tmp_path.rglob("*") if p.suffix in (".bwt", ".rbwt", ".sai", ".rsai")]
