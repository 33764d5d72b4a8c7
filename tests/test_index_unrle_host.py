"""The device RL decoder (csrc/fm_unrle.h, fm_unrle.hip) checked without a GPU.

1. The per-lane functions that the kernels call, compiled for the CPU (tests/host_tools/unrle_driver.cpp) and run in the
   kernels' order, against build_strand_image (fm_layout.cpp) on the same units, byte for byte: with the kernels' tiles and
   with small ones (a unit tile of 16 units, a chunk of two lanes, a symbol tile of two rank blocks), so that the paths over
   several tiles run on short inputs as well.
2. The seek alone, on a table of unit-tile starts whose positions and unit indexes straddle 2^32.
3. Defective streams are refused with build_strand_image's text.
4. lrsc_index_open_device / lrsc_index_from_units_device are declared and exported, the ABI version is still 2, the binding
   has the methods.
5. The decoder's kernels compile for gfx950 without scratch or spills, their registers within what their LDS allows.
6. `stride pbcorrect --load-on-device` with --build-index is an argument error.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO

LLVM = Path("/opt/rocm/lib/llvm/bin")
HDR = (REPO / "longreadselfcorrect_amd/csrc/fm_unrle.h").read_text()
SHAPES = {"kernel_tiles": 0, "small_tiles": 1}                    # the driver's <small> argument
LAYOUTS = {"block32": 0, "block64": 1}                            # the driver's <wide> argument
RUNS = [30, 31, 32, 61, 62, 63, 93]
CORRUPT = "corrupt RL unit in BWT"
EXCEED = "BWT runs exceed the symbol count in the header"
SHORT = "BWT runs do not add up to the symbol count in the header"


def tiles(small: int, wide: int) -> tuple[int, int, int]:
    """(symbols per rank block, symbols per symbol tile, units per unit tile) as fm_unrle.h names them, or the driver's small ones"""
    ksyms = 128 if wide else 192
    if small:
        return ksyms, 2 * ksyms, 16
    c = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (kUnrleLanes|kUnrleBlocks) = (\d+);", HDR)}
    assert re.search(r"kUnrleTile = kUnrleLanes \* 16;", HDR)
    return ksyms, c["kUnrleBlocks"] * ksyms, c["kUnrleLanes"] * 16


def sizes(ksyms: int, t: int) -> list[int]:
    m = 384 * (2 * t // 384 + 1)                                  # a multiple of the block size of either layout beyond two tiles
    s = {1, ksyms - 1, ksyms, ksyms + 1, t - 1, t, t + 1, 3 * t + 7, 384 * 5, 384 * 5 + 1, m, m + 1}
    return sorted(s)


# ---- streams ----------------------------------------------------------------------------------------------------
def encode(codes: np.ndarray) -> np.ndarray:
    """the canonical units of a symbol string: BWTWriterBinary::writeBWChar's rule"""
    n = codes.size
    starts = np.concatenate([[0], np.flatnonzero(np.diff(codes)) + 1])
    lens = np.diff(np.concatenate([starts, [n]]))
    full, rem = lens // 31, lens % 31
    cnt = full + (rem > 0)
    u_code = np.repeat(codes[starts], cnt).astype(np.uint8)
    u_run = np.full(u_code.size, 31, dtype=np.uint8)
    last = np.cumsum(cnt) - 1
    u_run[last[rem > 0]] = rem[rem > 0]
    return (u_code << 5) | u_run


def decode(units: np.ndarray) -> np.ndarray:
    return np.repeat(units >> 5, units & 31).astype(np.uint8)


def fit(u_code: np.ndarray, u_run: np.ndarray, n: int) -> np.ndarray:
    """the first units of the stream that hold n symbols, the last one cut short"""
    cum = np.cumsum(u_run.astype(np.int64))
    assert cum[-1] >= n
    k = int(np.searchsorted(cum, n, side="left"))
    run = u_run[: k + 1].astype(np.uint8).copy()
    run[k] -= np.uint8(cum[k] - n)
    return (u_code[: k + 1].astype(np.uint8) << 5) | run


def _runs_of(n: int, r: int, symbols, lead: int = 0) -> np.ndarray:
    """runs of exactly r symbols, the first one `lead` symbols late"""
    k = -(-n // r) + 2
    syms = np.resize(np.asarray(symbols, dtype=np.uint8), k)
    c = np.repeat(syms, r)
    if lead:
        c = np.concatenate([np.full(lead, symbols[-1], dtype=np.uint8), c])
    return c[:n]


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


def patterns(n: int, ksyms: int, t: int, u: int, seed: int, every_phase: bool) -> dict[str, np.ndarray]:
    """name -> units of n symbols"""
    rng = np.random.default_rng(seed)
    rnd = lambda: rng.integers(1, 5, size=n, dtype=np.uint8)      # runs mostly of length 1
    p = {}
    # ---- from symbols, canonical units
    p["random_symbols"] = encode(rnd())
    for r in RUNS:                                                # runs of exactly r all through, at every phase against a tile
        for lead in (range(r) if every_phase else (0, 1, r - 1)):
            p[f"runs_{r}_lead{lead}"] = encode(_runs_of(n, r, [1, 2, 3, 4], lead))
        p[f"dollar_runs_{r}"] = encode(_runs_of(n, r, [0, 3]))
    c = rnd()
    for e in range(ksyms, n + ksyms, ksyms):                      # a run of two or three units across every block (and tile) edge
        _put(c, e - 17 - 9 * ((e // ksyms) % 3), 40 + 31 * ((e // ksyms) % 3), 3)
    p["across_block_edges"] = encode(c)
    for where, back in (("first", 0), ("middle", 4), ("last", 8)):
        c = rnd()
        for e in range(t, n, t):                                  # the tile begins on that symbol of a unit of nine
            _put(c, e - back, 9, 2)
        p[f"tile_begins_on_{where}"] = encode(c)
    c = rnd()
    c[0] = 0
    for e in range(ksyms, n + 1, ksyms):                          # '$' in the first and last row of every block, so of every group
        c[e - 1] = 0
        if e < n:
            c[e] = 0
    p["dollars_at_block_edges"] = encode(c)
    p["one_run"] = encode(np.full(n, 1, dtype=np.uint8))
    p["one_dollar_run"] = encode(np.zeros(n, dtype=np.uint8))
    # ---- from units
    i = np.arange(n)
    p["all_runs_31"] = fit(1 + i % 4, np.full(n, 31), n)
    p["all_runs_1"] = fit(1 + i % 4, np.full(n, 1), n)
    p["random_units"] = fit(rng.integers(0, 5, size=n), rng.integers(1, 32, size=n), n)
    p["dollar_dense"] = fit(rng.integers(0, 2, size=n) * rng.integers(1, 5, size=n), rng.integers(1, 4, size=n), n)
    p["non_canonical"] = fit(rng.integers(1, 3, size=n), rng.integers(1, 31, size=n), n)
    code, run = rng.integers(1, 5, size=n), rng.integers(1, 9, size=n)
    for e in range(u, n, u):                                      # one run across every unit-tile edge
        code[e - 1: e + 1] = 3
        run[e - 1] = 31
    p["across_unit_tile_edges"] = fit(code, run, n)
    code, run = rng.integers(1, 5, size=n), rng.integers(1, 3, size=n)
    if int(run[: 2 * u].sum()) < n and n > 2 * u:                 # a unit tile of '$' alone, where the stream holds one
        code[u: 2 * u] = 0
        p["dollar_unit_tile"] = fit(code, run, n)
    for name, units in p.items():
        assert units.dtype == np.uint8 and int((units & 31).astype(np.int64).sum()) == n, name
        assert ((units >> 5) <= 4).all() and ((units & 31) >= 1).all(), name
    return p


def cases(small: int, wide: int):
    """(name, N, units) of every input of the decoder test; also what a sanitizer build of the driver is run over"""
    ksyms, t, u = tiles(small, wide)
    for n in sizes(ksyms, t):
        for pat, units in patterns(n, ksyms, t, u, seed=11 * n + 2 * small + wide, every_phase=bool(small) and n == 3 * t + 7).items():
            yield f"N{n}-{pat}", n, units


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("unrle_driver") / "unrle_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(REPO / "tests/host_tools/unrle_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


def _images(blob: bytes):
    """the two images of the driver's output, each as its sections"""
    out, p = [], 0
    u64 = lambda at: int(np.frombuffer(blob, dtype=np.uint64, count=1, offset=at)[0])
    for _ in range(2):
        im = {}
        for name, width in (("blocks", 64), ("dollars", 8), ("dollar_dir", 4)):
            n = u64(p)
            im["n_" + name] = n
            im[name] = blob[p + 8: p + 8 + n * width]
            p += 8 + n * width
        im["pred"] = blob[p: p + 40]
        p += 40
        out.append(im)
    assert p == len(blob)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tiled_decoder_equals_the_host_builder(driver, shape, layout):
    small, wide = SHAPES[shape], LAYOUTS[layout]
    n_cases, seen = 0, set()
    for name, n, units in cases(small, wide):
        r = subprocess.run([driver, "pack", str(wide), str(small), str(n)], input=units.tobytes(), capture_output=True)
        assert r.returncode == 0, (name, r.returncode, r.stdout[:200], r.stderr)
        got, want = _images(r.stdout)
        for key in want:
            assert got[key] == want[key], (name, key)
        n_cases += 1
        seen.add(name.split("-", 1)[1])
    assert n_cases > 300 and "dollar_unit_tile" in seen


def test_the_cases_hold_what_they_are_named_for():
    ksyms, t, u = tiles(0, 0)
    n = 3 * t + 7
    p = patterns(n, ksyms, t, u, 1, False)
    cum = lambda units: np.concatenate([[0], np.cumsum((units & 31).astype(np.int64))])
    assert ((p["all_runs_31"] & 31)[:-1] == 31).all() and ((p["all_runs_1"] & 31) == 1).all() and p["all_runs_1"].size == n > 5 * u
    starts = cum(p["tile_begins_on_first"])
    assert t in starts and (p["tile_begins_on_first"][np.searchsorted(starts, t)] & 31) == 9
    assert t - 4 in cum(p["tile_begins_on_middle"]) and t - 8 in cum(p["tile_begins_on_last"])
    un = p["across_unit_tile_edges"]
    assert un.size > 2 * u and un[u - 1] == (3 << 5 | 31) and un[u] >> 5 == 3
    un = p["non_canonical"]
    same = (un[1:] >> 5) == (un[:-1] >> 5)
    assert (same & ((un[:-1] & 31) < 31)).sum() > un.size // 4, "adjacent units of one symbol, the first below 31"
    assert ((p["dollar_unit_tile"][u: 2 * u] >> 5) == 0).all()
    c = decode(p["dollars_at_block_edges"])
    assert c[0] == 0 and c[ksyms - 1] == 0 and c[ksyms] == 0 and c[8 * ksyms - 1] == 0 and c[8 * ksyms] == 0
    c = decode(p["across_block_edges"])
    assert (c[ksyms - 10: ksyms + 10] == 3).all() and (c[t - 10: t + 10] == 3).all()
    assert (np.diff(np.flatnonzero(np.diff(decode(p["runs_93_lead0"])))) == 93).all()
    assert p["one_run"].size == -(-n // 31) and decode(p["one_dollar_run"]).max() == 0
    # the small tiles see runs of every length at every phase against a symbol tile
    ks, ts, us = tiles(1, 1)
    names = {name for name, _, _ in cases(1, 1)}
    assert all(f"N{3 * ts + 7}-runs_{r}_lead{lead}" in names for r in RUNS for lead in range(r))


def test_seek_with_positions_and_unit_indexes_beyond_32_bits(driver):
    """Tile t of the driver's stream: kUnrleTile units of symbol t % 5 and run 1 + t % 31."""
    _, _, u = tiles(0, 0)
    n_tiles = (1 << 32) // u + 3                                  # the last tiles' units have indexes above 2^32
    tt = np.arange(n_tiles, dtype=np.int64)
    syms = u * (1 + tt % 31)
    pos = np.concatenate([[0], np.cumsum(syms)])
    slot = np.where(tt % 5 == 0, 4, tt % 5 - 1)
    before = [np.concatenate([[0], np.cumsum(np.where(slot == k, syms, 0))]) for k in range(5)]
    assert pos[-1] > 1 << 35
    t32 = int(np.searchsorted(pos, 1 << 32, side="right")) - 1   # the tile that holds position 2^32
    rng = np.random.default_rng(5)
    ps = [0, 1, int(pos[-1]) - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, int(pos[t32]), int(pos[t32]) - 1, int(pos[t32 + 1]) - 1,
          int(pos[t32 + 1]), int(pos[n_tiles - 3]), int(pos[n_tiles - 3]) - 1, int(pos[n_tiles - 3]) + 5 * 29 + 3]
    ps += [int(x) for x in rng.integers(0, pos[-1], size=200)]
    ps += [int(pos[t]) + int(rng.integers(0, syms[t])) for t in (t32, n_tiles - 3, n_tiles - 2, n_tiles - 1) for _ in range(20)]
    r = subprocess.run([driver, "seek", str(n_tiles)], input=np.array(ps, dtype=np.uint64).tobytes(), capture_output=True, check=True)
    got = np.frombuffer(r.stdout, dtype=np.uint64).reshape(len(ps), 7)
    above = 0
    for p, g in zip(ps, got.tolist()):
        t = int(np.searchsorted(pos, p, side="right")) - 1
        rel, run = p - int(pos[t]), 1 + t % 31
        want = [t * u + rel // run, rel % run] + [int(before[k][t]) + (rel if slot[t] == k else 0) for k in range(5)]
        assert g == want, (p, g, want)
        assert sum(want[2:]) == p
        above += want[0] >= 1 << 32
    assert above >= 40


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_defective_streams_are_refused_as_the_host_refuses_them(driver, shape, layout):
    small, wide = SHAPES[shape], LAYOUTS[layout]
    ksyms, t, u = tiles(small, wide)
    n = 3 * t + 7
    good = patterns(n, ksyms, t, u, 3, False)["dollar_dense"]
    assert good.size > 2 * u + 3

    def run(units, n_syms):
        r = subprocess.run([driver, "pack", str(wide), str(small), str(n_syms)], input=units.tobytes(), capture_output=True)
        assert r.returncode == 3, (r.returncode, r.stderr)
        mine, host, bad = r.stdout.decode().split("\n")[:3]
        return mine, host, int(bad)

    for at in (0, good.size // 2, u - 1, u, good.size - 1):       # first, middle, either side of a unit-tile edge, last
        for code in (5, 6, 7):
            units = good.copy()
            units[at] = (code << 5) | (units[at] & 31)
            assert run(units, n) == (CORRUPT, CORRUPT, at), (at, code)
        units = good.copy()
        units[at] &= 0xE0                                         # run 0
        assert run(units, n) == (CORRUPT, CORRUPT, at), at
    units = good.copy()
    units[[5, good.size - 2]] = 0xFF                              # two corrupt units: the first one is named
    assert run(units, n)[2] == 5
    assert run(np.append(good, np.uint8(1 << 5 | 1)), n) == (EXCEED, EXCEED, -1)
    assert run(good, n - 1) == (EXCEED, EXCEED, -1)
    assert run(good[:-1], n) == (SHORT, SHORT, -1)
    assert run(good, n + 1) == (SHORT, SHORT, -1)
    assert run(good[:1], n) == (SHORT, SHORT, -1)


# ---- the ABI, the kernels, the command line ----------------------------------------------------------------------
def test_device_open_is_declared_and_exported(api):
    from longreadselfcorrect_amd import capi

    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    for name in ("lrsc_index_open_device", "lrsc_index_from_units_device"):
        assert name in capi.declared_symbols()
        assert f" T {name}\n" in exported
    assert api.lib.lrsc_abi_version() == 2
    assert callable(capi.Lrsc.index_open_device) and callable(capi.Lrsc.index_from_units_device)


def test_decoder_kernels_build_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as g

    g.build()
    obj = REPO / "longreadselfcorrect_amd" / "_build" / "obj" / "fm_unrle.hip.o"
    assert obj.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp_path / "fm_unrle.fatbin", tmp_path / "fm_unrle.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    seen = {}
    for b in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(_ZN4lrsc\d+(unrle_tile_kernel|unrle_pack_kernel)\S*)\s", b + "\n")
        if not m or m.group(1).endswith(".kd"):
            continue
        md = {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
        seen.setdefault(m.group(2), []).append(md)
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, (m.group(1), md)
        # registers must not hold fewer wavefronts than LDS does: 160 KiB of LDS per CU, four wavefronts per workgroup, four SIMDs
        # per CU with 512 VGPRs per lane each, at most eight wavefronts per SIMD
        assert md["max_flat_workgroup_size"] == 256
        lds = md["group_segment_fixed_size"]
        assert 0 < lds <= 64 * 1024
        per_simd = min(8, (160 * 1024 // lds) * 4 // 4)
        assert md["vgpr_count"] <= 512 // per_simd // 8 * 8 and md.get("agpr_count", 0) == 0, (m.group(1), per_simd, md)
    # the tile kernel, and the pack kernel for both block layouts
    assert {k: len(v) for k, v in seen.items()} == {"unrle_tile_kernel": 1, "unrle_pack_kernel": 2}, seen


def test_load_on_device_excludes_build_index(api, tmp_path):
    stride = REPO / "longreadselfcorrect_amd" / "_build" / "stride"
    (tmp_path / "reads.fa").write_text(">r0\nACGTACGT\n")
    r = subprocess.run([str(stride), "pbcorrect", "--load-on-device", "--build-index", "-o", "o", "reads.fa"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "--load-on-device" in r.stderr and "Usage: StriDe PacBioSelfCorrection" in r.stderr
    usage = subprocess.run([str(stride), "pbcorrect", "--help"], capture_output=True, text=True).stderr
    assert "--load-on-device" in usage
