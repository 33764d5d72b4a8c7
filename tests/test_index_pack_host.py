"""The device index packer (csrc/fm_pack.h, fm_pack.hip) checked without a GPU.

1. The per-block functions that the kernels call, compiled for the CPU (tests/host_tools/pack_driver.cpp), against the host
   builder build_strand_image on the same BWT: blocks, '$' list, '$' directory and C[] byte for byte, both layouts.  Sizes: less
   than a block, the multiples of 128, 192 and 384 = lcm (terminal block) with their neighbours, and one, two and several
   directory groups (8 blocks: 1024 / 1536 symbols).
2. lrsc_index_build is declared in include/lrsc.h and exported; the ABI version is still 2.
3. The packer's kernels compile for gfx950 without scratch or spills.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from .conftest import REPO

LLVM = Path("/opt/rocm/lib/llvm/bin")
SIZES = [1, 5, 127, 128, 129, 191, 192, 193, 383, 384, 385, 1535, 1536, 1537, 3 * 1536 + 7]
PATTERNS = ["none", "first", "last", "boundaries", "whole_block", "third"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pack_driver") / "pack_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(REPO / "tests/host_tools/pack_driver.cpp"),
                    str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
    return str(exe)


def _codes(n: int, pattern: str, ksyms: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 5, size=n, dtype=np.uint8)
    if pattern == "first":
        c[0] = 0
    elif pattern == "last":
        c[n - 1] = 0
    elif pattern == "boundaries":            # one '$' on each side of every block boundary
        for b in range(ksyms, n + 1, ksyms):
            c[b - 1] = 0
            if b < n:
                c[b] = 0
    elif pattern == "whole_block":           # every symbol of a block (the last whole one, or all there is)
        b = max(n // ksyms - 1, 0)
        c[b * ksyms: min((b + 1) * ksyms, n)] = 0
    elif pattern == "third":
        c[rng.random(n) < 1 / 3] = 0
    return c


def _split(blob: bytes):
    """[(name, bytes)] of the two images in the driver's output, the packer's first."""
    out, p = [], 0
    for _ in range(2):
        fields = {}
        for name, width in (("blocks", 64), ("dollars", 8), ("dollar_dir", 4)):
            n = int(np.frombuffer(blob, dtype=np.uint64, count=1, offset=p)[0])
            p += 8
            fields["n_" + name] = n
            fields[name] = blob[p: p + n * width]
            p += n * width
        fields["pred"] = blob[p: p + 40]
        p += 40
        out.append(fields)
    assert p == len(blob)
    return out


@pytest.mark.parametrize("wide", [0, 1], ids=["block32", "block64"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_host_packer_equals_build_strand_image(driver, wide, pattern):
    ksyms = 128 if wide else 192
    for n in SIZES:
        codes = _codes(n, pattern, ksyms, seed=1000 * n + wide)
        r = subprocess.run([driver, str(wide)], input=codes.tobytes(), capture_output=True, check=True)
        packed, built = _split(r.stdout)
        assert built["n_blocks"] == n // ksyms + 1 and built["n_dollars"] == int((codes == 0).sum())
        assert built["n_dollar_dir"] == (built["n_blocks"] >> 3) + 2
        for key in built:
            assert packed[key] == built[key], f"{key} differs at N={n}, pattern {pattern}, {'Block64' if wide else 'Block32'}"


def test_index_build_is_declared_and_exported(api):
    from longreadselfcorrect_amd.capi import declared_symbols

    assert "lrsc_index_build" in declared_symbols()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(api.path)], capture_output=True, text=True, check=True).stdout
    assert " T lrsc_index_build\n" in exported
    assert api.lib.lrsc_abi_version() == 2
    assert callable(api.index_build)


def test_packer_kernels_build_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as g

    g.build()
    obj = REPO / "longreadselfcorrect_amd" / "_build" / "obj" / "fm_pack.hip.o"
    assert obj.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp_path / "fm_pack.fatbin", tmp_path / "fm_pack.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    seen = {}
    for b in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(_ZN4lrsc\d+(pack_hist_kernel|pack_blocks_kernel|dollar_dir_kernel)\S*)\s", b + "\n")
        if not m or m.group(1).endswith(".kd"):
            continue
        md = {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
        seen.setdefault(m.group(2), []).append(md)
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, (m.group(1), md)
        # registers must not hold fewer wavefronts than the LDS rows do: 160 KiB of LDS per CU, two wavefronts per workgroup, four
        # SIMDs per CU with 512 VGPRs per lane each, at most eight wavefronts per SIMD
        lds = md["group_segment_fixed_size"]
        per_simd = min(8, (160 * 1024 // lds) * 2 // 4) if lds else 8
        assert md["vgpr_count"] <= 512 // per_simd // 8 * 8 and md.get("agpr_count", 0) == 0, (m.group(1), per_simd, md)
    # both layouts of the two streaming kernels, and the directory kernel
    assert {k: len(v) for k, v in seen.items()} == {"pack_hist_kernel": 2, "pack_blocks_kernel": 2, "dollar_dir_kernel": 1}, seen
    for name in ("pack_hist_kernel", "pack_blocks_kernel"):
        assert sorted(md["group_segment_fixed_size"] for md in seen[name]) == [128 * 9 * 16, 128 * 13 * 16], seen[name]
