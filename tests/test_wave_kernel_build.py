"""Build properties of wp_extend_wave_kernel (wp_wave.hip), checked on the CPU from the code object inside the build.

Like wp_extend_kernel, the wavefront-cooperative kernel has the whole walk inlined (an out-of-line piece would move the Walk
object to scratch memory), and it keeps the occupancy the launches are sized for (two wavefronts per SIMD).  Resources as
-Rpass-analysis=kernel-resource-usage reported them when this was written: 256 VGPRs, 0 AGPRs, occupancy 2, scratch 432 B per
lane (narrow layout) / 560 B (wide), 12 / 28 VGPRs spilled, 236 / 273 scratch and 114 FLAT instructions."""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
OBJ = ROOT / "longreadselfcorrect_amd" / "_build" / "obj" / "wp_wave.hip.o"


def _code_object(tmp: Path) -> Path:
    import __graft_entry__ as g
    g.build()
    assert OBJ.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp / "wp_wave.fatbin", tmp / "wp_wave.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(OBJ)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    return co


def _sym(wide: bool) -> str:
    return f"_ZN4lrsc21wp_extend_wave_kernelILb{int(wide)}EEEvNS_10FmIndexDevENS_6WpArgsE"


def _metadata(co: Path, sym: str) -> dict[str, int]:
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    # one block of "  - .key: value" lines per kernel; find the one that names this kernel
    blocks = re.split(r"\n\s+- \.", notes)
    for b in blocks:
        if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", b + "\n"):
            return {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
    raise AssertionError(f"{sym} not in the code object")


@pytest.mark.parametrize("wide", [False, True])
def test_wave_kernel_is_one_inlined_body_with_bounded_scratch(tmp_path, wide):
    co = _code_object(tmp_path)
    out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={_sym(wide)}", str(co)],
                         check=True, capture_output=True, text=True).stdout
    ins = [l for l in out.splitlines() if re.match(r"^\s+[a-z_0-9]+\s", l)]
    assert len(ins) > 10000, "the kernel with the walk and the wavefront step inside is some 23-31 k instructions"
    assert not [l for l in ins if "s_swappc_b64" in l], "an out-of-line piece of the walk"
    n_scratch = sum("scratch_" in l for l in ins)
    n_flat = sum(re.match(r"^\s+flat_", l) is not None for l in ins)
    assert n_scratch < 400 and n_flat < 300, (n_scratch, n_flat)


@pytest.mark.parametrize("wide", [False, True])
def test_wave_kernel_resources(tmp_path, wide):
    md = _metadata(_code_object(tmp_path), _sym(wide))
    assert md["vgpr_count"] <= 256 and md.get("agpr_count", 0) == 0, md        # two wavefronts per SIMD
    assert md["private_segment_fixed_size"] <= 768, md
    assert md["group_segment_fixed_size"] <= 8192, md                           # the rank mask table only: no LDS frontier
