"""Build properties of wp_extend_deal_kernel (wp_deal.hip), read on the CPU from the metadata of the code object inside the build.

The kernel keeps wp_extend_kernel's launch shape -- two wavefronts per SIMD, which the launches are sized for -- so it has to stay
at 256 VGPRs with no AGPRs, and its private segment within what wp_extend_kernel had before it: 544 B per lane in the narrow
rank-block layout, 704 B in the wide one.  As -Rpass-analysis=kernel-resource-usage and the metadata reported them when this was
written: 256 VGPRs, 0 AGPRs, 496 B (narrow) / 640 B (wide), 85 / 97 VGPRs spilled.

That is the instantiation every launch without LRSC_CORRECT_PROFILE runs.  The profiling instantiation (PROF = true) carries the
tick slots the Walk object points to, an array in scratch memory, and is 608 B / 784 B; it is a diagnostic and is held only to
the register file."""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
OBJ = ROOT / "longreadselfcorrect_amd" / "_build" / "obj" / "wp_deal.hip.o"
PRIVATE_BOUND = {False: 544, True: 704}


@pytest.fixture(scope="module")
def code_object(tmp_path_factory) -> Path:
    import __graft_entry__ as g
    g.build()
    assert OBJ.exists(), "build() leaves the per-unit objects in _build/obj"
    tmp = tmp_path_factory.mktemp("wp_deal")
    fat, co = tmp / "wp_deal.fatbin", tmp / "wp_deal.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(OBJ)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    return co


def _metadata(co: Path, sym: str) -> dict[str, int]:
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    # one block of "  - .key: value" lines per kernel; find the one that names this kernel
    for b in re.split(r"\n\s+- \.", notes):
        if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", b + "\n"):
            return {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
    raise AssertionError(f"{sym} not in the code object")


def _sym(wide: bool, prof: bool) -> str:
    return f"_ZN4lrsc21wp_extend_deal_kernelILb{int(wide)}ELb{int(prof)}EEEvNS_10FmIndexDevENS_6WpArgsE"


@pytest.mark.parametrize("wide", [False, True])
def test_deal_kernel_resources(code_object, wide):
    md = _metadata(code_object, _sym(wide, False))
    print(md)
    assert md["vgpr_count"] <= 256 and md.get("agpr_count", 0) == 0, md        # two wavefronts per SIMD
    assert md["private_segment_fixed_size"] <= PRIVATE_BOUND[wide], md


@pytest.mark.parametrize("wide", [False, True])
def test_profiling_instantiation_keeps_the_occupancy(code_object, wide):
    md = _metadata(code_object, _sym(wide, True))
    assert md["vgpr_count"] <= 256 and md.get("agpr_count", 0) == 0, md
