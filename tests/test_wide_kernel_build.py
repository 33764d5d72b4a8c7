"""Build properties of wp_extend_wide_kernel (wp_wide.hip, the -l above 32 walks), checked on the CPU from the code object inside
the build.

Like wp_extend_wave_kernel it has the whole walk inlined (an out-of-line piece would move the Walk object to scratch memory) and
keeps the occupancy its launches are sized for (two wavefronts per SIMD); its slot bitsets sit in LDS beside the rank mask table.
Resources as -Rpass-analysis=kernel-resource-usage reported them when this was written: 254 / 255 VGPRs, 0 AGPRs, occupancy 2,
scratch 352 B per lane (narrow layout) / 448 B (wide), no VGPR spilled, LDS 6432 / 4368 B."""
from __future__ import annotations

import re
import subprocess

import pytest

from tests.test_wave_kernel_build import LLVM, ROOT, _metadata

OBJ = ROOT / "longreadselfcorrect_amd" / "_build" / "obj" / "wp_wide.hip.o"


def _code_object(tmp):
    import __graft_entry__ as g
    g.build()
    assert OBJ.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp / "wp_wide.fatbin", tmp / "wp_wide.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(OBJ)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    return co


def _sym(wide: bool) -> str:
    return f"_ZN4lrsc21wp_extend_wide_kernelILb{int(wide)}EEEvNS_10FmIndexDevENS_6WpArgsE"


@pytest.mark.parametrize("wide", [False, True])
def test_wide_kernel_is_one_inlined_body_with_bounded_scratch(tmp_path, wide):
    co = _code_object(tmp_path)
    out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={_sym(wide)}", str(co)],
                         check=True, capture_output=True, text=True).stdout
    ins = [l for l in out.splitlines() if re.match(r"^\s+[a-z_0-9]+\s", l)]
    assert len(ins) > 10000, "the kernel with the walk and the wavefront step inside"
    assert not [l for l in ins if "s_swappc_b64" in l], "an out-of-line piece of the walk"
    n_scratch = sum("scratch_" in l for l in ins)
    assert n_scratch < 600, n_scratch


@pytest.mark.parametrize("wide", [False, True])
def test_wide_kernel_resources(tmp_path, wide):
    md = _metadata(_code_object(tmp_path), _sym(wide))
    assert md["vgpr_count"] <= 256 and md.get("agpr_count", 0) == 0, md        # two wavefronts per SIMD
    assert md["private_segment_fixed_size"] <= 768, md
    assert md["group_segment_fixed_size"] <= 8192, md                           # the rank mask table and the slot bitsets
