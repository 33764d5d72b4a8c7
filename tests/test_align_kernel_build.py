"""Build properties of dp_align_kernel (dp_align.hip), checked on the CPU from the code object inside the build.

The kernel is sized for eight wavefronts per SIMD (they hide the wave scan's cross-lane latency), so both instantiations (LDS
staging / global-workspace staging) stay within 64 VGPRs with no scratch and nothing out of line.  Its fill -- every column's
wave scan and what lies between them -- is straight-line code under wave-uniform branches only: the row classes, the choice
of a cell's inputs and the traceback decision are selects and mask arithmetic, not exec-mask regions.  The fill is located by
its scans (v_max_i32 with the row_bcast:31 DPP step, which nothing else in the kernel uses): no s_*_saveexec may lie between
the first and the last of them.  For the record, `llvm-objdump -d --no-show-raw-insn --disassemble-symbols=<kernel>` counted
62 s_*_saveexec in either instantiation before the fill was made branch-free (16 of them in the one-column loop body), and 33
when this was written, all in the staging loops and the traceback."""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
OBJ = ROOT / "longreadselfcorrect_amd" / "_build" / "obj" / "dp_align.hip.o"
SAVEEXEC_BEFORE = 62


def _code_object(tmp: Path) -> Path:
    import __graft_entry__ as g
    g.build()
    assert OBJ.exists(), "build() leaves the per-unit objects in _build/obj"
    fat, co = tmp / "dp_align.fatbin", tmp / "dp_align.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(OBJ)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    return co


def _sym(global_stage: bool) -> str:
    return f"_ZN4lrsc15dp_align_kernelILb{int(global_stage)}EEEvNS_11DpAlignArgsE"


def _metadata(co: Path, sym: str) -> dict[str, int]:
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    for b in re.split(r"\n\s+- \.", notes):
        if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", b + "\n"):
            return {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
    raise AssertionError(f"{sym} not in the code object")


@pytest.mark.parametrize("global_stage", [False, True])
def test_align_kernel_resources(tmp_path, global_stage):
    md = _metadata(_code_object(tmp_path), _sym(global_stage))
    assert md["vgpr_count"] <= 64 and md.get("agpr_count", 0) == 0, md          # eight wavefronts per SIMD
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md


@pytest.mark.parametrize("global_stage", [False, True])
def test_align_kernel_fill_is_branch_free(tmp_path, global_stage):
    co = _code_object(tmp_path)
    out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={_sym(global_stage)}", str(co)],
                         check=True, capture_output=True, text=True).stdout
    ins = [l for l in out.splitlines() if re.match(r"^\s+[a-z_0-9]+\s", l)]
    assert len(ins) > 1000, "the kernel with its eight inlined column bodies is some 3 k instructions"
    assert not [l for l in ins if "s_swappc_b64" in l], "an out-of-line piece"
    scans = [k for k, l in enumerate(ins) if "row_bcast:31" in l]
    # four interior columns, four edge columns; every scan step is one v_max_i32 with the DPP operand folded in
    assert len(scans) == 8 and all(ins[k].split()[0].startswith("v_max_i32") for k in scans), [ins[k] for k in scans]
    fill = ins[scans[0]: scans[-1] + 1]
    assert not [l for l in fill if "saveexec" in l], "an exec-mask region inside the fill"
    assert sum("saveexec" in l for l in ins) < SAVEEXEC_BEFORE
