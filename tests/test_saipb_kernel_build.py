"""Build properties of saipb_merge_kernel and saipb_seed_kernel (csrc/saipb.hip), checked on the CPU from the gfx950 code object inside
the build, and the C-ABI surface of lrsc_saipb_merge.

The whole job (collect, tree, result choice with the alignment) is one inlined body: an out-of-line piece would need a call
sequence (s_swappc_b64) and a stack.  Resources as the code object's metadata reported them when this was written: the merge kernel
105 VGPRs (narrow layout) / 98 (wide), 0 AGPRs, no scratch (private segment 0 B, SGPR spills go to VGPR lanes), LDS 6176 B / 2064 B
(the rank mask table only), some 8.7 k instructions; the seed kernel 72 / 67 VGPRs, no scratch.  The assertions leave a slack of
six registers over each of those figures, and of the LDS nothing beyond rounding."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
OBJ = ROOT / "longreadselfcorrect_amd" / "_build" / "obj" / "saipb.hip.o"


@pytest.fixture(scope="module")
def code_object(tmp_path_factory) -> Path:
    import __graft_entry__ as g
    g.build()
    assert OBJ.exists(), "build() leaves the per-unit objects in _build/obj"
    tmp = tmp_path_factory.mktemp("saipb_co")
    fat, co = tmp / "saipb.fatbin", tmp / "saipb.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(OBJ)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    return co


def _merge_sym(wide: bool) -> str:
    return (f"_ZN4lrsc18saipb_merge_kernelILb{int(wide)}EEEvNS_10FmIndexDevEPKhPKNS_9SaipbSeedEPKNS_13SaipbSeedInfoEPKNS_8SaipbJobEjPhPcPNS_8SaipbOutE")


def _seed_sym(wide: bool) -> str:
    return f"_ZN4lrsc17saipb_seed_kernelILb{int(wide)}EEEvNS_10FmIndexDevEPKhPKNS_9SaipbSeedEjPNS_13SaipbSeedInfoE"


def _metadata(co: Path, sym: str) -> dict[str, int]:
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    for b in re.split(r"\n\s+- \.", notes):
        if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", b + "\n"):
            return {k: int(v) for k, v in re.findall(r"\.?([a-z_]+):\s+(\d+)\s*$", "." + b, flags=re.M)}
    raise AssertionError(f"{sym} not in the gfx950 code object")


@pytest.mark.parametrize("wide", [False, True])
def test_merge_kernel_is_one_inlined_body_without_scratch(code_object, wide):
    out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={_merge_sym(wide)}", str(code_object)],
                         check=True, capture_output=True, text=True).stdout
    ins = [l for l in out.splitlines() if re.match(r"^\s+[a-z_0-9]+\s", l)]
    assert 3000 < len(ins) < 14000, len(ins)
    assert not [l for l in ins if "s_swappc_b64" in l], "an out-of-line piece of the job"
    assert not [l for l in ins if "scratch_" in l], "scratch traffic in the tree kernel"
    assert any("global_atomic_cmpswap_x2" in l for l in ins) and any("global_atomic_add" in l for l in ins), "the table's integer atomics"


@pytest.mark.parametrize("wide", [False, True])
def test_kernel_resources(code_object, wide):
    md = _metadata(code_object, _merge_sym(wide))
    assert md["vgpr_count"] <= (104 if wide else 111) and md.get("agpr_count", 0) == 0, md     # 98 / 105 when written; 128 is the occupancy step
    assert md["private_segment_fixed_size"] == 0 and md.get("vgpr_spill_count", 0) == 0, md
    assert md["group_segment_fixed_size"] <= (2112 if wide else 6208), md         # the rank mask table only: 2064 / 6176 B
    sd = _metadata(code_object, _seed_sym(wide))
    assert sd["vgpr_count"] <= (73 if wide else 78) and sd["private_segment_fixed_size"] == 0, sd           # 67 / 72 when written


def test_abi_null_ctx_is_an_argument_error(api):
    used = C.c_uint64(7)
    assert api.lib.lrsc_saipb_merge(None, None, 0, None, 0, None, 0, None, None, None, 0, C.byref(used)) == -3
    assert api.lib.lrsc_abi_version() == 2


def test_header_with_the_saipb_records_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lrsc.h"\nint main(void){ lrsc_saipb_seed s; lrsc_saipb_job j; lrsc_saipb_result r; (void)s; (void)j; (void)r;\n'
                   '  return lrsc_saipb_merge(0, 0, 0, &s, 0, &j, 0, &r, 0, 0, 0, 0) == LRSC_ERR_ARG && LRSC_SAIPB_OK == 0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
