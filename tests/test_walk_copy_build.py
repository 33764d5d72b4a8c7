"""The serial walk's block moves in the built gfx950 code (walk_device.h: burst_copy16, burst_copy4, leaf_move), checked on the CPU
from the code object inside the build.

A further child's ring and path copies, the survivors' copy-down and the trim's compaction are moves between disjoint slots of a
lane's own workspace.  Written element by element they compile to load -> s_waitcnt vmcnt(0) -> store per element, one memory
round trip each, because the compiler must order every load behind the store before it.  The helpers issue a chunk of loads,
wait once and store the chunk.  Both instantiations of wp_extend_kernel are held to that:

 * the number of ADJACENT triples `global/flat load` -> `s_waitcnt ... vmcnt(0)` -> `global/flat store` (three consecutive
   instructions of the disassembly) is below what it was before the helpers.  Counted this way, on the build of the commit before
   them: 20 in the narrow layout (10 ring doubles of the ten-times unrolled ring loop, 10 dwordx4 of leaf copies), 22 in the wide
   layout (10 + 12).  With the helpers: 3 and 3 -- the last of the seven loads of burst_copy4's tail in its three inlined copies,
   a burst's end rather than an element's round trip.  (A looser count over the compiler's assembly listing gave 30 for the narrow
   layout before; the bound here is the stricter figure.)
 * no innermost loop holds an 8-byte load, a full drain and an 8-byte store together: the shape of the old ring copy.  Before the
   helpers one such loop existed per layout (the ring copy), now none.

For the record, the same two builds (`llvm-objdump -d`, code object metadata), before -> after:
 narrow: 29 132 -> 29 598 instructions; 636 -> 610 s_waitcnt that drain vmcnt to 0 (546 -> 520 with no other counter); 256 VGPRs,
         608 B of scratch, 113 VGPR spills, 328-329 scratch instructions in both
 wide:   42 029 -> 42 443 instructions; 758 -> 723 (670 -> 635); 256 VGPRs, 720 B of scratch, 131 VGPR spills in both, 395 -> 388
         scratch instructions"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
OBJ = ROOT / "longreadselfcorrect_amd" / "_build" / "obj" / "wp.hip.o"
TRIPLES_BEFORE = {False: 20, True: 22}


@pytest.fixture(scope="module")
def code_object(tmp_path_factory) -> Path:
    import __graft_entry__ as g
    g.build()
    assert OBJ.exists(), "build() leaves the per-unit objects in _build/obj"
    tmp = tmp_path_factory.mktemp("wp_co")
    fat, co = tmp / "wp.fatbin", tmp / "wp.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(OBJ)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--unbundle", f"--output={co}"], check=True)
    return co


def _instructions(co: Path, wide: bool) -> list[tuple[int, str, int | None]]:
    """(address, instruction text, branch target address or None) of every instruction of the kernel"""
    sym = f"_ZN4lrsc16wp_extend_kernelILb{int(wide)}EEEvNS_10FmIndexDevENS_6WpArgsE"
    out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={sym}", str(co)],
                         check=True, capture_output=True, text=True).stdout
    base, ins = None, []
    for l in out.splitlines():
        m = re.match(r"^([0-9a-f]+) <" + re.escape(sym) + r">:", l)
        if m:
            base = int(m.group(1), 16)
        m = re.match(r"^\s+([a-z_0-9]+\s.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", l)
        if not m:
            continue
        t = re.search(r"<" + re.escape(sym) + r"\+0x([0-9a-f]+)>", m.group(3))
        ins.append((int(m.group(2), 16), m.group(1).strip(), base + int(t.group(1), 16) if t and "branch" in m.group(1) else None))
    assert base is not None and len(ins) > 20000, "the kernel with the whole walk inside is some 29 k instructions"
    return ins


def _is_load(t: str, width: str = "") -> bool:
    return re.match(r"(global|flat)_load_dword" + width + r"\b", t) is not None


def _is_store(t: str, width: str = "") -> bool:
    return re.match(r"(global|flat)_store_dword" + width + r"\b", t) is not None


def _is_drain(t: str) -> bool:
    return t.startswith("s_waitcnt") and "vmcnt(0)" in t


@pytest.mark.parametrize("wide", [False, True])
def test_fewer_load_drain_store_triples(code_object, wide):
    text = [t for _, t, _ in _instructions(code_object, wide)]
    triples = [k for k in range(len(text) - 2) if _is_load(text[k], r"(x\d)?") and _is_drain(text[k + 1]) and _is_store(text[k + 2], r"(x\d)?")]
    print("wide" if wide else "narrow", "adjacent load / drain / store triples:", len(triples), "before:", TRIPLES_BEFORE[wide])
    assert len(triples) < TRIPLES_BEFORE[wide], [text[k] for k in triples]


@pytest.mark.parametrize("wide", [False, True])
def test_no_loop_moves_doubles_one_round_trip_each(code_object, wide):
    ins = _instructions(code_object, wide)
    index = {a: k for k, (a, _, _) in enumerate(ins)}
    loops = sorted((index[tgt], k) for k, (a, _, tgt) in enumerate(ins) if tgt is not None and tgt <= a)
    assert len(loops) > 20, "backward branches of the kernel"
    innermost = [(s, e) for s, e in loops if not any((s2, e2) != (s, e) and s <= s2 and e2 <= e for s2, e2 in loops)]
    bad = []
    for s, e in innermost:
        body = [t for _, t, _ in ins[s: e + 1]]
        if any(_is_load(t, "x2") for t in body) and any(_is_drain(t) for t in body) and any(_is_store(t, "x2") for t in body):
            bad.append((s, e))
    print("wide" if wide else "narrow", len(loops), "loops,", len(innermost), "innermost; with 8-byte load + full drain + 8-byte store:", bad)
    assert not bad, [[t for _, t, _ in ins[s: e + 1]] for s, e in bad][:1]
