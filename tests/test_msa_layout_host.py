"""The pile-up kernel's memory layout (csrc/dp_msa_layout.h: msa_layout, which the kernel carves its pointers from and the host's
dp_msa_lds_bytes / dp_msa_small_bytes return the totals of) on the host.

tests/host_msa_layout/msa_layout_host.cpp is a stand-alone program that includes the header and prints every offset for
lq x n_str x wavefronts x {LDS, global workspace}, with the capacities DpStage::size_requests gives a request of that query length.
Here the byte counts are restated as the formulas the host used before there was a layout (one sum for the LDS of a pile-up, one for
the small arrays of the wide global variant), and the arrays' sizes as what the kernel indexes; asserted: the totals are those
formulas' (bucket membership and the launches' LDS do not move), no two arrays of one memory overlap, each is aligned for its
element type (cnt 8, the 32-bit arrays 4, insg 2, the string and the cigar 4 because they are staged by dwords), and each ends
inside its total."""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent / "host_msa_layout"
LQ = (1, 63, 64, 65, 250, 1024, 3500)
N_STR = (0, 1, 7, 64, 1000)
NW = (1, 2, 4, 8)
K_MAX_INS, K_MAX_INS_GLOBAL, K_XCHG_WORDS = 256, 4096, 96


def old_small_bytes(n_str):
    return K_XCHG_WORDS * 4 + K_MAX_INS_GLOBAL * 7 + (n_str + 2) * 8


def old_lds_bytes(w_cols, lq, str_cap, ops_cap, n_str, nw):
    W, E = w_cols, n_str + 2
    o = K_XCHG_WORDS * 4 if nw > 1 else 0
    o += W * 8                      # cnt
    o += E * 8                      # lead, size
    o += (lq + 2) * 4               # bpos
    o += K_MAX_INS * 4              # insx
    o += K_MAX_INS * 2              # insg
    o += K_MAX_INS                  # inss
    o += (W + 3) & ~3               # T
    o += (W + 3) & ~3               # Rw
    o += (str_cap + 7) & ~3         # S
    o += (ops_cap + 3) & ~3         # ops
    return o


@pytest.fixture(scope="module")
def rows():
    r = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building tests/host_msa_layout failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    r = subprocess.run([str(HERE / "_build" / "msa_layout_host")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [{k: int(v) for k, v in (f.split("=") for f in line.split())} for line in r.stdout.splitlines()]
    assert {(d["lq"], d["n_str"], d["nw"], d["global"]) for d in out} == {(a, b, c, g) for a in LQ for b in N_STR for c in NW for g in (0, 1)}
    assert len(out) == len(LQ) * len(N_STR) * len(NW) * 2
    return out


def arrays(d):
    """(name, memory, offset, bytes the kernel indexes, alignment) of every array of the row's variant."""
    split = d["global"] == 1 and d["nw"] > 1                      # the small arrays in LDS, the per-column ones in the workspace slot
    ki = K_MAX_INS_GLOBAL if split else K_MAX_INS
    assert d["max_ins"] == ki and d["xchg_words"] == K_XCHG_WORDS
    W, E = d["w_cols"], d["n_str"] + 2
    small, cols = "small", ("cols" if split else "small")
    a = [("insx", small, d["insx"], ki * 4, 4), ("insg", small, d["insg"], ki * 2, 2), ("inss", small, d["inss"], ki, 1),
         ("lead", small, d["lead"], E * 4, 4), ("size", small, d["size"], E * 4, 4),
         ("cnt", cols, d["cnt"], W * 8, 8), ("bpos", cols, d["bpos"], (d["lq"] + 2) * 4, 4), ("T", cols, d["T"], W, 1), ("Rw", cols, d["Rw"], W, 1),
         # the string is staged from the aligned address at or below its start: up to 3 bytes in front of it, whole dwords
         ("S", cols, d["S"], (3 + d["str_cap"] + 3) // 4 * 4, 4), ("ops", cols, d["ops"], (d["ops_cap"] + 3) // 4 * 4, 4)]
    if d["nw"] > 1:
        a.append(("xchg", small, d["xchg"], K_XCHG_WORDS * 4, 4))
    return split, a


def test_totals_are_the_former_formulas(rows):
    for d in rows:
        shape = (d["w_cols"], d["lq"], d["str_cap"], d["ops_cap"], d["n_str"])
        if d["global"] == 0:
            assert d["total"] == old_lds_bytes(*shape, d["nw"]), d
        elif d["nw"] == 1:
            assert d["total"] == old_lds_bytes(*shape, 1), d       # one wavefront keeps everything in its slot
        else:
            assert d["small_total"] == old_small_bytes(d["n_str"]), d
            # the slot holds the per-column arrays alone: the former sum less the exchange words and the small arrays it counted;
            # the host still sizes the slot by dp_msa_lds_bytes(.., nw)
            assert d["total"] == old_lds_bytes(*shape, d["nw"]) - K_XCHG_WORDS * 4 - K_MAX_INS * 7 - (d["n_str"] + 2) * 8, d


def test_arrays_are_disjoint_aligned_and_inside(rows):
    for d in rows:
        split, arr = arrays(d)
        for name, mem, off, size, align in arr:
            assert off % align == 0, (name, d)
            # lead / size: with the small arrays, but in LDS with several wavefronts behind everything else
            tail = d["global"] == 0 and d["nw"] > 1
            small = name in ("xchg", "insx", "insg", "inss") or (name in ("lead", "size") and not tail)
            assert off + size <= (d["small_total"] if small else d["total"]), (name, d)
            assert small or split or off >= d["small_total"], (name, d)   # one region: the per-column arrays behind the small ones
        for mem in ("small", "cols"):
            spans = sorted((off, off + size, name) for name, m, off, size, _ in arr if m == mem and size)
            for (_, e0, n0), (b1, _, n1) in zip(spans, spans[1:]):
                assert e0 <= b1, (n0, n1, d)
