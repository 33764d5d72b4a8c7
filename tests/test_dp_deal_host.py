"""csrc/dp_deal.h deals the MSA launches of a pass to the DP stage's side streams: by estimated work, the largest first, each to the
stream with the least so far; inside a stream the widest LDS first ("A part's DP stage beside the other part's
kernels").  It is plain host C++, so it is checked here without a device: tests/host_dp_deal/dp_deal_check.cpp (a program of its
own) is built with AddressSanitizer and UBSan and run.  It feeds seeded random launch sets and the edge cases -- no launches, one
launch, more streams than launches, equal weights, zero weights, no streams, weights whose sum passes 64 bits -- and holds that every
launch is dealt exactly once, that a stream runs its launches widest LDS first, and that the most loaded stream carries at most the
mean load plus the largest launch (the bound of the greedy deal)."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "longreadselfcorrect_amd" / "csrc"
SRC = ROOT / "tests" / "host_dp_deal" / "dp_deal_check.cpp"


def test_dp_deal(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host check"
    exe = tmp_path / "dp_deal_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", f"-I{CSRC}", str(SRC), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, f"building {SRC.name} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), f"{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


def test_dp_deal_header_has_no_hip():
    """The header compiles for the host alone, and the DP stage deals its MSA launches with it."""
    text = (CSRC / "dp_deal.h").read_text()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text
    assert '#include "dp_deal.h"' in (CSRC / "capi_dp.cpp").read_text() and "dp_deal(" in (CSRC / "capi_dp.cpp").read_text()
