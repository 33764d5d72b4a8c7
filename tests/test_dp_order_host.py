"""csrc/dp_order.h builds the job lists that the align launches' wavefronts draw from: one list per staging-size class, in index
order (longest first was measured and lost, DESIGN.md section 4b "Alignments from a queue").  It is plain host C++, so it is checked here without a device: tests/host_dp_order/dp_order_check.cpp (a program of
its own) is built with AddressSanitizer and UBSan and run.  It feeds seeded random request sets (1-300 requests of 0-40 strings, column
counts over all four classes, as requests and as single jobs) and the edge cases -- an empty set, requests without strings, one job, a
class with no jobs, all jobs in one class, the class bounds -- and holds that every job index appears exactly once, that class k's
list holds exactly the jobs of class k by dp_align_class, and that every list is in index order."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "longreadselfcorrect_amd" / "csrc"
SRC = ROOT / "tests" / "host_dp_order" / "dp_order_check.cpp"


def test_dp_order_lists(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host check"
    exe = tmp_path / "dp_order_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", f"-I{CSRC}", str(SRC), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, f"building {SRC.name} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), f"{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


def test_dp_order_header_has_no_hip():
    """The header compiles for the host alone: it includes nothing of HIP, and dp_dev.h takes the classes from it."""
    text = (CSRC / "dp_order.h").read_text()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text
    assert '#include "dp_order.h"' in (CSRC / "dp_dev.h").read_text()
