"""What a band column of dp_align_kernel (dp_align.hip) costs, checked on the CPU from the code object inside the build.

The fill stores two score comparisons per cell and the traceback finishes the decision tree at the cells it visits, so a column of
the fill is the recurrence, two compares and a select per cell and the packing of the eight bits.  The columns are located by their
scans as in test_align_kernel_build.py (v_max_i32 with the row_bcast:31 DPP step): the interior turn is four columns of straight-line
code, so the smallest distance between consecutive scans is one interior column.  `llvm-objdump -d --no-show-raw-insn` counted 165
instructions there (103 VALU) while the fill built the whole decision per cell; the bound is two thirds of that, above the 80-95 the
operation count gives to leave the compiler's scheduling room.  75 to 86 in the interior turn when this was written."""
from __future__ import annotations

import re
import subprocess

import pytest

from .test_align_kernel_build import LLVM, _code_object, _sym

COLUMN_BEFORE = 165
COLUMN_MAX = 110


@pytest.mark.parametrize("global_stage", [False, True])
def test_align_kernel_column_length(tmp_path, global_stage):
    out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={_sym(global_stage)}",
                          str(_code_object(tmp_path))], check=True, capture_output=True, text=True).stdout
    ins = [l for l in out.splitlines() if re.match(r"^\s+[a-z_0-9]+\s", l)]
    scans = [k for k, l in enumerate(ins) if "row_bcast:31" in l]
    assert len(scans) == 8, [ins[k] for k in scans]
    column = min(b - a for a, b in zip(scans, scans[1:]))
    print(f"global_stage={global_stage}: scans at {scans}, shortest column {column} instructions (was {COLUMN_BEFORE})")
    assert column <= COLUMN_MAX, (column, scans)
