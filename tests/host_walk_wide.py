"""ctypes loader of tests/host_walk_wide (TEST INFRASTRUCTURE ONLY): the product's wide walk (csrc/walk_device.h, Walk<WIDE, true>)
compiled for the host; the index half is tests/host_walk's."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.host_walk import _CODE, HostWalk, HwParams, _p

HERE = Path(__file__).resolve().parent / "host_walk_wide"
SO = HERE / "_build" / "liblrsc_host_walk_wide.so"


def build():
    r = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building tests/host_walk_wide failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")


class HostWalkWide(HostWalk):
    def __init__(self):
        build()
        self.lib = L = C.CDLL(str(SO))
        L.hw_index_create.restype = C.c_void_p
        L.hw_index_create.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_int]
        L.hw_index_free.argtypes = [C.c_void_p]
        L.hww_extend_walk.restype = C.c_int
        L.hww_extend_walk.argtypes = [C.c_void_p, C.POINTER(HwParams), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                      C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32)]

    def extend_walk_wide(self, h, params, src, path, trg, dis, initk, max_overlap, min_sa, mode):
        """-> (code, mergedSeq, steps, widest frontier) of Walk<WIDE, true> with capacity params.max_leaves; mode 0 = Walk::run,
        1 = the wide kernel's loop (single-leaf fast path with hand-over)."""
        hp = HwParams(params.idmer_len, params.min_kmer_len, params.max_leaves, params.pb_coverage, params.error_rate)
        q = (src[len(src) - initk:] + path + trg).encode()
        codes = _CODE[np.frombuffer(q, dtype=np.uint8)]
        assert codes.max(initial=0) < 4
        cap = 2 * len(q) + 4096
        out = np.zeros(cap, dtype=np.uint8)
        n, steps, front = C.c_uint32(), C.c_uint32(), C.c_uint32()
        code = self.lib.hww_extend_walk(h, C.byref(hp), _p(codes), initk, len(path), len(trg), dis, max_overlap, min_sa, mode, _p(out), cap,
                                        C.byref(n), C.byref(steps), C.byref(front))
        merged = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[out[: n.value]]).decode()
        return code, merged, steps.value, front.value
