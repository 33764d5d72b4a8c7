"""ctypes loader of tests/host_saipb (TEST INFRASTRUCTURE ONLY): the product's seed-pair merge (csrc/saipb_device.h) compiled for
the host and run with one lane."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from longreadselfcorrect_amd.capi import SaipbResult, saipb_pair_jobs, saipb_pair_results

HERE = Path(__file__).resolve().parent / "host_saipb"
SO = HERE / "_build" / "liblrsc_host_saipb.so"


def build():
    r = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building tests/host_saipb failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i


def codes_of(s: bytes) -> np.ndarray:
    c = _CODE[np.frombuffer(s, dtype=np.uint8)]
    assert c.max(initial=0) < 4
    return np.ascontiguousarray(c)


class HostSaipb:
    def __init__(self):
        build()
        self.lib = L = C.CDLL(str(SO))
        L.hs_index_create.restype = C.c_void_p
        L.hs_index_create.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_int]
        L.hs_index_free.argtypes = [C.c_void_p]
        L.hs_saipb_merge.restype = C.c_int
        L.hs_saipb_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.hs_saipb_align.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]

    def index(self, bwt_units, rbwt_units, num_symbols, wide=False, tables=()):
        a = np.ascontiguousarray(bwt_units, dtype=np.uint8)
        b = np.ascontiguousarray(rbwt_units, dtype=np.uint8)
        ks = np.ascontiguousarray(list(tables), dtype=np.int32)
        h = self.lib.hs_index_create(_p(a), a.size, _p(b), b.size, num_symbols, int(wide), _p(ks), ks.size)
        assert h, "hs_index_create failed"
        return h

    def index_free(self, h):
        self.lib.hs_index_free(h)

    def merge(self, h, seq: bytes, seeds, jobs):
        """The records of lrsc_saipb_merge -> (status, results, seed_freq, arena)."""
        codes = codes_of(seq)
        res = (SaipbResult * max(len(jobs), 1))()
        freq = np.zeros(max(len(seeds), 1), dtype=np.uint64)
        cap = 2 * len(seq) + 4096
        arena = C.create_string_buffer(cap)
        used = C.c_uint64()
        st = self.lib.hs_saipb_merge(h, _p(codes), codes.size, seeds, len(seeds), jobs, len(jobs), res, _p(freq), arena, cap, C.byref(used))
        return st, res, freq, arena.raw[: used.value]

    def merge_pairs(self, h, pairs, max_leaves=32):
        """pairs of (source, between, target, dis) -> [(code, merged, stats, status)], the shape of oracle.saipb_merge + status."""
        seq, seeds, jobs = saipb_pair_jobs(pairs, max_leaves)
        st, res, freq, arena = self.merge(h, seq, seeds, jobs)
        assert st == 0, st
        return saipb_pair_results(pairs, res, freq, arena)

    def align(self, s1: str, s2: str):
        a, b = codes_of(s1.encode()), codes_of(s2.encode())
        out = (C.c_int * 3)()
        self.lib.hs_saipb_align(_p(a), a.size, _p(b), b.size, out)
        return int(out[0]), int(out[1]), int(out[2])
