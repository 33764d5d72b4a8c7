"""Walk::begin_static (csrc/walk_device.h) sorts an interval list only when an idmer code repeats among its valid entries.  The
harness tests/host_begin compiles that header for the host and, per query, builds the tables with every list sorted
(LRSC_WP_BEGIN_SORT, the behaviour before) and by the default rule, and holds them against each other (begin_host.hip, hb_check):
along every bucket chain the val sequence filtered by code -- all seed_support_core can read -- is the same for every code present
on both strands, and a list with a repeated code is byte-identical to the always-sorted arrays.

The keys keep what the argument at build9 rests on: valid entries have equal keys exactly when they have equal codes (an injective
map of the code per strand, like the start of a k-mer's suffix-array interval)."""
from __future__ import annotations

import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent / "host_begin"
SO = HERE / "_build" / "liblrsc_host_begin.so"
SAN = HERE / "_build" / "begin_host_san"
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
SEED = 9


@pytest.fixture(scope="module")
def lib():
    r = subprocess.run(["make", "-C", str(HERE)], capture_output=True, text=True)
    assert r.returncode == 0, f"building tests/host_begin failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    L = C.CDLL(str(SO))
    L.hb_check.restype = C.c_int
    L.hb_check.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _codes_of(q, seed=SEED):
    n9 = max(len(q) - seed + 1, 0)
    c = np.zeros(n9, dtype=np.uint64)
    for t in range(seed):
        c = (c << np.uint64(2)) | q[t: t + n9].astype(np.uint64)
    return c


def _keys(q, valid_f, valid_r, seed=SEED):
    """Interval starts: injective in the code (odd multiplier modulo 2^40), different per strand; kNoKey where invalid."""
    c = _codes_of(q, seed)
    kf = (c * np.uint64(0x9E3779B1) + np.uint64(12345)) & np.uint64((1 << 40) - 1)
    kr = (c * np.uint64(0x85EBCA6B) + np.uint64(7)) & np.uint64((1 << 40) - 1)
    kf[~valid_f] = NO_KEY
    kr[~valid_r] = NO_KEY
    return kf, kr


def _case(q, valid_f=None, valid_r=None, seed=SEED):
    q = np.ascontiguousarray(q, dtype=np.uint8)
    n9 = max(len(q) - seed + 1, 0)
    vf = np.ones(n9, dtype=bool) if valid_f is None else np.asarray(valid_f, dtype=bool)
    vr = np.ones(n9, dtype=bool) if valid_r is None else np.asarray(valid_r, dtype=bool)
    kf, kr = _keys(q, vf, vr, seed)
    return q, seed, kf, kr


def _expected(case):
    q, seed, kf, kr = case
    c = _codes_of(q, seed)
    out = []
    for k in (kf, kr):
        v = c[k != NO_KEY]
        out.append((len(v), int(len(np.unique(v)) != len(v))))
    return out


def _random_query(rng, n, letters):
    return rng.integers(0, letters, size=n + SEED - 1 if n else SEED - 1, dtype=np.uint8)


def all_cases():
    """Every input of the suite, from a fixed seed: (name, case)."""
    rng = np.random.default_rng(0xB391)
    cases = []
    # n valid entries x alphabet: homopolymer, two letters (tandem-repeat rich), four letters
    for n in (0, 1, 2, 16, 17, 33, 300, 3000):
        for letters in (1, 2, 4):
            cases.append((f"n{n}_a{letters}", _case(_random_query(rng, n, letters))))
        # the same number of valid entries among invalid ones (compaction moves entries)
        q = _random_query(rng, 2 * n + 5, 4)
        n9 = len(q) - SEED + 1
        valid = np.zeros(n9, dtype=bool)
        valid[rng.permutation(n9)[:n]] = True
        cases.append((f"n{n}_sparse", _case(q, valid, np.roll(valid, 3))))
    cases.append(("shorter_than_seed", _case(np.zeros(SEED - 1, dtype=np.uint8))))
    cases.append(("empty", _case(np.zeros(0, dtype=np.uint8))))
    # exact tandem repeats of period 1..12 (period >= seed: the repeat is one code apart by the period)
    for period in (2, 3, 7, 9, 12):
        unit = rng.integers(0, 4, size=period, dtype=np.uint8)
        cases.append((f"tandem{period}", _case(np.tile(unit, 400 // period + 2))))
    # a repeat only at the two ends of the query: a de Bruijn-free middle from distinct codes
    for n in (40, 300, 3000):
        q = _distinct_query(rng, n)
        q[-SEED:] = q[:SEED]
        cases.append((f"ends{n}", _case(q)))
        cases.append((f"distinct{n}", _case(_distinct_query(rng, n))))
    # a repeated code whose entries are invalid on one strand only
    q = _distinct_query(rng, 300)
    q[150: 150 + SEED] = q[20: 20 + SEED]
    n9 = len(q) - SEED + 1
    inv = np.ones(n9, dtype=bool)
    c = _codes_of(q)
    inv[c == c[20]] = False
    assert (~inv).sum() == 2
    cases.append(("repeat_invalid_fwd", _case(q, inv, None)))
    cases.append(("repeat_invalid_rvc", _case(q, None, inv)))
    one = np.ones(n9, dtype=bool)
    one[150] = False
    cases.append(("repeat_one_copy_invalid_fwd", _case(q, one, None)))
    # 2 000 random queries: the bench's lengths (most without a repeat), validity like a real strand (most offsets valid)
    for i in range(2000):
        n = int(rng.integers(1, 600))
        q = _random_query(rng, n, 4)
        n9 = len(q) - SEED + 1
        cases.append((f"random{i}", _case(q, rng.random(n9) < 0.9, rng.random(n9) < 0.9)))
    return cases


def _distinct_query(rng, n):
    """n + SEED - 1 letters in which no SEED-mer occurs twice (rejection by position)."""
    while True:
        q = rng.integers(0, 4, size=n + SEED - 1, dtype=np.uint8)
        c = _codes_of(q)
        for _ in range(64):
            u, first, counts = np.unique(c, return_index=True, return_counts=True)
            if (counts == 1).all():
                return q
            dup = np.setdiff1d(np.arange(len(c)), first)
            q[dup + SEED // 2] = rng.integers(0, 4, size=len(dup), dtype=np.uint8)
            c = _codes_of(q)


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def _check(lib, case):
    q, seed, kf, kr = case
    nv = (C.c_uint32 * 2)()
    rp = (C.c_uint32 * 2)()
    r = lib.hb_check(q.ctypes.data_as(C.c_void_p), len(q), seed, kf.ctypes.data_as(C.c_void_p), kr.ctypes.data_as(C.c_void_p), nv, rp)
    return r, [(nv[0], rp[0]), (nv[1], rp[1])]


def test_tables_by_rule_equal_tables_always_sorted(lib, cases):
    n_lists = n_rep = 0
    for name, case in cases:
        r, got = _check(lib, case)
        assert r == 0, f"{name}: hb_check = {r} (10 * property + strand, see begin_host.hip)"
        assert got == _expected(case), name
        n_lists += 2
        n_rep += got[0][1] + got[1][1]
    # both classes are exercised, and the random queries are mostly repeat-free like the bench's
    assert n_rep > 100 and n_lists - n_rep > 2000


def test_named_cases_take_the_expected_path(lib, cases):
    by = dict(cases)
    want = {
        "n0_a4": [(0, 0), (0, 0)], "n1_a1": [(1, 0), (1, 0)], "n2_a1": [(2, 1), (2, 1)], "n3000_a1": [(3000, 1), (3000, 1)],
        "n300_a2": [(300, 1), (300, 1)], "distinct3000": [(3000, 0), (3000, 0)], "ends300": [(300, 1), (300, 1)],
        "ends3000": [(3000, 1), (3000, 1)], "repeat_invalid_fwd": [(298, 0), (300, 1)], "repeat_invalid_rvc": [(300, 1), (298, 0)],
        "repeat_one_copy_invalid_fwd": [(299, 0), (300, 1)], "shorter_than_seed": [(0, 0), (0, 0)], "empty": [(0, 0), (0, 0)],
        "n17_sparse": None, "n33_sparse": None,
    }
    for name, w in want.items():
        r, got = _check(lib, by[name])
        assert r == 0, name
        if w is not None:
            assert got == w, name
        else:
            assert got[0][0] == int(name[1:3]) and got[1][0] == int(name[1:3]), name


def test_same_cases_under_address_and_ub_sanitizer(lib, cases, tmp_path):
    """The stand-alone build of the harness (its own main, -fsanitize=address,undefined) over the same cases."""
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, (q, seed, kf, kr) in cases:
            f.write(struct.pack("<II", len(q), seed))
            f.write(q.tobytes()); f.write(kf.tobytes()); f.write(kr.tobytes())
    r = subprocess.run([str(SAN), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert f"{len(cases)} cases ok" in r.stdout
