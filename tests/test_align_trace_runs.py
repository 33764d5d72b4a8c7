"""The traceback of dp_align_kernel (csrc/dp_align.hip) a run at a time against the step-by-step walk, on random code matrices -- CPU only.

Both sides are Python twins written from the kernel's statements.  `walk_steps` is the walk one cell per trip: the 2-bit code of the
cell, the homopolymer tests and the mismatch test from the two sequences, one entry of the step table, one op.  `walk_runs` is the loop
the kernel runs: the 16 columns of the trace window are evaluated by the lanes (c << 2 | r >> 6) all at once, each as if the walk stood
in its column on the current diagonal; ballots give the M run from the current column downward and the mismatches inside it, and the
trip takes the run, cut by its limits (ti and tj stay positive before each step, the columns stay in the 16-column window, the rows
in the 64-row window of s2, the ops do not pass the next flush of 64, and 15 steps), and the I or D step behind it where that one is inside the limits
too.  The twin keeps the lane layout, the wrapping cross-lane read, the shifts and the masks, so an off-by-one in any of them shows as a
different path.  What this checks is the derivation; the HIP code itself is held to the oracle by tests/test_gpu_dp_align_runs.py."""
import random

import pytest

MASK64 = (1 << 64) - 1


def dir_finish(A, B, h1, h2):
    """dp_dir_finish without the mismatch: 0 = M, 2 = I, 3 = D."""
    if h2:
        return 2 if A else 3 if B else 0
    if h1:
        return 3 if B else 2 if A else 0
    return 0 if A else 3 if B else 2


STEP_TABLE = 0
for _m in range(16):
    _d = dir_finish(_m & 1, _m & 2, _m & 4, _m & 8)
    STEP_TABLE |= (3 if _d == 0 else 2 if _d == 2 else 1) << (2 * _m)


class Job:
    """Two sequences, a band and a matrix of 2-bit codes codes[i][r] for the columns 0 .. L1 + 16 (a trace window reads 16 columns from a
    multiple of 16, so up to 15 beyond the last one; their codes are whatever the memory holds) and the band rows 0 .. 255."""

    def __init__(self, s1, s2, origin, bw, codes):
        self.s1, self.s2, self.origin, self.bw, self.codes = s1, s2, origin, bw, codes
        self.L1, self.L2 = len(s1), len(s2)

    def S1(self, i):
        return self.s1[i] if i < self.L1 else 4

    def S2(self, j):
        return self.s2[j] if 0 <= j < self.L2 else 4


def walk_steps(J, ti, tj):
    ops, edit, bad = [], 0, False
    while ti > 0 and tj > 0:
        r = tj - J.origin - ti
        if not 0 <= r < J.bw:
            bad = True
            break
        ab = J.codes[ti][r]
        c, e = J.S1(ti - 1), J.S2(tj - 1)
        h1, h2 = c == J.S1(ti), e == J.S2(tj)
        step = (STEP_TABLE >> (2 * (ab | h1 << 2 | h2 << 3))) & 3
        edit += 1 if step != 3 or c != e else 0
        ti -= step & 1
        tj -= step >> 1
        ops.append(" DIM"[step])
    return "".join(ops), edit, ti, tj, bad


def ballot(bits):
    return sum(1 << l for l in range(64) if bits[l])


def clz64(x):
    return 64 - x.bit_length()


def walk_runs(J, ti, tj):
    ops, edit, bad, trips = [], 0, False, 0
    wb, s2_base = -1, 0x40000000
    words = v1 = v2 = None
    while ti > 0 and tj > 0:
        r = tj - J.origin - ti
        if not 0 <= r < J.bw:
            bad = True
            break
        if (ti & ~15) != wb:
            wb = ti & ~15
            # lane (c << 2 | q), word d: band rows 64 q + 16 d .. of column wb + c, two bits each
            words = [[sum(J.codes[wb + (l >> 2)][64 * (l & 3) + 16 * d + t] << (2 * t) for t in range(16)) for d in range(4)] for l in range(64)]
            v1 = []
            for l in range(64):
                x = min(max(wb + (l >> 2), 1), J.L1)
                v1.append(J.S1(x - 1) << 4 | (4 if J.S1(x - 1) == J.S1(x) else 0))
        wcur = [words[l][(r >> 4) & 3] for l in range(64)]
        if not 0 <= tj - 1 - s2_base <= 63:
            s2_base = tj - 64
            v2 = [J.S2(s2_base + l) << 4 | (8 if J.S2(s2_base + l) == J.S2(s2_base + l + 1) else 0) for l in range(64)]
        trips += 1
        col, t0 = ti - wb, tj - 1 - s2_base
        step, x = [0] * 64, [0] * 64
        for l in range(64):
            ab = (wcur[l] >> (2 * (r & 15))) & 3
            x[l] = v1[l] ^ v2[(((l & ~3) + 4 * (t0 - col)) >> 2) & 63]               # ds_bpermute: the lane index wraps
            step[l] = (STEP_TABLE >> (2 * (ab | (x[l] & 12)))) & 3
        up = 63 - (col << 2 | r >> 6)
        mine = (0x1111111111111111 << (r >> 6)) & MASK64
        stop = ((ballot([s != 3 for s in step]) & mine) << up) & MASK64
        mism = ((ballot([v > 15 for v in x]) & mine) << up) & MASK64
        ins = (ballot([s == 2 for s in step]) << up) & MASK64
        run = clz64(stop | 1) >> 2
        lim = min(ti, tj, 64 - (len(ops) & 63), col + 1, t0 + 1, 15)             # 15: what the guard bit lets `run` tell
        assert lim >= 1
        n = min(run, lim)
        other = 1 if run < lim else 0
        is_i = other & (((ins << (4 * run)) & MASK64) >> 63)
        edit += other + bin((mism >> 4) >> (60 - 4 * n)).count("1")
        ti -= n + (other ^ is_i)
        tj -= n + is_i
        ops.extend("M" * n + ("I" if is_i else "D") * other)
    return "".join(ops), edit, ti, tj, bad, trips


def _seq(rng, n, letters, longest):
    out = []
    while len(out) < n:
        out.extend([rng.choice(letters)] * rng.randint(1, longest))
    return out[:n]


def _job(rng, kind):
    L1 = rng.choice([1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 100, 129, 200, 300])
    L2 = max(1, L1 + rng.randint(-20, 20))
    bw = rng.choice([3, 41, 201, 255])
    letters, longest = rng.choice([([0], 1), ([0, 1], 3), ([0, 1, 2, 3], 1), ([0, 1, 2, 3], 6)])
    s1, s2 = _seq(rng, L1, letters, longest), _seq(rng, L2, letters, longest)
    if kind == "all_m":                                       # code 1 = "the diagonal ties" where no homopolymer test holds: no equal neighbours
        s1, s2 = [i & 1 for i in range(L1)], [j & 1 for j in range(L2)]
        code = lambda i, r: 1
    elif kind == "no_m":                                      # without a test code 0 is I and code 2 ("left ties") is D
        s1, s2 = [i & 1 for i in range(L1)], [j & 1 for j in range(L2)]
        code = lambda i, r: 2 if (i + r) % 3 else 0
    elif kind == "alternating":
        code = lambda i, r: 1 if (2 * i + r) % 2 == 0 else 2
    elif kind == "mostly_m":
        code = lambda i, r: 1 if rng.random() < 0.9 else rng.randint(0, 3)
    else:
        code = lambda i, r: rng.randint(0, 3)
    codes = [[code(i, r) for r in range(256)] for i in range(((L1 + 16) | 15) + 1)]
    origin = rng.randint(-2, 2) - bw // 2 - 1 + rng.choice([0, 0, L2 - L1])
    return Job(s1, s2, origin, bw, codes)


@pytest.mark.parametrize("kind", ["all_m", "no_m", "alternating", "mostly_m", "random"])
def test_run_trips_walk_the_serial_path(kind):
    rng = random.Random({"all_m": 1, "no_m": 2, "alternating": 3, "mostly_m": 4, "random": 5}[kind])
    walked = steps = trips = 0
    for _ in range(60):
        J = _job(rng, kind)
        starts = [(J.L1, J.L2), (J.L1, rng.randint(1, J.L2)), (rng.randint(1, J.L1), J.L2)]
        for ti, tj in starts:
            r = tj - J.origin - ti
            if not 0 <= r < J.bw:                               # start inside the band, as the kernel's best cell is
                tj = min(max(J.origin + ti + rng.randint(0, J.bw - 1), 1), J.L2)
            want = walk_steps(J, ti, tj)
            got = walk_runs(J, ti, tj)
            assert got[:5] == want, (kind, J.L1, J.L2, J.origin, J.bw, ti, tj)
            walked += 1
            steps += len(want[0])
            trips += got[5]
    assert walked and steps
    if kind == "all_m":
        assert steps > 6 * trips                                # whole windows at a time
    if kind == "no_m":
        assert steps == trips                                   # and one step where no cell says M
