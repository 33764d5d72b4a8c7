"""The pile-up kernel's passes in a workgroup of several wavefronts (csrc/dp_msa.hip, msa_pileup with NW > 1) against the
step-by-step cigar walk -- CPU only, as tests/test_msa_row_passes.py holds the single-wavefront derivation.

`add_row_wide` is a Python twin of msa_pileup's row, written from the kernel's statements with the wavefront width and the number of
wavefronts as parameters: every pass goes chunk by chunk of width x NW entries, every wavefront ballots its own `width` entries,
posts its counts, and a thread adds up the wavefronts in front of its own; the carries (bases seen, M/D and M/I ops, new columns,
the position behind the last M/D op) are the sums over all wavefronts.  At widths of 4 and 8 lanes and 1-4 wavefronts every
boundary is crossed many times in a 30-base row: runs of I that start in one wavefront's chunk and end in the next one's or in
the next trip, chunks without any M/D op, and n_ops, size_b - ti0 and nout one below, at and one above a multiple of
width x NW.  The state after every row must equal the walk's.  The right shift moves `shift_chunks` chunks per barrier pair from
the top down, as the kernel does.  One planted break (the position behind the last M/D op not carried across wavefronts) must be
caught."""
import random

import pytest

from tests.test_msa_row_passes import GAP, UNSET, Pile, add_row_walk, random_row


def popc_before(mask, lane):
    return sum(mask[:lane])


def add_row_wide(p, m0s, m1s, ops, S, stats, width, nw, shift_chunks=2, max_ins=256, drop_run_carry=False):
    """msa_pileup's row in a workgroup of nw wavefronts; False when the row must take the walk (nothing but scratch has been touched
    then)."""
    NT = width * nw
    n_ops = len(ops)
    size_b = p.size_b
    T = p.T

    def exchange(flags):
        """per-wavefront ballots of one chunk: (mask of the thread's own wavefront, counts per wavefront)"""
        masks = [flags[w * width:(w + 1) * width] for w in range(nw)]
        return masks, [sum(m) for m in masks]

    # getPaddedPositionOfBase(m0s)
    ti, seen = 0, 0
    for base in range(0, size_b, NT):
        ng = [base + t < size_b and T[base + t] != GAP for t in range(NT)]
        masks, cnts = exchange(ng)
        if seen + sum(cnts) > m0s:
            hits = [base + t for t in range(NT)
                    if ng[t] and seen + sum(cnts[:t // width]) + popc_before(masks[t // width], t % width) == m0s]
            assert len(hits) == 1
            ti = hits[0]
            break
        seen += sum(cnts)
    if n_ops == 0 or (ti == 0 and ops[0] == 'I'):
        return False
    ti0, tl = ti, p.lead_b
    il = ti0 + tl
    stats["edge"].add(("span", NT, (size_b - ti0) % NT, (size_b - ti0) >= NT - 1))

    # bases from ti0 on
    bpos, Rw, nbr = {}, {}, 0
    for base in range(ti0, size_b, NT):
        ng = [base + t < size_b and T[base + t] != GAP for t in range(NT)]
        masks, cnts = exchange(ng)
        for t in range(NT):
            i = base + t
            if ng[t]:
                bpos[nbr + sum(cnts[:t // width]) + popc_before(masks[t // width], t % width)] = i
            if i < size_b:
                Rw[i] = UNSET if ng[t] else GAP
        nbr += sum(cnts)
    bpos[nbr] = size_b

    # the cigar
    md_tot = mi_tot = st_tot = run_carry = 0
    insx, inss, last_y, written = {}, {}, None, set()
    for cb in range(0, n_ops, NT):
        op = [ops[cb + t] if cb + t < n_ops else None for t in range(NT)]
        isMD = [o in ('M', 'D') for o in op]
        isMI = [o in ('M', 'I') for o in op]
        mMD, nMD = exchange(isMD)
        mMI, nMI = exchange(isMI)
        # position behind each wavefront's last M/D op (0: none)
        wave_last = [0] * nw
        for w in range(nw):
            for l in range(width):
                if mMD[w][l]:
                    wave_last[w] = cb + w * width + l + 1
        if any(not any(m) for w, m in enumerate(mMD) if cb + w * width < n_ops):
            stats["md_free_chunks"] += 1
        carry_all = run_carry
        for w in range(nw):
            if wave_last[w]:
                carry_all = wave_last[w]
        st, fill, ys, syms, bad = [False] * NT, [False] * NT, [0] * NT, [0] * NT, False
        for t in range(NT):
            if op[t] is None:
                continue
            w, l = t // width, t % width
            j = cb + t
            carry_before = run_carry
            if not drop_run_carry:
                for x in range(w):
                    if wave_last[x]:
                        carry_before = wave_last[x]
            brel = md_tot + sum(nMD[:w]) + popc_before(mMD[w], l)
            inc = m1s + mi_tot + sum(nMI[:w]) + popc_before(mMI[w], l)
            lower = [k for k in range(l) if mMD[w][k]]
            run_start = cb + w * width + lower[-1] + 1 if lower else carry_before
            i_rank = j - run_start
            if run_start < cb + w * width and op[t] == 'I' and i_rank > 0:
                stats["runs_across_waves"] += 1
            if op[t] not in ('M', 'D', 'I') or brel >= nbr:
                bad = True
                continue
            pb = bpos[brel]
            if op[t] == 'I':
                G, y = 0, 0
                if brel > 0:
                    pp = bpos[brel - 1]; G = pb - pp - 1; y = pp + 1 + i_rank
                fill[t] = i_rank < G; st[t] = not fill[t]
                if st[t]:
                    y = pb - 1
            else:
                y = pb
            ys[t] = y
            syms[t] = (S[inc] if inc < len(S) else 0) if op[t] in ('M', 'I') else GAP
        mS, nS = exchange(st)
        if bad or st_tot + sum(nS) > max_ins:
            return False
        for t in range(NT):
            if op[t] is None:
                continue
            w, l = t // width, t % width
            if op[t] in ('M', 'D') or fill[t]:
                assert ys[t] not in written, "two ops of one row write the same position"
                written.add(ys[t])
                Rw[ys[t]] = syms[t]
            if st[t]:
                k = st_tot + sum(nS[:w]) + popc_before(mS[w], l)
                insx[k] = ys[t] + 1; inss[k] = syms[t]
            if cb + t == n_ops - 1:
                last_y = ys[t]
        md_tot += sum(nMD); mi_tot += sum(nMI); st_tot += sum(nS)
        run_carry = carry_all
    stats["edge"].add(("n_ops", NT, n_ops % NT, n_ops >= NT - 1))

    nin = st_tot
    stats["ins"] += nin
    if nin:
        xs = [insx[k] for k in range(nin)]
        assert xs == sorted(xs)
        insg = [sum(1 for le, se in zip(p.lead, p.size) if le < x + tl and x + tl - le < se) for x in xs]
        for e in range(len(p.lead)):
            le, se = p.lead[e], p.size[e]
            p.lead[e] = le + sum(1 for x in xs if x + tl <= le)
            p.size[e] = se + sum(1 for x in xs if le < x + tl and x + tl - le < se)
        # the right shift: from the top down, shift_chunks x NT columns read, a barrier, and written
        x0 = xs[0]
        T.extend([None] * nin)
        hi = size_b
        while hi > x0:
            n = min(hi - x0, NT * shift_chunks)
            block = []
            for idx in range(n):
                yy = hi - 1 - idx
                block.append((yy, p.cnt.get(yy + tl, [0, 0, 0, 0, 0]), T[yy], Rw[yy], sum(1 for x in xs if x <= yy)))
            for yy, v, t_, r_, sh in block:
                if sh:
                    p.cnt[yy + sh + tl] = v; T[yy + sh] = t_; Rw[yy + sh] = r_
            hi -= n
        for k in range(nin):
            np_ = xs[k] + k
            T[np_] = GAP; Rw[np_] = inss[k]
            p.cnt[np_ + tl] = [0, 0, 0, 0, insg[k] + 1]
        assert None not in T
    nout = last_y + 1 - ti0 + nin
    stats["edge"].add(("nout", NT, nout % NT, nout >= NT - 1))
    for z in range(nout):
        sym = Rw[ti0 + z]
        assert sym <= GAP, "a position of the walked range without a symbol"
        c = p.col(ti0 + z + tl)
        p.cnt[ti0 + z + tl] = [v + (1 if s == sym else 0) for s, v in enumerate(c)]
    p.lead.append(il); p.size.append(nout)
    return True


def new_stats():
    return {"ins": 0, "edge": set(), "md_free_chunks": 0, "runs_across_waves": 0}


def run_rows(width, nw, trials, seed, max_ins=256, drop_run_carry=False, lq_max=None):
    """Random piles at this shape; returns (rows, rows by the walk, stats, first mismatch or None)."""
    rng = random.Random(seed)
    stats = new_stats()
    NT = width * nw
    rows = by_walk = 0
    for trial in range(trials):
        lq = rng.randint(1, lq_max or max(30, 3 * NT + 2))
        query = [rng.randrange(4) for _ in range(lq)]
        a, b = Pile(query), Pile(query)
        for _ in range(rng.randint(1, 10)):
            m0s, m1s, ops, S = random_row(rng, a, lq)
            add_row_walk(a, m0s, m1s, ops, S)
            before = b.state()
            if not add_row_wide(b, m0s, m1s, ops, S, stats, width, nw, shift_chunks=rng.randint(1, 3), max_ins=max_ins,
                                drop_run_carry=drop_run_carry):
                assert b.state() == before                 # a refused row has touched nothing
                add_row_walk(b, m0s, m1s, ops, S)
                by_walk += 1
            rows += 1
            if a.state() != b.state():
                return rows, by_walk, stats, (trial, m0s, m1s, "".join(ops))
    return rows, by_walk, stats, None


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("nw", [1, 2, 3, 4])
def test_wide_passes_equal_the_step_walk(width, nw):
    rows, by_walk, stats, bad = run_rows(width, nw, 250, 20261021 + 16 * width + nw)
    assert bad is None, bad
    assert rows > 1000 and 0.05 < by_walk / rows < 0.6 and stats["ins"] > 3000
    NT = width * nw
    # every edge of a trip was met: the three lengths one below, at and one above a multiple of width x NW (beyond the first trip)
    for what in ("n_ops", "span", "nout"):
        for r in (NT - 1, 0, 1 % NT):
            assert (what, NT, r, True) in stats["edge"], (what, NT, r)
    if nw > 1:
        assert stats["runs_across_waves"] > 200 and stats["md_free_chunks"] > 200


@pytest.mark.parametrize("width,nw", [(4, 2), (4, 4), (8, 3)])
def test_more_new_columns_than_a_row_may_open(width, nw):
    """A low ceiling on new columns per row, so that rows cross it in the first trip, in a later trip and exactly at the limit."""
    rows, by_walk, stats, bad = run_rows(width, nw, 150, 77 + width + nw, max_ins=5)
    assert bad is None, bad
    assert by_walk / rows > 0.2
    # the kernel's own ceilings: 256 new columns per row (kMaxIns), and 4096 in the wide global-workspace variant (kMaxInsGlobal)
    for n_i, ceiling, batched in ((300, 256, False), (256, 256, True), (300, 4096, True), (4096, 4096, True), (4097, 4096, False)):
        q = [0, 1, 2, 3]
        a, b = Pile(q), Pile(q)
        ops = ['M', 'M'] + ['I'] * n_i + ['M', 'M']
        S = [i % 4 for i in range(n_i + 4)]
        add_row_walk(a, 0, 0, ops, S)
        ok = add_row_wide(b, 0, 0, ops, S, new_stats(), width, nw, max_ins=ceiling)
        assert ok == batched
        if not ok:
            add_row_walk(b, 0, 0, ops, S)
        assert a.state() == b.state()


def test_lengths_at_the_edges_of_a_trip():
    """Directed: a first row of exactly k x NT - 1, k x NT and k x NT + 1 ops over a fresh pile (there n_ops = nout), starting at base 0
    (size_b - ti0 = lq) and inside, with an I run laid across every wavefront boundary of the first trip."""
    for width, nw in ((4, 1), (4, 2), (4, 3), (8, 2), (8, 4)):
        NT = width * nw
        for k in (1, 2, 3):
            for d in (-1, 0, 1):
                n = k * NT + d
                for m0s in (0, 3):
                    for i_at in [None] + [w * width - 1 for w in range(1, nw + 1)]:
                        ops = ['M'] * n
                        if i_at is not None and 0 < i_at < n - 3:
                            ops[i_at:i_at + 3] = ['I'] * 3                     # starts in one wavefront's chunk, ends in the next
                        if ops[0] == 'I':
                            continue
                        lq = m0s + sum(o != 'I' for o in ops)
                        query = [(i * 7) % 4 for i in range(lq)]
                        S = [(i * 5) % 4 for i in range(n)]
                        a, b = Pile(query), Pile(query)
                        for _ in range(2):                                     # the second row meets the first one's gap columns
                            add_row_walk(a, m0s, 0, ops, S)
                            assert add_row_wide(b, m0s, 0, ops, S, new_stats(), width, nw)
                            assert a.state() == b.state(), (width, nw, n, m0s, i_at)


def test_a_dropped_carry_across_wavefronts_is_caught():
    """The planted break: run_start falls back to the previous trip's carry although a wavefront in front of this one had an M/D op."""
    caught = 0
    for width, nw in ((4, 2), (4, 4), (8, 3)):
        try:
            rows, by_walk, stats, bad = run_rows(width, nw, 250, 5 + nw, drop_run_carry=True)
        except (AssertionError, KeyError, IndexError, TypeError):
            bad = "the twin's own checks"
        caught += bad is not None
    assert caught == 3
    # and with one wavefront there is nothing to drop
    assert run_rows(4, 1, 100, 5, drop_run_carry=True)[3] is None
