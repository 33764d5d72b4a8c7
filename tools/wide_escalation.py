"""-l above 32 on the bench's data: the share of walks that escalate to the wide kernel, and corrected Mbases/s at -l 32 and -l L.

    python tools/wide_escalation.py [--reads 100000] [--correct 25000] [--leaves 32 64]

Builds bench.py's configs[2] workload (the same seeds: 11.1 Mb genome, 100k x 10 kb reads, indexed on the GPU) and corrects its
first --correct reads (one resident part of a bench step) once per -l, each in a child process: one timed pass after a warm-up pass,
then a pass under LRSC_CORRECT_PROFILE=1 whose log reports the escalated walks.  Prints one JSON line per -l.  For the wide launches'
kernel time run one child under rocprofv3:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/wide_escalation.py --child 64
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def child(args) -> dict:
    from longreadselfcorrect_amd import Lrsc
    from longreadselfcorrect_amd.capi import K_EXTEND, K_EXTEND_WIDE

    api = Lrsc()
    genome = api.synth_genome(0x5EED0001, int(11.1e6 * args.reads / 100_000))
    bases, off = api.synth_reads(0x5EED0002, genome, args.reads, 10_000, first_read=0)
    n_sym = int(off[-1]) + args.reads
    units = [api.build_bwt(bases, off, rev, 0) for rev in (False, True)]
    index = api.index_from_units(units[0], units[1], args.reads, n_sym)
    index.upload(0)
    p = api.params_default(5, 90)
    p.max_leaves = args.child
    ctx = index.ctx(p, 0)
    n = min(args.correct, args.reads)
    sub = bases[: int(off[n])]
    batch = ctx.batch(sub, off[: n + 1].copy())
    out = {"max_leaves": args.child, "reads": n, "mbases": int(off[n]) / 1e6}
    passes = 1 if os.environ.get("LRSC_CORRECT_PROFILE") else 2
    for i in range(passes):
        ctx.stats_reset()
        t = time.time()
        res, _, seq = batch.correct()
        dt = time.time() - t
    out.update(seconds=dt, corrected_mbases_per_s=out["mbases"] / dt, walks=sum(r.total_walk_num for r in res),
               exceed_leave=sum(r.exceed_leave_num for r in res), corrected_bases=int(seq.size),
               extend_ms=ctx.stats(K_EXTEND).total_ms, wide_ms=ctx.stats(K_EXTEND_WIDE).total_ms,
               wide_launches=ctx.stats(K_EXTEND_WIDE).launches)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--correct", type=int, default=25_000)
    ap.add_argument("--leaves", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--child", type=int, default=0, help="(internal) run one -l in this process")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    base = [sys.executable, __file__, "--reads", str(args.reads), "--correct", str(args.correct)]
    for L in args.leaves:
        r = subprocess.run(base + ["--child", str(L)], capture_output=True, text=True, check=True)
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        # the escalated walks: the flow's log line of each round (LRSC_CORRECT_PROFILE)
        r = subprocess.run(base + ["--child", str(L)], capture_output=True, text=True, check=True,
                           env=dict(os.environ, LRSC_CORRECT_PROFILE="1"))
        esc = [int(m) for m in re.findall(r"(\d+) walks escalated so far", r.stderr)]
        ent = [int(m) for m in re.findall(r"round 0: (\d+) entries", r.stderr)]
        rec["escalated_walks"] = esc[-1] if esc else 0
        rec["round0_walks"] = sum(ent)
        rec["escalated_share"] = rec["escalated_walks"] / max(1, rec["round0_walks"])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
