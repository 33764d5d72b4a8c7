"""Rate of lrsc_kmer_correct (csrc/fm_kcorrect.hip), `stride correct -a kmer`'s device step, on one box in one run:

  1. a random genome (--genome-mb, default 1), 150-base reads at 40x from random places, half of them reverse-complemented, with
     1 % substitutions; their own index by lrsc_index_build, which stays resident;
  2. lrsc_kmer_correct over all reads in batches of 100 000, as `stride correct` calls it, with -k 31 -x 3 -i 10 and no
     qualities: one warm-up run, then three timed runs.  Per run: wall seconds of the calls, corrected Mbases/s (bases of the reads
     over the wall time), the kernel's own milliseconds, its LF steps per second (one LF step is two Occ queries, from
     lrsc_ctx_stats under K_FIND) and block loads per LF step;
  3. the share of reads that passed QC, the share of changed bases that are back to the genome's base, and the passes per read.

Writes profiles/kmer_correct.json (or --out)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

from longreadselfcorrect_amd import Lrsc, capi  # noqa: E402

READ_LEN, COVERAGE, P_SUB, BATCH = 150, 40, 0.01, 100000


def workload(genome_mb: float):
    """-> (reads as ASCII with errors, the same without, offsets)"""
    rng = np.random.default_rng(0xEC0DE)
    n = int(genome_mb * 1e6)
    genome = rng.integers(0, 4, size=n, dtype=np.uint8)
    n_reads = n * COVERAGE // READ_LEN
    starts = rng.integers(0, n - READ_LEN, size=n_reads)
    truth = genome[starts[:, None] + np.arange(READ_LEN)[None, :]]
    flip = rng.random(n_reads) < 0.5
    truth[flip] = 3 - truth[flip, ::-1]
    reads = truth.copy()
    hit = rng.random(reads.shape) < P_SUB
    reads[hit] = (reads[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) & 3
    ascii_of = np.frombuffer(b"ACGT", dtype=np.uint8)
    off = (np.arange(n_reads + 1, dtype=np.uint64) * READ_LEN).astype(np.uint64)
    return ascii_of[reads].reshape(-1), ascii_of[truth].reshape(-1), off


def one_run(ctx, bases, off):
    n_reads = off.size - 1
    ctx.stats_reset()
    out_bases = np.empty_like(bases)
    res = np.zeros(n_reads, dtype=capi.KCORRECT_DTYPE)
    t = time.perf_counter()
    for a in range(0, n_reads, BATCH):
        b = min(a + BATCH, n_reads)
        lo, hi = int(off[a]), int(off[b])
        out_bases[lo:hi], res[a:b] = ctx.kmer_correct(bases[lo:hi], off[a: b + 1] - off[a], None, 31, 3, 10, 20)
    wall = time.perf_counter() - t
    s = ctx.stats(capi.K_FIND)
    lf = s.rank_queries / 2
    return out_bases, res, {"wall_s": wall, "corrected_mbases_per_s": bases.size / wall / 1e6, "kernel_ms": s.total_ms, "launches": s.launches,
                            "lf_steps": lf, "lf_steps_per_s": lf / (s.total_ms / 1e3), "block_loads_per_lf_step": s.block_loads / lf}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=1.0)
    ap.add_argument("--out", default=str(REPO / "profiles" / "kmer_correct.json"))
    args = ap.parse_args()
    api = Lrsc()
    bases, truth, off = workload(args.genome_mb)
    t = time.perf_counter()
    index = api.index_build(bases, off, 0)
    build_s = time.perf_counter() - t
    ctx = index.ctx(api.params_default(5, 90), 0)
    one_run(ctx, bases, off)                                           # warm-up: buffers, code objects
    runs = []
    for _ in range(3):
        corrected, res, r = one_run(ctx, bases, off)
        runs.append(r)
        print(r, flush=True)
    ctx.close()
    index.close()
    changed = corrected != bases
    wrong_before, wrong_after = int((bases != truth).sum()), int((corrected != truth).sum())
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": int(off.size - 1), "read_length": READ_LEN, "coverage": COVERAGE, "substitution_rate": P_SUB,
                     "bases": int(bases.size), "batch": BATCH, "kmer_length": 31, "kmer_threshold": 3, "kmer_rounds": 10, "index_build_s": build_s},
        "runs": runs,
        "median": {k: statistics.median(r[k] for r in runs) for k in ("wall_s", "corrected_mbases_per_s", "kernel_ms", "lf_steps_per_s", "block_loads_per_lf_step")},
        "outcome": {"reads_passed_qc_share": float(res["kmer_qc"].mean()), "passes_per_read": float(res["passes"].mean()),
                    "bases_changed": int(changed.sum()), "changed_bases_now_the_genome_s_share": float((corrected[changed] == truth[changed]).mean()),
                    "wrong_bases_before": wrong_before, "wrong_bases_after": wrong_after},
        # tools/index_build_rate.py --filter has never been run: there is no profiles/index_filter.json to set this against
        "duplicate_check_lf_steps_per_s": None,
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
