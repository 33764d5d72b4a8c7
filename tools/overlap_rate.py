"""Rate of lrsc_overlap_exact (csrc/fm_overlap.hip), `stride overlap`'s device step, on one box in one run:

  1. a genome from the testkit generator (--genome-mb, default 1); error-free 100-base reads from random places at 30x, half of
     them reverse-complemented, each sequence once (what `stride filter`, the step before overlap in the pipeline, leaves of its
     duplicates); the reads' own index by lrsc_index_build, which stays resident;
  2. lrsc_overlap_exact over all reads in batches of 100 000, as `stride overlap` calls it, with -m 45: one warm-up run, then three
     timed runs.  Per run: wall seconds of the calls, reads/s, the kernels' own milliseconds, their interval steps per second (one
     step is two Occ queries, from lrsc_ctx_stats under K_FIND) and block loads per step;
  3. the same per-read code compiled for the CPU (tests/host_tools/overlap_driver.cpp, g++ -O2) on the first --cpu-reads reads of
     the same set against the same index, in --cpu-threads processes of equal shares at once (default 16).  A process also reads
     the index and builds its image; the wall time of the same processes with no reads is taken off.  Both ends give the same
     blocks, which is checked.

Writes profiles/overlap_exact.json (or --out)."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

from longreadselfcorrect_amd import Lrsc, capi  # noqa: E402

READ_LEN, COVERAGE, BATCH, MIN_OVERLAP = 100, 30, 100000, 45


def workload(api, genome_mb: float):
    """-> (the reads as ASCII, n + 1 offsets)"""
    rng = np.random.default_rng(0x0E11A9)
    n = int(genome_mb * 1e6)
    ascii_of = np.frombuffer(b"ACGT", dtype=np.uint8)
    code_of = np.zeros(256, dtype=np.uint8)
    code_of[ascii_of] = np.arange(4, dtype=np.uint8)
    genome = code_of[np.frombuffer(api.synth_genome(0x5EED0002, n), dtype=np.uint8)]
    n_reads = n * COVERAGE // READ_LEN
    starts = rng.integers(0, n - READ_LEN, size=n_reads)
    cols = np.arange(READ_LEN)
    fwd = genome[starts[:, None] + cols[None, :]]
    rvc = 3 - genome[(starts + READ_LEN - 1)[:, None] - cols[None, :]]
    reads = np.where((rng.random(n_reads) < 0.5)[:, None], rvc, fwd)
    _, first = np.unique(reads, axis=0, return_index=True)
    reads = reads[np.sort(first)]
    off = (np.arange(reads.shape[0] + 1, dtype=np.uint64) * READ_LEN).astype(np.uint64)
    return ascii_of[reads].reshape(-1), off


def one_run(ctx, bases, off):
    n = off.size - 1
    ctx.stats_reset()
    per_read, blocks = [], []
    t = time.perf_counter()
    for a in range(0, n, BATCH):
        b = min(a + BATCH, n)
        p, q = ctx.overlap_exact(bases[int(off[a]): int(off[b])], off[a: b + 1] - off[a], MIN_OVERLAP, block_cap=8 * (b - a))
        per_read.append(p)
        blocks.append(q)
    wall = time.perf_counter() - t
    s = ctx.stats(capi.K_FIND)
    steps = s.rank_queries / 2
    return per_read, blocks, {"wall_s": wall, "reads_per_s": n / wall, "kernel_ms": s.total_ms, "launches": s.launches, "interval_steps": steps,
                              "interval_steps_per_s": steps / (s.total_ms / 1e3), "block_loads_per_step": s.block_loads / steps}


def cpu_driver(api, bases, off, n_cpu: int, threads: int):
    """-> (reads/s of the CPU driver on `threads` processes, the blocks it found per read as a list of arrays)"""
    n_sym = int(off[-1]) + off.size - 1
    images = b"".join(np.array([n_sym, u.size], dtype=np.uint64).tobytes() + u.tobytes() for u in (api.build_bwt(bases, off, rev, 0) for rev in (False, True)))
    with tempfile.TemporaryDirectory() as d:
        exe = Path(d) / "overlap_driver"
        subprocess.run(["g++", "-std=c++17", "-O2", "-o", str(exe), str(REPO / "tests/host_tools/overlap_driver.cpp"),
                        str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
        share = -(-n_cpu // threads)

        def inputs(with_reads: bool):
            out = []
            for k in range(threads):
                a, b = min(k * share, n_cpu), min((k + 1) * share, n_cpu) if with_reads else min(k * share, n_cpu)
                o = off[a: b + 1] - off[a]
                codes = (np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), bases[int(off[a]): int(off[b])])).astype(np.uint8)
                out.append(images + np.array([MIN_OVERLAP], dtype=np.int32).tobytes() + np.array([b - a], dtype=np.uint64).tobytes() + o.astype(np.uint64).tobytes() + codes.tobytes())
            return out

        def timed(blobs):
            files = []
            for k, blob in enumerate(blobs):
                (Path(d) / f"in{k}").write_bytes(blob)
                files.append(open(Path(d) / f"in{k}", "rb"))
            t = time.perf_counter()
            procs = [subprocess.Popen([str(exe), "0"], stdin=f, stdout=subprocess.PIPE) for f in files]
            outs = [p.communicate()[0] for p in procs]
            wall = time.perf_counter() - t
            assert all(p.returncode == 0 for p in procs)
            for f in files:
                f.close()
            return wall, outs

        idle, _ = timed(inputs(False))
        busy, outs = timed(inputs(True))
    found = []
    for k, out in enumerate(outs):
        n = min((k + 1) * share, n_cpu) - min(k * share, n_cpu)
        p = np.frombuffer(out, dtype=capi.OVERLAP_READ_DTYPE, count=n)
        q = np.frombuffer(out, dtype=capi.OVERLAP_BLOCK_DTYPE, count=int(p["n_blocks"].sum()), offset=n * 24)
        found += [q[int(r["first_block"]): int(r["first_block"]) + int(r["n_blocks"])] for r in p]
    return {"reads": n_cpu, "processes": threads, "wall_s": busy, "wall_s_without_reads": idle, "reads_per_s": n_cpu / max(busy - idle, 1e-9)}, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=1.0)
    ap.add_argument("--cpu-reads", type=int, default=32000)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default=str(REPO / "profiles" / "overlap_exact.json"))
    args = ap.parse_args()
    api = Lrsc()
    bases, off = workload(api, args.genome_mb)
    t = time.perf_counter()
    index = api.index_build(bases, off, 0)
    build_s = time.perf_counter() - t
    ctx = index.ctx(api.params_default(5, 90), 0)
    one_run(ctx, bases, off)                                           # warm-up: buffers, code objects
    runs = []
    for _ in range(3):
        per_read, blocks, r = one_run(ctx, bases, off)
        runs.append(r)
        print(r, flush=True)
    ctx.close()
    index.close()
    per_read, blocks = np.concatenate(per_read), blocks
    n_cpu = min(args.cpu_reads, off.size - 1)
    cpu, found = cpu_driver(api, bases, off, n_cpu, args.cpu_threads)
    first = blocks[0]
    for i in range(min(n_cpu, BATCH)):                                 # the first batch's reads: the same blocks from both ends
        a = int(per_read["first_block"][i])
        assert first[a: a + int(per_read["n_blocks"][i])].tobytes() == found[i].tobytes(), i
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": int(off.size - 1), "read_length": READ_LEN, "coverage": COVERAGE, "bases": int(bases.size), "batch": BATCH,
                     "min_overlap": MIN_OVERLAP, "index_build_s": build_s},
        "runs": runs,
        "median": {k: statistics.median(r[k] for r in runs) for k in ("wall_s", "reads_per_s", "kernel_ms", "interval_steps_per_s", "block_loads_per_step")},
        "outcome": {"blocks_per_read_mean": float(per_read["n_blocks"].mean()), "substring_reads": int(per_read["is_substring"].sum()),
                    "overflowed_reads": int((per_read["status"] != 0).sum())},
        "cpu_driver": cpu,
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    print(f"reads/s: device {result['median']['reads_per_s']:.0f}, CPU driver on {args.cpu_threads} processes {cpu['reads_per_s']:.0f}")


if __name__ == "__main__":
    main()
