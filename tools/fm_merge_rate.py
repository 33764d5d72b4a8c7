"""Rate of lrsc_fmmerge (csrc/fm_fmmerge.hip), `stride fm-merge`'s device step, on one box in one run:

  1. the workload of tools/overlap_rate.py: error-free 100-base reads from random places of a testkit genome at 30x, half of them
     reverse-complemented, each sequence once; here also only one of a read and its reverse complement, as rmdup leaves them
     (both would stand as two blocks on their neighbours' ends and end every chain there); the reads' own index by
     lrsc_index_build, which stays resident;
  2. lrsc_fmmerge over all reads with -m 45: one warm-up call, then three timed calls.  Per call: wall seconds, reads/s, the
     launches, and the kernels' milliseconds by phase (overlap, links, chains, place with the prefix sums, assemble) from the
     entry's LRSC_FMMERGE_PROFILE line;
  3. the same per-read and per-node code compiled for the CPU (tests/host_tools/fmmerge_driver.cpp, g++ -O2) on the same reads
     in one process: its chain phase (both rankings and the cut, run serially over the same links) against the device's, and its
     records and bases against the device's, which must be the same.

Nothing here is a pass mark.  Writes profiles/fm_merge.json (or --out)."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import numpy as np  # noqa: E402
from overlap_rate import MIN_OVERLAP, workload  # noqa: E402

from longreadselfcorrect_amd import Lrsc, capi  # noqa: E402

PHASES = ("overlap", "links", "chains", "place", "assemble")


def one_strand_each(bases, off):
    """the reads without those whose reverse complement stands earlier in the set"""
    length = int(off[1])
    reads = np.ascontiguousarray(bases.reshape(-1, length))
    comp = np.zeros(256, dtype=np.uint8)
    comp[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
    other = np.ascontiguousarray(comp[reads[:, ::-1]])
    a, b = reads.view(f"S{length}").ravel(), other.view(f"S{length}").ravel()
    _, first = np.unique(np.where(a < b, a, b), return_index=True)
    reads = reads[np.sort(first)]
    return reads.reshape(-1), (np.arange(reads.shape[0] + 1, dtype=np.uint64) * length).astype(np.uint64)


def one_call(ctx, bases, off, log: Path):
    """-> (per_read, seqs, merged bases, the figures of the call); the entry's profile line goes through the process' stderr"""
    ctx.stats_reset()
    sys.stderr.flush()
    saved = os.dup(2)
    with open(log, "wb") as f:
        os.dup2(f.fileno(), 2)
        try:
            t = time.perf_counter()
            per_read, seqs, merged = ctx.fmmerge(bases, off, MIN_OVERLAP)
            wall = time.perf_counter() - t
        finally:
            os.dup2(saved, 2)
            os.close(saved)
    line = re.search(r"fm-merge kernels: " + ", ".join(rf"{p} ([0-9.]+) ms" for p in PHASES), log.read_text())
    s = ctx.stats(capi.K_FIND)
    n = off.size - 1
    return per_read, seqs, merged, {"wall_s": wall, "reads_per_s": n / wall, "launches": s.launches, "kernel_ms": s.total_ms,
                                    **{f"{p}_ms": float(line.group(i + 1)) for i, p in enumerate(PHASES)}}


def cpu_driver(api, index, bases, off, workdir: Path):
    """-> (the driver's chain_ms, wall seconds, its output)"""
    n_sym = int(off[-1]) + off.size - 1
    images = b"".join(np.array([n_sym, u.size], dtype=np.uint64).tobytes() + u.tobytes() for u in (api.build_bwt(bases, off, rev, 0) for rev in (False, True)))
    codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), bases).astype(np.uint8)
    blob = b"".join([images, np.array([MIN_OVERLAP], dtype=np.int32).tobytes(), np.array([off.size - 1], dtype=np.uint64).tobytes(), off.astype(np.uint64).tobytes(),
                     codes.tobytes(), index.lexico_order(0).astype(np.uint32).tobytes(), index.lexico_order(1).astype(np.uint32).tobytes()])
    exe = workdir / "fmmerge_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", str(exe), str(REPO / "tests/host_tools/fmmerge_driver.cpp"), str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")],
                   check=True)
    (workdir / "in").write_bytes(blob)
    t = time.perf_counter()
    with open(workdir / "in", "rb") as f:
        r = subprocess.run([str(exe), "0"], stdin=f, capture_output=True, check=True)
    wall = time.perf_counter() - t
    return float(re.search(rb"chain_ms ([0-9.]+)", r.stderr).group(1)), wall, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=1.0)
    ap.add_argument("--out", default=str(REPO / "profiles" / "fm_merge.json"))
    args = ap.parse_args()
    os.environ["LRSC_FMMERGE_PROFILE"] = "1"
    api = Lrsc()
    bases, off = one_strand_each(*workload(api, args.genome_mb))
    n = off.size - 1
    t = time.perf_counter()
    index = api.index_build(bases, off, 0)
    build_s = time.perf_counter() - t
    index.locate_prepare(0, 0)                                         # the lexicographic orders: not part of the timed calls
    ctx = index.ctx(api.params_default(5, 90), 0)
    with tempfile.TemporaryDirectory() as d:
        one_call(ctx, bases, off, Path(d) / "log")                     # warm-up: buffers, code objects
        runs = []
        for _ in range(3):
            per_read, seqs, merged, r = one_call(ctx, bases, off, Path(d) / "log")
            runs.append(r)
            print(r, flush=True)
        chain_ms, cpu_wall, out = cpu_driver(api, index, bases, off, Path(d))
    ctx.close()
    index.close()
    # the driver's records and bases are the device's
    assert np.frombuffer(out, dtype=np.uint32, count=2).tolist() == [0, 0]
    assert out[8: 8 + 16 * n] == per_read.tobytes()
    n_seqs = int(np.frombuffer(out, dtype=np.uint64, count=1, offset=8 + 16 * n)[0])
    assert n_seqs == seqs.size and out[16 + 16 * n: 16 + 16 * n + 32 * n_seqs] == seqs.tobytes() and out[24 + 16 * n + 32 * n_seqs:] == merged
    median = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": int(n), "read_length": int(off[1]), "bases": int(bases.size), "min_overlap": MIN_OVERLAP, "index_build_s": build_s},
        "runs": runs,
        "median": median,
        "outcome": {"sequences": int(seqs.size), "merged_bases": len(merged), "reduction_factor": n / max(int(seqs.size), 1), "longest_chain_reads": int(seqs["n_reads"].max()),
                    "circular": int(seqs["circular"].sum()), "dropped_reads": int(((per_read["flags"] & 2) != 0).sum()), "reversed_reads": int((per_read["flags"] & 1).sum())},
        "chain_phase": {"device_kernel_ms": median["chains_ms"], "cpu_driver_serial_ms": chain_ms, "cpu_driver_wall_s_with_its_overlap": cpu_wall,
                        "nodes": 2 * int(n), "rounds_per_ranking": (2 * int(n) - 1).bit_length()},
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    print(f"reads/s: {median['reads_per_s']:.0f}; chain phase: device {median['chains_ms']:.2f} ms, CPU driver serially {chain_ms:.1f} ms")


if __name__ == "__main__":
    main()
