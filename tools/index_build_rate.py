"""From reads in host memory to an index on which lrsc_ctx_create succeeds: the file route against lrsc_index_build, on one box in
one process.

  files:  lrsc_build_bwt x2 (device sort, BWT to the host at a byte per symbol, host RL encoding), lrsc_write_bwt_file x2,
          lrsc_index_open (read, decode the runs into rank blocks on two host threads), lrsc_index_upload (copy, k-mer tables)
  build:  lrsc_index_build (device sort, device packer, k-mer tables; the host image is a copy of the packed one)

The reads are the bench workload's: --reads 10 kb templates from the testkit generator over a --genome-mb genome.  The defaults,
100k reads over 11.1 Mb = 90x, are bench.py's and BASELINE configs[2]'s size: 1.05 G symbols per strand.  After one warm-up of each
route, --runs (default 2) of each, alternating.  Every stage is timed with a host clock around a call that ends synchronised;
lrsc_index_build's own stages come from its LRSC_BWT_PROFILE line.  A sampling thread reads hipMemGetInfo every 10 ms for the device
memory peak of each route (the free memory of the whole device: only meaningful on a device nothing else is using).  The packer's
kernel times come from one child run of lrsc_index_build under `rocprofv3 --kernel-trace --stats`, and are turned into bytes/s
counting N bytes read and N/3 written per strand.

Writes profiles/index_in_memory.json (or --out)."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import threading
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
PROFILE_TIMEOUT_S = 600          # the child generates the reads again and builds one index under the profiler
sys.path.insert(0, str(REPO))

from longreadselfcorrect_amd import Lrsc  # noqa: E402

PACK_KERNELS = ("pack_hist_kernel", "pack_blocks_kernel", "dollar_dir_kernel", "IsDollar")


def say(*a):
    print(*a, file=sys.stderr, flush=True)


class MemPeak:
    """Lowest free device memory seen while the block runs, as bytes in use above the level at entry."""

    def __init__(self, hip):
        self.hip = hip

    def free(self):
        f, t = C.c_size_t(), C.c_size_t()
        assert self.hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    def __enter__(self):
        self.start = self.low = self.free()
        self.stop = threading.Event()

        def poll():
            assert self.hip.hipSetDevice(0) == 0
            while not self.stop.wait(0.01):
                self.low = min(self.low, self.free())
        self.thread = threading.Thread(target=poll)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.peak = self.start - self.low


def clock(stages, name, fn):
    t = time.perf_counter()
    out = fn()
    stages[name] = stages.get(name, 0.0) + time.perf_counter() - t
    return out


def route_files(api, bases, off, work: Path):
    n_reads = off.size - 1
    n_sym = int(off[-1]) + n_reads
    st = {}
    for rev, ext in ((False, "bwt"), (True, "rbwt")):
        u = clock(st, "build_bwt", lambda: api.build_bwt(bases, off, rev, 0))
        clock(st, "write_bwt_file", lambda: api.write_bwt_file(work / f"reads.{ext}", u, n_reads, n_sym))
        del u
    idx = clock(st, "index_open", lambda: api.index_open(str(work / "reads.bwt"), str(work / "reads.rbwt")))
    clock(st, "index_upload", lambda: idx.upload(0))
    return idx, st


def route_build(api, bases, off, work: Path):
    """lrsc_index_build with LRSC_BWT_PROFILE set and this process's stderr in a file for the length of the call"""
    st = {}
    log = work / "build.err"
    sys.stderr.flush()
    saved = os.dup(2)
    fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    os.dup2(fd, 2)
    os.environ["LRSC_BWT_PROFILE"] = "1"
    try:
        idx = clock(st, "index_build", lambda: api.index_build(bases, off, 0))
    finally:
        del os.environ["LRSC_BWT_PROFILE"]
        os.dup2(saved, 2)
        os.close(fd)
        os.close(saved)
    m = re.search(r"index build: bwt ([\d.]+) ms, pack ([\d.]+) ms, tables ([\d.]+) ms", log.read_text())
    if m:
        st["bwt_build"], st["pack"], st["tables"] = (float(x) / 1e3 for x in m.groups())
    return idx, st


def run(api, hip, route, bases, off, work):
    with MemPeak(hip) as mem:
        t = time.perf_counter()
        idx, stages = route(api, bases, off, work)
        wall = time.perf_counter() - t
        ctx = idx.ctx(api.params_default(5, 90), 0)          # the route's end: a context can be made
        ctx.close()
    info = idx.info()
    idx.close()
    return {"wall_s": wall, "stages_s": stages, "device_peak_bytes": mem.peak, "index_device_bytes": info.device_bytes}


def kernel_times(args, n_sym) -> dict:
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, __file__, "--call-only",
               "--genome-mb", str(args.genome_mb), "--reads", str(args.reads)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=PROFILE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            return {"error": f"the profiled run passed its limit of {PROFILE_TIMEOUT_S} s"}
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-400:]}
        out, total_ns = {}, 0.0
        for f in Path(d).rglob("*kernel_stats.csv"):
            for row in csv.DictReader(open(f)):
                name = row.get("Name", "")
                for k in PACK_KERNELS:
                    if k in name:
                        key = k if k != "IsDollar" else "select_if_IsDollar"
                        e = out.setdefault(key, {"calls": 0, "total_ms": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
                        total_ns += float(row["TotalDurationNs"])
        if total_ns:
            # both strands; N bytes read and N/3 written per strand (the scans of the per-block counts are not among these kernels)
            out["counted_bytes"] = 2 * (n_sym + n_sym // 3)
            out["listed_kernels_total_ms"] = total_ns / 1e6
            out["achieved_bytes_per_s"] = out["counted_bytes"] / (total_ns / 1e9)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=11.1)
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=str(REPO / "profiles" / "index_in_memory.json"))
    ap.add_argument("--call-only", action="store_true", help="one lrsc_index_build (the child run under the profiler)")
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    api = Lrsc()
    hip = C.CDLL("libamdhip64.so")
    genome = api.synth_genome(0x5EED0001, int(args.genome_mb * 1e6))
    n_reads = args.reads
    bases, off = api.synth_reads(0x5EED0002, genome, n_reads, 10000)
    n_sym = int(off[-1]) + n_reads
    say(f"{n_reads} reads, {n_sym} symbols per strand")
    if args.call_only:
        api.index_build(bases, off, 0).close()
        return
    with tempfile.TemporaryDirectory() as d:
        work = Path(d)
        routes = {"files": route_files, "build": route_build}
        for name, fn in routes.items():
            r = run(api, hip, fn, bases, off, work)
            say(f"warm-up {name}: {r['wall_s']:.2f} s")
        runs = {"files": [], "build": []}
        for i in range(args.runs):
            for name, fn in routes.items():
                r = run(api, hip, fn, bases, off, work)
                runs[name].append(r)
                say(f"run {i} {name}: {r['wall_s']:.2f} s {r['stages_s']} peak {r['device_peak_bytes'] / 2**30:.2f} GiB")
    walls = {k: [r["wall_s"] for r in v] for k, v in runs.items()}
    image = runs["build"][0]["index_device_bytes"] // 2           # one strand's packed image
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": n_reads, "symbols_per_strand": n_sym},
        "runs": runs,
        "wall_s": {k: {"all": v, "min": min(v), "max": max(v), "spread": max(v) - min(v)} for k, v in walls.items()},
        "build_below_files_in_every_pairing": max(walls["build"]) < min(walls["files"]),
        "device_peak_bytes": {k: max(r["device_peak_bytes"] for r in v) for k, v in runs.items()},
        "one_packed_strand_bytes": image,
    }
    result["build_peak_within_files_peak_plus_one_image"] = (
        result["device_peak_bytes"]["build"] <= result["device_peak_bytes"]["files"] + image)
    if not args.no_profile:
        say("profiled child run")
        result["packer_kernels"] = kernel_times(args, n_sym)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
