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

Writes profiles/index_in_memory.json (or --out).

--rle measures the device RL encoder (csrc/fm_rle.hip) on the same reads instead: lrsc_build_bwt for both strands with the encoder
and with LRSC_BWT_HOST_RLE=1 (BWT to the host at a byte per symbol, one host thread encodes), alternating, --runs of each after a
warm-up of each, and one lrsc_index_write from a built index.  The encoder's kernel times come from a child run under
`rocprofv3 --kernel-trace --stats` (both strands through lrsc_build_bwt: the byte BWT as the source; one lrsc_index_build +
lrsc_index_write: the rank blocks as the source), as bytes/s counting the source bytes each kernel reads plus the units the emit
kernel writes.  Writes profiles/index_rle.json (or --out).

--open measures the device RL decoder (csrc/fm_unrle.hip): loading a saved index of the same reads.  The .bwt/.rbwt files are
written once (lrsc_build_bwt + lrsc_write_bwt_file) and read once, so that both routes see a warm page cache; then lrsc_index_open +
lrsc_index_upload against lrsc_index_open_device, alternating, --runs of each after a warm-up of each.  The host route's stages are
its two calls (read + decode on two host threads; copy + k-mer tables) beside a plain read of both files; the device route's come
from its LRSC_BWT_PROFILE lines (file read, units to the device, decode + pack, image to the host, tables).  The decoder's kernel
times come from a child run of lrsc_index_open_device on the same files under `rocprofv3 --kernel-trace --stats`, as bytes/s
counting the units each kernel reads and the blocks the pack kernel writes.  Writes profiles/index_open.json (or --out).

--merge measures the device merge (csrc/fm_merge.hip): adding reads to an index that exists.  A = the first 90 % of the reads and
B = the last 10 % are built once and stay resident; then lrsc_index_merge(A, B) against lrsc_index_build of all the reads,
alternating, --runs of each after a warm-up of each.  The merge's stages come from its LRSC_BWT_PROFILE line (walk, interleave, pack,
tables), the rebuild's from lrsc_index_build's; the device-memory peak of either is what it takes above A and B.  Writes
profiles/index_merge.json (or --out).

--locate measures the device locate (csrc/fm_locate.hip) on the same reads.  The index is built once and its RL units kept; for
rate 0 and rate 32 a fresh index of those units (lrsc_index_from_units_device) gets its tables (lrsc_index_locate_prepare, timed
with a host clock around the synchronous call, --runs indexes per rate) and locates --rows (default 1 M) random rows of the .bwt
strand: rows/s and LF steps per row from the LRSC_K_LOCATE statistics, after one warm-up call.  The device bytes of the tables are
the fall of hipMemGetInfo's free memory across the prepare.  Beside them the host sort of whole reads that `stride index` uses
for the same .sai and .rsai (the testkit's hook into host/LexicoOrder.h), whose order the device's must equal.  Writes
profiles/index_locate.json (or --out).

--filter measures the duplicate check and the read removal (csrc/fm_dup.hip, fm_remove.hip): `stride filter`'s two device steps.
Every tenth read is replaced: by a copy of the read before it, by that read's reverse complement, or by a substring of it, in
turn.  The index of these reads is built once and stays resident.  lrsc_dupcheck_reads over all reads in batches of 10 000 (a
fresh session per run): Mbases/s by the call's wall clock and by the kernel's events, rank queries and block loads from the
LRSC_K_FIND statistics.  Then lrsc_index_remove of the reads it does not call UNIQUE against lrsc_index_build of the kept reads,
the only route to that index without the removal, alternating, --runs of each after a warm-up of each (which also checks that
the two routes' units are the same).  The removal's stages come from its LRSC_BWT_PROFILE line (walk, compact, pack, tables),
the rebuild's from lrsc_index_build's; the device-memory peak of either is what it takes above the resident input.  Writes
profiles/index_filter.json (or --out)."""
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
RLE_KERNELS = ("rle_summary_kernel", "rle_count_kernel", "rle_emit_kernel")
UNRLE_KERNELS = ("unrle_tile_kernel", "unrle_pack_kernel")


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


def build_both(api, bases, off, host_rle: bool):
    """lrsc_build_bwt for both strands on one route; (wall seconds, units per strand, a digest of the units)"""
    if host_rle:
        os.environ["LRSC_BWT_HOST_RLE"] = "1"
    else:
        os.environ.pop("LRSC_BWT_HOST_RLE", None)
    try:
        t = time.perf_counter()
        units = [api.build_bwt(bases, off, rev, 0) for rev in (False, True)]
        wall = time.perf_counter() - t
    finally:
        os.environ.pop("LRSC_BWT_HOST_RLE", None)
    return wall, [int(u.size) for u in units], [hash(u.tobytes()) for u in units]


def rle_kernel_times(args, n_sym, n_units) -> dict:
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, __file__, "--rle-call-only",
               "--genome-mb", str(args.genome_mb), "--reads", str(args.reads)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=PROFILE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            return {"error": f"the profiled run passed its limit of {PROFILE_TIMEOUT_S} s"}
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-400:]}
        out = {}
        for f in Path(d).rglob("*kernel_stats.csv"):
            for row in csv.DictReader(open(f)):
                name = row.get("Name", "")
                for k in RLE_KERNELS:
                    if k in name:
                        src = "byte_bwt" if "SrcBytes" in name else "rank_blocks"
                        e = out.setdefault(src, {}).setdefault(k, {"calls": 0, "total_ms": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
        # per source, both strands: every kernel reads the source once (N bytes, or the rank blocks: 64 bytes per block) and the
        # emit kernel writes the units (the scans over the per-tile entries are not among these kernels)
        ksyms = 128 if n_sym >= 2**31 or os.environ.get("LRSC_FORCE_WIDE") else 192
        source_bytes = {"byte_bwt": 2 * n_sym, "rank_blocks": 2 * 64 * (n_sym // ksyms + 1)}
        for src, kernels in out.items():
            total_ms = sum(e["total_ms"] for e in kernels.values())
            counted = 0
            for k, e in kernels.items():
                e["counted_bytes"] = source_bytes[src] + (sum(n_units) if k == "rle_emit_kernel" else 0)
                e["achieved_bytes_per_s"] = e["counted_bytes"] / (e["total_ms"] / 1e3) if e["total_ms"] else None
                counted += e["counted_bytes"]
            kernels["all"] = {"total_ms": total_ms, "counted_bytes": counted,
                              "achieved_bytes_per_s": counted / (total_ms / 1e3) if total_ms else None}
        return out


def rle_main(args, api, bases, off, n_sym):
    if args.rle_call_only:
        for rev in (False, True):
            api.build_bwt(bases, off, rev, 0)
        with tempfile.TemporaryDirectory() as d:
            idx = api.index_build(bases, off, 0)
            idx.write(Path(d) / "x.bwt", Path(d) / "x.rbwt", 0)
            idx.close()
        return
    routes = {"device_rle": False, "host_rle": True}
    digests = {}
    for name, host in routes.items():
        wall, n_units, digests[name] = build_both(api, bases, off, host)
        say(f"warm-up {name}: {wall:.2f} s, {n_units} units")
    assert digests["device_rle"] == digests["host_rle"], "the two routes' units differ"
    walls = {k: [] for k in routes}
    for i in range(args.runs):
        for name, host in routes.items():
            wall, _, dg = build_both(api, bases, off, host)
            assert dg == digests[name]
            walls[name].append(wall)
            say(f"run {i} {name}: {wall:.2f} s")
    stages = {}
    with tempfile.TemporaryDirectory() as d:
        idx = clock(stages, "index_build", lambda: api.index_build(bases, off, 0))
        clock(stages, "index_units_both_strands", lambda: [idx.units(s, 0) for s in (0, 1)])
        clock(stages, "index_write", lambda: idx.write(Path(d) / "x.bwt", Path(d) / "x.rbwt", 0))
        idx.close()
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": off.size - 1, "symbols_per_strand": n_sym, "units_per_strand": n_units},
        "build_bwt_both_strands_wall_s": {k: {"all": v, "min": min(v), "max": max(v)} for k, v in walls.items()},
        "device_below_host_in_every_pairing": max(walls["device_rle"]) < min(walls["host_rle"]),
        "built_index_stages_s": stages,
    }
    if not args.no_profile:
        say("profiled child run")
        result["encoder_kernels"] = rle_kernel_times(args, n_sym, n_units)
    out = args.out or str(REPO / "profiles" / "index_rle.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def route_open_host(api, files, _, work: Path):
    st = {}
    idx = clock(st, "index_open", lambda: api.index_open(*files))
    clock(st, "index_upload", lambda: idx.upload(0))
    return idx, st


def route_open_device(api, files, _, work: Path):
    """lrsc_index_open_device with LRSC_BWT_PROFILE set and this process's stderr in a file for the length of the call"""
    st = {}
    log = work / "open.err"
    sys.stderr.flush()
    saved = os.dup(2)
    fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    os.dup2(fd, 2)
    os.environ["LRSC_BWT_PROFILE"] = "1"
    try:
        idx = clock(st, "index_open_device", lambda: api.index_open_device(*files, 0))
    finally:
        del os.environ["LRSC_BWT_PROFILE"]
        os.dup2(saved, 2)
        os.close(fd)
        os.close(saved)
    text = log.read_text()
    m = re.search(r"file read ([\d.]+) ms", text)
    if m:
        st["file_read"] = float(m.group(1)) / 1e3
    m = re.search(r"units to the device ([\d.]+) ms, decode \+ pack ([\d.]+) ms, image to the host ([\d.]+) ms, tables ([\d.]+) ms", text)
    if m:
        st["units_to_device"], st["decode_pack"], st["image_to_host"], st["tables"] = (float(x) / 1e3 for x in m.groups())
    return idx, st


def unrle_kernel_times(files, n_sym, n_units) -> dict:
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, __file__, "--open-call-only",
               "--files", files[0], files[1]]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=PROFILE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            return {"error": f"the profiled run passed its limit of {PROFILE_TIMEOUT_S} s"}
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-400:]}
        out = {}
        for f in Path(d).rglob("*kernel_stats.csv"):
            for row in csv.DictReader(open(f)):
                for k in UNRLE_KERNELS:
                    if k in row.get("Name", ""):
                        e = out.setdefault(k, {"calls": 0, "total_ms": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
        # both strands: each kernel reads the units once, the pack kernel writes the rank blocks (the scans over the per-tile
        # entries are not among these kernels)
        ksyms = 128 if n_sym >= 2**31 or os.environ.get("LRSC_FORCE_WIDE") else 192
        counted = {"unrle_tile_kernel": sum(n_units), "unrle_pack_kernel": sum(n_units) + 2 * 64 * (n_sym // ksyms + 1)}
        for k, e in out.items():
            e["counted_bytes"] = counted[k]
            e["achieved_bytes_per_s"] = counted[k] / (e["total_ms"] / 1e3) if e["total_ms"] else None
        if out:
            total_ms = sum(e["total_ms"] for e in out.values())
            all_bytes = sum(e["counted_bytes"] for e in out.values())
            out["all"] = {"total_ms": total_ms, "counted_bytes": all_bytes, "achieved_bytes_per_s": all_bytes / (total_ms / 1e3) if total_ms else None}
        return out


def open_main(args, api, hip, bases, off, n_sym):
    n_reads = off.size - 1
    with tempfile.TemporaryDirectory() as d:
        work = Path(d)
        files = (str(work / "reads.bwt"), str(work / "reads.rbwt"))
        n_units = []
        for rev, f in zip((False, True), files):
            u = api.build_bwt(bases, off, rev, 0)
            api.write_bwt_file(f, u, n_reads, n_sym)
            n_units.append(int(u.size))
            del u
        t = time.perf_counter()
        for f in files:
            with open(f, "rb") as fh:
                while fh.read(1 << 26):
                    pass
        plain_read_s = time.perf_counter() - t
        say(f"files written and read once ({plain_read_s:.2f} s): {n_units} units")
        routes = {"host": route_open_host, "device": route_open_device}
        for name, fn in routes.items():
            r = run(api, hip, fn, files, None, work)
            say(f"warm-up {name}: {r['wall_s']:.2f} s")
        runs = {k: [] for k in routes}
        for i in range(args.runs):
            for name, fn in routes.items():
                r = run(api, hip, fn, files, None, work)
                runs[name].append(r)
                say(f"run {i} {name}: {r['wall_s']:.2f} s {r['stages_s']} peak {r['device_peak_bytes'] / 2**30:.2f} GiB")
        walls = {k: [r["wall_s"] for r in v] for k, v in runs.items()}
        peaks = {k: max(r["device_peak_bytes"] for r in v) for k, v in runs.items()}
        # the host route holds both packed images and the k-mer tables at its peak and nothing else
        bound = max(n_units) + peaks["host"]
        result = {
            "workload": {"genome_mb": args.genome_mb, "reads": n_reads, "symbols_per_strand": n_sym, "units_per_strand": n_units},
            "plain_read_of_both_files_s": plain_read_s,
            "runs": runs,
            "wall_s": {k: {"all": v, "min": min(v), "max": max(v), "spread": max(v) - min(v)} for k, v in walls.items()},
            "device_below_host_in_every_pairing": max(walls["device"]) < min(walls["host"]),
            "device_peak_bytes": peaks,
            "both_images_bytes": runs["device"][0]["index_device_bytes"],
            "device_peak_bound_bytes": bound,
            "device_peak_within_one_strands_units_plus_images_plus_tables": peaks["device"] <= bound,
        }
        if not args.no_profile:
            say("profiled child run")
            result["decoder_kernels"] = unrle_kernel_times(files, n_sym, n_units)
    out = args.out or str(REPO / "profiles" / "index_open.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def with_profile_line(work: Path, fn):
    """fn() with LRSC_BWT_PROFILE set and this process's stderr in a file for the length of the call -> (result, the text)"""
    log = work / "call.err"
    sys.stderr.flush()
    saved = os.dup(2)
    fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    os.dup2(fd, 2)
    os.environ["LRSC_BWT_PROFILE"] = "1"
    try:
        out = fn()
    finally:
        del os.environ["LRSC_BWT_PROFILE"]
        os.dup2(saved, 2)
        os.close(fd)
        os.close(saved)
    return out, log.read_text()


def merge_main(args, api, hip, bases, off, n_sym):
    n_reads = off.size - 1
    cut = n_reads * 9 // 10
    at = int(off[cut])
    part_a = (bases[:at], off[: cut + 1].copy())
    part_b = (bases[at:], (off[cut:] - off[cut]).astype(off.dtype))
    setup = {}
    a = clock(setup, "index_build_a", lambda: api.index_build(*part_a, 0))
    b = clock(setup, "index_build_b", lambda: api.index_build(*part_b, 0))
    say(f"A: {cut} reads, B: {n_reads - cut} reads, built in {setup}")

    def route_merge(api_, _bases, _off, work):
        st = {}
        idx, text = with_profile_line(work, lambda: clock(st, "index_merge", lambda: api_.index_merge(a, b, 0)))
        m = re.search(r"index merge: walk ([\d.]+) ms, interleave ([\d.]+) ms, pack ([\d.]+) ms, tables ([\d.]+) ms", text)
        if m:
            st["walk"], st["interleave"], st["pack"], st["tables"] = (float(x) / 1e3 for x in m.groups())
        return idx, st

    with tempfile.TemporaryDirectory() as d:
        work = Path(d)
        routes = {"merge": route_merge, "rebuild": route_build}
        units = {}
        for name, fn in routes.items():                           # warm-up, and the two routes' indexes are one
            idx, _ = fn(api, bases, off, work)
            units[name] = [hash(idx.units(s, 0).tobytes()) for s in (0, 1)]
            idx.close()
        assert units["merge"] == units["rebuild"], "the merged index is not the rebuilt one"
        runs = {k: [] for k in routes}
        for i in range(args.runs):
            for name, fn in routes.items():
                r = run(api, hip, fn, bases, off, work)
                runs[name].append(r)
                say(f"run {i} {name}: {r['wall_s']:.2f} s {r['stages_s']} peak {r['device_peak_bytes'] / 2**30:.2f} GiB")
    walls = {k: [r["wall_s"] for r in v] for k, v in runs.items()}
    n_b = int(part_b[1][-1]) + n_reads - cut
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": n_reads, "symbols_per_strand": n_sym, "reads_a": cut, "reads_b": n_reads - cut,
                     "symbols_per_strand_b": n_b},
        "setup_s": setup,
        "runs": runs,
        "wall_s": {k: {"all": v, "min": min(v), "max": max(v), "spread": max(v) - min(v)} for k, v in walls.items()},
        "merge_below_rebuild_in_every_pairing": max(walls["merge"]) < min(walls["rebuild"]),
        "merge_over_rebuild": {"best": min(walls["merge"]) / max(walls["rebuild"]), "worst": max(walls["merge"]) / min(walls["rebuild"])},
        # above the resident A and B: one strand's BWT and ranks or packer workspace, the packed images, the k-mer tables
        "device_peak_bytes": {k: max(r["device_peak_bytes"] for r in v) for k, v in runs.items()},
        "bwt_plus_ranks_bytes": n_sym + 8 * n_b,
    }
    a.close()
    b.close()
    out = args.out or str(REPO / "profiles" / "index_merge.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def locate_main(args, api, hip, bases, off, n_sym):
    import numpy as np

    from longreadselfcorrect_amd.capi import K_LOCATE

    n_reads = off.size - 1
    mem = MemPeak(hip)
    setup, host = {}, {}
    built = clock(setup, "index_build", lambda: api.index_build(bases, off, 0))
    units = [built.units(s, 0) for s in (0, 1)]
    built.close()
    host_order = [clock(host, name, lambda rev=rev: api.host_lexico_order(bases, off, rev)) for rev, name in ((False, "sai"), (True, "rsai"))]
    say(f"index built in {setup}; host sort of whole reads {host}")
    rows = np.random.default_rng(0x10CA7E).integers(0, n_sym, size=args.rows, dtype=np.uint64)
    rates, answers = {}, {}
    for rate in (0, 32):
        prepare, table_bytes, calls = [], [], []
        for run_i in range(args.runs):
            idx = api.index_from_units_device(units[0], units[1], n_reads, n_sym, 0)
            free0 = mem.free()
            st = {}
            clock(st, "prepare", lambda: idx.locate_prepare(rate, 0))
            table_bytes.append(free0 - mem.free())
            prepare.append(st["prepare"])
            for strand in (0, 1):
                assert np.array_equal(idx.lexico_order(strand, 0), host_order[strand]), "the device's order is not the host sort's"
            ctx = idx.ctx(None, 0)
            ctx.locate(0, rows[:1024])                            # warm-up
            ctx.stats_reset()
            wall = {}
            got = clock(wall, "locate", lambda: ctx.locate(0, rows))
            ks = ctx.stats(K_LOCATE)
            calls.append({"wall_s": wall["locate"], "kernel_ms": ks.total_ms, "rows_per_s_kernel": rows.size / (ks.total_ms / 1e3),
                          "rows_per_s_call": rows.size / wall["locate"], "lf_steps_per_row": ks.rank_queries / rows.size})
            answers.setdefault(rate, got)
            assert np.array_equal(got, answers[rate])
            say(f"rate {rate} run {run_i}: prepare {st['prepare']:.3f} s, tables {table_bytes[-1] / 2**20:.1f} MiB, {calls[-1]}")
            ctx.close()
            idx.close()
        rates[str(rate)] = {"prepare_s": {"all": prepare, "min": min(prepare), "max": max(prepare)}, "table_device_bytes": max(table_bytes),
                            "table_bytes_by_formula": 2 * ((n_sym // rate + 1) * 8 if rate else 0) + 2 * 8 * n_reads, "locate": calls}
    assert np.array_equal(answers[0], answers[32]), "the two rates locate differently"
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": n_reads, "symbols_per_strand": n_sym, "rows": int(rows.size)},
        "setup_s": setup,
        "host_lexico_order_s": {**host, "both": sum(host.values())},
        "rates": rates,
    }
    out = args.out or str(REPO / "profiles" / "index_locate.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def filter_main(args, api, hip, bases, off, n_sym):
    import numpy as np

    from longreadselfcorrect_amd.capi import DUP_UNIQUE, K_FIND

    n_reads = off.size - 1
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    reads = []
    for i in range(n_reads):
        r = bases[int(off[i]): int(off[i + 1])]
        if i % 10 == 9:
            src = reads[i - 1]
            r = (src, comp[src[::-1]], src[src.size // 4: src.size // 4 * 3])[(i // 10) % 3]
        reads.append(r)
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    bases = np.concatenate(reads)
    del reads
    n_sym = int(off[-1]) + n_reads
    setup = {}
    index = clock(setup, "index_build", lambda: api.index_build(bases, off, 0))
    say(f"{n_reads} reads with every tenth replaced, {n_sym} symbols per strand, built in {setup}")

    batch, checks, cls = 10000, [], None
    for run_i in range(args.runs + 1):                            # the first is the warm-up
        ctx = index.ctx(None, 0)
        session = ctx.dupcheck()
        t = time.perf_counter()
        got = [session.reads(bases[int(off[a]): int(off[min(a + batch, n_reads)])], off[a: min(a + batch, n_reads) + 1] - off[a])
               for a in range(0, n_reads, batch)]
        wall = time.perf_counter() - t
        ks = ctx.stats(K_FIND)
        session.close()
        ctx.close()
        got = np.concatenate(got)["cls"]
        assert cls is None or np.array_equal(cls, got), "the classes differ between two runs"
        cls = got
        if run_i:
            checks.append({"wall_s": wall, "kernel_ms": ks.total_ms, "mbases_per_s_call": int(off[-1]) / wall / 1e6,
                           "mbases_per_s_kernel": int(off[-1]) / (ks.total_ms / 1e3) / 1e6, "launches": ks.launches, "rank_queries": ks.rank_queries,
                           "block_loads": ks.block_loads})
            say(f"duplicate check run {run_i}: {checks[-1]}")
    drop = (cls != DUP_UNIQUE).astype(np.uint8)
    keep = np.flatnonzero(drop == 0)
    kept_bases = np.concatenate([bases[int(off[i]): int(off[i + 1])] for i in keep])
    kept_off = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[keep])]).astype(np.uint64)
    say(f"classes: {np.bincount(cls, minlength=4).tolist()} (unique, substring, full length, absent); {keep.size} reads kept")

    def route_remove(api_, _bases, _off, work):
        st = {}
        idx, text = with_profile_line(work, lambda: clock(st, "index_remove", lambda: index.remove(drop, 0)))
        m = re.search(r"index remove: walk ([\d.]+) ms, compact ([\d.]+) ms, pack ([\d.]+) ms, tables ([\d.]+) ms", text)
        if m:
            st["walk"], st["compact"], st["pack"], st["tables"] = (float(x) / 1e3 for x in m.groups())
        return idx, st

    with tempfile.TemporaryDirectory() as d:
        work = Path(d)
        routes = {"remove": route_remove, "rebuild": route_build}
        units = {}
        for name, fn in routes.items():                           # warm-up, and the two routes' indexes are one
            idx, _ = fn(api, kept_bases, kept_off, work)
            units[name] = [hash(idx.units(s, 0).tobytes()) for s in (0, 1)]
            idx.close()
        assert units["remove"] == units["rebuild"], "the index without the dropped reads is not the rebuilt one"
        runs = {k: [] for k in routes}
        for i in range(args.runs):
            for name, fn in routes.items():
                r = run(api, hip, fn, kept_bases, kept_off, work)
                runs[name].append(r)
                say(f"run {i} {name}: {r['wall_s']:.2f} s {r['stages_s']} peak {r['device_peak_bytes'] / 2**30:.2f} GiB")
    walls = {k: [r["wall_s"] for r in v] for k, v in runs.items()}
    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": n_reads, "symbols_per_strand": n_sym, "bases": int(off[-1]),
                     "classes_unique_substring_full_absent": np.bincount(cls, minlength=4).tolist(), "reads_kept": int(keep.size),
                     "symbols_per_strand_kept": int(kept_off[-1]) + int(keep.size), "dupcheck_batch": batch},
        "setup_s": setup,
        "dupcheck": checks,
        "runs": runs,
        "wall_s": {k: {"all": v, "min": min(v), "max": max(v), "spread": max(v) - min(v)} for k, v in walls.items()},
        "remove_below_rebuild_in_every_pairing": max(walls["remove"]) < min(walls["rebuild"]),
        "remove_over_rebuild": {"best": min(walls["remove"]) / max(walls["rebuild"]), "worst": max(walls["remove"]) / min(walls["rebuild"])},
        # above the resident input: the bitmap, one strand's BWT of the kept reads or the sort's workspace, the packed images, the k-mer tables
        "device_peak_bytes": {k: max(r["device_peak_bytes"] for r in v) for k, v in runs.items()},
    }
    index.close()
    out = args.out or str(REPO / "profiles" / "index_filter.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=11.1)
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="default: profiles/index_in_memory.json; profiles/index_rle.json with --rle, index_open.json with --open, index_merge.json with --merge, index_locate.json with --locate, index_filter.json with --filter")
    ap.add_argument("--rle", action="store_true", help="measure the device RL encoder instead (see the module text)")
    ap.add_argument("--rle-call-only", action="store_true", help="the encoder's calls once (the child run under the profiler)")
    ap.add_argument("--call-only", action="store_true", help="one lrsc_index_build (the child run under the profiler)")
    ap.add_argument("--open", action="store_true", help="measure the device RL decoder instead (see the module text)")
    ap.add_argument("--open-call-only", action="store_true", help="one lrsc_index_open_device of --files (the child run under the profiler)")
    ap.add_argument("--merge", action="store_true", help="measure the device merge instead (see the module text)")
    ap.add_argument("--locate", action="store_true", help="measure the device locate instead (see the module text)")
    ap.add_argument("--filter", action="store_true", help="measure the duplicate check and the read removal instead (see the module text)")
    ap.add_argument("--rows", type=int, default=1000000, help="--locate: random rows to locate")
    ap.add_argument("--files", nargs=2, metavar=("BWT", "RBWT"))
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    api = Lrsc()
    hip = C.CDLL("libamdhip64.so")
    if args.open_call_only:
        api.index_open_device(args.files[0], args.files[1], 0).close()
        return
    genome = api.synth_genome(0x5EED0001, int(args.genome_mb * 1e6))
    n_reads = args.reads
    bases, off = api.synth_reads(0x5EED0002, genome, n_reads, 10000)
    n_sym = int(off[-1]) + n_reads
    say(f"{n_reads} reads, {n_sym} symbols per strand")
    if args.rle or args.rle_call_only:
        return rle_main(args, api, bases, off, n_sym)
    if args.open:
        return open_main(args, api, hip, bases, off, n_sym)
    if args.merge:
        return merge_main(args, api, hip, bases, off, n_sym)
    if args.locate:
        return locate_main(args, api, hip, bases, off, n_sym)
    if args.filter:
        return filter_main(args, api, hip, bases, off, n_sym)
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
    out = args.out or str(REPO / "profiles" / "index_in_memory.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
