"""Rate of lrsc_saipb_merge (the batched seed-pair merge kernels) against the host SAIPBSelfCorrectTree over the C ABI, on one box
in one run:

  1. a bench-shaped read set (testkit, 90x, 10 kb templates), indexed by the product's own builder;
  2. seeds from lrsc_batch_find_seeds; seed pairs by the rule of tests/test_saipb_oracle._pairs (60 bases of source context, a
     positive gap; targets of at least 17 bases) until there are at least --pairs of them (default 100 000);
  3. (a) the new call on all pairs, warm, median of three, as pairs/s -- and its kernels' times from one separate
     `rocprofv3 --kernel-trace --stats` child run;
  4. (b) the host class (tests/host_tools/saipb_driver.cpp, FM access = lrsc_find_kmers / lrsc_rank / lrsc_lf_walk) on the first
     --host-pairs (default 500) of the same pairs, as pairs/s; its set-up (index load and upload) is measured by a run without
     pairs and taken off.

Writes profiles/saipb_kernel_rate.json (or --out)."""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
# A time limit for every child that opens the GPU, sized to the step at the default sizes (subprocess.run kills the child when it
# passes): the profiled run repeats the set-up and one call, which take well under two minutes without the profiler; the driver loads
# the index in seconds and does some hundred pairs a second.
PROFILE_TIMEOUT_S = 600
DRIVER_TIMEOUT_S = 300
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

from longreadselfcorrect_amd import Lrsc  # noqa: E402
from longreadselfcorrect_amd.capi import saipb_pair_jobs  # noqa: E402


def workload(api, genome_mb: float, want_pairs: int, workdir: Path):
    genome = api.synth_genome(0x5EED0001, int(genome_mb * 1e6))
    n_reads = int(genome_mb * 1e6 * 90 / 10000)
    bases, off = api.synth_reads(0x5EED0002, genome, n_reads, 10000)
    n_sym = int(off[-1]) + n_reads
    units = [api.build_bwt(bases, off, rev, 0) for rev in (False, True)]
    for u, ext in zip(units, ("bwt", "rbwt")):
        api.write_bwt_file(workdir / f"reads.{ext}", u, n_reads, n_sym)
    idx = api.index_open(str(workdir / "reads.bwt"), str(workdir / "reads.rbwt"))
    idx.upload(0)
    ctx = idx.ctx(api.params_default(5, 90), 0)
    batch = ctx.batch(bases, off)
    batch.find_seeds()
    count, seeds, _ = batch.seeds(want_attribute=False)
    batch.close()
    text = bases.tobytes()
    first = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    pairs = []
    for r in range(n_reads):
        read = text[int(off[r]): int(off[r + 1])].decode()
        s = seeds[first[r]: first[r + 1]]
        for j in range(1, len(s)):
            s_end, t0, t_len = int(s[j - 1]["start"]) + int(s[j - 1]["len"]), int(s[j]["start"]), int(s[j]["len"])
            if s_end < 60 or t0 <= s_end or t_len < 17:
                continue
            pairs.append((read[s_end - 60: s_end], read[s_end: t0], read[t0: t0 + t_len], t0 - s_end))
        if len(pairs) >= want_pairs:
            break
    return idx, ctx, pairs, n_reads, n_sym


def kernel_times(args) -> dict:
    """One child run of this tool under rocprofv3 --kernel-trace --stats: total time per kernel of the saipb call and its set-up."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, __file__, "--call-only",
               "--genome-mb", str(args.genome_mb), "--pairs", str(args.pairs)]
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
                if "saipb" in name:
                    out[name.split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=0.3)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--host-pairs", type=int, default=500)
    ap.add_argument("--out", default=str(REPO / "profiles" / "saipb_kernel_rate.json"))
    ap.add_argument("--call-only", action="store_true", help="set-up and one call (the child run under the profiler)")
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    api = Lrsc()
    with tempfile.TemporaryDirectory() as d:
        work = Path(d)
        idx, ctx, pairs, n_reads, n_sym = workload(api, args.genome_mb, args.pairs, work)
        seq, seeds, jobs = saipb_pair_jobs(pairs)
        if args.call_only:
            ctx.saipb_merge(seq, seeds, jobs)
            return
        res, _, _ = ctx.saipb_merge(seq, seeds, jobs)                      # warm-up (buffers, code objects)
        times = []
        for _ in range(3):
            t = time.perf_counter()
            res, _, _ = ctx.saipb_merge(seq, seeds, jobs)
            times.append(time.perf_counter() - t)
        codes = {}
        for r in res[: len(pairs)]:
            key = str(r.code) if r.status == 0 else f"status{r.status}"
            codes[key] = codes.get(key, 0) + 1
        dev_s = statistics.median(times)
        ctx.close(); idx.close()

        # (b) the host class over the C ABI, in its own process (tests/host_tools/saipb_driver.cpp in `device` mode)
        build = REPO / "longreadselfcorrect_amd" / "_build"
        exe = work / "saipb_driver"
        subprocess.run(["g++", "-std=c++14", "-O2", "-o", str(exe), str(REPO / "tests/host_tools/saipb_driver.cpp"),
                        str(REPO / "longreadselfcorrect_amd/host/SAIPBSelfCTree.cpp"), f"-L{build}", "-llrsc_hip", f"-Wl,-rpath,{build}",
                        "-Wl,-rpath,/opt/rocm/lib"], check=True)
        sub = pairs[: args.host_pairs]
        text = "".join(f"{s} {b or '-'} {t} {dis}\n" for s, b, t, dis in sub)

        def drive(inp):
            t = time.perf_counter()
            out = subprocess.run([str(exe), "device", str(work / "reads.bwt"), str(work / "reads.rbwt")], input=inp, capture_output=True,
                                 text=True, check=True, timeout=DRIVER_TIMEOUT_S).stdout
            return time.perf_counter() - t, out
        setup_s, _ = drive("")
        host_total_s, host_out = drive(text)
        host_s = max(host_total_s - setup_s, 1e-9)
        host_codes = [int(l.split(" ")[0]) for l in host_out.split("\n")[:-1]]
        agree = host_codes == [r.code for r in res[: len(sub)]]

    result = {
        "workload": {"genome_mb": args.genome_mb, "reads": n_reads, "symbols": n_sym, "pairs": len(pairs), "codes": codes},
        "kernel_call": {"seconds_median_of_3": dev_s, "seconds_all": times, "pairs_per_s": len(pairs) / dev_s},
        "host_class_over_abi": {"pairs": len(sub), "seconds": host_s, "setup_seconds": setup_s, "pairs_per_s": len(sub) / host_s,
                                "codes_equal_kernel": agree},
        "ratio": (len(pairs) / dev_s) / (len(sub) / host_s),
        "kernels": {} if args.no_profile else kernel_times(args),
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
