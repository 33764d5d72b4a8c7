"""Rate of lrsc_fmwalk_merge (csrc/fm_fmwalk.hip), `stride fmwalk -a merge`'s device step, on one box in one run:

  1. a genome from the testkit generator (--genome-mb, default 1); fragments of 250 to 400 bases from random places at 30x, half of
     them reverse-complemented; a pair is the 100-base ends of a fragment, the second end read from the other strand, with 1 %
     substitutions (--substitution-rate; with 0 the reads are what `stride correct`, the step before fmwalk in the pipeline, aims
     to leave); all reads' own index by lrsc_index_build, which stays resident;
  2. lrsc_fmwalk_merge over all pairs in batches of 100 000, as `stride fmwalk` calls it, with -k 31 -x 3 -m 81 -I 400 -L 32 and
     -M from the lengths: one warm-up run, then three timed runs.  Per run: wall seconds of the calls, pairs/s, merged output
     bases/s, the kernels' own milliseconds, their LF steps per second (one LF step is two Occ queries, from lrsc_ctx_stats under
     K_FIND) and block loads per LF step;
  3. the share of pairs merged, the share of merged strings that are the fragment (on either strand), and the walks' return codes.

Prints profiles/kmer_correct.json's LF steps per second beside the result: the k-mer corrector's chains are the same backward
search, a lane each with no frontier to keep.  Writes profiles/fmwalk_merge.json (or --out).

--algorithm hybrid runs lrsc_fmwalk_hybrid (csrc/fm_kmerize.hip) over the same pairs, its repeat cutoff from 100 000 sampled rows
through lrsc_kmer_sample_counts as `stride fmwalk --hybrid` takes it (the rows from a seeded generator here), and merge mode
alongside in the same session: three runs of each, alternating, and hybrid's ratio to merge.  --algorithm kmerize runs
lrsc_fmwalk_kmerize over the pairs' reads as single reads.  Both add the k-mers whose two single-strand counts a split takes
(KmerContext) per second.  They write profiles/fmwalk_hybrid.json and profiles/fmwalk_kmerize.json.

--algorithm validate runs lrsc_fmwalk_validate (csrc/fm_validate.hip) over the pairs' reads as single reads with --validate-overlap
as -m (default 31: a read of 100 bases is then walked over 69), and, on the first --cpu-reads of the same reads, the CPU build of the
same code, tests/host_tools/fmwalk_validate_driver.cpp (g++ -O2, one process, the lanes of a wavefront one after the other; its time
includes reading the index's RL units and building the rank blocks, which is given apart from a run of no reads).  It writes
profiles/fmwalk_validate.json."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from collections import Counter
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

from longreadselfcorrect_amd import Lrsc, capi  # noqa: E402

READ_LEN, FRAG_MIN, FRAG_MAX, COVERAGE, P_SUB, BATCH = 100, 250, 400, 30, 0.01, 100000
OPTIONS = dict(kmer_length=31, kmer_threshold=3, min_overlap=81, max_overlap=-1, max_insert=400, max_leaves=32)


def workload(api, genome_mb: float, p_sub: float):
    """-> (the pairs' reads as ASCII, 2 n + 1 offsets, the fragments as ASCII strings)"""
    rng = np.random.default_rng(0xF3A1C)
    n = int(genome_mb * 1e6)
    ascii_of = np.frombuffer(b"ACGT", dtype=np.uint8)
    code_of = np.zeros(256, dtype=np.uint8)
    code_of[ascii_of] = np.arange(4, dtype=np.uint8)
    genome = code_of[np.frombuffer(api.synth_genome(0x5EED0001, n), dtype=np.uint8)]
    n_pairs = n * COVERAGE // (2 * READ_LEN)
    sizes = rng.integers(FRAG_MIN, FRAG_MAX + 1, size=n_pairs)
    starts = rng.integers(0, n - FRAG_MAX, size=n_pairs)
    flip = rng.random(n_pairs) < 0.5
    cols = np.arange(READ_LEN)
    left = genome[starts[:, None] + cols[None, :]]
    right = 3 - genome[(starts + sizes - 1)[:, None] - cols[None, :]]          # the other strand, from the fragment's end
    first, second = np.where(flip[:, None], right, left), np.where(flip[:, None], left, right)
    reads = np.stack([first, second], axis=1).reshape(2 * n_pairs, READ_LEN)
    hit = rng.random(reads.shape) < p_sub
    reads[hit] = (reads[hit] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) & 3
    off = (np.arange(2 * n_pairs + 1, dtype=np.uint64) * READ_LEN).astype(np.uint64)
    text = ascii_of[genome].tobytes().decode()
    return ascii_of[reads].reshape(-1), off, [text[s: s + z] for s, z in zip(starts.tolist(), sizes.tolist())]


def one_run(ctx, bases, off):
    n_pairs = (off.size - 1) // 2
    ctx.stats_reset()
    rows, res = [], np.zeros(n_pairs, dtype=capi.FMWALK_DTYPE)
    t = time.perf_counter()
    for a in range(0, n_pairs, BATCH):
        b = min(a + BATCH, n_pairs)
        lo, hi = int(off[2 * a]), int(off[2 * b])
        merged, res[a:b] = ctx.fmwalk_merge(bases[lo:hi], off[2 * a: 2 * b + 1] - off[2 * a], **OPTIONS)
        rows.append(merged)
    wall = time.perf_counter() - t
    s = ctx.stats(capi.K_FIND)
    lf = s.rank_queries / 2
    out_bases = int(res["length"][res["merged"] != 0].sum())
    return np.concatenate(rows), res, {"wall_s": wall, "pairs_per_s": n_pairs / wall, "merged_bases_per_s": out_bases / wall, "kernel_ms": s.total_ms,
                                       "launches": s.launches, "lf_steps": lf, "lf_steps_per_s": lf / (s.total_ms / 1e3),
                                       "block_loads_per_lf_step": s.block_loads / lf}


def _rates(ctx, wall, units, name, context_kmers):
    s = ctx.stats(capi.K_FIND)
    lf = s.rank_queries / 2
    return {"wall_s": wall, f"{name}_per_s": units / wall, "kernel_ms": s.total_ms, "launches": s.launches, "lf_steps": lf,
            "lf_steps_per_s": lf / (s.total_ms / 1e3), "block_loads_per_lf_step": s.block_loads / lf, "context_kmers": context_kmers,
            "context_kmers_per_s": context_kmers / wall}


def hybrid_run(ctx, bases, off, repeat):
    n_pairs = (off.size - 1) // 2
    ctx.stats_reset()
    res, kmers = np.zeros(n_pairs, dtype=capi.FMWALK_HYBRID_DTYPE), 0
    t = time.perf_counter()
    for a in range(0, n_pairs, BATCH):
        b = min(a + BATCH, n_pairs)
        lo, hi = int(off[2 * a]), int(off[2 * b])
        _, res[a:b], _, _ = ctx.fmwalk_hybrid(bases[lo:hi], off[2 * a: 2 * b + 1] - off[2 * a], repeat, **OPTIONS)
    wall = time.perf_counter() - t
    split = res["read"]["n_pieces"] > 0
    kmers = int((res["read"]["length"][split].astype(np.int64) - OPTIONS["kmer_length"] + 1).sum())
    return res, _rates(ctx, wall, n_pairs, "pairs", kmers)


def kmerize_run(ctx, bases, off):
    n = off.size - 1
    ctx.stats_reset()
    res = np.zeros(n, dtype=capi.FMWALK_READ_DTYPE)
    t = time.perf_counter()
    for a in range(0, n, 2 * BATCH):
        b = min(a + 2 * BATCH, n)
        res[a:b], _, _ = ctx.fmwalk_kmerize(bases[int(off[a]): int(off[b])], off[a: b + 1] - off[a], OPTIONS["kmer_length"], OPTIONS["kmer_threshold"])
    wall = time.perf_counter() - t
    kmers = int((res["length"][res["n_pieces"] > 0].astype(np.int64) - OPTIONS["kmer_length"] + 1).sum())
    return res, _rates(ctx, wall, n, "reads", kmers)


def validate_run(ctx, bases, off, options):
    n = off.size - 1
    ctx.stats_reset()
    res = np.zeros(n, dtype=capi.FMWALK_VALIDATE_DTYPE)
    t = time.perf_counter()
    for a in range(0, n, 2 * BATCH):
        b = min(a + 2 * BATCH, n)
        _, res[a:b], _, _ = ctx.fmwalk_validate(bases[int(off[a]): int(off[b])], off[a: b + 1] - off[a], **options)
    wall = time.perf_counter() - t
    kmers = int((res["read"]["length"][res["read"]["n_pieces"] > 0].astype(np.int64) - options["kmer_length"] + 1).sum())
    return res, _rates(ctx, wall, n, "reads", kmers)


def cpu_driver_rate(index, bases, off, options, n_reads):
    """the CPU build of fm_validate.h on the first n_reads reads: (seconds with the reads, seconds of an empty run, its records)"""
    info = index.info()
    images = b"".join(np.array([info.num_symbols, u.size], dtype=np.uint64).tobytes() + u.tobytes() for u in (index.units(0), index.units(1)))
    params = np.array([options["kmer_length"], options["kmer_threshold"], options["min_overlap"], options["max_overlap"], 0, options["max_leaves"]], dtype=np.int32)
    code_of = np.zeros(256, dtype=np.uint8)
    code_of[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        exe = str(Path(d) / "fmwalk_validate_driver")
        subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, str(REPO / "tests/host_tools/fmwalk_validate_driver.cpp"),
                        str(REPO / "longreadselfcorrect_amd/csrc/fm_layout.cpp")], check=True)
        seconds = []
        for n in (n_reads, 1):
            blob = images + params.tobytes() + np.array([n], dtype=np.uint64).tobytes() + off[: n + 1].tobytes() + code_of[bases[: int(off[n])]].tobytes()
            t = time.perf_counter()
            r = subprocess.run([exe, "0"], input=blob, capture_output=True, check=True)
            seconds.append(time.perf_counter() - t)
            if n == n_reads:
                records = np.frombuffer(r.stdout, dtype=capi.FMWALK_VALIDATE_DTYPE, count=n)
    return seconds[0], seconds[1], records


def validate_algorithm(args, index, ctx, bases, off, workload_info):
    out = Path(args.out) if args.out else REPO / "profiles" / "fmwalk_validate.json"
    options = {k: v for k, v in OPTIONS.items() if k != "max_insert"}
    options["min_overlap"] = args.validate_overlap
    validate_run(ctx, bases, off, options)                                 # warm-up
    runs = []
    for _ in range(3):
        res, r = validate_run(ctx, bases, off, options)
        runs.append(r)
        print(r, flush=True)
    n_cpu = min(args.cpu_reads, off.size - 1)
    cpu_s, cpu_empty_s, cpu_res = cpu_driver_rate(index, bases, off, options, n_cpu)
    same = all(bool((cpu_res[f] == res[f][:n_cpu]).all()) for f in ("merged", "length", "status", "max_used_leaves", "coverage", "walk_length", "chosen"))
    med = _median(runs)
    cpu = {"reads": n_cpu, "wall_s": cpu_s, "index_load_s": cpu_empty_s, "reads_per_s": n_cpu / max(cpu_s - cpu_empty_s, 1e-9), "records_equal_the_device_s": same}
    merged, split = res["merged"] != 0, res["read"]["n_pieces"] > 0
    result = {"workload": {**workload_info, **options, "reads": int(off.size - 1)}, "runs": runs, "median": med, "cpu_driver": cpu,
              "device_to_cpu_driver": med["reads_per_s"] / cpu["reads_per_s"],
              "outcome": {"reads_merged_share": float(merged.mean()), "merged_with_a_walk_s_string_share": float((res["chosen"][merged] >= 0).mean()) if merged.any() else 0.0,
                          "reads_split_share": float(split.mean()), "pieces_per_split_read_mean": float(res["read"]["n_pieces"][split].mean()) if split.any() else 0.0,
                          "walk_codes": {str(k): int(v) for k, v in sorted(Counter(res["status"].reshape(-1).tolist()).items())}}}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def _median(runs):
    return {k: statistics.median(r[k] for r in runs) for k in runs[0] if k != "launches"}


def other_algorithms(args, api, ctx, bases, off, workload_info):
    """--algorithm hybrid and kmerize"""
    out = Path(args.out) if args.out else REPO / "profiles" / f"fmwalk_{args.algorithm}.json"
    result = {"workload": workload_info}
    if args.algorithm == "kmerize":
        kmerize_run(ctx, bases, off)                                   # warm-up
        runs = []
        for _ in range(3):
            res, r = kmerize_run(ctx, bases, off)
            runs.append(r)
            print(r, flush=True)
        pieces = res["n_pieces"][res["n_pieces"] > 0]
        result.update(runs=runs, median=_median(runs),
                      outcome={"reads_kmerized_share": float((res["kmerize"] != 0).mean()), "reads_in_one_piece_share": float((pieces == 1).mean()),
                               "pieces_per_read_mean": float(pieces.mean()), "reads_with_a_main_piece_share": float((res["main_piece"] >= 0).mean())})
    else:
        rows = np.random.default_rng(0xC0FFEE).integers(0, off.size - 1, size=100000).astype(np.uint64)
        ctx.stats_reset()
        t = time.perf_counter()
        counts = ctx.kmer_sample_counts(rows, OPTIONS["min_overlap"])
        sample = {"wall_s": time.perf_counter() - t, "kernel_ms": ctx.stats(capi.K_FIND).total_ms, "samples": int(rows.size)}
        q2 = int(np.sort(counts)[counts.size // 2])
        repeat = int(q2 * 1.3)
        hybrid_run(ctx, bases, off, repeat)                                # warm-up
        one_run(ctx, bases, off)
        hybrid, merge = [], []
        for _ in range(3):                                                 # alternating, one session
            res, r = hybrid_run(ctx, bases, off, repeat)
            hybrid.append(r)
            print("hybrid", r, flush=True)
            _, mres, r = one_run(ctx, bases, off)
            merge.append(r)
            print("merge", r, flush=True)
        hm, mm = _median(hybrid), _median(merge)
        merged = res["walk"]["merged"] != 0
        result.update(sample=sample, median_count=q2, repeat_kmer_freq=repeat, runs=hybrid, median=hm, merge_mode_runs=merge, merge_mode_median=mm,
                      hybrid_to_merge={"wall": hm["wall_s"] / mm["wall_s"], "kernel_ms": hm["kernel_ms"] / mm["kernel_ms"]},
                      outcome={"pairs_merged_share": float(merged.mean()), "merge_mode_pairs_merged_share": float((mres["merged"] != 0).mean()),
                               "pairs_walked_share": float((res["walk"]["status"][:, 0] != 0).mean()),
                               "reads_kmerized_share": float((res["read"]["kmerize"] != 0).mean()), "reads_split_share": float((res["read"]["n_pieces"] > 0).mean()),
                               "pieces_per_split_read_mean": float(res["read"]["n_pieces"][res["read"]["n_pieces"] > 0].mean())})
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=1.0)
    ap.add_argument("--substitution-rate", type=float, default=P_SUB, help="0: reads as `stride correct` would leave them")
    ap.add_argument("--algorithm", choices=["merge", "hybrid", "kmerize", "validate"], default="merge")
    ap.add_argument("--validate-overlap", type=int, default=31, help="validate: -m")
    ap.add_argument("--cpu-reads", type=int, default=2000, help="validate: the reads the CPU driver build is given")
    ap.add_argument("--out", default=None, help="default: profiles/fmwalk_<algorithm>.json")
    args = ap.parse_args()
    if args.algorithm == "merge" and args.out is None:
        args.out = str(REPO / "profiles" / "fmwalk_merge.json")
    api = Lrsc()
    bases, off, fragments = workload(api, args.genome_mb, args.substitution_rate)
    t = time.perf_counter()
    index = api.index_build(bases, off, 0)
    build_s = time.perf_counter() - t
    ctx = index.ctx(api.params_default(5, 90), 0)
    if args.algorithm != "merge":
        info = {"genome_mb": args.genome_mb, "pairs": (off.size - 1) // 2, "read_length": READ_LEN, "fragment_bases": [FRAG_MIN, FRAG_MAX], "coverage": COVERAGE,
                "substitution_rate": args.substitution_rate, "bases": int(bases.size), "batch": BATCH, "index_build_s": build_s}
        if args.algorithm == "validate":
            validate_algorithm(args, index, ctx, bases, off, info)
        else:
            other_algorithms(args, api, ctx, bases, off, {**info, **OPTIONS})
        ctx.close()
        index.close()
        return
    one_run(ctx, bases, off)                                           # warm-up: buffers, code objects
    runs = []
    for _ in range(3):
        rows, res, r = one_run(ctx, bases, off)
        runs.append(r)
        print(r, flush=True)
    ctx.close()
    index.close()
    merged = np.flatnonzero(res["merged"])
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    exact = 0
    for i in merged.tolist():
        s = rows[i, : int(res["length"][i])].tobytes()
        exact += s.decode() == fragments[i] or s.translate(comp)[::-1].decode() == fragments[i]
    kc = REPO / "profiles" / "kmer_correct.json"
    kc_rate = json.loads(kc.read_text())["median"]["lf_steps_per_s"] if kc.exists() else None
    result = {
        "workload": {"genome_mb": args.genome_mb, "pairs": int(res.size), "read_length": READ_LEN, "fragment_bases": [FRAG_MIN, FRAG_MAX], "coverage": COVERAGE,
                     "substitution_rate": args.substitution_rate, "bases": int(bases.size), "batch": BATCH, **OPTIONS, "index_build_s": build_s},
        "runs": runs,
        "median": {k: statistics.median(r[k] for r in runs) for k in ("wall_s", "pairs_per_s", "merged_bases_per_s", "kernel_ms", "lf_steps_per_s",
                                                                      "block_loads_per_lf_step")},
        "outcome": {"pairs_merged_share": float(merged.size / res.size), "merged_strings_that_are_the_fragment_share": float(exact / max(merged.size, 1)),
                    "walk_codes": {str(k): int(v) for k, v in sorted(Counter(res["status"].reshape(-1).tolist()).items())},
                    "max_used_leaves_mean": float(res["max_used_leaves"].mean())},
        "kmer_correct_lf_steps_per_s": kc_rate,                        # profiles/kmer_correct.json, for context
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    if kc_rate:
        print(f"LF steps/s: fmwalk merge {result['median']['lf_steps_per_s'] / 1e9:.2f} G, kmer correct {kc_rate / 1e9:.1f} G")


if __name__ == "__main__":
    main()
