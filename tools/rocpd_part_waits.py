"""Where a part's DP stage waits for the other part, from a rocprofv3 --kernel-trace rocpd database of bench.py's default
(two parts per step, each on its own context): python tools/rocpd_part_waits.py DB

Per long-gap launch (wp_extend_wave_kernel on a context's side stream), that is per step and part:
  (a) start of the part's first dp_retrieve minus the end of the long-gap launch (negative: the DP call runs beside it);
  (c) start of the second DP call's first kernel (dp_seed) minus the end of the long-gap launch (it needs that launch's
      results, so it cannot be negative; what is above a few ms is a wait for something else).
Then (b) every dp_msa_kernel dispatch with more than 64 KB of LDS, its duration and the extension kernel that was in flight beside
it for the longest time, and (d) the stream -> hardware queue map of the run's lrsc kernels."""
import collections, sqlite3, sys

db = sqlite3.connect(sys.argv[1]); cur = db.cursor()
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
disp = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
sym = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
cols = [r[1] for r in cur.execute(f"pragma table_info({disp})")]
lds_col = next((c for c in ("group_segment_size", "lds_block_size", "lds_size") if c in cols), None)
lds_sql = lds_col if lds_col else "0"
q_sql = "queue_id" if "queue_id" in cols else "0"
ks = dict(cur.execute(f"select id, kernel_name from {sym}"))
K = collections.namedtuple("K", "start end name stream queue grid lds")
rows = [K(s, e, ks[k], st, q, gx, lds) for k, s, e, st, q, gx, lds in
        cur.execute(f"select kernel_id,start,end,stream_id,{q_sql},grid_size_x,{lds_sql} from {disp} order by start")]
w = [r for r in rows if "lrsc" in r.name]
if not w:
    sys.exit("no lrsc kernels in the trace")
t0 = w[0].start
queues = {q: i + 1 for i, q in enumerate(sorted({r.queue for r in rows}))}
ms = lambda t: (t - t0) / 1e6
dur = lambda r: (r.end - r.start) / 1e6
has = lambda r, s: s in r.name

by_stream = collections.defaultdict(list)
for r in w:
    by_stream[r.stream].append(r)
mains = sorted((s for s, v in by_stream.items() if any(has(r, "wp_begin_kernel") for r in v)), key=lambda s: by_stream[s][0].start)
part_of = {s: i + 1 for i, s in enumerate(mains)}
ext = [r for r in w if has(r, "wp_extend")]
# the long-gap launches: wave kernels on a stream that is no context's main stream
longs = [r for r in ext if has(r, "wp_extend_wave_kernel") and r.stream not in part_of]

print("# (a), (c): per long-gap launch; times in ms from the first lrsc kernel of the run")
step_of = collections.Counter()
for L in longs:
    # its context: the main stream whose bulk launch (wp_extend_kernel) ended last before it started
    prev = [r for r in ext if r.stream in part_of and has(r, "wp_extend_kernel") and r.end <= L.start + 1_000_000]
    if not prev:
        continue
    bulk = max(prev, key=lambda r: r.end)
    m = bulk.stream
    after = [r for r in by_stream[m] if r.start >= bulk.end]
    stitch = next((r.start for r in after if has(r, "wp_stitch")), after[-1].end + 1 if after else L.end)
    win = [r for r in after if r.start < stitch]
    retr = [r for r in win if has(r, "dp_retrieve")]
    seeds = [r for r in win if has(r, "dp_seed")]
    step_of[m] += 1
    a = f"{(retr[0].start - L.end) / 1e6:+8.1f}" if retr else "     n/a"
    c = f"{(seeds[1].start - L.end) / 1e6:+8.1f}" if len(seeds) > 1 else "     n/a"
    print(f"step {step_of[m]} part {part_of[m]}: long-gap launch stream {L.stream} queue {queues[L.queue]}  {ms(L.start):9.1f} + {dur(L):6.1f} = {ms(L.end):9.1f};"
          f"  (a) first dp_retrieve (stream {m} queue {queues[by_stream[m][0].queue]}) {a} ms from its end;  (c) second DP call {c} ms from its end")

print("# (b): dp_msa_kernel dispatches with more than 64 KB of LDS" + ("" if lds_col else " (the trace has no LDS column: every dispatch of 20 ms and more)"))
for r in w:
    if not has(r, "dp_msa_kernel") or (r.lds <= 65536 if lds_col else dur(r) < 20):
        continue
    beside = [(min(r.end, x.end) - max(r.start, x.start), x) for x in ext if x.start < r.end and x.end > r.start]
    part = part_of.get(r.stream, "?")
    line = f"t={ms(r.start):9.1f}  dur={dur(r):7.1f} ms  stream {r.stream} queue {queues[r.queue]}  grid {r.grid:6d}  lds {r.lds:6d} B;"
    if beside:
        ov, x = max(beside, key=lambda p: p[0])
        kind = "long-gap" if x.stream not in part_of else "on a main stream"
        line += f"  beside it for {ov / 1e6:6.1f} ms: {x.name.split('lrsc')[1][:24]} ({kind}, stream {x.stream}) of {dur(x):6.1f} ms -> MSA / extension = {dur(r) / max(dur(x), 1e-9):.2f}"
    else:
        line += "  no extension kernel in flight"
    print(line)

print("# (d): stream -> hardware queue {queue: dispatches} of every lrsc kernel of the run; main streams " + ", ".join(map(str, mains))
      + "; long-gap streams " + ", ".join(map(str, sorted({r.stream for r in longs}))))
sq = collections.defaultdict(collections.Counter)
for r in w:
    sq[r.stream][queues[r.queue]] += 1
for s in sorted(sq):
    print(f"#  stream {s} {dict(sq[s])}")
