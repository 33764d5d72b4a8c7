// capi_dp.cpp -- the DP/MSA fallback: the align launches per staging-size class, the DP stage (seeds -> retrieve -> align -> MSA)
// and the two entry points that expose them, lrsc_dp_align and lrsc_dp_consensus.
#include "capi_internal.h"
#include "dp_deal.h"

using namespace lrsc;

// The launches of one set of alignments: one per non-empty staging-size class (dp_dev.h), each with the LDS, the traceback stride and
// the wavefront count of its own largest alignment, then the global-workspace variant for what is beyond the LDS stage.
// Each launch's wavefronts draw its alignments from the class's list in `order` (dp_order.h), uploaded by the caller, and from one
// head word per class.
struct DpAlignClasses {
    struct Class { uint32_t max_s1 = 0, stage_max = 0; uint64_t jobs = 0; } cls[kDpAlignClasses + 1];
    std::vector<DpOrderRun> runs;
    DpOrder order;                         // set by sort(); the host copy outlives its asynchronous upload
    // jobs first_job .. first_job + n_jobs - 1: alignments of s1_len columns that need stage_bytes of staging
    void add(uint32_t s1_len, uint32_t stage_bytes, uint32_t first_job, uint32_t n_jobs)
    {
        const uint32_t k = dp_align_class(stage_bytes);
        Class& c = cls[k];
        c.max_s1 = std::max(c.max_s1, s1_len); c.stage_max = std::max(c.stage_max, stage_bytes); c.jobs += n_jobs;
        if(n_jobs) runs.push_back({k, first_job, n_jobs});
    }
    void sort() { order = dp_order_build(runs); }
    // wavefronts of class k's launch; wave_cap: LRSC_DP_ALIGN_WAVES (0 = none)
    uint32_t waves(uint32_t k, uint32_t lds_waves, uint32_t wave_cap) const
    {
        const Class& c = cls[k];
        if(!c.jobs) return 0;
        uint64_t want = k < kDpAlignClasses ? lds_waves : 1024;
        if(wave_cap) want = std::min<uint64_t>(want, wave_cap);
        const uint64_t stride = (uint64_t)(c.max_s1 + 17) * kDpTraceStride;
        return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, c.jobs), (4ull << 30) / stride));
    }
    // `order` to the device and the head words zeroed, on the ctx's stream; d_heads: kDpAlignClasses + 1 words
    int upload(lrsc_ctx* ctx, DevBuf<uint32_t>& d_order, DevBuf<uint32_t>& d_heads) const
    {
        HIP_TRY(d_order.reserve(std::max<size_t>(order.list.size(), 1)));
        HIP_TRY(d_heads.reserve(kDpAlignClasses + 1));
        if(!order.list.empty())
            HIP_TRY(hipMemcpyAsync(d_order.p, order.list.data(), order.list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(d_heads.p, 0, (kDpAlignClasses + 1) * sizeof(uint32_t), ctx->stream));
        return LRSC_OK;
    }
    // `al`: everything but the per-launch fields; lds_waves: wavefronts of an LDS launch (the traceback scratch is capped at 4 GB);
    // d_order, d_heads: as upload() left them
    int launch(lrsc_ctx* ctx, DpAlignArgs al, uint32_t lds_waves, uint32_t wave_cap, DevBuf<uint8_t>& d_trace, DevBuf<uint8_t>& d_seq_ws,
               const DevBuf<uint32_t>& d_order, const DevBuf<uint32_t>& d_heads) const
    {
        uint32_t nw[kDpAlignClasses + 1] = {};
        uint64_t stride[kDpAlignClasses + 1] = {}, trace_bytes = 0, ws_bytes = 0;
        for(uint32_t k = 0; k <= kDpAlignClasses; ++k) {
            const Class& c = cls[k];
            if(!c.jobs) continue;
            stride[k] = (uint64_t)(c.max_s1 + 17) * kDpTraceStride;
            nw[k] = waves(k, lds_waves, wave_cap);
            trace_bytes = std::max(trace_bytes, stride[k] * nw[k]);
            if(k == kDpAlignClasses) ws_bytes = (((uint64_t)c.stage_max + 255) & ~255ull) * nw[k];
        }
        HIP_TRY(d_trace.reserve(std::max<uint64_t>(trace_bytes, 64)));
        if(ws_bytes) HIP_TRY(d_seq_ws.reserve(ws_bytes));
        al.trace = d_trace.p;
        for(uint32_t k = 0; k <= kDpAlignClasses; ++k) {
            if(!nw[k]) continue;
            if(order.size(k) != cls[k].jobs) return fail(LRSC_ERR_DEVICE, "dp_align: a class's job list does not hold its jobs");
            al.list = d_order.p + order.begin[k]; al.n_list = order.size(k); al.head = d_heads.p + k;
            al.stage_max = cls[k].stage_max;
            al.trace_stride = stride[k];
            al.seq_ws = k < kDpAlignClasses ? nullptr : d_seq_ws.p;
            al.seq_ws_stride = k < kDpAlignClasses ? 0 : ((uint64_t)cls[k].stage_max + 255) & ~255ull;
            const uint32_t n = nw[k];
            const int st = timed_launch(ctx, LRSC_K_DP, [&]() { return launch_dp_align(al, n, ctx->stream); });
            if(st != LRSC_OK) return st;
        }
        return LRSC_OK;
    }
};

DpStage::~DpStage()
{
    for(int i = 0; i < kSide; ++i) {
        if(side_done[i]) (void)hipEventDestroy(side_done[i]);
        if(side[i]) (void)hipStreamDestroy(side[i]);
    }
}

// Requests [begin, end) of a run: as many as fit the memory budget at once, with the sizes of their strings and edit scripts.
struct DpStage::Chunk {
    uint32_t begin = 0, end = 0, lds = 0;
    uint64_t jobs = 0, sbytes = 0, obytes = 0;
    DpAlignClasses classes;
    DpPipeArgs args{};                     // the chunk's launches (set once its buffers are reserved)
    uint32_t size() const { return end - begin; }
};

// capacities of every request's strings, edit scripts, consensus and pile-up columns; the consensus buffer's layout
int DpStage::size_requests(std::vector<DpRequest>& reqs)
{
    for(DpRequest& r : reqs) {
        if(r.k == 0 || r.lq < r.k) return fail(LRSC_ERR_ARG, "dp request: kmer_len must satisfy 1 <= kmer_len <= query length");
        if(r.coverage > 1000) return fail(LRSC_ERR_UNSUPPORTED, "dp request: coverage above 1000 (12-bit column counters)");
        r.max_len = (uint32_t)(size_t)(r.lq * 1.1 + 20);                 // LongReadOverlap.cpp:618
        r.str_cap = (std::max(r.max_len, r.k) + 3) & ~3u;
        r.ops_cap = (r.lq + r.str_cap + 1 + 3) & ~3u;
        r.cons_cap = dp_cons_capacity(r.lq);
        r.w_cols = dp_msa_columns(r.lq);
        r.cons_off = cons_total;
        cons_total += r.cons_cap;
    }
    return LRSC_OK;
}

// the chunk that starts at `begin`: requests (after the seed kernel counted their strings) until the next would pass the budget
DpStage::Chunk DpStage::plan_chunk(std::vector<DpRequest>& reqs, uint32_t begin, uint64_t budget)
{
    Chunk ch;
    ch.begin = ch.end = begin;
    while(ch.end < reqs.size()) {
        DpRequest& r = reqs[ch.end];
        r.n_str = r.cnt[0] + r.cnt[1] + r.cnt[2] + r.cnt[3];
        const uint64_t sb = (uint64_t)r.n_str * r.str_cap, ob = (uint64_t)r.n_str * r.ops_cap;
        if(ch.end > begin && ch.sbytes + ch.obytes + sb + ob + (ch.jobs + r.n_str) * (sizeof(DpJob) + sizeof(DpAlignOut)) > budget) break;
        r.job_first = ch.jobs; r.str_off = ch.sbytes; r.ops_off = ch.obytes;
        ch.jobs += r.n_str; ch.sbytes += sb; ch.obytes += ob;
        ch.classes.add(r.lq, dp_align_stage_bytes(r.lq, r.str_cap), (uint32_t)r.job_first, r.n_str);
        ch.lds = std::max(ch.lds, dp_msa_lds_bytes(r.w_cols, r.lq, r.str_cap, r.ops_cap, r.n_str));
        ++ch.end;
    }
    return ch;
}

// The LDS of a CU that an MSA launch may count on.  Two ctxs share the device, and beside a DP stage the other ctx's long-gap launch
// (WpFlow::start_long_walks) is usually in flight: wp_side_waves() workgroups of wp_extend_wave_kernel, each with the kernel's static
// LDS (its mask table), resident for hundreds of ms.  A launch sized for an empty CU cannot be placed beside them: its workgroups
// wait until that launch drains.  So the budget is the CU's LDS less what those workgroups hold, each rounded up to the granule in
// which LDS is handed out; LRSC_MSA_LDS_MAX lowers it further (a test hook: small pile-ups then cross the ceilings).
int DpStage::msa_lds_budget(lrsc_ctx* ctx, const Tunables& tn, uint32_t* budget) const
{
    uint32_t wg_lds = 0;
    HIP_TRY(wp_extend_wave_static_lds(ctx->fm.wide != 0, &wg_lds));
    int cus = 256;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const uint64_t wgs_per_cu = (wp_side_waves(tn) + (uint64_t)cus - 1) / (uint64_t)cus;
    const uint64_t held = wgs_per_cu * (((uint64_t)wg_lds + kLdsGranule - 1) / kLdsGranule * kLdsGranule);
    uint32_t b = held < kLdsPerCu ? (uint32_t)(kLdsPerCu - held) : 0u;
    if(tn.msa_lds_max) b = std::min(b, tn.msa_lds_max);
    *budget = b;
    return LRSC_OK;
}

int DpStage::run(lrsc_ctx* ctx, const Tunables& tn, const uint8_t* d_query_codes, std::vector<DpRequest>& reqs)
{
    const uint32_t n = (uint32_t)reqs.size();
    n_strings = 0; cons_total = 0;
    if(n == 0) return LRSC_OK;
    int st = size_requests(reqs);
    if(st == LRSC_OK) st = msa_lds_budget(ctx, tn, &lds_budget);
    if(st != LRSC_OK) return st;
    if(tn.profile) std::fprintf(stderr, "[lrsc] msa: LDS budget per CU %u B\n", (unsigned)lds_budget);
    HIP_TRY(d_reqs.reserve(n));
    HIP_TRY(d_msa.reserve(n));
    HIP_TRY(d_cons.reserve(cons_total));
    HIP_TRY(hipMemcpyAsync(d_reqs.p, reqs.data(), (size_t)n * sizeof(DpRequest), hipMemcpyHostToDevice, ctx->stream));
    DpPipeArgs a{};
    a.codes = d_query_codes; a.reqs = d_reqs.p; a.n_reqs = n; a.ctr = ctx->d_ctr;
    a.row_batch = tn.msa_batch; a.msa_nw = 1;
    st = timed_launch(ctx, LRSC_K_LF, [&]() { return launch_dp_seeds(ctx->fm, a, ctx->stream); });
    if(st != LRSC_OK) return st;
    COPY_TRY(ctx, reqs.data(), d_reqs.p, (size_t)n * sizeof(DpRequest), hipMemcpyDeviceToHost);

    // 8 wavefronts per SIMD hide the scan's cross-lane latency
    const uint32_t n_waves = resident_waves(ctx, 8);
    for(uint32_t begin = 0; begin < n;) {
        Chunk ch = plan_chunk(reqs, begin, tn.dp_chunk_bytes);
        if(ch.jobs >= (1ull << 32)) return fail(LRSC_ERR_UNSUPPORTED, "dp chunk: too many alignments");
        HIP_TRY(hipMemcpyAsync(d_reqs.p + begin, reqs.data() + begin, (size_t)ch.size() * sizeof(DpRequest), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(d_strings.reserve(std::max<uint64_t>(ch.sbytes, 64)));
        HIP_TRY(d_ops.reserve(std::max<uint64_t>(ch.obytes, 64)));
        HIP_TRY(d_jobs.reserve(std::max<uint64_t>(ch.jobs, 1)));
        HIP_TRY(d_align.reserve(std::max<uint64_t>(ch.jobs, 1)));
        DpPipeArgs& c = ch.args;
        c = a;
        c.reqs = d_reqs.p + begin; c.n_reqs = ch.size(); c.n_jobs = ch.jobs;
        c.strings = d_strings.p; c.jobs = d_jobs.p; c.align = d_align.p; c.ops = d_ops.p;
        c.cons = d_cons.p; c.msa = d_msa.p + begin; c.lds_bytes = ch.lds;
        // the align launches' job lists go up before the retrieve launch: the copy is then not between it and the first align launch
        ch.classes.sort();
        st = ch.classes.upload(ctx, d_align_order, d_align_heads);
        if(st != LRSC_OK) return st;
        st = timed_launch(ctx, LRSC_K_LF, [&]() { return launch_dp_retrieve(ctx->fm, c, ctx->stream); });
        if(st == LRSC_OK) st = align_chunk(ctx, tn, reqs, ch, (uint32_t)std::min<uint64_t>(n_waves, ch.jobs));
        if(st == LRSC_OK) st = msa_chunk(ctx, tn, reqs, ch);
        if(st != LRSC_OK) return st;
        n_strings += ch.jobs;
        begin = ch.end;
    }
    return LRSC_OK;
}

// extendMatch for every retrieved string of the chunk, then the statistics LRSC_CORRECT_PROFILE / LRSC_DP_DEBUG ask for
int DpStage::align_chunk(lrsc_ctx* ctx, const Tunables& tn, const std::vector<DpRequest>& reqs, const Chunk& ch, uint32_t lds_waves)
{
    const uint64_t jobs = ch.jobs;
    if(jobs) {
        DpAlignArgs al{};
        al.codes = ch.args.codes; al.strings = d_strings.p; al.jobs = d_jobs.p; al.n_jobs = (uint32_t)jobs;
        al.band_width = 200; al.match_score = 1; al.gap_penalty = -1; al.mismatch_penalty = -8;   // LongReadOverlap.cpp:635-643
        al.ops = d_ops.p; al.out = d_align.p; al.reqs = ch.args.reqs;
        const int st = ch.classes.launch(ctx, al, lds_waves, tn.dp_align_waves, d_trace, d_seq_ws, d_align_order, d_align_heads);
        if(st != LRSC_OK) return st;
    }
    if(tn.profile && ch.begin == 0 && jobs) {
        std::vector<DpAlignOut> ao(jobs);
        (void)hipMemcpy(ao.data(), d_align.p, jobs * sizeof(DpAlignOut), hipMemcpyDeviceToHost);
        double tf = 0, tt = 0, cols = 0, na = 0, trips = 0;
        for(const DpAlignOut& o : ao) if(!o.skipped) { tf += o.t_fill; tt += o.t_trace; cols += o.total_columns; na += 1; trips += o.t_trips; }
        // how evenly the queue loaded the wavefronts of the class with the most alignments: every alignment records who drew it
        uint32_t big = 0;
        for(uint32_t k = 1; k <= kDpAlignClasses; ++k) if(ch.classes.cls[k].jobs > ch.classes.cls[big].jobs) big = k;
        const uint32_t nw = ch.classes.waves(big, lds_waves, tn.dp_align_waves);
        std::vector<double> wave(std::max(nw, 1u), 0.0);
        const DpOrder& order = ch.classes.order;
        for(uint32_t t = order.begin[big]; t < order.begin[big + 1]; ++t) {
            const DpAlignOut& o = ao[order.list[t]];
            wave[o.wave % wave.size()] += (double)o.t_fill + o.t_trace;
        }
        double w_max = 0, w_sum = 0;
        for(double w : wave) { w_max = std::max(w_max, w); w_sum += w; }
        std::fprintf(stderr, "[lrsc] align: %llu jobs (%.0f aligned), %.0f columns avg, per job %.0f ticks fill + %.0f ticks traceback, %.1f trips of %.2f steps; "
                             "%u waves, busiest / mean %.3f; jobs / lds B per class:",
                     (unsigned long long)jobs, na, cols / std::max(na, 1.0), tf / std::max(na, 1.0), tt / std::max(na, 1.0), trips / std::max(na, 1.0),
                     cols / std::max(trips, 1.0), (unsigned)nw, w_sum > 0 ? w_max * wave.size() / w_sum : 0.0);
        for(const DpAlignClasses::Class& k : ch.classes.cls) std::fprintf(stderr, " %llu / %u", (unsigned long long)k.jobs, k.stage_max);
        std::fprintf(stderr, " (the last from global memory)\n");
    }
    if(tn.dp_debug) {
        std::vector<DpAlignOut> ao(jobs);
        std::vector<DpJob> jj(jobs);
        (void)hipMemcpy(ao.data(), d_align.p, jobs * sizeof(DpAlignOut), hipMemcpyDeviceToHost);
        (void)hipMemcpy(jj.data(), d_jobs.p, jobs * sizeof(DpJob), hipMemcpyDeviceToHost);
        for(uint32_t i = ch.begin; i < ch.end && i < ch.begin + 3; ++i) {
            const DpRequest& r = reqs[i];
            std::fprintf(stderr, "[dp] req %u lq %u k %u cov %u cnt %u %u %u %u rows %llu %llu %llu %llu n_str %u max_len %u\n", i, r.lq, r.k,
                         r.coverage, r.cnt[0], r.cnt[1], r.cnt[2], r.cnt[3], (unsigned long long)r.row_lo[0], (unsigned long long)r.row_lo[1],
                         (unsigned long long)r.row_lo[2], (unsigned long long)r.row_lo[3], r.n_str, r.max_len);
            for(uint32_t s = 0; s < r.n_str; ++s) {
                const DpAlignOut& o = ao[r.job_first + s];
                std::fprintf(stderr, "[dp]   str %u len %u mode %u skipped %u accept %u cols %d edit %d m0 %d-%d m1 %d-%d nops %u\n", s,
                             jj[r.job_first + s].s2_len, jj[r.job_first + s].mode, o.skipped, o.accept, o.total_columns, o.edit_distance,
                             o.m0s, o.m0e, o.m1s, o.m1e, o.n_ops);
            }
        }
    }
    return LRSC_OK;
}

// One MSA launch: the requests of one LDS-size bucket, d_list[list_first .. list_first + args.n_list).
struct DpStage::MsaLaunch {
    DpPipeArgs args;
    size_t list_first;
    bool global_ws;                        // the bucket beyond the LDS budget: pile-up state in d_msa_ws
    uint64_t work;                         // sum of query length x strings over its requests (dp_deal.h)
};

// The launches for the chunk's requests `todo`, one per non-empty bucket, and their request lists back to back in `lists`; returns
// the bytes of global workspace the last bucket's launch needs (0: none).  A bucket holds the requests of which kWgsPerCu[..]
// workgroups fit the LDS budget of a CU (lds_budget) and one more does not; what is beyond the budget goes to the global-workspace
// variant.  Wavefronts per workgroup: `waves` where LRSC_MSA_WAVES sets it, else the bucket's own (kMsaWideWaves in the global launch
// and in the bucket of two workgroups per CU, whose launches are shorter with them; 1 in the others).  A wide workgroup's
// cross-wavefront words count towards its LDS, so a request is sized per bucket.
uint64_t DpStage::msa_buckets(const std::vector<DpRequest>& reqs, const Chunk& ch, const std::vector<uint32_t>& todo, bool force_global,
                              uint32_t waves, std::vector<MsaLaunch>& launches, std::vector<uint32_t>& lists) const
{
    static const struct { uint32_t wgs_per_cu, waves; } kBuckets[] = {{20, 1}, {13, 1}, {10, 1}, {8, 1}, {6, 1}, {5, 1}, {4, 1},
                                                                      {2, kMsaWideWaves}, {1, 1}, {0, kMsaWideWaves}};   // 0: the global-workspace launch
    std::vector<uint8_t> taken(todo.size(), 0);
    uint64_t ws_bytes = 0;
    for(const auto& b : kBuckets) {
        const uint32_t w = b.wgs_per_cu;
        if(force_global && w) continue;
        const uint32_t bk = w ? (lds_budget / w) & ~15u : 0xFFFFFFFFu;
        const uint32_t nw = waves ? waves : b.waves;
        const size_t first = lists.size();
        uint32_t need_max = 0, str_max = 0;
        for(size_t t = 0; t < todo.size(); ++t) {
            if(taken[t]) continue;
            const DpRequest& r = reqs[ch.begin + todo[t]];
            const uint32_t need = dp_msa_lds_bytes(r.w_cols, r.lq, r.str_cap, r.ops_cap, r.n_str, nw);
            if(need > bk) continue;
            taken[t] = 1;
            lists.push_back(todo[t]); need_max = std::max(need_max, need); str_max = std::max(str_max, r.n_str);
        }
        if(lists.size() == first) continue;
        // a launch hands its requests to the wavefronts round-robin: the biggest pile-ups (rows x columns) first, so that the
        // launch does not end on one of them
        std::sort(lists.begin() + (std::ptrdiff_t)first, lists.end(), [&](uint32_t x, uint32_t y) {
            const DpRequest& rx = reqs[ch.begin + x]; const DpRequest& ry = reqs[ch.begin + y];
            const uint64_t wx = (uint64_t)rx.lq * rx.n_str, wy = (uint64_t)ry.lq * ry.n_str;
            return wx != wy ? wx > wy : x < y;
        });
        MsaLaunch L{ch.args, first, w == 0, 0};
        for(size_t t = first; t < lists.size(); ++t) { const DpRequest& r = reqs[ch.begin + lists[t]]; L.work += (uint64_t)r.lq * r.n_str; }
        L.args.n_list = (uint32_t)(lists.size() - first);
        L.args.lds_bytes = (need_max + 15) & ~15u;
        L.args.msa_nw = nw;
        L.args.lds_small = dp_msa_small_bytes(str_max);
        if(L.global_ws) {
            // one slot per workgroup of the launch: as many as its list has requests, or, where this bucket is the pass's first
            // (nothing fits the LDS, or LRSC_MSA_FORCE_GLOBAL), as many as the chunk has (dp_msa_waves counts n_reqs without a list)
            DpPipeArgs sized = L.args;
            sized.req_list = first ? d_list.p : nullptr;
            ws_bytes = (uint64_t)L.args.lds_bytes * dp_msa_waves(sized, true, lds_budget);
        }
        launches.push_back(L);
    }
    return ws_bytes;
}

// Multiple alignments of the chunk: one launch per LDS-size bucket (a wide pile-up must not cut everyone's occupancy), dealt to the
// side streams (dp_deal.h), a global-memory variant for the few that exceed the LDS budget; a pile-up that opened more gap columns
// than its capacity is redone with twice the columns.
int DpStage::msa_chunk(lrsc_ctx* ctx, const Tunables& tn, std::vector<DpRequest>& reqs, const Chunk& ch)
{
    const uint32_t nc = ch.size(), begin = ch.begin;
    std::vector<DpMsaOut> mo(nc);
    std::vector<uint32_t> todo(nc), redo;
    for(uint32_t i = 0; i < nc; ++i) todo[i] = i;
    HIP_TRY(d_list.reserve(nc));
    while(!todo.empty()) {
        std::vector<MsaLaunch> launches;
        std::vector<uint32_t> all_lists;
        const uint64_t ws_bytes = msa_buckets(reqs, ch, todo, tn.msa_force_global, tn.msa_waves, launches, all_lists);
        HIP_TRY(d_list.reserve(std::max<size_t>(all_lists.size(), 1)));
        if(ws_bytes) HIP_TRY(d_msa_ws.reserve(ws_bytes));
        HIP_TRY(hipMemcpyAsync(d_list.p, all_lists.data(), all_lists.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(d_msa_ctr.reserve(std::max<size_t>(launches.size(), 16)));
        HIP_TRY(hipMemsetAsync(d_msa_ctr.p, 0, launches.size() * sizeof(uint32_t), ctx->stream));
        for(size_t j = 0; j < launches.size(); ++j) {
            MsaLaunch& L = launches[j];
            L.args.req_list = d_list.p + L.list_first;
            if(L.global_ws) L.args.msa_ws = d_msa_ws.p;
            L.args.work_ctr = d_msa_ctr.p + j;
        }
        for(int i = 0; i < kSide; ++i) {
            if(!side[i]) HIP_TRY(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
            if(!side_done[i]) HIP_TRY(hipEventCreateWithFlags(&side_done[i], hipEventDisableTiming));
        }
        std::vector<DpDealLaunch> dl;
        for(const MsaLaunch& L : launches) dl.push_back({L.work, L.global_ws ? 0u : L.args.lds_bytes});
        const std::vector<std::vector<uint32_t>> deal = dp_deal(dl, (uint32_t)kSide);
        const int st = timed_launch(ctx, LRSC_K_MSA, [&]() -> hipError_t {
            // ctx->ev0 was just recorded on ctx->stream: the side streams start after it (and after the list upload)
            hipError_t e = hipSuccess;
            for(size_t i = 0; i < deal.size() && e == hipSuccess; ++i) {
                if(deal[i].empty()) continue;
                e = hipStreamWaitEvent(side[i], ctx->ev0, 0);
                for(size_t t = 0; t < deal[i].size() && e == hipSuccess; ++t) e = launch_dp_msa(launches[deal[i][t]].args, lds_budget, side[i]);
                if(e == hipSuccess) e = hipEventRecord(side_done[i], side[i]);
            }
            // the waits after every launch: where a side stream shares its hardware queue with ctx->stream, a wait enqueued before
            // that stream's launches would hold them back until the other streams are done
            for(size_t i = 0; i < deal.size() && e == hipSuccess; ++i)
                if(!deal[i].empty()) e = hipStreamWaitEvent(ctx->stream, side_done[i], 0);
            return e;
        });
        if(st != LRSC_OK) return st;
        COPY_TRY(ctx, mo.data(), d_msa.p + begin, (size_t)nc * sizeof(DpMsaOut), hipMemcpyDeviceToHost);
        if(tn.profile) {
            // a request's ticks are a difference of two counter reads; one that came out negative (seen once in 18 720 requests of a
            // wide launch, not explained) counts as 0, so that it cannot pose as the launch's longest request
            for(DpMsaOut& o : mo) if((int32_t)o.kc_total < 0) o.kc_total = 0;
            // one line per launch: is it as long as its longest pile-up?
            for(const MsaLaunch& L : launches) {
                uint64_t sum = 0;
                uint32_t top = all_lists[L.list_first];
                for(uint32_t t = 0; t < L.args.n_list; ++t) {
                    const uint32_t i = all_lists[L.list_first + t];
                    sum += mo[i].kc_total;
                    if(mo[i].kc_total > mo[top].kc_total) top = i;
                }
                const DpRequest& r = reqs[begin + top];
                char where[24];
                if(L.global_ws) std::snprintf(where, sizeof where, "global");
                else std::snprintf(where, sizeof where, "LDS %u B", (unsigned)L.args.lds_bytes);
                std::fprintf(stderr, "[lrsc] msa launch: %s, %u requests, %u workgroups of %u wavefronts, k-ticks sum %llu max %u (w_cols %u, n_str %u, n_rows %u)\n",
                             where, (unsigned)L.args.n_list, (unsigned)dp_msa_waves(L.args, L.global_ws, lds_budget), (unsigned)L.args.msa_nw,
                             (unsigned long long)sum, (unsigned)mo[top].kc_total, (unsigned)r.w_cols, (unsigned)r.n_str, (unsigned)mo[top].n_rows);
            }
        }
        redo.clear();
        for(uint32_t i : todo) {
            if(mo[i].error != 1) continue;                       // 0 = done; 2 = consensus beyond its capacity: stays an error of this request
            DpRequest& r = reqs[begin + i];
            if(r.w_cols > 64u * (r.lq + 128)) continue;           // gives up on this pile-up: the request keeps its error
            r.w_cols *= 2;
            redo.push_back(i);
        }
        if(tn.profile && begin == 0) {
            double kt = 0, ks = 0, ki = 0, ni = 0, rows = 0, walked = 0;
            for(uint32_t i = 0; i < nc; ++i) { kt += mo[i].kc_total; ks += mo[i].kc_stage; ki += mo[i].kc_insert; ni += mo[i].n_insert; rows += mo[i].n_rows; walked += mo[i].pad; }
            std::fprintf(stderr, "[lrsc] msa: %u requests, %.1f rows avg (%.2f by the step walk), %.0f insertions avg, per request %.0f k-ticks (staging %.0f, insertions %.0f), redo %zu\n",
                         nc, rows / nc, walked / nc, ni / nc, kt / nc, ks / nc, ki / nc, redo.size());
        }
        todo = redo;
        if(!todo.empty())
            HIP_TRY(hipMemcpyAsync(d_reqs.p + begin, reqs.data() + begin, (size_t)nc * sizeof(DpRequest), hipMemcpyHostToDevice, ctx->stream));
    }
    return LRSC_OK;
}

extern "C" int lrsc_dp_align(lrsc_ctx* ctx, const char* seq, uint64_t seq_len, const lrsc_dp_job* jobs, uint32_t n, int band_width,
                             int match_score, int gap_penalty, int mismatch_penalty, lrsc_dp_result* results, char* cigar_arena,
                             uint64_t arena_cap, uint64_t* arena_used)
{
    if(!ctx || (!jobs && n) || (!results && n) || !arena_used || (!seq && seq_len)) return fail(LRSC_ERR_ARG, "null");
    *arena_used = 0;
    if(n == 0) return LRSC_OK;
    if(band_width < 2 || (band_width / 2) * 2 + 1 > (int)kDpMaxBand) return fail(LRSC_ERR_UNSUPPORTED, "band_width must be 2..254");
    if(gap_penalty > 0) return fail(LRSC_ERR_ARG, "gap_penalty must be <= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint8_t> codes(seq_len);
    int st = encode_acgt(seq, seq_len, codes.data());
    if(st != LRSC_OK) return st;
    std::vector<DpJob> dj(n);
    uint64_t ops_total = 0;
    DpAlignClasses classes;
    for(uint32_t i = 0; i < n; ++i) {
        const lrsc_dp_job& j = jobs[i];
        if(j.s1_off + j.s1_len > seq_len || j.s2_off + j.s2_len > seq_len) return fail(LRSC_ERR_ARG, "dp job: sequence out of range");
        if(j.s1_len > kDpMaxSeq || j.s2_len > kDpMaxSeq) return fail(LRSC_ERR_UNSUPPORTED, "dp job: sequence too long");
        DpJob& d = dj[i];
        d.s1_off = j.s1_off; d.s2_off = j.s2_off; d.s1_len = j.s1_len; d.s2_len = j.s2_len; d.start1 = j.start1; d.start2 = j.start2;
        d.mode = 0; d.req = 0; d.ops_off = ops_total;
        ops_total += (uint64_t)j.s1_len + j.s2_len + 1;
        classes.add(j.s1_len, dp_align_stage_bytes(j.s1_len, j.s2_len), i, 1);
    }
    classes.sort();
    DevBuf<uint8_t> d_codes, d_ops, d_trace, d_stage;
    DevBuf<uint32_t> d_order, d_heads;                   // of this call: another ctx may be in its own align launches on this device
    DevBuf<DpJob> d_jobs;
    DevBuf<DpAlignOut> d_out;
    DpAlignArgs a{};
    HIP_TRY(d_codes.reserve(std::max<uint64_t>(seq_len, 1)));
    HIP_TRY(d_ops.reserve(ops_total));
    HIP_TRY(d_jobs.reserve(n));
    HIP_TRY(d_out.reserve(n));
    HIP_TRY(hipMemcpyAsync(d_codes.p, codes.data(), seq_len, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_jobs.p, dj.data(), (size_t)n * sizeof(DpJob), hipMemcpyHostToDevice, ctx->stream));
    a.codes = d_codes.p; a.strings = d_codes.p; a.jobs = d_jobs.p; a.n_jobs = n; a.band_width = (uint32_t)band_width;
    a.match_score = match_score; a.gap_penalty = gap_penalty; a.mismatch_penalty = mismatch_penalty;
    a.ops = d_ops.p; a.out = d_out.p;
    // one launch per staging-size class; sequences beyond the 64 KB LDS stage: the same kernel with its staging in a global slice per
    // wavefront (fewer wavefronts)
    st = classes.upload(ctx, d_order, d_heads);
    if(st == LRSC_OK) st = classes.launch(ctx, a, resident_waves(ctx, 2), read_tunables(ctx).dp_align_waves, d_trace, d_stage, d_order, d_heads);
    if(st != LRSC_OK) return st;
    std::vector<DpAlignOut> out(n);
    std::vector<uint8_t> ops(ops_total);
    COPY_TRY(ctx, out.data(), d_out.p, (size_t)n * sizeof(DpAlignOut), hipMemcpyDeviceToHost);
    COPY_TRY(ctx, ops.data(), d_ops.p, ops_total, hipMemcpyDeviceToHost);
    uint64_t used = 0;
    for(uint32_t i = 0; i < n; ++i) {
        const DpAlignOut& o = out[i];
        if(o.n_ops == 0xFFFFFFFFu) return fail(LRSC_ERR_DEVICE, "dp_align: traceback left the band");
        lrsc_dp_result& r = results[i];
        r.match0_start = o.m0s; r.match0_end = o.m0e; r.match1_start = o.m1s; r.match1_end = o.m1e;
        r.score = o.score; r.edit_distance = o.edit_distance; r.total_columns = o.total_columns;
        r.cigar_len = o.n_ops; r.cigar_off = used;
        if(cigar_arena && used + o.n_ops <= arena_cap)
            for(uint32_t t = 0; t < o.n_ops; ++t) cigar_arena[used + t] = (char)ops[dj[i].ops_off + o.n_ops - 1 - t];
        used += o.n_ops;
    }
    *arena_used = used;
    if(used > arena_cap || (!cigar_arena && used)) return fail(LRSC_ERR_CAPACITY, "cigar arena too small");
    return LRSC_OK;
}

extern "C" int lrsc_dp_consensus(lrsc_ctx* ctx, const char* seq, uint64_t seq_len, const lrsc_msa_query* queries, uint32_t n,
                                 lrsc_msa_result* results, char* arena, uint64_t arena_cap, uint64_t* arena_used)
{
    if(!ctx || (!queries && n) || (!results && n) || !arena_used || (!seq && seq_len)) return fail(LRSC_ERR_ARG, "null");
    *arena_used = 0;
    if(n == 0) return LRSC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint8_t> codes(seq_len);
    int st = encode_acgt(seq, seq_len, codes.data());
    if(st != LRSC_OK) return st;
    std::vector<DpRequest> reqs(n);
    for(uint32_t i = 0; i < n; ++i) {
        const lrsc_msa_query& q = queries[i];
        if(q.seq_off + q.len > seq_len) return fail(LRSC_ERR_ARG, "msa query out of range");
        DpRequest& r = reqs[i];
        std::memset(&r, 0, sizeof(r));
        r.q_off = q.seq_off; r.lq = q.len; r.k = q.kmer_len; r.min_overlap = q.min_overlap; r.min_call_coverage = q.min_call_coverage;
        r.min_identity = q.min_identity; r.coverage = (uint32_t)ctx->params.pb_coverage;
    }
    DevBuf<uint8_t> d_codes;
    HIP_TRY(d_codes.reserve(std::max<uint64_t>(seq_len, 1)));
    HIP_TRY(hipMemcpyAsync(d_codes.p, codes.data(), seq_len, hipMemcpyHostToDevice, ctx->stream));
    DpStage stage;
    st = stage.run(ctx, read_tunables(ctx), d_codes.p, reqs);
    if(st != LRSC_OK) return st;
    std::vector<DpMsaOut> mo(n);
    std::vector<uint8_t> cons(stage.cons_total);
    COPY_TRY(ctx, mo.data(), stage.d_msa.p, (size_t)n * sizeof(DpMsaOut), hipMemcpyDeviceToHost);
    COPY_TRY(ctx, cons.data(), stage.d_cons.p, stage.cons_total, hipMemcpyDeviceToHost);
    uint64_t used = 0;
    for(uint32_t i = 0; i < n; ++i) {
        if(mo[i].error) return fail(LRSC_ERR_LIMIT, "msa: column capacity exceeded");
        results[i].n_rows = mo[i].n_rows; results[i].n_retrieved = reqs[i].n_str; results[i].cons_len = mo[i].cons_len; results[i].rows_by_step_walk = mo[i].pad;
        results[i].cons_off = used;
        if(arena && used + mo[i].cons_len <= arena_cap)
            for(uint32_t t = 0; t < mo[i].cons_len; ++t) arena[used + t] = "ACGT"[cons[reqs[i].cons_off + t] & 3u];
        used += mo[i].cons_len;
    }
    *arena_used = used;
    if(used > arena_cap || (!arena && used)) return fail(LRSC_ERR_CAPACITY, "consensus arena too small");
    return LRSC_OK;
}
