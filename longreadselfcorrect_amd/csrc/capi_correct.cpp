// capi_correct.cpp -- lrsc_batch_correct: the walk-parallel flow (wp.h / wp.hip), the default implementation of the whole
// per-read path on the device.  CorrectScratch holds what a ctx keeps between calls, WpFlow is one call.
#include "capi_internal.h"

using namespace lrsc;

// Device buffers of lrsc_batch_correct, kept in the ctx between calls (grow-only): hipMalloc / hipFree synchronise the whole
// device, which serialises contexts that correct sub-batches concurrently on one GPU and costs every call of a loop.
struct lrsc::CorrectScratch {
    DevBuf<ReadPlan> d_plan;
    DevBuf<uint32_t> d_pieces;
    DevBuf<uint8_t> d_codes_out;
    DevBuf<uint64_t> d_dst_off;
    DevBuf<char> d_dst;
    DevBuf<double> d_freqs;
    DpStage stage;
    // the walk-parallel rounds
    DevBuf<WpReadWork> d_work;
    DevBuf<WpRead> d_reads;
    DevBuf<WpSlot> d_slots;
    DevBuf<uint64_t> d_sz;                 // three arrays of (entries + 1)
    DevBuf<uint32_t> d_key, d_key_tmp, d_list, d_list_tmp;
    DevBuf<uint32_t> d_small;              // kWpSmallWords counters and queue heads, laid out by WpSmall (wp.h)
    DevBuf<WpDpItem> d_items, d_items2, d_items3;
    DevBuf<DevCounters> d_ctr2;
    hipEvent_t ev_side_t0 = nullptr, ev_side_t1 = nullptr;
    DevBuf<WpRequest> d_req;
    DevBuf<uint8_t> d_prep, d_lane, d_lane_side, d_lane_wide;
    DevBuf<uint32_t> d_wide_list;          // the escalated walks of a round (-l above the narrow cap)
    DevBuf<uint32_t> d_sort9;              // the interval lists of a round that take the sort (WpArgs::sort9)
    hipStream_t side = nullptr;
    hipEvent_t ev_ready = nullptr;
    DevBuf<unsigned long long> d_prof;
    DevArena persist;
    void* cub_tmp = nullptr;
    size_t cub_cap = 0;
    ~CorrectScratch()
    {
        if(cub_tmp) (void)hipFree(cub_tmp);
        if(side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
        if(ev_ready) (void)hipEventDestroy(ev_ready);
        if(ev_side_t0) (void)hipEventDestroy(ev_side_t0);
        if(ev_side_t1) (void)hipEventDestroy(ev_side_t1);
    }
};

// The scratch goes before the stream and the events it was used with; the ctx's own DevBufs follow as members.
lrsc_ctx::~lrsc_ctx()
{
    (void)hipSetDevice(device);
    if(stream) (void)hipStreamSynchronize(stream);
    delete cs;
    if(d_ctr) (void)hipFree(d_ctr);
    if(ev0) (void)hipEventDestroy(ev0);
    if(ev1) (void)hipEventDestroy(ev1);
    if(stream) (void)hipStreamDestroy(stream);
}

namespace {

// A WpRequest is two words: the request records of a round travel in the front 2 n words of the uint32_t buffer d_list_tmp.
static_assert(sizeof(WpRequest) == 2 * sizeof(uint32_t), "WpRequest records are staged in a uint32_t buffer");

// ---------------------------------------------------------------------------------------
// One lrsc_batch_correct call over a resident batch whose seeds are found.  A batch is cut into read ranges whose prepared
// tables fit the budget; a range runs in rounds until its stitch pass asks for nothing more.
// ---------------------------------------------------------------------------------------
struct WpFlow {
    lrsc_ctx* const ctx;
    lrsc_batch* const b;
    CorrectScratch& sc;
    const lrsc_params& p;
    const Tunables tn;
    const uint32_t n;                      // reads of the batch
    const uint32_t lbytes;
    // -l above the narrow cap (32; LRSC_WP_WIDE_CAP lowers it, a test hook): the narrow launches run every walk with the cap, and a
    // walk that outgrows it runs again in the wide launch with the true -l (escalate_walks)
    const bool escalate;
    WpArgs a{};
    // per read: bounds, output slots, skipped reads
    std::vector<ReadPlan> plan;
    std::vector<uint32_t> seed_count;
    std::vector<uint64_t> off;
    std::vector<WpReadWork> work;
    std::vector<int> skipped;
    uint64_t out_total = 0, piece_total = 0, n_slots = 0;
    // the read range in progress: reads [r0, r1), slots [slot_base, slot_base + n_range)
    uint32_t r0 = 0, r1 = 0, n_range = 0;
    uint64_t slot_base = 0;
    // host staging, reused by every round
    std::vector<WpDpItem> items;
    std::vector<DpRequest> reqs;
    std::vector<WpRequest> hreq;
    std::vector<uint32_t> hlist;
    uint64_t n_escalated = 0;

    struct Round {
        uint32_t index = 0;
        uint32_t n_ent = 0;                // entries: every slot of the range (round 0) or what the stitch pass asked for
        uint64_t tot[3] = {};              // bytes of the query / prepared-table / path arenas
        uint32_t stats[4] = {};            // WpArgs::plan_stats
        const uint32_t* ext_list = nullptr;    // launch order of the extension
        uint32_t n_mid = 0;                // its first n_mid entries are the walks across long gaps (round 0)
        bool long_launch = false;          // they go to the side stream, beside the first DP call ...
        bool long_pending = false;         // ... and are running there
        uint32_t n_items = 0;              // DP requests of the round
        unsigned long long begin_stats[4] = {};    // WpArgs::begin_stats (LRSC_CORRECT_PROFILE)
    };

    WpFlow(lrsc_ctx* ctx_, lrsc_batch* b_)
        : ctx(ctx_), b(b_), sc(*ctx_->cs), p(ctx_->params), tn(read_tunables(ctx_)), n(b_->n_reads),
          lbytes((uint32_t)leaf_bytes(ctx_->fm.wide != 0)), escalate((uint32_t)ctx_->params.max_leaves > tn.wp_wide_cap)
    {
    }

    uint32_t* small(WpSmall word) const { return sc.d_small.p + word; }

    int bounds_and_slots();
    int bind_args();
    void choose_range(uint32_t first);
    int run_range();
    int gather_results(lrsc_read_result* res, uint64_t* piece_off, uint64_t piece_cap, char* out, uint64_t out_cap,
                       uint64_t* n_pieces_out, uint64_t* out_used);
    int print_extension_profile();

    // the steps of a round, in order
    int round_entries(Round& R, bool* done);
    int plan_and_materialise(Round& R);
    int launch_order(Round& R);
    int extension_launches(Round& R);
    int escalate_walks(const WpArgs& x0, uint32_t n_ent, uint32_t pathw);
    int start_long_walks(Round& R);
    int dp_calls(Round& R);
    int finish_long_walks();
    int stitch();
    int dump_range_walks();
    void print_round(const Round& R) const;

    hipError_t extend_range(WpArgs x, const uint32_t* list, const WpRequest* rq, uint32_t count, uint32_t pathw, hipStream_t st,
                            bool side, uint32_t stride);
    int fetch_items(DevBuf<WpDpItem>& d_list, const uint32_t* d_count, uint32_t cap, Round& R, std::vector<WpDpItem>& out);
    int dp_call(std::vector<WpDpItem>& its);
};

// ---- per-read bounds (longest gap / query any walk of the read can have) -> output slots, skipped reads -----------
int WpFlow::bounds_and_slots()
{
    double freqs[101];
    kmer_freq_table(p, freqs);
    HIP_TRY(sc.d_plan.reserve(n));
    HIP_TRY(sc.d_freqs.reserve(101));
    HIP_TRY(hipMemcpyAsync(sc.d_freqs.p, freqs, sizeof(freqs), hipMemcpyHostToDevice, ctx->stream));

    WpArgs pa{};
    pa.codes = b->d_codes; pa.read_off = b->d_off; pa.seeds = b->d_seeds; pa.seed_count = b->d_seed_count;
    pa.n_reads = n; pa.min_k = b->min_k; pa.next_target = p.next_target;
    hipError_t e = launch_wp_bounds(pa, sc.d_plan.p, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "wp_bounds");
    plan.resize(n); seed_count.resize(n); off.resize(n + 1);
    HIP_TRY(hipMemcpyAsync(plan.data(), sc.d_plan.p, (size_t)n * sizeof(ReadPlan), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(seed_count.data(), b->d_seed_count, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(off.data(), b->d_off, (size_t)(n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));

    work.resize(n);
    skipped.assign(n, 0);
    for(uint32_t r = 0; r < n; ++r) {
        WpReadWork& w = work[r];
        std::memset(&w, 0, sizeof(w));
        const uint64_t rlen = off[r + 1] - off[r];
        const uint32_t ns = seed_count[r];
        w.out_off = out_total; w.piece_off = piece_total; w.slot_first = n_slots;
        if(ns < 2) continue;                                          // nothing to correct: the read is discarded
        // every walk appends at most maxLength + 1 + |target| - initk characters, walks <= seeds, gaps sum to <= |read|
        // (a DP consensus can be longer than its query by the insertion columns it keeps: budget 2x the raw segment)
        const uint64_t cap = rlen + (uint64_t)((p.no_dp ? 1.2 : 2.0) * (double)rlen) + (uint64_t)ns * (2 * kMaxInitK + 16 + (p.no_dp ? 0 : 128)) + 64;
        if(cap >= (1ull << 32)) { skipped[r] = LRSC_READ_TOO_LONG; continue; }
        if(plan[r].lq_max >= 65535) { skipped[r] = LRSC_READ_WALK_QUERY_TOO_LONG; continue; }
        w.out_cap = (uint32_t)cap;
        w.piece_cap = p.split ? ns : 1;
        w.n_seeds = ns;
        out_total += ((uint64_t)w.out_cap + 15) & ~15ull;
        piece_total += w.piece_cap;
        n_slots += ns - 1;
    }
    if(n_slots >= (1ull << 32)) return fail(LRSC_ERR_UNSUPPORTED, "batch: more than 2^32 seed pairs (split the input)");

    HIP_TRY(sc.d_work.reserve(n));
    HIP_TRY(sc.d_reads.reserve(n));
    HIP_TRY(sc.d_slots.reserve(std::max<uint64_t>(n_slots, 1)));
    HIP_TRY(sc.d_small.reserve(kWpSmallWords));
    HIP_TRY(sc.d_req.reserve(n));
    HIP_TRY(sc.d_codes_out.reserve(std::max<uint64_t>(out_total, 64)));
    HIP_TRY(sc.d_pieces.reserve(std::max<uint64_t>(piece_total, 1)));
    HIP_TRY(hipMemcpyAsync(sc.d_work.p, work.data(), (size_t)n * sizeof(WpReadWork), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(sc.d_reads.p, 0, (size_t)n * sizeof(WpRead), ctx->stream));
    return LRSC_OK;
}

// the arguments every launch of the call shares, and the objects they need: walk log, profile counters, side stream
int WpFlow::bind_args()
{
    a.codes = b->d_codes; a.read_off = b->d_off; a.seeds = b->d_seeds; a.seed_count = b->d_seed_count;
    a.n_reads = n; a.min_k = b->min_k;
    a.work = sc.d_work.p; a.reads = sc.d_reads.p; a.slots = sc.d_slots.p; a.n_slots = n_slots;
    a.seed_size = (uint32_t)p.idmer_len; a.min_overlap = (uint32_t)p.min_kmer_len; a.max_leaves = (uint32_t)p.max_leaves;
    if(escalate) { a.max_leaves = tn.wp_wide_cap; a.escalate = 1; }
    a.start_kmer_len = p.start_kmer_len; a.next_target = p.next_target; a.split = p.split; a.no_dp = p.no_dp;
    a.pb_coverage = (uint64_t)p.pb_coverage; a.pacbio_error_rate = p.error_rate;
    a.freqs_of_kmer_size = sc.d_freqs.p;
    a.psz = ctx->fm.wide ? 8 : 4; a.lbytes = lbytes;
    a.plan_stats = small(kWpSmallPlanStats); a.queue = small(kWpSmallQueue); a.n_dp_items = small(kWpSmallDpItems);
    a.n_req_out = small(kWpSmallReqOut);
    a.n_sort9 = small(kWpSmallSort9); a.begin_sort = tn.wp_begin_sort ? 1u : 0u;
    a.req_out = sc.d_req.p; a.req_cap = n;
    a.out_codes = sc.d_codes_out.p; a.piece_start = sc.d_pieces.p;
    a.auto_dp = (!p.no_dp && p.next_target == 1) ? 1u : 0u;
    a.general_quorum_pct = tn.wp_gen_quorum; a.general_max_wait = tn.wp_gen_wait; a.deal_level = tn.wp_deal;
    a.ctr = ctx->d_ctr;
    if(b->debug_flags & LRSC_DEBUG_WALKS) {
        if(!b->d_walk_log) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b->d_walk_log), b->seed_cap));
        HIP_TRY(hipMemsetAsync(b->d_walk_log, 0, b->seed_cap, ctx->stream));
        a.walk_log = b->d_walk_log;
        b->walk_log_done = false;
    }
    if(tn.profile) {
        HIP_TRY(sc.d_prof.reserve(kWpProfWords));                              // [16..32): the long-gap walks' side launch on its own
        HIP_TRY(hipMemsetAsync(sc.d_prof.p, 0, kWpProfWords * sizeof(unsigned long long), ctx->stream));
        a.prof = sc.d_prof.p;
        a.begin_stats = sc.d_prof.p + 32;                                    // [32..36): wp_begin's interval lists, zeroed every round
                                                                             // [36..58): WpArgs::gen_stats of round 0's bulk launch
    }
    // side stream: the few walks across long gaps run beside the DP stage of the bulk's failed walks instead of before it (they are
    // latency-bound on their own: a walk is a chain of dependent steps)
    // It gets the lowest stream priority.  The runtime keeps the hardware queues of each priority apart, so the side streams of two
    // ctxs get a queue each that no other stream of the process shares: with the four queues a process has by default, streams of
    // the default priority are dealt to them round robin, and a side stream then shares its queue with the other ctx's side stream
    // and with MSA streams -- whatever is enqueued there after a long-gap launch waits until that launch has ended, the event
    // that finish_long_walks() records included.  And the launch is the filler beside the DP stage, not the other way round.
    if(!sc.side) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&sc.side, hipStreamNonBlocking, least));
    }
    if(!sc.ev_ready) HIP_TRY(hipEventCreateWithFlags(&sc.ev_ready, hipEventDisableTiming));
    return LRSC_OK;
}

// ---- read ranges whose prepared tables fit the budget (about 40 bytes per query character + 6 KB per walk) -------------------
void WpFlow::choose_range(uint32_t first)
{
    r0 = r1 = first;
    uint64_t est = 0;
    while(r1 < n) {
        const uint64_t ns = work[r1].n_seeds;
        const uint64_t need = ns >= 2 ? 55 * (off[r1 + 1] - off[r1]) + ns * 4400 : 0;     // 39 B per query character + 16 B per target character + 3.3 KB per walk
        if(r1 > r0 && est + need > tn.wp_prep_bytes) break;
        est += need;
        ++r1;
    }
    slot_base = work[r0].slot_first;
    const uint64_t slot_end = r1 < n ? work[r1].slot_first : n_slots;
    n_range = (uint32_t)(slot_end - slot_base);
    a.r0 = r0; a.r1 = r1; a.slot_base = slot_base;
}

int WpFlow::run_range()
{
    sc.persist.reset();
    if(n_range == 0) return LRSC_OK;
    for(uint32_t round = 0;; ++round) {
        Round R;
        R.index = round;
        bool done = false;
        int st = round_entries(R, &done);
        if(st != LRSC_OK) return st;
        if(done) break;
        st = plan_and_materialise(R);
        if(st == LRSC_OK) st = launch_order(R);
        if(st == LRSC_OK) st = extension_launches(R);
        if(st == LRSC_OK && escalate) st = escalate_walks(a, R.n_ent, std::max(R.stats[2], 1u));
        if(st == LRSC_OK && R.long_launch) st = start_long_walks(R);
        if(st == LRSC_OK) st = dp_calls(R);
        if(st == LRSC_OK) st = stitch();
        if(st == LRSC_OK && tn.profile && round == 0 && tn.wp_dump) st = dump_range_walks();
        if(st != LRSC_OK) return st;
        if(tn.profile) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipMemcpy(R.begin_stats, a.begin_stats, sizeof(R.begin_stats), hipMemcpyDeviceToHost));
            print_round(R);
        }
        if(round > 100000) return fail(LRSC_ERR_LIMIT, "walk-parallel flow: too many rounds");
    }
    return LRSC_OK;
}

// entries of this round: every slot of the range (round 0) or what the stitch pass asked for; then the per-entry buffers
int WpFlow::round_entries(Round& R, bool* done)
{
    uint32_t n_ent = n_range;
    a.list = nullptr; a.reqs = nullptr;
    if(R.index != 0) {
        uint32_t n_req = 0;
        COPY_TRY(ctx, &n_req, a.n_req_out, sizeof(uint32_t), hipMemcpyDeviceToHost);
        if(n_req == 0) { *done = true; return LRSC_OK; }
        if(n_req > n) return fail(LRSC_ERR_LIMIT, "walk-parallel flow: request list overflow");
        hreq.resize(n_req);
        COPY_TRY(ctx, hreq.data(), sc.d_req.p, (size_t)n_req * sizeof(WpRequest), hipMemcpyDeviceToHost);
        std::sort(hreq.begin(), hreq.end(), [](const WpRequest& x, const WpRequest& y) { return x.slot < y.slot; });
        hlist.resize(n_req);
        for(uint32_t i = 0; i < n_req; ++i) hlist[i] = hreq[i].slot;
        n_ent = n_req;
    }
    R.n_ent = n_ent;
    HIP_TRY(sc.d_sz.reserve(3 * ((size_t)n_ent + 1)));
    HIP_TRY(sc.d_key.reserve(n_ent));
    HIP_TRY(sc.d_key_tmp.reserve(n_ent));
    HIP_TRY(sc.d_list.reserve(n_ent));
    HIP_TRY(sc.d_list_tmp.reserve(n_ent));
    HIP_TRY(sc.d_items.reserve(n_ent));
    HIP_TRY(sc.d_sort9.reserve(2 * (size_t)n_ent));
    a.sort9 = sc.d_sort9.p;
    if(a.begin_stats) HIP_TRY(hipMemsetAsync(a.begin_stats, 0, 4 * sizeof(unsigned long long), ctx->stream));
    a.sz_q = sc.d_sz.p; a.sz_prep = sc.d_sz.p + (n_ent + 1); a.sz_path = sc.d_sz.p + 2 * ((size_t)n_ent + 1);
    a.sort_key = sc.d_key.p;
    a.n_list = n_ent;
    a.dp_items = sc.d_items.p; a.dp_items_cap = n_ent;
    HIP_TRY(hipMemsetAsync(sc.d_sz.p, 0, 3 * ((size_t)n_ent + 1) * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(sc.d_small.p, 0, kWpSmallWords * sizeof(uint32_t), ctx->stream));
    if(R.index != 0) {
        // the request records move to the front half of a second buffer so that the stitch pass can write new ones
        HIP_TRY(sc.d_list_tmp.reserve(2 * (size_t)n_ent));
        WpRequest* d_reqs_in = reinterpret_cast<WpRequest*>(sc.d_list_tmp.p);
        HIP_TRY(hipMemcpyAsync(d_reqs_in, hreq.data(), (size_t)n_ent * sizeof(WpRequest), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(sc.d_list.p, hlist.data(), (size_t)n_ent * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        a.list = sc.d_list.p; a.reqs = d_reqs_in;
    }
    return LRSC_OK;
}

// plan (bytes per entry) -> scan (offsets, totals) -> arenas -> materialise (queries, slots)
int WpFlow::plan_and_materialise(Round& R)
{
    const uint32_t n_ent = R.n_ent;
    hipError_t e = launch_wp_plan(a, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "wp_plan");
    for(int j = 0; j < 3; ++j) {
        e = wp_scan(sc.d_sz.p + (size_t)j * (n_ent + 1), (uint64_t)n_ent + 1, &sc.cub_tmp, &sc.cub_cap, ctx->stream);
        if(e != hipSuccess) return hip_fail(e, "wp_scan");
    }
    for(int j = 0; j < 3; ++j)
        HIP_TRY(hipMemcpyAsync(&R.tot[j], sc.d_sz.p + (size_t)j * (n_ent + 1) + n_ent, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(R.stats, small(kWpSmallPlanStats), sizeof(R.stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(sc.persist.alloc(R.tot[0] + 64, &a.arena_q));
    HIP_TRY(sc.persist.alloc(R.tot[2] + 64, &a.arena_path));
    HIP_TRY(sc.d_prep.reserve(R.tot[1] + 64));
    a.arena_prep = sc.d_prep.p;
    e = launch_wp_materialize(a, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "wp_materialize");
    return LRSC_OK;
}

// launch order of round 0: long walks first (the few walks across long gaps need bigger path slots: own launches)
int WpFlow::launch_order(Round& R)
{
    R.ext_list = a.list;
    if(R.index != 0) return LRSC_OK;
    // list_tmp = slot_base + i
    hlist.resize(R.n_ent);
    for(uint32_t i = 0; i < R.n_ent; ++i) hlist[i] = (uint32_t)slot_base + i;
    HIP_TRY(hipMemcpyAsync(sc.d_list_tmp.p, hlist.data(), (size_t)R.n_ent * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = wp_sort_list(sc.d_key.p, sc.d_key_tmp.p, sc.d_list.p, sc.d_list_tmp.p, R.n_ent, &sc.cub_tmp, &sc.cub_cap, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "wp_sort_list");
    R.ext_list = sc.d_list.p;
    R.n_mid = R.stats[0];
    return LRSC_OK;
}

// One launch of the extension over `count` list entries, stride 64 = one walk per wavefront.  The side launch (side: the long-gap
// walks beside the DP stage) and the launches on ctx->stream are persistent and share the device, so the side launch gets half of
// the resident wavefronts and a quarter of the lane budget -- a launch that fills every slot first would keep the others out
// until it ends.
// LRSC_WP_WAVE, one-walk-per-wavefront launches: 1 = the frontier across the wavefront (wp_extend_wave_kernel), 0 = lane 0 walks alone
// (wp_extend_kernel); 2 = test hook: every extension launch goes through wp_extend_wave_kernel at stride 64
// LRSC_WP_DEAL, lane-per-walk launches: 0 = the serial step (wp_extend_kernel); 1..3 = wp_extend_deal_kernel with extendLeaves'
// per-leaf work dealt across the wavefront, from 2 PrunedBySeedSupport too, from 3 isTerminated's scans too (wp_deal_level.h)
hipError_t WpFlow::extend_range(WpArgs x, const uint32_t* list, const WpRequest* rq, uint32_t count, uint32_t pathw, hipStream_t st,
                                bool side, uint32_t stride)
{
    if(count == 0) return hipSuccess;
    if(tn.wp_wave == 2) stride = 64;
    const WpLaneLayout LL = wp_lane_layout(lbytes, pathw);
    const uint64_t slots = tn.wp_lanes / 64;                                      // resident wavefronts of these kernels
    const uint64_t share = side ? wp_side_waves(tn) : slots;
    uint64_t lanes = std::min<uint64_t>(stride == 1 ? (((uint64_t)count + 63) & ~63ull) : count, share * 64 / stride);
    lanes = std::max<uint64_t>(1, std::min<uint64_t>(lanes, (tn.wp_lane_bytes / (side ? 4 : 1)) / LL.total));
    if(stride == 1) lanes = std::max<uint64_t>(64, lanes & ~63ull);
    DevBuf<uint8_t>& buf = side ? sc.d_lane_side : sc.d_lane;
    hipError_t e = buf.reserve(lanes * LL.total);
    if(e != hipSuccess) return e;
    x.list = list; x.reqs = rq; x.n_list = count;
    x.lane_ws = buf.p; x.lane_ws_bytes = LL.total; x.lane_pathw = pathw; x.n_lanes = (uint32_t)lanes; x.lane_stride = stride;
    x.queue = small(side ? kWpSmallSideQueue : kWpSmallExtQueue);
    e = hipMemsetAsync(x.queue, 0, sizeof(uint32_t), st);
    if(e != hipSuccess) return e;
    if(stride == 64 && tn.wp_wave != 0) return launch_wp_extend_wave(ctx->fm, x, st);
    if(stride == 1 && tn.wp_deal != 0) return launch_wp_extend_deal(ctx->fm, x, st);
    return launch_wp_extend(ctx->fm, x, st);
}

// prepare + begin + the extension launches of the round on ctx->stream, timed as one LRSC_K_EXTEND span
int WpFlow::extension_launches(Round& R)
{
    return timed_launch(ctx, LRSC_K_EXTEND, [&]() -> hipError_t {
        hipError_t e = launch_wp_prepare(ctx->fm, a, ctx->stream);
        if(e == hipSuccess) e = launch_wp_begin(ctx->fm, a, ctx->stream);
        if(e != hipSuccess) return e;
        // later rounds: the re-queued walks, spread thinner the fewer they are (64 / 16 / 1 lanes per walk)
        if(R.index != 0)
            return extend_range(a, a.list, a.reqs, R.n_ent, std::max(R.stats[2], 1u), ctx->stream, false,
                                R.n_ent <= 16384 ? 64u : R.n_ent <= 65536 ? 16u : 1u);
        // round 0: the bulk, one walk per lane
        WpArgs xb = a;
        if(a.prof) xb.gen_stats = a.prof + 36;
        e = extend_range(xb, R.ext_list + R.n_mid, nullptr, R.n_ent - R.n_mid, std::min(R.stats[2], kWpPathwSmall), ctx->stream, false, 1);
        if(e != hipSuccess || R.n_mid == 0) return e;
        // then the walks across long gaps (the first n_mid of the launch order), one walk per wavefront: a lane-per-walk wavefront
        // advances at the pace of its slowest lane, and these are thousands of wide steps long.  With --nodp, or escalating (the
        // wide launch takes their overflows before the DP call), they follow the bulk here; with the DP fallback on they start on
        // the side stream (start_long_walks), beside the DP stage of the bulk's failed walks
        if(p.no_dp || escalate) return extend_range(a, R.ext_list, nullptr, R.n_mid, R.stats[2], ctx->stream, false, 64);
        R.long_launch = true;
        return e;
    });
}

// The escalated walks of a round (entries of a.list / the range whose narrow walk ended with LRSC_WALK_NEEDS_WIDE) run again
// from their start with the true -l, one walk per wavefront (wp_wide.hip); their failures join the round's DP items.  A
// wavefront's workspace is wp_wide_layout(pathw, -l): the launch takes as many of them as the lane budget / 4 holds.
int WpFlow::escalate_walks(const WpArgs& x0, uint32_t n_ent, uint32_t pathw)
{
    HIP_TRY(sc.d_wide_list.reserve(n_ent));
    uint32_t* d_count = small(kWpSmallWideCount);
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), ctx->stream));
    hipError_t e = launch_wp_wide_collect(x0, sc.d_wide_list.p, d_count, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "wp_wide_collect");
    uint32_t n_wide = 0;
    HIP_TRY(hipMemcpyAsync(&n_wide, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if(n_wide > n_ent) return fail(LRSC_ERR_LIMIT, "walk-parallel flow: escalation list overflow");
    n_escalated += n_wide;
    if(n_wide == 0) return LRSC_OK;
    WpArgs x = x0;
    x.max_leaves = (uint32_t)p.max_leaves; x.escalate = 0;
    x.list = sc.d_wide_list.p; x.reqs = nullptr; x.n_list = n_wide;
    const WpWideLayout WL = wp_wide_layout(lbytes, pathw, x.max_leaves);
    uint64_t waves = std::min<uint64_t>(n_wide, tn.wp_lanes / 64);
    waves = std::max<uint64_t>(1, std::min<uint64_t>(waves, (tn.wp_lane_bytes / 4) / WL.total));
    HIP_TRY(sc.d_lane_wide.reserve(waves * WL.total));
    x.lane_ws = sc.d_lane_wide.p; x.lane_ws_bytes = WL.total; x.lane_pathw = pathw; x.n_lanes = (uint32_t)waves; x.lane_stride = 64;
    x.queue = small(kWpSmallWideQueue);
    HIP_TRY(hipMemsetAsync(x.queue, 0, sizeof(uint32_t), ctx->stream));
    return timed_launch(ctx, LRSC_K_EXTEND_WIDE, [&]() { return launch_wp_extend_wide(ctx->fm, x, ctx->stream); });
}

// the long-gap walks of round 0 on the side stream, with a DP item list and statistics counters of their own
int WpFlow::start_long_walks(Round& R)
{
    HIP_TRY(sc.d_items2.reserve(R.n_mid));
    WpArgs xl = a;
    xl.dp_items = sc.d_items2.p; xl.n_dp_items = small(kWpSmallSideDpItems); xl.dp_items_cap = R.n_mid;
    // its own statistics counters: the DP stage's timed launches zero and read the ctx's while it runs
    HIP_TRY(sc.d_ctr2.reserve(kCtrShards));
    HIP_TRY(hipMemsetAsync(sc.d_ctr2.p, 0, kCtrShards * sizeof(DevCounters), ctx->stream));
    xl.ctr = sc.d_ctr2.p;
    if(a.prof) xl.prof = a.prof + 16;
    // the side stream starts after what is on ctx->stream now
    HIP_TRY(hipEventRecord(sc.ev_ready, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(sc.side, sc.ev_ready, 0));
    if(!sc.ev_side_t0) HIP_TRY(hipEventCreate(&sc.ev_side_t0));
    HIP_TRY(hipEventRecord(sc.ev_side_t0, sc.side));
    hipError_t e = extend_range(xl, R.ext_list, nullptr, R.n_mid, R.stats[2], sc.side, true, 64);
    if(e != hipSuccess) return hip_fail(e, "wp_extend (long walks)");
    R.long_pending = true;
    return LRSC_OK;
}

int WpFlow::fetch_items(DevBuf<WpDpItem>& d_list, const uint32_t* d_count, uint32_t cap, Round& R, std::vector<WpDpItem>& out)
{
    uint32_t cnt = 0;
    COPY_TRY(ctx, &cnt, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if(cnt > cap) return fail(LRSC_ERR_LIMIT, "walk-parallel flow: DP item list overflow");
    R.n_items += cnt;
    out.resize(cnt);
    if(cnt) COPY_TRY(ctx, out.data(), d_list.p, (size_t)cnt * sizeof(WpDpItem), hipMemcpyDeviceToHost);
    std::sort(out.begin(), out.end(), [](const WpDpItem& x, const WpDpItem& y) { return x.slot < y.slot; });
    return LRSC_OK;
}

// one DP call over `its` (sorted by slot): requests, DpStage, a persistent copy of the consensus buffer, answers into the slots
int WpFlow::dp_call(std::vector<WpDpItem>& its)
{
    const uint32_t cnt = (uint32_t)its.size();
    if(cnt == 0) return LRSC_OK;
    reqs.clear();
    reqs.reserve(cnt);
    for(const WpDpItem& it : its) {
        DpRequest q;
        std::memset(&q, 0, sizeof(q));
        q.q_off = it.q;                                                          // absolute device address (base pointer 0)
        q.lq = it.lq; q.k = it.k;
        q.coverage = (uint32_t)p.pb_coverage;
        q.min_overlap = it.lq / 10;                                              // path.length() / 10
        // identity / min_call_coverage from the two seeds' maxFixedMerFreq (:225-229)
        const size_t total = (size_t)it.total_freq;
        double identity = 0.65;
        size_t min_call_coverage = 15;
        identity += (total > 50 ? 0.05 : 0);
        identity += (total > 100 ? 0.05 : 0);
        min_call_coverage = total > 50 ? total * 0.4 : min_call_coverage;
        q.min_identity = identity; q.min_call_coverage = (int32_t)min_call_coverage;
        reqs.push_back(q);
    }
    const int sd = sc.stage.run(ctx, tn, nullptr, reqs);
    if(sd != LRSC_OK) return sd;
    uint8_t* cons_keep = nullptr;
    HIP_TRY(sc.persist.alloc(sc.stage.cons_total + 64, &cons_keep));
    HIP_TRY(hipMemcpyAsync(cons_keep, sc.stage.d_cons.p, sc.stage.cons_total, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(sc.d_items3.reserve(cnt));
    HIP_TRY(hipMemcpyAsync(sc.d_items3.p, its.data(), (size_t)cnt * sizeof(WpDpItem), hipMemcpyHostToDevice, ctx->stream));
    WpArgs c2 = a;
    c2.dp_reqs = sc.stage.d_reqs.p; c2.dp_msa = sc.stage.d_msa.p; c2.dp_cons = cons_keep; c2.n_dp = cnt;
    hipError_t ec = launch_wp_dp_collect(c2, sc.d_items3.p, ctx->stream);
    if(ec != hipSuccess) return hip_fail(ec, "wp_dp_collect");
    HIP_TRY(hipStreamSynchronize(ctx->stream));                                  // the stage's buffers are reused by the next call
    return LRSC_OK;
}

// the side launch's end: its time and counters go to LRSC_K_EXTEND
int WpFlow::finish_long_walks()
{
    if(!sc.ev_side_t1) HIP_TRY(hipEventCreate(&sc.ev_side_t1));
    HIP_TRY(hipEventRecord(sc.ev_side_t1, sc.side));
    HIP_TRY(hipEventSynchronize(sc.ev_side_t1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, sc.ev_side_t0, sc.ev_side_t1));
    lrsc_kernel_stats& s = ctx->stats[LRSC_K_EXTEND];
    s.total_ms += ms;             // overlaps the DP stage: the stage times then add up to more than the wall time
    std::vector<DevCounters> shards(kCtrShards);
    COPY_TRY(ctx, shards.data(), sc.d_ctr2.p, kCtrShards * sizeof(DevCounters), hipMemcpyDeviceToHost);
    for(const DevCounters& dcn : shards) {
        s.rank_queries += dcn.rank_queries;
        s.block_loads += dcn.block_loads;
        s.table_loads += dcn.table_loads;
    }
    return LRSC_OK;
}

// ---- the DP stage for every failed walk of this round (and the explicit requests) ---------------------------------
int WpFlow::dp_calls(Round& R)
{
    int sd = fetch_items(sc.d_items, a.n_dp_items, R.n_ent, R, items);
    if(sd != LRSC_OK) return sd;
    sd = dp_call(items);
    if(sd != LRSC_OK || !R.long_pending) return sd;
    // The long-gap walks ran on the side stream beside that DP call; their failures go to the DP stage in a call of
    // their own.
    sd = finish_long_walks();
    if(sd != LRSC_OK) return sd;
    std::vector<WpDpItem> longs;
    sd = fetch_items(sc.d_items2, small(kWpSmallSideDpItems), R.n_mid, R, longs);
    if(sd != LRSC_OK) return sd;
    return dp_call(longs);
}

int WpFlow::stitch()
{
    HIP_TRY(hipMemsetAsync(a.n_req_out, 0, sizeof(uint32_t), ctx->stream));
    hipError_t e = launch_wp_stitch(a, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "wp_stitch");
    return LRSC_OK;
}

// ---- LRSC_CORRECT_PROFILE output ------------------------------------------------------------------------------------------------
// LRSC_WP_DUMP: the hardest walks of the range (a walk is a chain of dependent steps: they bound the launch from below)
int WpFlow::dump_range_walks()
{
    std::vector<WpSlot> hs(n_range);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(hs.data(), sc.d_slots.p + slot_base, (size_t)n_range * sizeof(WpSlot), hipMemcpyDeviceToHost));
    std::vector<uint32_t> ord(n_range);
    for(uint32_t i = 0; i < n_range; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return hs[x].leaf_steps > hs[y].leaf_steps; });
    unsigned long long tot = 0, tot_steps = 0;
    for(const WpSlot& q : hs) { tot += q.leaf_steps; tot_steps += q.steps; }
    std::fprintf(stderr, "[lrsc] wp walks of the range: %u, %llu steps, %llu leaf-steps; hardest (gap, k, steps, leaf-steps, code):", n_range, tot_steps, tot);
    for(uint32_t i = 0; i < std::min<uint32_t>(n_range, 12); ++i)
        std::fprintf(stderr, " (%u,%u,%u,%u,%d)", hs[ord[i]].gap, (unsigned)hs[ord[i]].k, hs[ord[i]].steps, hs[ord[i]].leaf_steps, hs[ord[i]].code);
    unsigned long long hist[34] = {0}, wsteps[34] = {0};
    for(const WpSlot& q : hs) { const unsigned m = std::min<unsigned>(q.max_front, 33); hist[m]++; wsteps[m] += q.leaf_steps; }
    std::fprintf(stderr, "; walks (and their leaf-steps in %%) by widest frontier:");
    for(unsigned m = 1; m < 34; ++m)
        if(hist[m]) std::fprintf(stderr, " %u:%.2f%%(%.1f%%)", m, 100.0 * hist[m] / n_range, 100.0 * wsteps[m] / std::max(tot, 1ull));
    const uint32_t qs[] = {n_range / 2, n_range / 10, n_range / 100, n_range / 1000, n_range / 10000};
    std::fprintf(stderr, "; leaf-steps at the median / top 10%% / 1%% / 0.1%% / 0.01%%: %u %u %u %u %u\n", hs[ord[qs[0]]].leaf_steps, hs[ord[qs[1]]].leaf_steps,
                 hs[ord[qs[2]]].leaf_steps, hs[ord[qs[3]]].leaf_steps, hs[ord[qs[4]]].leaf_steps);
    return LRSC_OK;
}

void WpFlow::print_round(const Round& R) const
{
    std::fprintf(stderr, "[lrsc] wp reads [%u, %u) round %u: %u entries, %u DP requests (%llu strings), arenas q %.1f MB prep %.1f MB path %.1f MB, %llu walks escalated so far\n",
                 r0, r1, R.index, R.n_ent, R.n_items, (unsigned long long)sc.stage.n_strings, R.tot[0] / 1048576.0, R.tot[1] / 1048576.0, R.tot[2] / 1048576.0,
                 (unsigned long long)n_escalated);
    const unsigned long long* g = R.begin_stats;
    if(tn.wp_begin_sort)                                                     // every list sorted: repeats are not looked for
        std::fprintf(stderr, "[lrsc] wp reads [%u, %u) round %u: wp_begin %llu interval lists, %llu entries, every list sorted (LRSC_WP_BEGIN_SORT)\n",
                     r0, r1, R.index, g[0], g[2] + g[3]);
    else
        std::fprintf(stderr, "[lrsc] wp reads [%u, %u) round %u: wp_begin %llu interval lists, %llu with a repeated code (%.1f%%); entries %llu in the lists without one, %llu in those with one\n",
                     r0, r1, R.index, g[0], g[1], 100.0 * g[1] / std::max(g[0], 1ull), g[2], g[3]);
}

// per-region lane ticks of the extension kernels over the whole call
int WpFlow::print_extension_profile()
{
    unsigned long long prs[kWpProfWords];
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipStreamSynchronize(sc.side));
    HIP_TRY(hipMemcpy(prs, sc.d_prof.p, sizeof(prs), hipMemcpyDeviceToHost));
    for(int part = 0; part < 2; ++part) {
        const unsigned long long* pr = prs + 16 * part;
        if(pr[10] == 0) continue;
        const double all = (double)pr[10], st = (double)std::max<unsigned long long>(pr[11], 1);
        std::fprintf(stderr, "[lrsc] wp extension kernel (%s), lane wall ticks: %.3g total, %.0f per step over %.3g steps; extendLeaves %.1f%% (refine %.1f%%, attempToExtend %.1f%% of which "
                             "getFMIndexExtensions %.1f%%; SelectFreqsOfrange %.1f%%), PrunedBySeedSupport %.1f%%, materialise+commit %.1f%%, isTerminated %.1f%%, refill %.1f%%, finish %.1f%%; single-leaf fast steps %.1f%% of the steps in %.1f%% of the ticks\n",
                     part ? "long-gap walks, one per wavefront" : "bulk and later rounds",
                     all, all / st, st, 100 * pr[0] / all, 100 * pr[1] / all, 100 * pr[2] / all, 100 * pr[3] / all, 100 * pr[13] / all, 100 * pr[4] / all, 100 * pr[5] / all, 100 * pr[6] / all,
                     100 * pr[8] / all, 100 * pr[9] / all, 100 * pr[12] / st, 100 * pr[7] / all);
    }
    // what a general step of a lane-per-walk wavefront costs against the work in it: the serial step lasts as long as the widest
    // frontier among the lanes taking part, so it pays (maximum x lanes) leaf passes for (sum) leaves
    const unsigned long long* g = prs + 36;
    if(g[0]) {
        const double s = (double)g[0];
        std::fprintf(stderr, "[lrsc] wp bulk launches, general steps of a wavefront: %llu, %.1f lanes taking part; leaves per step %.1f in all, %.2f per lane, %.2f in the widest "
                             "(widest x lanes / all = %.2f; %.2f passes of 64 lanes); children after extendLeaves %.1f in all, %.2f per lane, %.2f in the widest "
                             "(%.2f; %.2f passes); counters %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n",
                     g[0], g[1] / s, g[2] / s, (double)g[2] / std::max(g[1], 1ull), g[3] / s, (double)g[6] / std::max(g[2], 1ull), g[8] / s,
                     g[4] / s, (double)g[4] / std::max(g[1], 1ull), g[5] / s, (double)g[7] / std::max(g[4], 1ull), g[9] / s,
                     g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9]);
        // the same question for the two phases that follow extendLeaves (wp_extend_deal_kernel counts them): per phase, items and
        // the loads behind them
        const unsigned long long* h = g + 10;
        if(h[0] | h[6])
            std::fprintf(stderr, "[lrsc] wp bulk launches, phases of a general step: PrunedBySeedSupport, children that need the seed search %.1f in all, %.2f in the widest "
                                 "(widest x lanes / all = %.2f), chain entries %.1f in all, %.1f in the widest (%.2f); isTerminated, leaves past the filter %.2f in all, "
                                 "%.2f in the widest (%.2f), term rows %.1f in all, %.1f in the widest (%.2f); counters %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n",
                         h[0] / s, h[1] / s, (double)h[2] / std::max(h[0], 1ull), h[3] / s, h[4] / s, (double)h[5] / std::max(h[3], 1ull),
                         h[6] / s, h[7] / s, (double)h[8] / std::max(h[6], 1ull), h[9] / s, h[10] / s, (double)h[11] / std::max(h[9], 1ull),
                         h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11]);
    }
    return LRSC_OK;
}

// ---- results ---------------------------------------------------------------------------------------------------------------------
int WpFlow::gather_results(lrsc_read_result* res, uint64_t* piece_off, uint64_t piece_cap, char* out, uint64_t out_cap,
                           uint64_t* n_pieces_out, uint64_t* out_used)
{
    std::vector<WpRead> ro(n);
    COPY_TRY(ctx, ro.data(), sc.d_reads.p, (size_t)n * sizeof(WpRead), hipMemcpyDeviceToHost);
    std::vector<uint32_t> pieces(std::max<uint64_t>(piece_total, 1));
    if(piece_total) COPY_TRY(ctx, pieces.data(), sc.d_pieces.p, (size_t)piece_total * sizeof(uint32_t), hipMemcpyDeviceToHost);
    std::vector<uint64_t> dst_off(n + 1, 0);
    uint64_t n_pieces = 0;
    for(uint32_t r = 0; r < n; ++r) {
        const WpRead& o = ro[r];
        int status = skipped[r];
        if(o.error == LRSC_WALK_ERR_GEOMETRY) status = LRSC_READ_GEOMETRY;
        else if(o.error == LRSC_WALK_ERR_CODE) status = LRSC_READ_INTERNAL;
        else if(o.error == LRSC_WALK_ERR_DP) status = LRSC_READ_DP_LIMIT;
        else if(o.error == LRSC_WALK_ERR_OUTPUT) status = LRSC_READ_OUTPUT_LIMIT;
        else if(o.error != 0) status = LRSC_READ_FRONTIER_LIMIT;
        lrsc_read_result& R = res[r];
        if(status != LRSC_READ_OK) {
            // this read alone could not be corrected: it comes back as "not merged" (-> discard.fa) with its status
            std::memset(&R, 0, sizeof(R));
            R.piece_first = n_pieces;
            R.status = status;
            dst_off[r + 1] = dst_off[r];
            continue;
        }
        R.merge = (int32_t)o.merge; R.n_pieces = o.n_pieces; R.piece_first = n_pieces;
        R.total_reads_len = (int64_t)(off[r + 1] - off[r]); R.corrected_len = o.c[1]; R.total_seed_num = seed_count[r]; R.total_walk_num = o.c[3];
        R.high_error_num = o.c[4]; R.exceed_depth_num = o.c[5]; R.exceed_leave_num = o.c[6]; R.fm_num = o.c[7];
        R.dp_num = o.c[8]; R.seed_dis = o.c[9];
        R.status = LRSC_READ_OK; R.pad = 0;
        dst_off[r + 1] = dst_off[r] + o.out_len;
        for(uint32_t j = 0; j < o.n_pieces; ++j) {
            if(piece_off && n_pieces < piece_cap) piece_off[n_pieces] = dst_off[r] + pieces[work[r].piece_off + j];
            ++n_pieces;
        }
    }
    const uint64_t used = dst_off[n];
    if(piece_off && n_pieces < piece_cap) piece_off[n_pieces] = used;
    *n_pieces_out = n_pieces;
    *out_used = used;
    if(!out || !piece_off || used > out_cap || n_pieces + 1 > piece_cap) return fail(LRSC_ERR_CAPACITY, "output buffers too small");
    if(used) {
        HIP_TRY(sc.d_dst_off.reserve(n + 1));
        HIP_TRY(sc.d_dst.reserve(used));
        HIP_TRY(hipMemcpyAsync(sc.d_dst_off.p, dst_off.data(), (size_t)(n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        hipError_t e = launch_wp_gather(a, sc.d_dst_off.p, sc.d_dst.p, ctx->stream);
        if(e != hipSuccess) return hip_fail(e, "wp_gather");
        HIP_TRY(hipMemcpyAsync(out, sc.d_dst.p, used, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return LRSC_OK;
}

int batch_correct_wp(lrsc_ctx* ctx, lrsc_batch* b, lrsc_read_result* res, uint64_t* piece_off, uint64_t piece_cap, char* out,
                     uint64_t out_cap, uint64_t* n_pieces_out, uint64_t* out_used)
{
    if(!ctx->cs) ctx->cs = new(std::nothrow) CorrectScratch();
    if(!ctx->cs) return fail(LRSC_ERR_NOMEM, "correct scratch");
    WpFlow f(ctx, b);
    int st = f.bounds_and_slots();
    if(st == LRSC_OK) st = f.bind_args();
    for(uint32_t first = 0; st == LRSC_OK && first < f.n; first = f.r1) {
        f.choose_range(first);
        st = f.run_range();
    }
    if(st == LRSC_OK && f.a.prof) st = f.print_extension_profile();
    if(st != LRSC_OK) return st;
    if(f.a.walk_log) b->walk_log_done = true;
    return f.gather_results(res, piece_off, piece_cap, out, out_cap, n_pieces_out, out_used);
}

} // namespace

// ---------------------------------------------------------------------------------------
// the whole per-read path on the device
// ---------------------------------------------------------------------------------------
// PacBioSelfCorrectionProcess::process for a resident batch: seeds (if not found yet), then the walk-parallel flow
// (WpFlow above: wp.hip) and a gather of the corrected strings.  The host only sizes buffers and copies results.
extern "C" int lrsc_batch_correct(lrsc_ctx* ctx, lrsc_batch* b, lrsc_read_result* res, uint64_t* piece_off, uint64_t piece_cap,
                                  char* out, uint64_t out_cap, uint64_t* n_pieces_out, uint64_t* out_used)
{
    if(!ctx || !b || b->ctx != ctx || !res || !n_pieces_out || !out_used) return fail(LRSC_ERR_ARG, "null / foreign batch");
    *n_pieces_out = 0; *out_used = 0;
    const lrsc_params& p = ctx->params;
    int st = check_walk_params(p);
    if(st != LRSC_OK) return st;
    if(p.next_target < 1) return fail(LRSC_ERR_ARG, "next_target must be >= 1");
    const uint32_t n = b->n_reads;
    if(n == 0) return LRSC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if(!b->seeds_done) {
        st = lrsc_batch_find_seeds(ctx, b);
        if(st != LRSC_OK) return st;
    }
    return batch_correct_wp(ctx, b, res, piece_off, piece_cap, out, out_cap, n_pieces_out, out_used);
}
