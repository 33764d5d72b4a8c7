// capi_fmmerge.cpp -- what `stride fm-merge` needs of the library: every run of unambiguously overlapping reads of a context's
// index merged into one sequence (fm_fmmerge.hip), after the exact overlap of the same reads (capi_overlap.cpp).
#include "capi_internal.h"
#include "fm_fmmerge.h"

using namespace lrsc;

static_assert(kFmmMaxReads == LRSC_FMMERGE_MAX_READS, "the limit that lrsc.h states");
static_assert(sizeof(FmmOutRead) == sizeof(lrsc_fmmerge_read) && sizeof(FmmOutSeq) == sizeof(lrsc_fmmerge_seq), "the records are lrsc.h's");

namespace {

template <class F>
int find_launch(lrsc_ctx* ctx, F&& f) { return timed_launch(ctx, LRSC_K_FIND, f); }

// the lexicographic orders of both strands on the ctx's device, prepared at rate 0 when there are none
int lexico_orders(lrsc_ctx* ctx, const uint32_t* order[2])
{
    lrsc_index* idx = const_cast<lrsc_index*>(ctx->index);
    for(int attempt = 0; attempt < 2; ++attempt) {
        {
            std::lock_guard<std::mutex> lock(idx->mu);
            auto it = idx->copies.find(ctx->device);
            if(it == idx->copies.end()) return fail(LRSC_ERR_DEVICE, "index not uploaded to this device (call lrsc_index_upload)");
            if(it->second.located) {
                order[0] = it->second.locate[0].order;
                order[1] = it->second.locate[1].order;
                return LRSC_OK;
            }
        }
        const int st = lrsc_index_locate_prepare(idx, ctx->device, 0);
        if(st != LRSC_OK) return st;
    }
    return fail(LRSC_ERR_DEVICE, "fm-merge: no lexicographic order on this device");
}

} // namespace

// FMMergeProcess::process over every read (Algorithm/FMMergeProcess.cpp:30-230), FMMergePostProcess::process' names and order
// (313-329), Bigraph::simplify and merge of each chain (Bigraph/Bigraph.cpp:162-220, 452-524)
extern "C" int lrsc_fmmerge(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap, lrsc_fmmerge_read* per_read,
                            lrsc_fmmerge_seq* seqs, uint32_t* n_seqs_out, char* bases, uint64_t bases_cap, uint64_t* n_bases_out)
{
    if(!ctx || !n_seqs_out || !n_bases_out || (n_reads && (!reads || !read_off || !per_read || !seqs)) || (bases_cap && !bases)) return fail(LRSC_ERR_ARG, "null");
    int st = overlap_check_min(min_overlap);
    if(st != LRSC_OK) return st;
    if(n_reads != ctx->index->num_strings)
        return fail(LRSC_ERR_ARG, "fm-merge: " + std::to_string(n_reads) + " reads, the index holds " + std::to_string(ctx->index->num_strings));
    if(n_reads == 0) {
        *n_seqs_out = 0;
        *n_bases_out = 0;
        return LRSC_OK;
    }
    if(n_reads > kFmmMaxReads) return fail(LRSC_ERR_UNSUPPORTED, "fm-merge: 2^31 reads or more");
    HIP_TRY(hipSetDevice(ctx->device));
    OverlapPlan plan;
    st = overlap_plan(ctx, reads, read_off, n_reads, min_overlap, plan);
    if(st != LRSC_OK) return st;
    const uint32_t* order[2] = {nullptr, nullptr};
    st = lexico_orders(ctx, order);
    if(st != LRSC_OK) return st;

    // ---- the state, O(reads)
    const uint64_t n = n_reads, tiles = fmmerge_scan_tiles(n_reads);
    HIP_TRY(ctx->fm_links.reserve(2 * n * sizeof(FmmLink)));
    HIP_TRY(ctx->fm_nodes.reserve(2 * 2 * n * sizeof(FmmNode)));
    HIP_TRY(ctx->fm_words.reserve((2 * n + 7 * n + tiles + kFmmBadCount + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx->fm_longs.reserve((3 * n + tiles + 2) * sizeof(uint64_t)));
    HIP_TRY(ctx->fm_recs.reserve(n * (sizeof(FmmOutRead) + sizeof(FmmOutSeq))));
    uint32_t* w = reinterpret_cast<uint32_t*>(ctx->fm_words.p);
    uint64_t* q = reinterpret_cast<uint64_t*>(ctx->fm_longs.p);
    FmmState s{};
    s.read_off = ctx->s_off.p;
    s.n = n_reads;
    s.links = reinterpret_cast<FmmLink*>(ctx->fm_links.p);
    s.cut = w;
    s.seed = w + 2 * n;
    s.mark = w + 3 * n;
    s.aux = w + 4 * n;
    s.key_of = w + 5 * n;
    s.root_of = w + 6 * n;
    s.key_reads = w + 7 * n;
    s.key_seq = w + 8 * n;
    uint32_t* d_tile_seqs = w + 9 * n;
    uint32_t* d_first_bad = d_tile_seqs + tiles;
    s.off_in_seq = q;
    s.key_len = q + n;
    s.key_off = q + 2 * n;
    unsigned long long* d_tile_bases = reinterpret_cast<unsigned long long*>(q + 3 * n);
    unsigned long long* d_totals = d_tile_bases + tiles;
    FmmNode* d_nodes[2] = {reinterpret_cast<FmmNode*>(ctx->fm_nodes.p), reinterpret_cast<FmmNode*>(ctx->fm_nodes.p) + 2 * n};
    FmmOutRead* d_reads = reinterpret_cast<FmmOutRead*>(ctx->fm_recs.p + n * sizeof(FmmOutSeq));
    FmmOutSeq* d_seqs = reinterpret_cast<FmmOutSeq*>(ctx->fm_recs.p);
    HIP_TRY(hipMemsetAsync(d_first_bad, 0xFF, kFmmBadCount * sizeof(uint32_t), ctx->stream));

    // the kernels' milliseconds by phase: overlap, links, chains, place (with the prefix sums and the records), assemble
    double phase_ms[5] = {0, 0, 0, 0, 0};
    double mark_ms = ctx->stats[LRSC_K_FIND].total_ms;
    auto phase_end = [&](int which) {
        phase_ms[which] += ctx->stats[LRSC_K_FIND].total_ms - mark_ms;
        mark_ms = ctx->stats[LRSC_K_FIND].total_ms;
    };
    // ---- links: the overlap's launches and the links' per chunk; the blocks stay in the pool
    for(uint64_t r0 = 0; r0 < n; r0 += plan.chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(plan.chunk, n - r0);
        st = overlap_chunk(ctx, plan, r0, m);
        if(st != LRSC_OK) return st;
        phase_end(0);
        st = find_launch(ctx, [&]() {
            return launch_fmmerge_links(s, (uint32_t)r0, m, plan.min_overlap, reinterpret_cast<const OvOutRead*>(ctx->ov_outs.p), reinterpret_cast<const OvOutBlock*>(ctx->ov_pool.p + 8),
                                        reinterpret_cast<const unsigned long long*>(ctx->ov_pool.p), reinterpret_cast<const OvChainHead*>(ctx->ov_heads.p), order[0], order[1],
                                        d_first_bad, ctx->stream);
        });
        if(st != LRSC_OK) return st;
        phase_end(1);
        // what the chunk's final blocks refuse is refused now, not after the overlap of every later chunk
        int broken = 0;
        uint32_t bad[kFmmBadCount];
        HIP_TRY(hipMemcpyAsync(&broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        COPY_TRY(ctx, bad, d_first_bad, sizeof(bad), hipMemcpyDeviceToHost);
        if(broken) return fail(LRSC_ERR_FORMAT, "overlap: an interval leaves the strand (the index is no BWT of a string set)");
        if(bad[kFmmBadOverflow] != kFmmNone)
            return fail(LRSC_ERR_LIMIT, "fm-merge: the overlap lists of read " + std::to_string(bad[kFmmBadOverflow]) + " outgrow the kernel's workspace");
        if(bad[kFmmBadFilter] != kFmmNone)
            return fail(LRSC_ERR_ARG, "fm-merge requires `stride filter` first: read " + std::to_string(bad[kFmmBadFilter]) + " is a duplicate or a substring of another read");
        if(bad[kFmmBadOwnRow] != kFmmNone)
            return fail(LRSC_ERR_ARG, "fm-merge: the row of read " + std::to_string(bad[kFmmBadOwnRow]) + " is not in its interval (the index is not that of these reads)");
        if(bad[kFmmBadPool] != kFmmNone) return fail(LRSC_ERR_FORMAT, "fm-merge: the blocks of read " + std::to_string(bad[kFmmBadPool]) + " lie outside the pool");
    }
    // ---- chains: rank, cut, rank again; 2 * (1 + fmm_rounds(n)) + 1 launches, a function of n alone
    const uint32_t rounds = fmm_rounds(n_reads);
    int cur = 0;
    for(int pass = 0; pass < 2; ++pass) {
        st = find_launch(ctx, [&]() { return launch_fmmerge_init(s, d_nodes[cur], ctx->stream); });
        if(st != LRSC_OK) return st;
        for(uint32_t r = 0; r < rounds; ++r) {
            st = find_launch(ctx, [&]() { return launch_fmmerge_round(s, d_nodes[cur], d_nodes[cur ^ 1], ctx->stream); });
            if(st != LRSC_OK) return st;
            cur ^= 1;
        }
        if(pass == 0) {
            st = find_launch(ctx, [&]() { return launch_fmmerge_cut(s, d_nodes[cur], ctx->stream); });
            if(st != LRSC_OK) return st;
        }
    }
    phase_end(2);
    // ---- place, and the prefix sums over the keys
    st = find_launch(ctx, [&]() { return launch_fmmerge_place(s, d_nodes[cur], ctx->stream); });
    if(st != LRSC_OK) return st;
    for(int step = 0; step < 3; ++step) {
        st = find_launch(ctx, [&]() { return launch_fmmerge_scan(s, step, d_tile_seqs, d_tile_bases, d_totals, ctx->stream); });
        if(st != LRSC_OK) return st;
    }
    unsigned long long totals[2] = {0, 0};
    COPY_TRY(ctx, totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost);
    if(totals[0] > n) return fail(LRSC_ERR_FORMAT, "fm-merge: more sequences than reads");
    if(totals[1] > bases_cap) {
        *n_bases_out = totals[1];
        return fail(LRSC_ERR_CAPACITY, "fm-merge: " + std::to_string(totals[1]) + " bases, room for " + std::to_string(bases_cap));
    }
    st = find_launch(ctx, [&]() { return launch_fmmerge_finish(s, d_reads, d_seqs, ctx->stream); });
    if(st != LRSC_OK) return st;
    phase_end(3);
    // ---- assemble
    HIP_TRY(ctx->fm_bases.reserve(std::max<uint64_t>(1, totals[1])));
    st = find_launch(ctx, [&]() { return launch_fmmerge_assemble(s, ctx->s_codes.p, reinterpret_cast<char*>(ctx->fm_bases.p), totals[1], ctx->stream); });
    if(st != LRSC_OK) return st;
    phase_end(4);
    if(std::getenv("LRSC_FMMERGE_PROFILE"))
        std::fprintf(stderr, "[lrsc] fm-merge kernels: overlap %.3f ms, links %.3f ms, chains %.3f ms, place %.3f ms, assemble %.3f ms\n", phase_ms[0], phase_ms[1],
                     phase_ms[2], phase_ms[3], phase_ms[4]);
    // the records go to vectors first: a failed copy leaves the caller's arrays untouched
    std::vector<FmmOutRead> h_reads(n);
    std::vector<FmmOutSeq> h_seqs(totals[0]);
    HIP_TRY(hipMemcpyAsync(h_reads.data(), d_reads, n * sizeof(FmmOutRead), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_seqs.data(), d_seqs, totals[0] * sizeof(FmmOutSeq), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    COPY_TRY(ctx, bases, ctx->fm_bases.p, totals[1], hipMemcpyDeviceToHost);
    std::memcpy(per_read, h_reads.data(), n * sizeof(FmmOutRead));
    if(totals[0]) std::memcpy(seqs, h_seqs.data(), totals[0] * sizeof(FmmOutSeq));
    *n_seqs_out = (uint32_t)totals[0];
    *n_bases_out = totals[1];
    return LRSC_OK;
}
