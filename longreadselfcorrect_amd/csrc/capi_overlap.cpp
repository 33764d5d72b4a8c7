// capi_overlap.cpp -- what `stride overlap` needs of the library: the exact irreducible overlaps of a batch of reads against a
// context's index (fm_overlap.hip).
#include "capi_internal.h"
#include "fm_overlap.h"

using namespace lrsc;

static_assert(kOvMaxRead == LRSC_OVERLAP_MAX_READ && kOvMaxMinOverlap == LRSC_OVERLAP_MAX_MIN_OVERLAP && kOvOverflow == LRSC_OVERLAP_OVERFLOW,
              "the limits and the status that lrsc.h states");
static_assert(sizeof(OvOutRead) == sizeof(lrsc_overlap_read) && sizeof(OvOutBlock) == sizeof(lrsc_overlap_block), "the records are lrsc.h's");

// the wavefronts' slices together stay below this: fewer wavefronts reduce when the parameters make a slice large
constexpr uint64_t kOvWorkspaceBytes = 1ull << 30;
// what the chains of a chunk of reads leave stays below this, and a chunk has at most this many reads
constexpr uint64_t kOvChainBytes = 256ull << 20;
constexpr uint64_t kOvChunkReads = 1ull << 15;

// min_overlap within 2 .. the kernel's limit: both entries ask before anything else, an empty batch included
int lrsc::overlap_check_min(int32_t min_overlap)
{
    if(min_overlap < 2) return fail(LRSC_ERR_ARG, "overlap: invalid min overlap: " + std::to_string(min_overlap));
    if((uint32_t)min_overlap > kOvMaxMinOverlap) return fail(LRSC_ERR_UNSUPPORTED, "overlap: above the kernel's limits (min overlap 2000, read length 2000)");
    return LRSC_OK;
}

// What lrsc_overlap_exact and lrsc_fmmerge do before their first launch, after overlap_check_min: the reads' checks, the reads
// staged, the chunk and the grids sized, the ctx's overlap buffers reserved.  n_reads != 0.
int lrsc::overlap_plan(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap, OverlapPlan& plan)
{
    int st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    OvParams p{(uint32_t)min_overlap, 0u};
    for(uint32_t i = 0; i < n_reads; ++i) {
        const uint64_t len = read_off[i + 1] - read_off[i];
        if(len == 0) return fail(LRSC_ERR_ARG, "overlap: read " + std::to_string(i) + " is empty");
        if(len > kOvMaxRead) return fail(LRSC_ERR_UNSUPPORTED, "overlap: above the kernel's limits (min overlap 2000, read length 2000)");
        p.max_len = std::max(p.max_len, (uint32_t)len);
    }
    st = stage_reads(ctx, "overlap", 31, reads, read_off, n_reads, 0);
    if(st != LRSC_OK) return st;
    const uint64_t slots = ov_slots(p), slice = ov_workspace_bytes(p);
    const uint64_t per_read_bytes = kOvChains * (slots * sizeof(OvBlock) + sizeof(OvChainHead));
    uint64_t chunk = std::min<uint64_t>(kOvChunkReads, std::max<uint64_t>(kOvReadsPerWave, kOvChainBytes / per_read_bytes / kOvReadsPerWave * kOvReadsPerWave));
    chunk = std::min<uint64_t>(chunk, n_reads);
    const uint32_t waves_per_group = kOvThreads / kOvLanes;
    const uint64_t resident = std::max<uint64_t>(1, resident_waves(ctx, kOvWavesPerSimd) / waves_per_group);
    const uint64_t reduce_groups = std::max<uint64_t>(1, std::min<uint64_t>({(chunk + waves_per_group - 1) / waves_per_group, resident, kOvWorkspaceBytes / (slice * waves_per_group)}));
    const uint64_t collect_groups = std::max<uint64_t>(1, std::min<uint64_t>((chunk + kOvReadsPerWave * waves_per_group - 1) / (kOvReadsPerWave * waves_per_group), resident));
    const uint64_t pool_cap = chunk * kOvOutCap;
    HIP_TRY(ctx->ov_ws.reserve(reduce_groups * waves_per_group * slice));
    HIP_TRY(ctx->ov_heads.reserve(chunk * kOvChains * sizeof(OvChainHead)));
    HIP_TRY(ctx->ov_chain.reserve(std::max<uint64_t>(1, chunk * kOvChains * slots) * sizeof(OvBlock)));
    HIP_TRY(ctx->ov_outs.reserve(chunk * sizeof(OvOutRead)));
    HIP_TRY(ctx->ov_pool.reserve(8 + pool_cap * sizeof(OvOutBlock)));
    plan = OverlapPlan{p.min_overlap, p.max_len, (uint32_t)collect_groups, (uint32_t)reduce_groups, chunk, slice, pool_cap};
    return LRSC_OK;
}

// The collect and the reduce of the reads [r0, r0 + n), n <= plan.chunk: their results in ov_outs, their final blocks in ov_pool
// behind its counter, their chains' heads in ov_heads, all on the ctx's stream
int lrsc::overlap_chunk(lrsc_ctx* ctx, const OverlapPlan& plan, uint64_t r0, uint32_t n)
{
    const OvParams p{plan.min_overlap, plan.max_len};
    uint32_t* d_broken = reinterpret_cast<uint32_t*>(ctx->s_flag.p);
    OvChainHead* d_heads = reinterpret_cast<OvChainHead*>(ctx->ov_heads.p);
    OvBlock* d_chain = reinterpret_cast<OvBlock*>(ctx->ov_chain.p);
    unsigned long long* d_used = reinterpret_cast<unsigned long long*>(ctx->ov_pool.p);
    HIP_TRY(hipMemsetAsync(d_used, 0, 8, ctx->stream));
    int st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_overlap_collect(ctx->fm, ctx->s_codes.p, ctx->s_off.p + r0, n, p, plan.collect_groups, d_heads, d_chain, d_broken, ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    return timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_overlap_reduce(ctx->fm, ctx->s_off.p + r0, n, p, d_heads, d_chain, plan.reduce_groups, ctx->ov_ws.p, plan.slice, reinterpret_cast<OvOutRead*>(ctx->ov_outs.p),
                                     reinterpret_cast<OvOutBlock*>(ctx->ov_pool.p + 8), plan.pool_cap, d_used, d_broken, ctx->d_ctr, ctx->stream);
    });
}

// OverlapAlgorithm::overlapRead in exact mode, irreducible edges only (Algorithm/OverlapAlgorithm.cpp:22-44, 270-344)
extern "C" int lrsc_overlap_exact(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap, lrsc_overlap_read* per_read,
                                  lrsc_overlap_block* blocks, uint64_t block_cap, uint64_t* n_blocks_out)
{
    if(!ctx || !n_blocks_out || (n_reads && (!reads || !read_off || !per_read)) || (block_cap && !blocks)) return fail(LRSC_ERR_ARG, "null");
    int st = overlap_check_min(min_overlap);
    if(st != LRSC_OK) return st;
    if(n_reads == 0) {
        *n_blocks_out = 0;
        return LRSC_OK;
    }
    OverlapPlan plan;
    st = overlap_plan(ctx, reads, read_off, n_reads, min_overlap, plan);
    if(st != LRSC_OK) return st;
    const uint64_t chunk = plan.chunk, pool_cap = plan.pool_cap;
    OvOutRead* d_outs = reinterpret_cast<OvOutRead*>(ctx->ov_outs.p);
    unsigned long long* d_used = reinterpret_cast<unsigned long long*>(ctx->ov_pool.p);
    OvOutBlock* d_pool = reinterpret_cast<OvOutBlock*>(ctx->ov_pool.p + 8);

    std::vector<OvOutRead> res(n_reads);
    std::vector<OvOutBlock> all;                                  // in read order
    std::vector<OvOutBlock> pool;
    for(uint64_t r0 = 0; r0 < n_reads; r0 += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, n_reads - r0);
        st = overlap_chunk(ctx, plan, r0, n);
        if(st != LRSC_OK) return st;
        int broken = 0;
        unsigned long long used = 0;
        HIP_TRY(hipMemcpyAsync(&broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&used, d_used, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(res.data() + r0, d_outs, (uint64_t)n * sizeof(OvOutRead), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if(broken) return fail(LRSC_ERR_FORMAT, "overlap: an interval leaves the strand (the index is no BWT of a string set)");
        if(used > pool_cap) return fail(LRSC_ERR_FORMAT, "overlap: more final blocks than the pool holds");
        pool.resize(used);
        COPY_TRY(ctx, pool.data(), d_pool, used * sizeof(OvOutBlock), hipMemcpyDeviceToHost);
        // the pool's order is that in which the wavefronts finished: the reads' blocks are put in read order here
        for(uint64_t r = r0; r < r0 + n; ++r) {
            OvOutRead& q = res[r];
            if(q.n_blocks > kOvOutCap || q.first_block + q.n_blocks > used) return fail(LRSC_ERR_FORMAT, "overlap: a read's blocks lie outside the pool");
            const uint64_t first = all.size();
            all.insert(all.end(), pool.begin() + (long)q.first_block, pool.begin() + (long)(q.first_block + q.n_blocks));
            q.first_block = first;
        }
    }
    *n_blocks_out = all.size();
    if(all.size() > block_cap) return fail(LRSC_ERR_CAPACITY, "overlap: " + std::to_string(all.size()) + " blocks, room for " + std::to_string(block_cap));
    std::memcpy(per_read, res.data(), (uint64_t)n_reads * sizeof(OvOutRead));
    if(!all.empty()) std::memcpy(blocks, all.data(), all.size() * sizeof(OvOutBlock));
    return LRSC_OK;
}
