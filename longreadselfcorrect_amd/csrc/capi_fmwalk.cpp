// capi_fmwalk.cpp -- what `stride fmwalk -a merge` needs of the library: the merge of a batch of paired-end reads by walking a
// context's index (fm_fmwalk.hip).
#include "capi_internal.h"
#include "fm_fmwalk.h"

using namespace lrsc;

static_assert(kFwMaxLeaves == LRSC_FMWALK_MAX_LEAVES && kFwMaxInsert == LRSC_FMWALK_MAX_INSERT && kFwMaxOverlap == LRSC_FMWALK_MAX_MIN_OVERLAP &&
                  kFwMaxKmer == LRSC_FMWALK_MAX_KMER,
              "the limits that lrsc.h states");

// the wavefronts' slices together stay below this: fewer wavefronts walk when the parameters make a slice large
constexpr uint64_t kFwWorkspaceBytes = 1ull << 30;

// FMIndexWalkProcess::MergePairedReads (FMIndexWalk/FMIndexWalkProcess.cpp:153-226) with trimRead (825-870) and
// SAIntervalTree::mergeTwoReads (FMIndexWalk/SAIntervalTree.cpp:103-170)
extern "C" int lrsc_fmwalk_merge(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_pairs, const lrsc_fmwalk_params* p, char* merged,
                                 uint64_t stride, lrsc_fmwalk_result* out)
{
    if(!ctx || !p || (n_pairs && (!reads || !read_off || !merged || !out))) return fail(LRSC_ERR_ARG, "null");
    if(p->kmer_length <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid kmer length: " + std::to_string(p->kmer_length));
    if(p->kmer_threshold <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid kmer threshold: " + std::to_string(p->kmer_threshold));
    if(p->min_overlap < 2) return fail(LRSC_ERR_ARG, "fmwalk: invalid min overlap: " + std::to_string(p->min_overlap));
    if(p->max_overlap <= 0 && p->max_overlap != -1) return fail(LRSC_ERR_ARG, "fmwalk: invalid max overlap: " + std::to_string(p->max_overlap));
    if(p->max_insert <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid max insert size: " + std::to_string(p->max_insert));
    if(p->max_leaves <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid max leaves: " + std::to_string(p->max_leaves));
    if((uint32_t)p->max_leaves > kFwMaxLeaves || (uint32_t)p->max_insert > kFwMaxInsert || (uint32_t)p->min_overlap > kFwMaxOverlap ||
       (uint32_t)p->kmer_length > kFwMaxKmer)
        return fail(LRSC_ERR_UNSUPPORTED, "fmwalk: above the kernel's limits (max leaves 64, max insert size 2000, min overlap 255, kmer length 255)");
    if(stride < (uint64_t)std::max(p->max_insert + 1, p->min_overlap)) return fail(LRSC_ERR_ARG, "fmwalk: the stride of merged is below max(max insert size + 1, min overlap)");
    if(n_pairs == 0) return LRSC_OK;
    if(n_pairs >= (1u << 30)) return fail(LRSC_ERR_UNSUPPORTED, "fmwalk: 2^30 pairs or more in one call");
    const uint32_t n_reads = 2 * n_pairs;
    int st = stage_reads(ctx, "fmwalk", 31, reads, read_off, n_reads, 0);
    if(st != LRSC_OK) return st;
    const FwParams fp{p->kmer_length, p->kmer_threshold, p->min_overlap, p->max_overlap, p->max_insert, p->max_leaves};
    const uint64_t slice = fw_workspace_bytes(fp);
    const uint32_t waves_per_group = kFwThreads / kFwLanes, n_walks = 2 * n_pairs;
    uint64_t groups = std::min<uint64_t>(((uint64_t)n_walks + waves_per_group - 1) / waves_per_group, resident_waves(ctx, kFwWavesPerSimd) / waves_per_group);
    groups = std::max<uint64_t>(1, std::min<uint64_t>(groups, kFwWorkspaceBytes / (slice * waves_per_group)));
    const uint64_t m4 = ((uint64_t)p->min_overlap + 3) & ~3ull;
    HIP_TRY(ctx->fw_ws.reserve(groups * waves_per_group * slice));
    HIP_TRY(ctx->fw_strs.reserve((uint64_t)n_pairs * 4 * m4));
    HIP_TRY(ctx->fw_trimmed.reserve(n_reads));
    HIP_TRY(ctx->fw_best.reserve((uint64_t)n_walks * stride));
    HIP_TRY(ctx->fw_outs.reserve((uint64_t)n_walks * sizeof(FwWalkOut)));
    uint32_t* d_broken = reinterpret_cast<uint32_t*>(ctx->s_flag.p);
    FwWalkOut* d_outs = reinterpret_cast<FwWalkOut*>(ctx->fw_outs.p);
    st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_fmwalk_trim(ctx->fm, ctx->s_codes.p, ctx->s_off.p, n_pairs, fp, ctx->fw_strs.p, ctx->fw_trimmed.p, d_broken, ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_fmwalk_walks(ctx->fm, ctx->s_off.p, n_pairs, fp, ctx->fw_strs.p, ctx->fw_trimmed.p, (uint32_t)groups, ctx->fw_ws.p, slice, ctx->fw_best.p, stride,
                                   d_outs, d_broken, ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    int broken = 0;
    HIP_TRY(hipMemcpyAsync(&broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if(broken) return fail(LRSC_ERR_FORMAT, "fmwalk: an interval leaves the strand (the index is no BWT of a string set)");
    std::vector<uint8_t> codes((uint64_t)n_walks * stride);
    std::vector<FwWalkOut> outs(n_walks);
    std::vector<uint32_t> trimmed(n_reads);
    HIP_TRY(hipMemcpyAsync(codes.data(), ctx->fw_best.p, codes.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(outs.data(), d_outs, (uint64_t)n_walks * sizeof(FwWalkOut), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(trimmed.data(), ctx->fw_trimmed.p, (uint64_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // MergePairedReads' choice between the two walks (FMIndexWalkProcess.cpp:193-220)
    std::vector<FwResult> res(n_pairs);
    for(uint32_t i = 0; i < n_pairs; ++i) {
        const bool walked = trimmed[2 * i] >= (uint32_t)p->min_overlap && trimmed[2 * i + 1] >= (uint32_t)p->min_overlap;
        res[i] = fw_result(walked, &trimmed[2 * i], outs[2 * i], outs[2 * i + 1]);
        if(res[i].merged && res[i].length > stride) return fail(LRSC_ERR_FORMAT, "fmwalk: a merged string longer than its slot");
    }
    for(uint32_t i = 0; i < n_pairs; ++i) {
        if(!res[i].merged) continue;
        const uint8_t* from = codes.data() + (2ull * i + fw_choose(outs[2 * i], outs[2 * i + 1])) * stride;
        for(uint32_t j = 0; j < res[i].length; ++j) merged[(uint64_t)i * stride + j] = "ACGT"[from[j] & 3u];
    }
    static_assert(sizeof(FwResult) == sizeof(lrsc_fmwalk_result), "FwResult is lrsc_fmwalk_result");
    std::memcpy(out, res.data(), (uint64_t)n_pairs * sizeof(FwResult));
    return LRSC_OK;
}
