// capi_fmwalk.cpp -- what `stride fmwalk` needs of the library: the merge of a batch of paired-end reads by walking a context's
// index (fm_fmwalk.hip), the hybrid and kmerize algorithms with the sampled k-mer counts (fm_kmerize.hip), and the validate
// algorithm (fm_validate.hip).
#include "capi_internal.h"
#include "fm_fmwalk.h"
#include "fm_kmerize.h"
#include "fm_validate.h"

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

// ---- the hybrid and kmerize algorithms, the sampled k-mer counts (fm_kmerize.hip) ----
static_assert(kKmMaxSampleLength == LRSC_KMER_SAMPLE_MAX_LENGTH, "the limit that lrsc.h states");

// the slots of the reads' pieces: slot[i] = the sum over the reads j < i of max(len_j - k + 1, 0), slot[n_reads] = the sum over all
static std::vector<uint64_t> piece_slots(const uint64_t* read_off, uint32_t n_reads, uint32_t k)
{
    std::vector<uint64_t> slot((uint64_t)n_reads + 1, 0);
    for(uint32_t i = 0; i < n_reads; ++i) {
        const uint64_t len = read_off[i + 1] - read_off[i];
        slot[i + 1] = slot[i] + (len >= k ? len - k + 1 : 0);
    }
    return slot;
}

// The splits of `jobs` over the staged reads: pieces[0 .. n_slots) (only the jobs' own are meaningful) and outs[job].  validate:
// splitRead(std::string&)'s rules (fm_validate.hip), which have no `filters`.
static int run_splits(lrsc_ctx* ctx, const std::vector<KmJob>& jobs, uint32_t k, uint64_t threshold, bool filters, bool validate, uint64_t n_slots,
                      std::vector<KmPiece>& pieces, std::vector<KmJobOut>& outs)
{
    outs.assign(jobs.size(), KmJobOut{0u, -1});
    pieces.assign(n_slots, KmPiece{0u, 0u, 0u});
    if(jobs.empty()) return LRSC_OK;
    if(jobs.size() >= (1ull << 31)) return fail(LRSC_ERR_UNSUPPORTED, "fmwalk: 2^31 reads or more to split in one call");
    uint32_t longest = 0;
    for(const KmJob& j : jobs) longest = std::max(longest, j.len);
    const uint64_t slice = km_workspace_bytes(longest);
    const uint32_t waves_per_group = kKmThreads / kKmLanes;
    uint64_t groups = std::min<uint64_t>((jobs.size() + waves_per_group - 1) / waves_per_group, resident_waves(ctx, kKmWavesPerSimd) / waves_per_group);
    groups = std::max<uint64_t>(1, std::min<uint64_t>(groups, kFwWorkspaceBytes / (slice * waves_per_group)));
    HIP_TRY(ctx->km_ws.reserve(groups * waves_per_group * slice));
    HIP_TRY(ctx->km_jobs.reserve(jobs.size() * sizeof(KmJob)));
    HIP_TRY(ctx->km_outs.reserve(jobs.size() * sizeof(KmJobOut)));
    HIP_TRY(ctx->km_pieces.reserve(n_slots * sizeof(KmPiece)));
    HIP_TRY(hipMemcpyAsync(ctx->km_jobs.p, jobs.data(), jobs.size() * sizeof(KmJob), hipMemcpyHostToDevice, ctx->stream));
    uint32_t* d_broken = reinterpret_cast<uint32_t*>(ctx->s_flag.p);
    const int st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        const KmJob* d_jobs = reinterpret_cast<const KmJob*>(ctx->km_jobs.p);
        KmPiece* d_pieces = reinterpret_cast<KmPiece*>(ctx->km_pieces.p);
        KmJobOut* d_outs = reinterpret_cast<KmJobOut*>(ctx->km_outs.p);
        if(validate)
            return launch_validate_split(ctx->fm, ctx->s_codes.p, ctx->s_off.p, d_jobs, (uint32_t)jobs.size(), k, threshold, (uint32_t)groups, ctx->km_ws.p, slice, longest,
                                         d_pieces, d_outs, d_broken, ctx->d_ctr, ctx->stream);
        return launch_kmerize_split(ctx->fm, ctx->s_codes.p, ctx->s_off.p, d_jobs, (uint32_t)jobs.size(), k, (uint32_t)threshold, filters, (uint32_t)groups, ctx->km_ws.p,
                                    slice, longest, d_pieces, d_outs, d_broken, ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    int broken = 0;
    COPY_TRY(ctx, &broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost);
    if(broken) return fail(LRSC_ERR_FORMAT, "fmwalk: an interval leaves the strand (the index is no BWT of a string set)");
    HIP_TRY(hipMemcpyAsync(outs.data(), ctx->km_outs.p, jobs.size() * sizeof(KmJobOut), hipMemcpyDeviceToHost, ctx->stream));
    COPY_TRY(ctx, pieces.data(), ctx->km_pieces.p, n_slots * sizeof(KmPiece), hipMemcpyDeviceToHost);
    for(size_t j = 0; j < jobs.size(); ++j)
        if(outs[j].n_pieces == 0 || outs[j].n_pieces > jobs[j].len - k + 1 || outs[j].main_piece >= (int32_t)outs[j].n_pieces)
            return fail(LRSC_ERR_FORMAT, "fmwalk: a split with pieces it cannot have");
    return LRSC_OK;
}

// a job's result -> the read's record and its pieces in the caller's array, their starts within the untrimmed read
static void place_pieces(const KmJob& job, const KmJobOut& o, const std::vector<KmPiece>& from, KmRead& r, lrsc_fmwalk_piece* pieces)
{
    r.n_pieces = o.n_pieces;
    r.main_piece = o.main_piece;
    r.kmerize = 1;                                                // kmerReads is not empty
    for(uint32_t i = 0; i < o.n_pieces; ++i) {
        const KmPiece& q = from[job.slot + i];
        pieces[job.slot + i] = lrsc_fmwalk_piece{q.start + job.head, q.length, q.kept};
    }
}

// BWTAlgorithms::sampleKmerCounts without its rand() (SuffixTools/BWTAlgorithms.cpp:527-539, with 454-469 and 135-141)
extern "C" int lrsc_kmer_sample_counts(lrsc_ctx* ctx, const uint64_t* rows, uint32_t n, uint32_t len, uint32_t* counts)
{
    if(!ctx || (n && (!rows || !counts))) return fail(LRSC_ERR_ARG, "null");
    if(len == 0) return fail(LRSC_ERR_ARG, "kmer sample: a length of 0");
    if(len > kKmMaxSampleLength) return fail(LRSC_ERR_UNSUPPORTED, "kmer sample: a length above 4096");
    if(n == 0) return LRSC_OK;
    for(uint32_t i = 0; i < n; ++i)
        if(rows[i] >= ctx->fm.strand[1].n_dollars) return fail(LRSC_ERR_ARG, "kmer sample: row " + std::to_string(rows[i]) + " is none of the index's strings");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->s_flag.reserve(1));
    HIP_TRY(ctx->km_rows.reserve((uint64_t)n * sizeof(uint64_t)));
    HIP_TRY(ctx->km_counts.reserve((uint64_t)n * sizeof(uint32_t)));
    HIP_TRY(ctx->km_ws.reserve((uint64_t)n * len));
    HIP_TRY(hipMemcpyAsync(ctx->km_rows.p, rows, (uint64_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->s_flag.p, 0, sizeof(int), ctx->stream));
    const int st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_kmer_sample(ctx->fm, reinterpret_cast<const uint64_t*>(ctx->km_rows.p), n, len, ctx->km_ws.p, reinterpret_cast<uint32_t*>(ctx->km_counts.p),
                                  reinterpret_cast<uint32_t*>(ctx->s_flag.p), ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    int broken = 0;
    COPY_TRY(ctx, &broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost);
    if(broken) return fail(LRSC_ERR_FORMAT, "kmer sample: a row leaves the strand (the index is no BWT of a string set)");
    COPY_TRY(ctx, counts, ctx->km_counts.p, (uint64_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return LRSC_OK;
}

// FMIndexWalkProcess::KmerizeReads (FMIndexWalk/FMIndexWalkProcess.cpp:229-267) with splitRead(KmerContext&) (555-609), KmerContext
// (FMIndexWalkProcess.h:61-130), isSimple and numNextKmer (855-881)
extern "C" int lrsc_fmwalk_kmerize(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t kmer_length, int32_t kmer_threshold,
                                   lrsc_fmwalk_read_result* out, lrsc_fmwalk_piece* pieces, uint64_t n_piece_slots)
{
    if(!ctx || (n_reads && (!reads || !read_off || !out || !pieces))) return fail(LRSC_ERR_ARG, "null");
    if(kmer_length <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid kmer length: " + std::to_string(kmer_length));
    if(kmer_threshold <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid kmer threshold: " + std::to_string(kmer_threshold));
    if((uint32_t)kmer_length > kFwMaxKmer) return fail(LRSC_ERR_UNSUPPORTED, "fmwalk: above the kernel's limits (kmer length 255)");
    if(n_reads == 0) return LRSC_OK;
    int st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    const uint32_t k = (uint32_t)kmer_length;
    const std::vector<uint64_t> slot = piece_slots(read_off, n_reads, k);
    if(n_piece_slots < slot[n_reads]) return fail(LRSC_ERR_ARG, "fmwalk: fewer piece slots than the reads' k-mers");
    st = stage_reads(ctx, "fmwalk", 31, reads, read_off, n_reads, 0);
    if(st != LRSC_OK) return st;
    std::vector<KmJob> jobs;
    for(uint32_t i = 0; i < n_reads; ++i) {
        const uint64_t len = read_off[i + 1] - read_off[i];
        if(len >= k) jobs.push_back(KmJob{i, 0u, (uint32_t)len, 0u, slot[i]});
    }
    std::vector<KmPiece> got;
    std::vector<KmJobOut> outs;
    st = run_splits(ctx, jobs, k, (uint32_t)kmer_threshold, false, false, slot[n_reads], got, outs);
    if(st != LRSC_OK) return st;
    std::vector<KmRead> res(n_reads, KmRead{0u, 0, 0u, 0u, -1, 0u});
    for(size_t j = 0; j < jobs.size(); ++j) {
        res[jobs[j].read].length = jobs[j].len;
        place_pieces(jobs[j], outs[j], got, res[jobs[j].read], pieces);
    }
    static_assert(sizeof(KmRead) == sizeof(lrsc_fmwalk_read_result), "KmRead is lrsc_fmwalk_read_result");
    std::memcpy(out, res.data(), (uint64_t)n_reads * sizeof(KmRead));
    return LRSC_OK;
}

// FMIndexWalkProcess::MergeAndKmerize (FMIndexWalk/FMIndexWalkProcess.cpp:29-150) with trimRead (825-851), isSuitableForFMWalk
// (394-415), SAIntervalTree::mergeTwoReads, splitRead(KmerContext&) (555-609), isLowComplexity (418-445) and maxCon (448-477)
extern "C" int lrsc_fmwalk_hybrid(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_pairs, const lrsc_fmwalk_params* p, uint64_t repeat_kmer_freq,
                                  char* merged, uint64_t stride, lrsc_fmwalk_hybrid_result* out, lrsc_fmwalk_piece* pieces, uint64_t n_piece_slots)
{
    if(!ctx || !p || (n_pairs && (!reads || !read_off || !merged || !out || !pieces))) return fail(LRSC_ERR_ARG, "null");
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
    const uint32_t n_reads = 2 * n_pairs, k = (uint32_t)p->kmer_length;
    int st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    const std::vector<uint64_t> slot = piece_slots(read_off, n_reads, k);
    if(n_piece_slots < slot[n_reads]) return fail(LRSC_ERR_ARG, "fmwalk: fewer piece slots than the reads' k-mers");
    st = stage_reads(ctx, "fmwalk", 31, reads, read_off, n_reads, 0);
    if(st != LRSC_OK) return st;
    const FwParams gp{p->kmer_length, p->kmer_threshold, p->min_overlap, p->max_overlap, p->max_insert, p->max_leaves};
    FwParams wp = gp;
    wp.kmer_threshold = (int32_t)kKmWalkThreshold;                // MergeAndKmerize gives its trees no threshold: the constructor's 3
    const uint64_t slice = fw_workspace_bytes(wp);
    const uint32_t waves_per_group = kFwThreads / kFwLanes, n_walks = 2 * n_pairs;
    uint64_t groups = std::min<uint64_t>(((uint64_t)n_walks + waves_per_group - 1) / waves_per_group, resident_waves(ctx, kFwWavesPerSimd) / waves_per_group);
    groups = std::max<uint64_t>(1, std::min<uint64_t>(groups, kFwWorkspaceBytes / (slice * waves_per_group)));
    const uint64_t m4 = ((uint64_t)p->min_overlap + 3) & ~3ull;
    HIP_TRY(ctx->fw_ws.reserve(groups * waves_per_group * slice));
    HIP_TRY(ctx->fw_strs.reserve((uint64_t)n_pairs * 4 * m4));
    HIP_TRY(ctx->km_gates.reserve((uint64_t)n_pairs * sizeof(KmGate)));
    HIP_TRY(ctx->fw_best.reserve((uint64_t)n_walks * stride));
    HIP_TRY(ctx->fw_outs.reserve((uint64_t)n_walks * sizeof(FwWalkOut)));
    uint32_t* d_broken = reinterpret_cast<uint32_t*>(ctx->s_flag.p);
    FwWalkOut* d_outs = reinterpret_cast<FwWalkOut*>(ctx->fw_outs.p);
    KmGate* d_gates = reinterpret_cast<KmGate*>(ctx->km_gates.p);
    st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_hybrid_gate(ctx->fm, ctx->s_codes.p, ctx->s_off.p, n_pairs, gp, repeat_kmer_freq, ctx->fw_strs.p, d_gates, d_broken, ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    int broken = 0;
    COPY_TRY(ctx, &broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost);      // a gate that was not written is not read
    if(broken) return fail(LRSC_ERR_FORMAT, "fmwalk: an interval leaves the strand (the index is no BWT of a string set)");
    st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_hybrid_walks(ctx->fm, ctx->s_off.p, n_pairs, wp, ctx->fw_strs.p, d_gates, (uint32_t)groups, ctx->fw_ws.p, slice, ctx->fw_best.p, stride, d_outs,
                                   d_broken, ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    COPY_TRY(ctx, &broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost);
    if(broken) return fail(LRSC_ERR_FORMAT, "fmwalk: an interval leaves the strand (the index is no BWT of a string set)");
    std::vector<uint8_t> codes((uint64_t)n_walks * stride);
    std::vector<FwWalkOut> outs(n_walks);
    std::vector<KmGate> gates(n_pairs);
    HIP_TRY(hipMemcpyAsync(codes.data(), ctx->fw_best.p, codes.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(outs.data(), d_outs, (uint64_t)n_walks * sizeof(FwWalkOut), hipMemcpyDeviceToHost, ctx->stream));
    COPY_TRY(ctx, gates.data(), d_gates, (uint64_t)n_pairs * sizeof(KmGate), hipMemcpyDeviceToHost);
    // the three accept rules (FMIndexWalkProcess.cpp:77-103), then case 3's splits for the pairs that are left
    std::vector<KmHybrid> res(n_pairs);
    std::vector<uint32_t> pick(n_pairs, kFwNone);
    std::vector<KmJob> jobs;
    for(uint32_t i = 0; i < n_pairs; ++i) {
        const KmGate& g = gates[i];
        const bool walked = (g.flags & kKmWalk) != 0, gate = (g.flags & kKmGate) != 0;
        KmHybrid& r = res[i];
        r.walk = FwResult{0u, 0u, {0, 0}, {0u, 0u}, {0ull, 0ull}, {g.trimmed[0], g.trimmed[1]}};
        for(uint32_t e = 0; e < 2; ++e) {
            const uint64_t len = read_off[2 * i + e + 1] - read_off[2 * i + e];
            if(g.trimmed[e] > len || (uint64_t)g.head[e] + g.trimmed[e] > len || g.head[e] < 0) return fail(LRSC_ERR_FORMAT, "fmwalk: a trim beyond its read");
            r.read[e] = KmRead{gate ? 1u : 0u, g.head[e], g.trimmed[e], 0u, -1, gate ? 1u : 0u};
        }
        if(walked) {
            const FwWalkOut &w0 = outs[2 * i], &w1 = outs[2 * i + 1];
            if(w0.length > stride || w1.length > stride) return fail(LRSC_ERR_FORMAT, "fmwalk: a merged string longer than its slot");
            bool same = w0.length != 0 && w0.length == w1.length;
            const uint8_t *s0 = codes.data() + 2ull * i * stride, *s1 = s0 + stride;
            for(uint32_t j = 0; same && j < w0.length; ++j) same = (s0[j] & 3u) == ((s1[w0.length - 1 - j] & 3u) ^ 3u);
            pick[i] = km_choose(w0, w1, same);
            r.walk.status[0] = w0.status; r.walk.status[1] = w1.status;
            r.walk.max_used_leaves[0] = w0.max_used; r.walk.max_used_leaves[1] = w1.max_used;
            r.walk.coverage[0] = w0.coverage; r.walk.coverage[1] = w1.coverage;
            if(pick[i] != kFwNone) {
                r.walk.merged = 1;
                r.walk.length = pick[i] ? w1.length : w0.length;
                continue;
            }
        }
        if(g.flags & kKmReturned) continue;
        for(uint32_t e = 0; e < 2; ++e)
            if(g.trimmed[e] >= k) jobs.push_back(KmJob{2 * i + e, (uint32_t)g.head[e], g.trimmed[e], 0u, slot[2 * i + e]});
    }
    std::vector<KmPiece> got;
    std::vector<KmJobOut> jouts;
    st = run_splits(ctx, jobs, k, (uint32_t)p->kmer_threshold, true, false, slot[n_reads], got, jouts);
    if(st != LRSC_OK) return st;
    for(size_t j = 0; j < jobs.size(); ++j) place_pieces(jobs[j], jouts[j], got, res[jobs[j].read >> 1].read[jobs[j].read & 1u], pieces);
    for(uint32_t i = 0; i < n_pairs; ++i) {
        if(!res[i].walk.merged) continue;
        const uint8_t* from = codes.data() + (2ull * i + pick[i]) * stride;
        for(uint32_t j = 0; j < res[i].walk.length; ++j) merged[(uint64_t)i * stride + j] = "ACGT"[from[j] & 3u];
    }
    static_assert(sizeof(KmHybrid) == sizeof(lrsc_fmwalk_hybrid_result), "KmHybrid is lrsc_fmwalk_hybrid_result");
    std::memcpy(out, res.data(), (uint64_t)n_pairs * sizeof(KmHybrid));
    return LRSC_OK;
}

// FMIndexWalkProcess::ValidateReads (FMIndexWalk/FMIndexWalkProcess.cpp:269-391) with SAIntervalTree's single-read constructor and
// validate() (FMIndexWalk/SAIntervalTree.cpp:59-94, 173-237), splitRead(std::string&) (613-722) and isLowComplexity (418-445)
extern "C" int lrsc_fmwalk_validate(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, const lrsc_fmwalk_params* p, char* merged,
                                    uint64_t stride, lrsc_fmwalk_validate_result* out, lrsc_fmwalk_piece* pieces, uint64_t n_piece_slots)
{
    if(!ctx || !p || (n_reads && (!reads || !read_off || !merged || !out || !pieces))) return fail(LRSC_ERR_ARG, "null");
    if(p->kmer_length <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid kmer length: " + std::to_string(p->kmer_length));
    if(p->kmer_threshold <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid kmer threshold: " + std::to_string(p->kmer_threshold));
    if(p->min_overlap < 2) return fail(LRSC_ERR_ARG, "fmwalk: invalid min overlap: " + std::to_string(p->min_overlap));
    if(p->max_overlap <= 0 && p->max_overlap != -1) return fail(LRSC_ERR_ARG, "fmwalk: invalid max overlap: " + std::to_string(p->max_overlap));
    if(p->max_leaves <= 0) return fail(LRSC_ERR_ARG, "fmwalk: invalid max leaves: " + std::to_string(p->max_leaves));
    if((uint32_t)p->max_leaves > kFwMaxLeaves || (uint32_t)p->min_overlap > kFwMaxOverlap || (uint32_t)p->kmer_length > kFwMaxKmer)
        return fail(LRSC_ERR_UNSUPPORTED, "fmwalk: above the kernel's limits (max leaves 64, min overlap 255, kmer length 255)");
    if(n_reads == 0) return LRSC_OK;
    if(n_reads >= (1u << 30)) return fail(LRSC_ERR_UNSUPPORTED, "fmwalk: 2^30 reads or more in one call");
    int st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    const uint32_t k = (uint32_t)p->kmer_length, m = (uint32_t)p->min_overlap;
    uint64_t longest = 0;
    bool any_walk = false;
    for(uint32_t i = 0; i < n_reads; ++i) {
        const uint64_t len = read_off[i + 1] - read_off[i];
        // the longest string a walk of the read can leave is one base beyond its depth limit
        if(len >> 31 || vd_depth((uint32_t)len) + 1 > kFwMaxInsert)
            return fail(LRSC_ERR_UNSUPPORTED, "fmwalk: read " + std::to_string(i) + " has " + std::to_string(len) + " bases: a walk of it could leave more than " +
                                                  std::to_string(kFwMaxInsert));
        longest = std::max(longest, len);
        any_walk = any_walk || len > m;
    }
    const uint32_t depth = vd_depth((uint32_t)longest);
    if(stride < (uint64_t)depth + 1) return fail(LRSC_ERR_ARG, "fmwalk: the stride of merged is below 1.1 * the longest read + 1");
    const std::vector<uint64_t> slot = piece_slots(read_off, n_reads, k);
    if(n_piece_slots < slot[n_reads]) return fail(LRSC_ERR_ARG, "fmwalk: fewer piece slots than the reads' k-mers");
    st = stage_reads(ctx, "fmwalk", 31, reads, read_off, n_reads, 0);
    if(st != LRSC_OK) return st;
    const uint32_t n_walks = 2 * n_reads;
    const uint64_t row = (uint64_t)depth + 1;                     // of a walk's string on the device
    std::vector<uint8_t> codes;
    std::vector<FwWalkOut> outs(n_walks, FwWalkOut{0, 0u, 0u, 0u, 0ull});
    if(any_walk) {
        const FwParams fp{p->kmer_length, p->kmer_threshold, p->min_overlap, p->max_overlap, (int32_t)std::max(depth, 1u), p->max_leaves};
        const uint64_t slice = fw_workspace_bytes(fp);
        const uint32_t waves_per_group = kVdThreads / kVdLanes;
        uint64_t groups = std::min<uint64_t>(((uint64_t)n_walks + waves_per_group - 1) / waves_per_group, resident_waves(ctx, kVdWavesPerSimd) / waves_per_group);
        groups = std::max<uint64_t>(1, std::min<uint64_t>(groups, kFwWorkspaceBytes / (slice * waves_per_group)));
        HIP_TRY(ctx->fw_ws.reserve(groups * waves_per_group * slice));
        HIP_TRY(ctx->fw_best.reserve((uint64_t)n_walks * row));
        HIP_TRY(ctx->fw_outs.reserve((uint64_t)n_walks * sizeof(FwWalkOut)));
        uint32_t* d_broken = reinterpret_cast<uint32_t*>(ctx->s_flag.p);
        FwWalkOut* d_outs = reinterpret_cast<FwWalkOut*>(ctx->fw_outs.p);
        st = timed_launch(ctx, LRSC_K_FIND, [&]() {
            return launch_validate_walks(ctx->fm, ctx->s_codes.p, ctx->s_off.p, n_reads, fp, (uint32_t)groups, ctx->fw_ws.p, slice, ctx->fw_best.p, row, d_outs, d_broken,
                                         ctx->d_ctr, ctx->stream);
        });
        if(st != LRSC_OK) return st;
        int broken = 0;
        COPY_TRY(ctx, &broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost);
        if(broken) return fail(LRSC_ERR_FORMAT, "fmwalk: an interval leaves the strand (the index is no BWT of a string set)");
        codes.resize((uint64_t)n_walks * row);
        HIP_TRY(hipMemcpyAsync(codes.data(), ctx->fw_best.p, codes.size(), hipMemcpyDeviceToHost, ctx->stream));
        COPY_TRY(ctx, outs.data(), d_outs, (uint64_t)n_walks * sizeof(FwWalkOut), hipMemcpyDeviceToHost);
    }
    // the short reads, the decision (FMIndexWalkProcess.cpp:280-294, 318-352), then the splits of the reads that are left
    std::vector<VdResult> res(n_reads);
    std::vector<KmJob> jobs;
    std::vector<uint8_t> own;
    for(uint32_t i = 0; i < n_reads; ++i) {
        const uint32_t len = (uint32_t)(read_off[i + 1] - read_off[i]);
        if(len <= m) {
            own.resize(len);
            st = encode_acgt(reads + read_off[i], len, own.data());
            if(st != LRSC_OK) return st;
            res[i] = vd_result(len, FwWalkOut{0, 0u, 0u, 0u, 0ull}, FwWalkOut{0, 0u, 0u, 0u, 0ull});
            res[i].read.whole = 1;
            res[i].read.kmerize = km_low_complexity(own.data(), len) ? 0u : 1u;
            continue;
        }
        res[i] = vd_result(len, outs[2 * i], outs[2 * i + 1]);
        if(outs[2 * i].length > row || outs[2 * i + 1].length > row) return fail(LRSC_ERR_FORMAT, "fmwalk: a walk's string longer than its slot");
        if(!res[i].merged && len >= k) jobs.push_back(KmJob{i, 0u, len, 0u, slot[i]});
    }
    std::vector<KmPiece> got;
    std::vector<KmJobOut> jouts;
    st = run_splits(ctx, jobs, k, vd_split_threshold(p->kmer_threshold), false, true, slot[n_reads], got, jouts);
    if(st != LRSC_OK) return st;
    for(size_t j = 0; j < jobs.size(); ++j) place_pieces(jobs[j], jouts[j], got, res[jobs[j].read].read, pieces);
    for(uint32_t i = 0; i < n_reads; ++i) {
        if(!res[i].merged) continue;
        char* to = merged + (uint64_t)i * stride;
        if(res[i].chosen < 0) std::memcpy(to, reads + read_off[i], res[i].length);
        else {
            const uint8_t* from = codes.data() + (2ull * i + (uint32_t)res[i].chosen) * row;
            for(uint32_t j = 0; j < res[i].length; ++j) to[j] = "ACGT"[from[j] & 3u];
        }
    }
    static_assert(sizeof(VdResult) == sizeof(lrsc_fmwalk_validate_result), "VdResult is lrsc_fmwalk_validate_result");
    std::memcpy(out, res.data(), (uint64_t)n_reads * sizeof(VdResult));
    return LRSC_OK;
}
