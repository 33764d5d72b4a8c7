// capi_kcorrect.cpp -- what `stride correct -a kmer` needs of the library: the k-mer correction of a batch of reads against a
// context's index (fm_kcorrect.hip).
#include "capi_internal.h"
#include "fm_kcorrect.h"

using namespace lrsc;

// ErrorCorrectProcess::kmerCorrection (Algorithm/ErrorCorrectProcess.cpp:287-438) with attemptKmerCorrection (488-544)
extern "C" int lrsc_kmer_correct(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, const uint8_t* phred,
                                 const lrsc_kcorrect_params* p, char* corrected, lrsc_kcorrect_result* out)
{
    if(!ctx || !p || (n_reads && (!reads || !read_off || !corrected || !out))) return fail(LRSC_ERR_ARG, "null");
    if(p->kmer_length <= 0) return fail(LRSC_ERR_ARG, "kmer correct: invalid kmer length: " + std::to_string(p->kmer_length));
    if(p->kmer_threshold <= 0) return fail(LRSC_ERR_ARG, "kmer correct: invalid kmer threshold: " + std::to_string(p->kmer_threshold));
    if(p->kmer_rounds <= 0) return fail(LRSC_ERR_ARG, "kmer correct: invalid number of kmer rounds: " + std::to_string(p->kmer_rounds));
    if(n_reads == 0) return LRSC_OK;
    int st = stage_reads(ctx, "kmer correct", 31, reads, read_off, n_reads, 0);
    if(st != LRSC_OK) return st;
    // the reads that do not fit LDS get a slice of the workspace
    std::vector<uint64_t> ws_off(n_reads, 0);
    uint64_t ws_bytes = 0;
    for(uint32_t i = 0; i < n_reads; ++i) {
        const uint64_t len = read_off[i + 1] - read_off[i];
        if(len > kKcLdsBases) {
            ws_off[i] = ws_bytes;
            ws_bytes += kc_workspace_bytes(len);
        }
    }
    const uint64_t total = read_off[n_reads];
    HIP_TRY(ctx->s_out.reserve(total));
    HIP_TRY(ctx->kc_ws_off.reserve(n_reads));
    HIP_TRY(ctx->kc_ws.reserve(std::max<uint64_t>(ws_bytes, 4)));
    HIP_TRY(ctx->kc_res.reserve(n_reads));
    if(phred) HIP_TRY(hipMemcpyAsync(ctx->s_in.p, phred, total, hipMemcpyHostToDevice, ctx->stream));   // the ASCII bases are done with
    HIP_TRY(hipMemcpyAsync(ctx->kc_ws_off.p, ws_off.data(), (uint64_t)n_reads * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    const KcParams kp{p->kmer_length, p->kmer_threshold, p->kmer_rounds, p->quality_cutoff};
    st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_kmer_correct(ctx->fm, ctx->s_codes.p, ctx->s_off.p, phred ? ctx->s_in.p : nullptr, n_reads, kp, ctx->kc_ws.p, ctx->kc_ws_off.p, ctx->s_out.p,
                                   reinterpret_cast<KcResult*>(ctx->kc_res.p), reinterpret_cast<uint32_t*>(ctx->s_flag.p), ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    int broken = 0;
    HIP_TRY(hipMemcpyAsync(&broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if(broken) return fail(LRSC_ERR_FORMAT, "kmer correct: an interval leaves the strand (the index is no BWT of a string set)");
    std::vector<uint8_t> codes(total);
    std::vector<lrsc_kcorrect_result> res(n_reads);
    HIP_TRY(hipMemcpyAsync(codes.data(), ctx->s_out.p, total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(res.data(), ctx->kc_res.p, (uint64_t)n_reads * sizeof(lrsc_kcorrect_result), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for(uint64_t i = 0; i < total; ++i) corrected[i] = "ACGT"[codes[i] & 3u];
    std::copy(res.begin(), res.end(), out);
    return LRSC_OK;
}
