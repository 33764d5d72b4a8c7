// capi_filter.cpp -- what `stride filter` needs of the library: the duplicate check of a batch of reads against a context's
// index (fm_dup.hip) and the index without some of its reads (fm_remove.hip).
#include "capi_internal.h"
#include "fm_dup.h"
#include "fm_remove.h"

using namespace lrsc;

// the bit vector of a filter run and the per-call claims, on the ctx's device
struct lrsc_dupcheck {
    lrsc_ctx* ctx = nullptr;
    uint64_t n_slots = 0;                  // num_strings
    DevBuf<uint32_t> bits;                 // n_slots bits
    DevBuf<uint32_t> winner;               // n_slots words, kDupNoWinner between calls
    DevBuf<DupChainOut> chains;
    DevBuf<DupResult> results;
    DevBuf<uint64_t> slots;
};

extern "C" int lrsc_dupcheck_create(lrsc_ctx* ctx, lrsc_dupcheck** out)
{
    if(!ctx || !out) return fail(LRSC_ERR_ARG, "null");
    const uint64_t n = ctx->index->num_strings;
    if(n == 0 || n >= (1ull << 32)) return fail(LRSC_ERR_UNSUPPORTED, "duplicate check: an index without reads, or with 2^32 or more");
    HIP_TRY(hipSetDevice(ctx->device));
    lrsc_dupcheck* dc = new(std::nothrow) lrsc_dupcheck();
    if(!dc) return fail(LRSC_ERR_NOMEM, "lrsc_dupcheck");
    dc->ctx = ctx;
    dc->n_slots = n;
    const uint64_t words = (n + 31) / 32;
    hipError_t e = dc->bits.reserve(words);
    if(e == hipSuccess) e = dc->winner.reserve(n);
    if(e == hipSuccess) e = hipMemsetAsync(dc->bits.p, 0, words * sizeof(uint32_t), ctx->stream);
    if(e == hipSuccess) e = hipMemsetAsync(dc->winner.p, 0xFF, n * sizeof(uint32_t), ctx->stream);
    if(e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if(e != hipSuccess) { delete dc; return hip_fail(e, "lrsc_dupcheck_create"); }
    *out = dc;
    return LRSC_OK;
}

extern "C" void lrsc_dupcheck_destroy(lrsc_dupcheck* dc)
{
    if(!dc) return;
    (void)hipSetDevice(dc->ctx->device);
    (void)hipStreamSynchronize(dc->ctx->stream);
    delete dc;
}

extern "C" int lrsc_dupcheck_reads(lrsc_dupcheck* dc, const char* reads, const uint64_t* read_off, uint32_t n_reads, lrsc_dup_result* out)
{
    if(!dc || (n_reads && (!reads || !read_off || !out))) return fail(LRSC_ERR_ARG, "null");
    if(n_reads == 0) return LRSC_OK;
    lrsc_ctx* ctx = dc->ctx;
    // the codes are read as 32-bit words up to the one that holds the last base; a base other than A,C,G,T is rejected before
    // anything is claimed
    int st = stage_reads(ctx, "duplicate check", 32, reads, read_off, n_reads, 4);
    if(st != LRSC_OK) return st;
    HIP_TRY(dc->chains.reserve((uint64_t)n_reads * kDupKinds));
    HIP_TRY(dc->results.reserve(n_reads));
    HIP_TRY(dc->slots.reserve(n_reads));
    st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_dup_chains(ctx->fm, reinterpret_cast<const uint32_t*>(ctx->s_codes.p), ctx->s_off.p, n_reads, dc->chains.p, ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    hipError_t e = launch_dup_classify(ctx->fm, dc->chains.p, n_reads, dc->n_slots, dc->results.p, dc->slots.p, dc->winner.p, dc->bits.p,
                                       reinterpret_cast<uint32_t*>(ctx->s_flag.p), ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "duplicate check: classify");
    int broken = 0;
    HIP_TRY(hipMemcpyAsync(&broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, dc->results.p, (uint64_t)n_reads * sizeof(lrsc_dup_result), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if(broken) return fail(LRSC_ERR_FORMAT, "duplicate check: an interval leaves the strand (the index is no BWT of a string set)");
    return LRSC_OK;
}

// ---------------------------------------------------------------------------------------
// an index without some of its reads (fm_remove.hip)
// ---------------------------------------------------------------------------------------
// One strand of lrsc_index_remove: mark + compact -> BWT of the kept reads on the device -> packed image on the device (dc.*[s])
// -> host image (adopt_packed).  The first strand's walks tell the result's length and with it its
// layout; the second strand's must come to the same.  ms: walk, compact, pack.
static int remove_strand(const FmStrand& fs, bool wide_in, const std::vector<uint32_t>& ids, int s, lrsc_index* res, DeviceCopy& dc, double ms[3],
                         std::string& err)
{
    uint8_t* d_bwt = nullptr;
    uint64_t N = 0;
    int st = remove_strand_device(fs, wide_in, ids.data(), ids.size(), &d_bwt, &N, ms, err);
    if(st != LRSC_OK) return st;
    if(s == 0) {
        res->num_symbols = N;
        res->wide = index_is_wide(N);
    } else if(N != res->num_symbols) {
        (void)hipFree(d_bwt);
        err = "index remove: .bwt and .rbwt disagree on the lengths of the dropped reads";
        return LRSC_ERR_FORMAT;
    }
    return adopt_packed(d_bwt, N, res->wide, s, dc, res->image[s], ms[2], err);
}

extern "C" int lrsc_index_remove(lrsc_index* idx, const uint8_t* drop, uint64_t n_reads, int device, lrsc_index** out)
{
    if(!idx || !drop || !out) return fail(LRSC_ERR_ARG, "null");
    if(n_reads != idx->num_strings) return fail(LRSC_ERR_ARG, "index remove: drop[] has " + std::to_string(n_reads) + " entries, the index " +
                                                                  std::to_string(idx->num_strings) + " reads");
    if(n_reads >= (1ull << 32)) return fail(LRSC_ERR_UNSUPPORTED, "index remove: 2^32 reads or more");
    std::vector<uint32_t> ids;
    for(uint64_t i = 0; i < n_reads; ++i)
        if(drop[i]) ids.push_back((uint32_t)i);
    if(ids.size() == n_reads) return fail(LRSC_ERR_ARG, "index remove: nothing is kept");
    FmStrand fs[2];
    bool wide_in = false;
    int st = resident_strands(idx, device, fs, wide_in);
    if(st != LRSC_OK) return st;
    HIP_TRY(hipSetDevice(device));
    lrsc_index* res = new(std::nothrow) lrsc_index();
    if(!res) return fail(LRSC_ERR_NOMEM, "lrsc_index");
    const uint64_t n_kept = n_reads - ids.size();
    res->num_strings = n_kept;
    DeviceCopy dc;
    double ms[4] = {0., 0., 0., 0.};
    std::string err;
    for(int s = 0; s < 2 && st == LRSC_OK; ++s) {
        st = remove_strand(fs[s], wide_in, ids, s, res, dc, ms, err);
        if(st != LRSC_OK) st = fail(st, err);
    }
    st = finish_index(res, device, dc, st, n_kept, LRSC_ERR_FORMAT, "index remove: the '$' rows of the result are not those of the kept reads", ms, 3,
                      "[lrsc] index remove: walk %.3f ms, compact %.3f ms, pack %.3f ms, tables %.3f ms\n");
    if(st != LRSC_OK) return st;
    *out = res;
    return LRSC_OK;
}
