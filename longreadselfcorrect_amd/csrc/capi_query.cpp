// capi_query.cpp -- point queries on a context: rank, BWT characters, LF walks, locate, k-mer look-ups and the k-mer grid of a read set.
#include "capi_internal.h"

using namespace lrsc;

extern "C" int lrsc_rank(lrsc_ctx* ctx, const lrsc_rank_query* q, uint64_t n, uint64_t* out)
{
    if(!ctx || (!q && n) || (!out && n)) return fail(LRSC_ERR_ARG, "null");
    if(n == 0) return LRSC_OK;
    const uint64_t N = ctx->index->num_symbols;
    for(uint64_t i = 0; i < n; ++i) {
        const uint8_t b = q[i].base;
        if(q[i].idx < -1 || q[i].idx >= (int64_t)N || (b != 'A' && b != 'C' && b != 'G' && b != 'T') || q[i].strand > 1)
            return fail(LRSC_ERR_ARG, "rank query out of range");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->s_in.reserve(n * sizeof(lrsc_rank_query)));
    HIP_TRY(ctx->s_out.reserve(n * sizeof(uint64_t)));
    HIP_TRY(hipMemcpyAsync(ctx->s_in.p, q, n * sizeof(lrsc_rank_query), hipMemcpyHostToDevice, ctx->stream));
    const int st = timed_launch(ctx, LRSC_K_RANK, [&]() {
        return launch_rank(ctx->fm, reinterpret_cast<const lrsc_rank_query*>(ctx->s_in.p), n,
                           reinterpret_cast<uint64_t*>(ctx->s_out.p), ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    HIP_TRY(hipMemcpy(out, ctx->s_out.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return LRSC_OK;
}

extern "C" int lrsc_bwt_chars(lrsc_ctx* ctx, int strand, const uint64_t* idx, uint64_t n, char* out)
{
    if(!ctx || (!idx && n) || (!out && n) || strand < 0 || strand > 1) return fail(LRSC_ERR_ARG, "null");
    if(n == 0) return LRSC_OK;
    const uint64_t N = ctx->index->num_symbols;
    for(uint64_t i = 0; i < n; ++i)
        if(idx[i] >= N) return fail(LRSC_ERR_ARG, "BWT position out of range");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->s_in.reserve(n * sizeof(uint64_t)));
    HIP_TRY(ctx->s_out.reserve(n));
    HIP_TRY(hipMemcpyAsync(ctx->s_in.p, idx, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = launch_bwt_chars(ctx->fm, strand, reinterpret_cast<const uint64_t*>(ctx->s_in.p), n,
                                    reinterpret_cast<char*>(ctx->s_out.p), ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "bwt_chars");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(out, ctx->s_out.p, n, hipMemcpyDeviceToHost));
    return LRSC_OK;
}

extern "C" int lrsc_lf_walk(lrsc_ctx* ctx, const uint64_t* rows, const uint8_t* strand, const uint32_t* max_steps,
                            const uint64_t* out_off, uint64_t n, char* out, uint64_t out_cap, uint32_t* out_len)
{
    if(!ctx || ((!rows || !strand || !max_steps || !out_off || !out || !out_len) && n)) return fail(LRSC_ERR_ARG, "null");
    if(n == 0) return LRSC_OK;
    const uint64_t N = ctx->index->num_symbols;
    std::vector<LfJob> jobs(n);
    uint64_t need = 0;
    for(uint64_t i = 0; i < n; ++i) {
        if(rows[i] >= N || strand[i] > 1) return fail(LRSC_ERR_ARG, "LF job out of range");
        jobs[i].row = rows[i]; jobs[i].out_off = out_off[i]; jobs[i].max_steps = max_steps[i]; jobs[i].strand = strand[i];
        need = std::max(need, out_off[i] + max_steps[i]);
    }
    if(need > out_cap) return fail(LRSC_ERR_CAPACITY, "LF output buffer too small");
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<LfJob> d_jobs;
    DevBuf<uint8_t> d_out;
    DevBuf<uint32_t> d_len;
    HIP_TRY(d_jobs.reserve(n));
    HIP_TRY(d_out.reserve(std::max<uint64_t>(need, 1)));
    HIP_TRY(d_len.reserve(n));
    HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(LfJob), hipMemcpyHostToDevice, ctx->stream));
    const int st = timed_launch(ctx, LRSC_K_LF, [&]() { return launch_lf_walk(ctx->fm, d_jobs.p, n, d_out.p, d_len.p, ctx->d_ctr, ctx->stream); });
    if(st != LRSC_OK) return st;
    HIP_TRY(hipMemcpy(out_len, d_len.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint8_t> codes(need);
    HIP_TRY(hipMemcpy(codes.data(), d_out.p, need, hipMemcpyDeviceToHost));
    for(uint64_t i = 0; i < n; ++i)
        for(uint32_t t = 0; t < out_len[i]; ++t) out[out_off[i] + t] = "ACGT"[codes[out_off[i] + t] & 3];
    return LRSC_OK;
}

extern "C" int lrsc_locate(lrsc_ctx* ctx, int strand, const uint64_t* rows, uint64_t n, lrsc_sa_elem* out)
{
    if(!ctx || (!rows && n) || (!out && n)) return fail(LRSC_ERR_ARG, "null");
    if(strand != LRSC_BWT && strand != LRSC_RBWT) return fail(LRSC_ERR_ARG, "strand must be LRSC_BWT or LRSC_RBWT");
    const uint64_t N = ctx->index->num_symbols;
    for(uint64_t i = 0; i < n; ++i)
        if(rows[i] >= N) return fail(LRSC_ERR_ARG, "BWT row out of range");
    // the tables of the ctx's device, under the index's mutex: lrsc_index_locate_prepare may be filling another copy's
    std::lock_guard<std::mutex> lock(ctx->index->mu);
    auto it = ctx->index->copies.find(ctx->device);
    if(it == ctx->index->copies.end() || !it->second.located)
        return fail(LRSC_ERR_DEVICE, "no locate tables on this device (call lrsc_index_locate_prepare)");
    if(n == 0) return LRSC_OK;
    const LocateTables& t = it->second.locate[strand];
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->s_in.reserve(n * sizeof(uint64_t)));
    HIP_TRY(ctx->s_out.reserve(n * sizeof(lrsc_sa_elem)));
    HIP_TRY(ctx->s_flag.reserve(1));
    HIP_TRY(hipMemcpyAsync(ctx->s_in.p, rows, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->s_flag.p, 0, sizeof(int), ctx->stream));
    const int st = timed_launch(ctx, LRSC_K_LOCATE, [&]() {
        return launch_locate(ctx->fm.strand[strand], ctx->fm.wide != 0, t, reinterpret_cast<const uint64_t*>(ctx->s_in.p), n,
                             reinterpret_cast<SaElem*>(ctx->s_out.p), reinterpret_cast<uint32_t*>(ctx->s_flag.p), ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    int broken = 0;
    HIP_TRY(hipMemcpy(&broken, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost));
    if(broken) return fail(LRSC_ERR_FORMAT, "locate: a backward walk does not end (the index is no BWT of a string set)");
    HIP_TRY(hipMemcpy(out, ctx->s_out.p, n * sizeof(lrsc_sa_elem), hipMemcpyDeviceToHost));
    return LRSC_OK;
}

extern "C" int lrsc_find_kmers(lrsc_ctx* ctx, const char* kmers, uint32_t k, uint64_t n, lrsc_biinterval* out)
{
    if(!ctx || (!kmers && n) || (!out && n) || k == 0) return fail(LRSC_ERR_ARG, "null / k == 0");
    if(n == 0) return LRSC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->s_codes.reserve(n * k));
    HIP_TRY(ctx->s_out.reserve(n * sizeof(lrsc_biinterval)));
    int st = upload_and_encode(ctx, kmers, n * k, ctx->s_codes.p);
    if(st != LRSC_OK) return st;
    st = timed_launch(ctx, LRSC_K_FIND, [&]() {
        return launch_find_kmers(ctx->fm, ctx->s_codes.p, k, n, reinterpret_cast<lrsc_biinterval*>(ctx->s_out.p),
                                 ctx->d_ctr, ctx->stream);
    });
    if(st != LRSC_OK) return st;
    HIP_TRY(hipMemcpy(out, ctx->s_out.p, n * sizeof(lrsc_biinterval), hipMemcpyDeviceToHost));
    return LRSC_OK;
}

static int check_pool(const uint8_t* ks, uint32_t n_k)
{
    if(!ks || n_k == 0 || n_k > kMaxPool) return fail(LRSC_ERR_ARG, "pool must hold 1..8 k-mer sizes");
    for(uint32_t i = 0; i < n_k; ++i) {
        if(ks[i] == 0 || (i && ks[i] <= ks[i - 1])) return fail(LRSC_ERR_ARG, "pool sizes must be ascending and > 0");
    }
    return LRSC_OK;
}

extern "C" int lrsc_kmer_grid(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads,
                              const uint8_t* ks, uint32_t n_k, lrsc_biinterval* out_iv, uint8_t* out_size,
                              uint8_t* out_count)
{
    if(!ctx) return fail(LRSC_ERR_ARG, "null ctx");
    int st = check_pool(ks, n_k);
    if(st != LRSC_OK) return st;
    if(n_reads == 0) return LRSC_OK;
    st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    const uint64_t total = read_off[n_reads];
    if(total == 0) return LRSC_OK;
    if(!reads) return fail(LRSC_ERR_ARG, "null reads");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->s_codes.reserve(total));
    HIP_TRY(ctx->s_off.reserve(n_reads + 1));
    const uint64_t n_chunks = (total + (1ull << kChunkShift) - 1) >> kChunkShift;
    HIP_TRY(ctx->s_chunk.reserve(n_chunks));
    st = upload_and_encode(ctx, reads, total, ctx->s_codes.p);
    if(st != LRSC_OK) return st;
    HIP_TRY(hipMemcpyAsync(ctx->s_off.p, read_off, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = launch_chunk_table(ctx->s_off.p, n_reads, total, ctx->s_chunk.p, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "chunk_table");

    const uint64_t recs = total * n_k;
    DevBuf<lrsc_biinterval> d_iv;
    DevBuf<uint8_t> d_size, d_count;
    if(out_iv) HIP_TRY(d_iv.reserve(recs));
    if(out_size) HIP_TRY(d_size.reserve(recs));
    if(out_count) HIP_TRY(d_count.reserve(recs * 4));

    GridArgs a{};
    a.codes = ctx->s_codes.p;
    a.read_off = ctx->s_off.p;
    a.chunk_read = ctx->s_chunk.p;
    a.total_bases = total;
    a.n_reads = n_reads;
    a.n_k = n_k;
    for(uint32_t i = 0; i < n_k; ++i) a.ks[i] = ks[i];
    a.out_iv = d_iv.p;
    a.out_size = d_size.p;
    a.out_count = d_count.p;
    st = timed_launch(ctx, LRSC_K_GRID, [&]() { return launch_kmer_grid(ctx->fm, a, ctx->d_ctr, ctx->stream); });
    if(st != LRSC_OK) return st;
    if(out_iv) HIP_TRY(hipMemcpy(out_iv, d_iv.p, recs * sizeof(lrsc_biinterval), hipMemcpyDeviceToHost));
    if(out_size) HIP_TRY(hipMemcpy(out_size, d_size.p, recs, hipMemcpyDeviceToHost));
    if(out_count) HIP_TRY(hipMemcpy(out_count, d_count.p, recs * 4, hipMemcpyDeviceToHost));
    return LRSC_OK;
}
