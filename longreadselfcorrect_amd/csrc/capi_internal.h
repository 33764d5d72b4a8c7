// capi_internal.h -- what the translation units that implement include/lrsc.h (capi_*.cpp) share: the error helpers, the device
// buffer types, the three opaque ABI objects, the per-call tunables and the few helpers that more than one stage needs.
//
// There is deliberately NO CPU fallback behind the ABI: every compute entry point needs a HIP device and returns
// LRSC_ERR_DEVICE (with the HIP error text in lrsc_last_error()) when there is none.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "fm_layout.h"
#include "fm_locate.h"
#include "fm_pack.h"
#include "kernels.h"
#include "extend.h"
#include "correct_dev.h"
#include "dp_dev.h"
#include "wp.h"
#include "saipb.h"

#pragma GCC visibility push(hidden)      // private to liblrsc_hip.so: only include/lrsc.h is exported
namespace lrsc {

// errors (capi_core.cpp holds the one thread-local message behind lrsc_last_error())
int fail(int status, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
#define HIP_TRY(expr)                                              \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if(_e != hipSuccess) return hip_fail(_e, #expr);           \
    } while(0)

// device memory
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { if(p) (void)hipFree(p); }
    // hipFree / hipMalloc wait for every kernel on the device, those of another ctx included: a buffer that has to grow again grows by
    // a quarter at least, so that batches that are each a little larger than the last do not pay that wait every time.  The callers'
    // budgets bound n, not the slack: where the device cannot hold the slack the buffer gets exactly n.
    hipError_t reserve(size_t n)
    {
        if(n <= cap) return hipSuccess;
        size_t want = cap ? std::max(n, cap + cap / 4) : n;
        if(p) { (void)hipFree(p); p = nullptr; cap = 0; }
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
        if(e != hipSuccess && want > n) {
            (void)hipGetLastError();
            p = nullptr; want = n;
            e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
        }
        if(e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
};

// Bump allocator over grow-only device chunks: results that later rounds still read (queries, result paths, DP consensus)
// live here until the read range is done.  reset() keeps the chunks, so a loop over same-shaped batches stops allocating.
struct DevArena {
    std::vector<DevBuf<uint8_t>*> chunks;
    size_t cur = 0, off = 0;
    ~DevArena() { for(auto* c : chunks) delete c; }
    void reset() { cur = 0; off = 0; }
    hipError_t alloc(size_t bytes, uint8_t** out)
    {
        bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
        while(cur < chunks.size()) {
            if(chunks[cur]->cap - off >= bytes) { *out = chunks[cur]->p + off; off += bytes; return hipSuccess; }
            // an empty chunk that is too small is replaced rather than skipped (grow-only, few chunks; DevBuf::reserve adds its quarter)
            if(off == 0) { hipError_t e = chunks[cur]->reserve(bytes + bytes / 8); if(e != hipSuccess) return e; continue; }
            ++cur; off = 0;
        }
        auto* c = new(std::nothrow) DevBuf<uint8_t>();
        if(!c) return hipErrorOutOfMemory;
        hipError_t e = c->reserve(std::max<size_t>(bytes + bytes / 8, 64u << 20));
        if(e != hipSuccess) { delete c; return e; }
        chunks.push_back(c);
        cur = chunks.size() - 1;
        *out = c->p; off = bytes;
        return hipSuccess;
    }
};

// per-call tunables: every LRSC_WP_* / LRSC_DP_* / LRSC_MSA_* / LRSC_CORRECT_PROFILE switch, read once per ABI call
// (read_tunables, capi_core.cpp; the tests change them between calls of one process, so never cached)
struct Tunables {
    bool profile, wp_dump, dp_debug;
    uint32_t wp_wide_cap, wp_wave, wp_deal, wp_lanes;
    bool wp_begin_sort;
    uint64_t wp_prep_bytes, wp_lane_bytes;
    uint32_t wp_gen_quorum, wp_gen_wait;
    uint64_t dp_chunk_bytes;
    uint32_t dp_align_waves;
    bool msa_batch, msa_force_global;
    uint32_t msa_waves;                    // LRSC_MSA_WAVES: wavefronts per MSA workgroup in every launch (0 = not set: chosen per launch)
    uint32_t msa_lds_max;                  // LRSC_MSA_LDS_MAX: upper bound of the MSA launches' LDS budget per CU (0 = not set)
};

struct DeviceCopy {
    void* blocks[2] = {nullptr, nullptr};
    uint64_t* dollars[2] = {nullptr, nullptr};
    uint32_t* dollar_dir[2] = {nullptr, nullptr};
    void* ktab[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    FmIndexDev dev{};
    // the locate tables of both strands (lrsc_index_locate_prepare); located = false: none yet
    LocateTables locate[2];
    bool located = false;
};

// The DP stage for a set of requests whose queries are already on the device: seeds -> (chunked by memory)
// retrieve -> align -> MSA (capi_dp.cpp).  Results stay on the device (d_msa[i], consensus codes at d_cons + reqs[i].cons_off).
struct DpStage {
    DevBuf<DpRequest> d_reqs;
    DevBuf<DpMsaOut> d_msa;
    DevBuf<uint8_t> d_cons, d_strings, d_ops, d_trace;
    DevBuf<DpJob> d_jobs;
    DevBuf<DpAlignOut> d_align;
    DevBuf<uint32_t> d_list;
    DevBuf<uint8_t> d_msa_ws, d_seq_ws;
    DevBuf<uint32_t> d_msa_ctr;
    // the align launches' job lists (dp_order.h) and their head words, one per staging-size class: this stage's own, since two ctxs
    // run their DP stages on one device at the same time
    DevBuf<uint32_t> d_align_order, d_align_heads;
    uint64_t cons_total = 0, n_strings = 0;
    // LDS per CU the MSA launches of a run() may count on (msa_lds_budget), set by run()
    uint32_t lds_budget = 0;
    // the MSA size buckets of a round run concurrently on side streams (each bucket's launch ends with a tail of a few long
    // pile-ups; serialised, those tails cost more than the work); dp_deal.h deals the launches to the streams
    static constexpr int kSide = 3;
    hipStream_t side[kSide] = {};
    hipEvent_t side_done[kSide] = {};
    ~DpStage();

    int run(lrsc_ctx* ctx, const Tunables& tn, const uint8_t* d_query_codes, std::vector<DpRequest>& reqs);

private:
    struct Chunk;
    struct MsaLaunch;
    int size_requests(std::vector<DpRequest>& reqs);
    Chunk plan_chunk(std::vector<DpRequest>& reqs, uint32_t begin, uint64_t budget);
    int msa_lds_budget(lrsc_ctx* ctx, const Tunables& tn, uint32_t* budget) const;
    int align_chunk(lrsc_ctx* ctx, const Tunables& tn, const std::vector<DpRequest>& reqs, const Chunk& ch, uint32_t lds_waves);
    uint64_t msa_buckets(const std::vector<DpRequest>& reqs, const Chunk& ch, const std::vector<uint32_t>& todo, bool force_global,
                         uint32_t waves, std::vector<MsaLaunch>& launches, std::vector<uint32_t>& lists) const;
    int msa_chunk(lrsc_ctx* ctx, const Tunables& tn, std::vector<DpRequest>& reqs, const Chunk& ch);
};

struct CorrectScratch;                                   // device buffers lrsc_batch_correct keeps between calls (capi_correct.cpp)

} // namespace lrsc

// the opaque objects of include/lrsc.h
struct lrsc_index {
    lrsc::StrandImage image[2];     // [LRSC_BWT], [LRSC_RBWT]
    uint64_t num_strings = 0;
    uint64_t num_symbols = 0;
    bool wide = false;
    mutable std::mutex mu;          // guards copies, the locate tables of a copy included
    std::map<int, lrsc::DeviceCopy> copies;
};

struct lrsc_ctx {
    lrsc::CorrectScratch* cs = nullptr;
    const lrsc_index* index = nullptr;
    lrsc_params params{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    lrsc::FmIndexDev fm{};
    lrsc::DevCounters* d_ctr = nullptr;
    lrsc_kernel_stats stats[LRSC_K_COUNT]{};
    // reusable device scratch
    lrsc::DevBuf<uint8_t> s_in, s_codes, s_out;
    lrsc::DevBuf<uint64_t> s_off;
    lrsc::DevBuf<uint32_t> s_chunk;
    lrsc::DevBuf<int> s_flag;
    // lrsc_saipb_merge's buffers, kept between calls (grown, never shrunk)
    lrsc::DevBuf<uint8_t> sp_codes, sp_ws;
    lrsc::DevBuf<lrsc::SaipbSeed> sp_seeds, sp_live;
    lrsc::DevBuf<lrsc::SaipbSeedInfo> sp_info, sp_live_info;
    lrsc::DevBuf<lrsc::SaipbJob> sp_jobs;
    lrsc::DevBuf<lrsc::SaipbOut> sp_out;
    lrsc::DevBuf<char> sp_text;
    // lrsc_kmer_correct's: the long reads' workspace and their places in it, the results
    lrsc::DevBuf<uint8_t> kc_ws;
    lrsc::DevBuf<uint64_t> kc_ws_off;
    lrsc::DevBuf<lrsc_kcorrect_result> kc_res;
    // lrsc_fmwalk_merge's: the wavefronts' workspace, the walks' start and end strings, their strings, the trimmed lengths
    lrsc::DevBuf<uint8_t> fw_ws, fw_strs, fw_best, fw_outs;
    lrsc::DevBuf<uint32_t> fw_trimmed;
    // lrsc_fmwalk_hybrid's, lrsc_fmwalk_kmerize's and lrsc_kmer_sample_counts': the splits' workspace, jobs, pieces and results, the
    // pairs' gates, the samples' rows and counts
    lrsc::DevBuf<uint8_t> km_ws, km_jobs, km_pieces, km_outs, km_gates, km_rows, km_counts;
    // lrsc_overlap_exact's: the wavefronts' workspace, the chains' heads and blocks, the reads' results, the pool of final blocks
    // behind its 8-byte counter
    lrsc::DevBuf<uint8_t> ov_ws, ov_heads, ov_chain, ov_outs, ov_pool;
    // lrsc_fmmerge's: the links, the two node buffers, the words and the 64-bit words of the state, the records, the bases
    lrsc::DevBuf<uint8_t> fm_links, fm_nodes, fm_words, fm_longs, fm_recs, fm_bases;
    ~lrsc_ctx();                                        // drains the stream, then frees cs and the ctx's own objects (capi_correct.cpp)
};

struct lrsc_batch {
    lrsc_ctx* ctx = nullptr;
    uint32_t n_reads = 0;
    uint64_t total_bases = 0;
    uint8_t* d_codes = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t* d_chunk = nullptr;
    // compact grid features (resident)
    uint32_t n_k = 0;
    uint8_t ks[lrsc::kMaxPool]{};
    int8_t freq_index[lrsc::kMaxPool]{};
    int8_t row_of_k[64]{};
    uint32_t n_rows = 0;
    int32_t* d_freq = nullptr;
    uint8_t* d_base_counted = nullptr;
    uint8_t* d_valid = nullptr;
    bool grid_done = false;
    // seed finding
    uint32_t min_k = 1;
    uint64_t seed_cap = 0;
    unsigned long long* d_flags = nullptr;
    uint32_t* d_zeros = nullptr;
    uint8_t* d_attr = nullptr;
    unsigned long long* d_start_bits = nullptr;
    int32_t* d_seeds = nullptr;
    uint32_t* d_seed_count = nullptr;
    float* d_thr = nullptr;
    void* d_scan_tmp = nullptr;
    size_t scan_tmp_cap = 0;
    bool seeds_done = false;
    // --debugseed collection (lrsc_batch_set_debug)
    int debug_flags = 0;
    int32_t* d_outcasts = nullptr;
    uint32_t* d_outcast_count = nullptr;
    uint8_t* d_walk_log = nullptr;
    float* d_ratio = nullptr;
    bool walk_log_done = false;
};

namespace lrsc {

// helpers shared by the stages (capi_core.cpp)
Tunables read_tunables(const lrsc_ctx* ctx);
// max(1, value of the variable) << shift, or dflt when it is not set
uint64_t env_bytes(const char* name, uint64_t dflt, unsigned shift);
// wavefronts the device holds at `per_simd` per SIMD (4 SIMDs per CU)
uint32_t resident_waves(const lrsc_ctx* ctx, uint32_t per_simd);
// wavefronts of the long-gap walks' side launch: it shares the device with the launches on the ctx's stream and takes half of the
// extension kernels' resident wavefronts (WpFlow::extend_range); the MSA launches leave its LDS free (DpStage::msa_lds_budget)
inline uint64_t wp_side_waves(const Tunables& tn) { return std::max<uint64_t>(1, tn.wp_lanes / 64 / 2); }
int check_offsets(const uint64_t* off, uint32_t n_reads);
// the walk's -l / idmer / minimum k-mer limits (lrsc_extend_walks and lrsc_batch_correct)
int check_walk_params(const lrsc_params& p);
// pow() table of the walk's constructor (LongReadCorrectByOverlap.cpp:68-70), computed with the host libm like the reference does
void kmer_freq_table(const lrsc_params& p, double freqs[101]);
// ASCII -> 2-bit codes on the host; rejects non-ACGT
int encode_acgt(const char* seq, uint64_t n, uint8_t* codes);
// upload ASCII bases, encode to 2-bit codes on the device, reject non-ACGT
int upload_and_encode(lrsc_ctx* ctx, const char* ascii, uint64_t n, uint8_t* d_codes);
// How the entries that search a strand for a batch of reads open (duplicate check, k-mer correction, fmwalk): the offsets are
// checked, every read has a base and fewer than 2^limit_log2 ("<tool>: read i is empty", "<tool>: a read of 2^K bases or more");
// then s_codes = the reads' codes with `slack` bytes behind them, s_off = their offsets, s_flag = 0, on the ctx's device.
int stage_reads(lrsc_ctx* ctx, const char* tool, unsigned limit_log2, const char* reads, const uint64_t* read_off, uint32_t n_reads, uint64_t slack);

// the exact overlap of a batch of reads chunk by chunk, for lrsc_overlap_exact and lrsc_fmmerge (capi_overlap.cpp)
struct OverlapPlan {
    uint32_t min_overlap, max_len, collect_groups, reduce_groups;
    uint64_t chunk, slice, pool_cap;                              // reads per chunk, a wavefront's workspace, blocks the pool holds
};
int overlap_check_min(int32_t min_overlap);
int overlap_plan(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap, OverlapPlan& plan);
int overlap_chunk(lrsc_ctx* ctx, const OverlapPlan& plan, uint64_t r0, uint32_t n);

// what the entries that make an index on the device share (capi_index.cpp)
void free_device_copy(DeviceCopy& dc);
// describes the image that dc holds on the current device, builds its k-mer tables and enters it as `device`'s copy; the caller
// holds idx->mu and frees dc on failure
int register_copy(lrsc_index* idx, int device, DeviceCopy& dc);
// the host image of a strand that was packed on the device
int image_from_device(const PackedStrand& ps, uint64_t N, uint64_t n_runs, StrandImage& im, std::string& err);
// Block64 (64-bit counters, 128 symbols per block) from 2^31 symbols per strand; LRSC_FORCE_WIDE=1 selects it for any index so
// that the wide code path can be tested on small data
bool index_is_wide(uint64_t num_symbols);
// One strand of an index that is made on the device: ps, packed there from N symbols (n_runs RL units, 0 when it never had any),
// becomes strand s of dc, and im its host image, a copy of the packed arrays (a third of a byte per symbol).
int adopt_packed(const PackedStrand& ps, uint64_t N, uint64_t n_runs, int s, DeviceCopy& dc, StrandImage& im, std::string& err);
// The same from the byte-per-symbol BWT d_bwt, which is packed first and released either way; pack_ms += the pack.
int adopt_packed(uint8_t* d_bwt, uint64_t N, bool wide, int s, DeviceCopy& dc, StrandImage& im, double& pack_ms, std::string& err);
// How such an entry ends, st being what its strands left.  Both strands must hold n_dollars '$' rows, else bad_status with
// bad_msg (nullptr: not checked).  Then dc becomes idx's copy on `device`, ms[tables_slot] = that, and with LRSC_BWT_PROFILE set
// profile_fmt is printed with ms[0..3].  On any failure dc and idx are released.
int finish_index(lrsc_index* idx, int device, DeviceCopy& dc, int st, uint64_t n_dollars, int bad_status, const char* bad_msg, double ms[4],
                 int tables_slot, const char* profile_fmt);
// the strands of idx's copy on `device` (LRSC_ERR_DEVICE without one)
int resident_strands(lrsc_index* idx, int device, FmStrand fs[2], bool& wide);

// A blocking copy on the ctx's own stream.  A plain hipMemcpy goes through the null stream, whose hardware queue also carries streams
// of other contexts when the process has few queues: the copy would wait for their kernels.  Whatever the copy reads was written on
// ctx->stream, or on a side stream whose end the host has already waited for.
inline int copy_sync(lrsc_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    if(bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LRSC_OK;
}
#define COPY_TRY(ctx, dst, src, bytes, kind)                                   \
    do {                                                                       \
        const int _st = lrsc::copy_sync((ctx), (dst), (src), (bytes), (kind)); \
        if(_st != LRSC_OK) return _st;                                         \
    } while(0)

// Bracket one kernel launch with HIP events on the ctx stream and fold the device counters
// into the per-kernel stats.  `launch` enqueues on ctx->stream.
template <class F>
int timed_launch(lrsc_ctx* ctx, int which, F&& launch)
{
    HIP_TRY(hipMemsetAsync(ctx->d_ctr, 0, kCtrShards * sizeof(DevCounters), ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    hipError_t e = launch();
    if(e != hipSuccess) return hip_fail(e, "kernel launch");
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    std::vector<DevCounters> shards(kCtrShards);
    COPY_TRY(ctx, shards.data(), ctx->d_ctr, kCtrShards * sizeof(DevCounters), hipMemcpyDeviceToHost);
    DevCounters h{};
    for(const DevCounters& d : shards) { h.rank_queries += d.rank_queries; h.block_loads += d.block_loads; h.table_loads += d.table_loads; }
    lrsc_kernel_stats& s = ctx->stats[which];
    s.launches += 1;
    s.total_ms += ms;
    s.rank_queries += h.rank_queries;
    s.block_loads += h.block_loads;
    s.table_loads += h.table_loads;
    return LRSC_OK;
}

} // namespace lrsc
#pragma GCC visibility pop
