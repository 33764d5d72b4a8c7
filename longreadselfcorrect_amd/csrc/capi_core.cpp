// capi_core.cpp -- errors, parameters, the context and its statistics, and the helpers the stages share (capi_internal.h).
#include <cmath>
#include <limits>

#include "capi_internal.h"

using namespace lrsc;

static thread_local std::string g_last_error;

int lrsc::fail(int status, const std::string& msg)
{
    g_last_error = msg;
    return status;
}
int lrsc::hip_fail(hipError_t e, const char* what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return LRSC_ERR_DEVICE;
}

extern "C" const char* lrsc_strerror(int status)
{
    switch(status) {
        case LRSC_OK: return "ok";
        case LRSC_ERR_IO: return "I/O error";
        case LRSC_ERR_FORMAT: return "BWT file is not properly formatted";
        case LRSC_ERR_ARG: return "invalid argument";
        case LRSC_ERR_NOMEM: return "out of memory";
        case LRSC_ERR_DEVICE: return "HIP device error";
        case LRSC_ERR_CAPACITY: return "output buffer too small";
        case LRSC_ERR_UNSUPPORTED: return "unsupported";
        case LRSC_ERR_LIMIT: return "internal capacity exceeded";
        default: return "unknown error";
    }
}
extern "C" const char* lrsc_last_error(void) { return g_last_error.c_str(); }
extern "C" int lrsc_abi_version(void) { return LRSC_ABI_VERSION; }

extern "C" int lrsc_params_default(int genome, int coverage, lrsc_params* out)
{
    if(!out) return fail(LRSC_ERR_ARG, "null params");
    int order;
    switch(genome) {                                  // opt::order, PacBioSelfCorrection.cpp:104
        case 5: order = 0; break;
        case 10: order = 1; break;
        case 100: order = 2; break;
        default: return fail(LRSC_ERR_ARG, "genome must be 5, 10 or 100");
    }
    static const int size[3] = {17, 19, 21};         // opt::size, :105
    std::memset(out, 0, sizeof(*out));
    out->pb_coverage = coverage;
    out->error_rate = 0.15;
    out->start_kmer_len = size[order];               // :197
    out->offset[0] = 0;
    out->offset[1] = 2 * std::min(std::max(coverage / 30 - 1, 0), order + 1);   // :198
    out->offset[2] = -2 * (order + 1);               // :199
    out->mode = 1;
    out->manual = 0;
    out->scan_kmer_len = 19;
    out->kmer_len_up_bound = 50;
    out->radius = 100;
    out->hh_ratio = 0.6f;
    out->next_target = 1;
    out->max_leaves = 32;
    out->idmer_len = 9;
    out->min_kmer_len = 13;
    out->split = 0;
    out->no_dp = 0;
    return LRSC_OK;
}

// ---------------------------------------------------------------------------------------
// tunables
// ---------------------------------------------------------------------------------------
uint64_t lrsc::env_bytes(const char* name, uint64_t dflt, unsigned shift)
{
    if(const char* e = std::getenv(name)) return std::max<uint64_t>(1, (uint64_t)std::atoll(e)) << shift;
    return dflt;
}

static uint32_t env_clamped(const char* name, uint32_t dflt, int lo, int hi)
{
    if(const char* e = std::getenv(name)) return (uint32_t)std::min(hi, std::max(lo, std::atoi(e)));
    return dflt;
}

uint32_t lrsc::resident_waves(const lrsc_ctx* ctx, uint32_t per_simd)
{
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    return (uint32_t)cus * 4u * per_simd;
}

// Every switch of the correction flow and the DP stage: name, default, clamp.  One line per switch, in the order of the rows of
// DESIGN.md section 10; called once per ABI call (the tests change the switches between calls of one process).
Tunables lrsc::read_tunables(const lrsc_ctx* ctx)
{
    const int kIntMax = std::numeric_limits<int>::max();
    Tunables t;
    t.wp_prep_bytes = env_bytes("LRSC_WP_PREP_MB", 24ull << 30, 20);                         // 24576 MB, at least 1
    t.wp_lane_bytes = env_bytes("LRSC_WP_LANE_MB", 32ull << 30, 20);                         // 32768 MB, at least 1
    t.wp_lanes = env_clamped("LRSC_WP_LANES", resident_waves(ctx, 2) * 64u, 64, kIntMax);    // 2 wavefronts per SIMD x 64, at least 64
    t.wp_gen_quorum = env_clamped("LRSC_WP_GEN_QUORUM", 50, 0, 100);                         // 50 %, 0..100
    t.wp_gen_wait = env_clamped("LRSC_WP_GEN_WAIT", 6, 0, kIntMax);                          // 6, at least 0
    t.wp_wide_cap = env_clamped("LRSC_WP_WIDE_CAP", kNarrowLeaves, 1, (int)kNarrowLeaves);   // 32, 1..32
    t.wp_wave = env_clamped("LRSC_WP_WAVE", 1, 0, 2);                                        // 1, 0..2
    t.wp_deal = env_clamped("LRSC_WP_DEAL", (int)kDealLevelDefault, 0, (int)kDealLevelTerm);   // 1, 0..3
    { const char* e = std::getenv("LRSC_WP_BEGIN_SORT"); t.wp_begin_sort = e && e[0] != '0'; } // off; on unless the value starts with 0
    t.dp_chunk_bytes = env_bytes("LRSC_DP_CHUNK_MB", 16ull << 30, 20);                       // 16384 MB, at least 1
    t.dp_align_waves = env_clamped("LRSC_DP_ALIGN_WAVES", 0, 0, kIntMax);                    // 0 = sized as usual, at least 0
    t.msa_force_global = std::getenv("LRSC_MSA_FORCE_GLOBAL") != nullptr;                    // off; on when set
    t.msa_lds_max = env_clamped("LRSC_MSA_LDS_MAX", 0, 1, kIntMax);                          // not set = the computed budget; bytes, at least 1
    { const char* e = std::getenv("LRSC_MSA_BATCH"); t.msa_batch = !(e && e[0] == '0'); }    // on; off when the value starts with 0
    t.msa_waves = env_clamped("LRSC_MSA_WAVES", 0, 1, 8);                                    // not set = by launch (msa_buckets); 1, 2, 4, 8 (3 -> 2, 5..7 -> 4)
    t.msa_waves = t.msa_waves >= 8 ? 8 : t.msa_waves >= 4 ? 4 : t.msa_waves;
    if(t.msa_waves == 3) t.msa_waves = 2;
    t.profile = std::getenv("LRSC_CORRECT_PROFILE") != nullptr;                              // off; on when set
    t.wp_dump = std::getenv("LRSC_WP_DUMP") != nullptr;                                      // off; on when set (with LRSC_CORRECT_PROFILE)
    t.dp_debug = std::getenv("LRSC_DP_DEBUG") != nullptr;                                    // off; on when set
    return t;
}

// ---------------------------------------------------------------------------------------
// shared checks and encoders
// ---------------------------------------------------------------------------------------
int lrsc::check_offsets(const uint64_t* off, uint32_t n_reads)
{
    if(!off) return fail(LRSC_ERR_ARG, "null read offsets");
    if(off[0] != 0) return fail(LRSC_ERR_ARG, "read_off[0] must be 0");
    for(uint32_t i = 0; i < n_reads; ++i)
        if(off[i + 1] < off[i]) return fail(LRSC_ERR_ARG, "read offsets must be non-decreasing");
    return LRSC_OK;
}

static const char* const kMaxLeavesMsg = "max_leaves must be 1..256";        // 256 = kWideMaxLeaves
static_assert(kWideMaxLeaves == 256, "kMaxLeavesMsg names the cap");

int lrsc::check_walk_params(const lrsc_params& p)
{
    if(p.max_leaves < 1 || p.max_leaves > (int)kWideMaxLeaves) return fail(LRSC_ERR_UNSUPPORTED, kMaxLeavesMsg);
    if(p.idmer_len < 5 || p.idmer_len > 16) return fail(LRSC_ERR_UNSUPPORTED, "idmer_len must be 5..16");
    if(p.min_kmer_len < p.idmer_len || p.min_kmer_len > 62) return fail(LRSC_ERR_UNSUPPORTED, "min_kmer_len out of range");
    return LRSC_OK;
}

void lrsc::kmer_freq_table(const lrsc_params& p, double freqs[101])
{
    for(int i = 0; i <= 100; ++i) freqs[i] = 0;
    for(int i = p.min_kmer_len; i <= 100; i++) freqs[i] = pow(1 - p.error_rate, i) * (size_t)p.pb_coverage;
}

int lrsc::encode_acgt(const char* seq, uint64_t n, uint8_t* codes)
{
    for(uint64_t i = 0; i < n; ++i) {
        switch(seq[i]) {
            case 'A': codes[i] = 0; break; case 'C': codes[i] = 1; break; case 'G': codes[i] = 2; break; case 'T': codes[i] = 3; break;
            default: return fail(LRSC_ERR_ARG, "sequence contains a base other than A,C,G,T");
        }
    }
    return LRSC_OK;
}

int lrsc::upload_and_encode(lrsc_ctx* ctx, const char* ascii, uint64_t n, uint8_t* d_codes)
{
    HIP_TRY(ctx->s_in.reserve(n));
    HIP_TRY(ctx->s_flag.reserve(1));
    HIP_TRY(hipMemsetAsync(ctx->s_flag.p, 0, sizeof(int), ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->s_in.p, ascii, n, hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = launch_encode(reinterpret_cast<const char*>(ctx->s_in.p), d_codes, n, ctx->s_flag.p, ctx->stream);
    if(e != hipSuccess) return hip_fail(e, "encode");
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, ctx->s_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // SeqReader exits on a non-ACGT base (Util/SeqReader.cpp:115-126); the library reports it
    if(bad) return fail(LRSC_ERR_ARG, "sequence contains a base other than A,C,G,T");
    return LRSC_OK;
}

int lrsc::stage_reads(lrsc_ctx* ctx, const char* tool, unsigned limit_log2, const char* reads, const uint64_t* read_off, uint32_t n_reads, uint64_t slack)
{
    const int st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    for(uint32_t i = 0; i < n_reads; ++i) {
        const uint64_t len = read_off[i + 1] - read_off[i];
        if(len == 0) return fail(LRSC_ERR_ARG, std::string(tool) + ": read " + std::to_string(i) + " is empty");
        if(len >> limit_log2) return fail(LRSC_ERR_UNSUPPORTED, std::string(tool) + ": a read of 2^" + std::to_string(limit_log2) + " bases or more");
    }
    const uint64_t total = read_off[n_reads];
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->s_codes.reserve(total + slack));
    HIP_TRY(ctx->s_off.reserve((uint64_t)n_reads + 1));
    const int enc = upload_and_encode(ctx, reads, total, ctx->s_codes.p);    // reserves s_flag; the stream is idle after it
    if(enc != LRSC_OK) return enc;
    HIP_TRY(hipMemcpyAsync(ctx->s_off.p, read_off, ((uint64_t)n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->s_flag.p, 0, sizeof(int), ctx->stream));
    return LRSC_OK;
}

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
extern "C" int lrsc_ctx_create(const lrsc_index* idx, const lrsc_params* params, int device, lrsc_ctx** out)
{
    if(!idx || !out) return fail(LRSC_ERR_ARG, "null");
    lrsc_index* midx = const_cast<lrsc_index*>(idx);
    FmIndexDev fm;
    {
        std::lock_guard<std::mutex> lock(midx->mu);
        auto it = midx->copies.find(device);
        if(it == midx->copies.end()) return fail(LRSC_ERR_DEVICE, "index not uploaded to this device (call lrsc_index_upload)");
        fm = it->second.dev;
    }
    HIP_TRY(hipSetDevice(device));
    lrsc_ctx* ctx = new(std::nothrow) lrsc_ctx();
    if(!ctx) return fail(LRSC_ERR_NOMEM, "lrsc_ctx");
    ctx->index = idx;
    ctx->device = device;
    ctx->fm = fm;
    if(params) ctx->params = *params;
    else (void)lrsc_params_default(10, 90, &ctx->params);
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if(e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if(e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if(e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&ctx->d_ctr), kCtrShards * sizeof(DevCounters));
    if(e == hipSuccess) e = hipMemset(ctx->d_ctr, 0, kCtrShards * sizeof(DevCounters));
    if(e != hipSuccess) { lrsc_ctx_destroy(ctx); return hip_fail(e, "lrsc_ctx_create"); }
    *out = ctx;
    return LRSC_OK;
}

extern "C" void lrsc_ctx_destroy(lrsc_ctx* ctx) { delete ctx; }     // ~lrsc_ctx is in capi_correct.cpp, beside the scratch it frees

extern "C" int lrsc_ctx_get_params(const lrsc_ctx* ctx, lrsc_params* out)
{
    if(!ctx || !out) return fail(LRSC_ERR_ARG, "null");
    *out = ctx->params;
    return LRSC_OK;
}

extern "C" int lrsc_ctx_sync(lrsc_ctx* ctx)
{
    if(!ctx) return fail(LRSC_ERR_ARG, "null ctx");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LRSC_OK;
}

extern "C" int lrsc_ctx_stats(lrsc_ctx* ctx, int kernel, lrsc_kernel_stats* out)
{
    if(!ctx || !out || kernel < 0 || kernel >= LRSC_K_COUNT) return fail(LRSC_ERR_ARG, "bad stats query");
    *out = ctx->stats[kernel];
    return LRSC_OK;
}
extern "C" int lrsc_ctx_stats_reset(lrsc_ctx* ctx)
{
    if(!ctx) return fail(LRSC_ERR_ARG, "null ctx");
    for(auto& s : ctx->stats) s = lrsc_kernel_stats{};
    return LRSC_OK;
}
