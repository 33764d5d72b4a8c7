// fm_locate.hip -- the locate tables of a resident strand and the locate query.  The arithmetic is fm_locate.h's.
//
//   1. locate_prepare_kernel<WIDE>   one lane per read: the backward walk from the read's sentinel row to its '$' row; samples of
//                                    the visited rows that are multiples of the rate, order[] and read_len[].  A step is one
//                                    64-byte load and popcounts against the layout's mask table in LDS.  The chain is
//                                    latency-bound: the kernel is held to the registers of kLocateWavesPerSimd wavefronts per SIMD.
//                                    One very long read is one lane's chain: the launch lasts as long as its longest read.
//   2. locate_fixup_kernel           streaming, one lane per sample: steps from the sentinel row -> position in the read
//   3. locate_kernel<WIDE>           one lane per queried row: calcSA.  Sized as the prepare walk.
// No atomics on the tables: every row is visited by one walk.  A lane whose walk is cut short stores 1 to *broken.
#include "fm_launch.h"
#include "fm_locate.h"

namespace lrsc {

static_assert(sizeof(SaElem) == sizeof(lrsc_sa_elem) && offsetof(SaElem, pos) == offsetof(lrsc_sa_elem, pos), "SaElem is lrsc_sa_elem");

template <bool WIDE>
__global__ __launch_bounds__(kLocateThreads) __attribute__((amdgpu_waves_per_eu(kLocateWavesPerSimd, kLocateWavesPerSimd)))
void locate_prepare_kernel(StrandView<typename BlockOf<WIDE>::type> S, uint32_t rate, SaElem* __restrict__ samples, uint32_t* __restrict__ order,
                           uint32_t* __restrict__ read_len, uint32_t* __restrict__ broken)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    fill_mask_table<B>(mtab);
    __syncthreads();
    const uint64_t read = (uint64_t)blockIdx.x * kLocateThreads + threadIdx.x;
    if(read >= S.n_dollars) return;
    if(locate_prepare_read<B>(S, mtab, (uint32_t)read, rate, samples, order, read_len) != kWalkOk) *broken = 1u;
}

__global__ __launch_bounds__(256) void locate_fixup_kernel(SaElem* __restrict__ samples, uint64_t n_samples, uint32_t rate, uint64_t n_symbols,
                                                           const uint32_t* __restrict__ read_len, uint64_t n_reads, uint32_t* __restrict__ broken)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if(s >= n_samples) return;
    SaElem e = samples[s];
    if(locate_fix_sample(e, s, rate, n_symbols, read_len, n_reads) != kWalkOk) { *broken = 1u; return; }
    samples[s] = e;
}

template <bool WIDE>
__global__ __launch_bounds__(kLocateThreads) __attribute__((amdgpu_waves_per_eu(kLocateWavesPerSimd, kLocateWavesPerSimd)))
void locate_kernel(StrandView<typename BlockOf<WIDE>::type> S, uint32_t rate, const SaElem* __restrict__ samples, const uint32_t* __restrict__ order,
                   const uint64_t* __restrict__ rows, uint64_t n, SaElem* __restrict__ out, uint32_t* __restrict__ broken, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    fill_mask_table<B>(mtab);
    __syncthreads();
    const uint64_t q = (uint64_t)blockIdx.x * kLocateThreads + threadIdx.x;
    uint32_t steps = 0;
    if(q < n) {
        SaElem e;
        if(locate_row<B>(S, mtab, rows[q], rate, samples, order, e, steps) != kWalkOk) *broken = 1u;
        out[q] = e;
    }
    // an LF step is one Occ query and one block load (every lane of the wavefront is here)
    const unsigned long long total = wave_sum(steps);
    wave_count(ctr, total, total);
}

constexpr int kOomStatus = LRSC_ERR_NOMEM;                       // what DEV_TRY answers when device memory runs out

void locate_free_device(LocateTables& t)
{
    if(t.samples) (void)hipFree(t.samples);
    if(t.order) (void)hipFree(t.order);
    if(t.read_len) (void)hipFree(t.read_len);
    t = LocateTables{};
}

template <bool WIDE>
static int locate_prepare_t(const FmStrand& s, uint32_t rate, LocateTables& out, std::string& err)
{
    using B = typename BlockOf<WIDE>::type;
    hipStream_t st = nullptr;
    Owned d;                                                      // the tables too, until the walks are known to cover the strand
    LocateTables t;
    uint32_t* d_broken = nullptr;
    const uint64_t n_reads = s.n_dollars, N = s.n_symbols;
    if(s.n_blocks != N / B::kSyms + 1) { err = "locate: block count does not fit the symbol count"; return LRSC_ERR_FORMAT; }
    if(n_reads == 0 || n_reads > N || n_reads >= (1ull << 32)) { err = "locate: an index without reads, or with 2^32 or more"; return LRSC_ERR_UNSUPPORTED; }
    const uint64_t groups = (n_reads + kLocateThreads - 1) / kLocateThreads;
    t.rate = rate;
    t.n_samples = locate_sample_count(N, rate);
    const uint64_t fix_groups = (t.n_samples + 255) / 256;
    if(groups >= (1ull << 31) || fix_groups >= (1ull << 31)) { err = "locate: more than 2^31 workgroups"; return LRSC_ERR_UNSUPPORTED; }
    DEV_TRY(d.alloc(&d_broken, 1));
    DEV_TRY(d.alloc(&t.order, n_reads));
    DEV_TRY(d.alloc(&t.read_len, n_reads));
    if(t.n_samples) DEV_TRY(d.alloc(&t.samples, t.n_samples));
    DEV_TRY(hipMemsetAsync(d_broken, 0, sizeof(uint32_t), st));
    DEV_TRY(hipMemsetAsync(t.order, 0xFF, n_reads * sizeof(uint32_t), st));
    DEV_TRY(hipMemsetAsync(t.read_len, 0xFF, n_reads * sizeof(uint32_t), st));
    if(t.n_samples) DEV_TRY(hipMemsetAsync(t.samples, 0xFF, t.n_samples * sizeof(SaElem), st));
    const StrandView<B> S = strand_view<B>(s);
    hipLaunchKernelGGL((locate_prepare_kernel<WIDE>), dim3((unsigned)groups), dim3(kLocateThreads), 0, st, S, rate, t.samples, t.order, t.read_len, d_broken);
    DEV_TRY(hipGetLastError());
    if(t.n_samples) {
        hipLaunchKernelGGL(locate_fixup_kernel, dim3((unsigned)fix_groups), dim3(256), 0, st, t.samples, t.n_samples, rate, N, t.read_len, n_reads,
                           d_broken);
        DEV_TRY(hipGetLastError());
    }
    uint32_t broken = 0;
    DEV_TRY(hipMemcpy(&broken, d_broken, sizeof(uint32_t), hipMemcpyDeviceToHost));
    // the walks of all reads cover the strand: their lengths and sentinels add up to its rows, and every '$' row has its read
    std::vector<uint32_t> len(n_reads), order(n_reads);
    DEV_TRY(hipMemcpy(len.data(), t.read_len, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    DEV_TRY(hipMemcpy(order.data(), t.order, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t total = n_reads;
    bool whole = broken == 0;
    for(uint64_t i = 0; i < n_reads && whole; ++i) {
        whole = len[i] != kLocateUnset && order[i] != kLocateUnset;
        total += len[i];
    }
    if(!whole || total != N) {
        err = "locate: the index is no BWT of a string set (a backward walk from a sentinel row does not end at a '$' row, or the walks do not cover it)";
        return LRSC_ERR_FORMAT;
    }
    d.keep(t.order); d.keep(t.read_len); d.keep(t.samples);
    out = t;
    return LRSC_OK;
}

int locate_prepare_device(const FmStrand& s, bool wide, uint32_t rate, LocateTables& out, std::string& err)
{
    out = LocateTables{};
    return wide ? locate_prepare_t<true>(s, rate, out, err) : locate_prepare_t<false>(s, rate, out, err);
}

hipError_t launch_locate(const FmStrand& s, bool wide, const LocateTables& t, const uint64_t* rows, uint64_t n, SaElem* out, uint32_t* broken,
                         DevCounters* ctr, hipStream_t stream)
{
    const uint64_t groups = (n + kLocateThreads - 1) / kLocateThreads;
    if(groups >= (1ull << 31)) return hipErrorInvalidValue;
    if(wide)
        hipLaunchKernelGGL((locate_kernel<true>), dim3((unsigned)groups), dim3(kLocateThreads), 0, stream, strand_view<Block64>(s), t.rate, t.samples, t.order,
                           rows, n, out, broken, ctr);
    else
        hipLaunchKernelGGL((locate_kernel<false>), dim3((unsigned)groups), dim3(kLocateThreads), 0, stream, strand_view<Block32>(s), t.rate, t.samples, t.order,
                           rows, n, out, broken, ctr);
    return hipGetLastError();
}

} // namespace lrsc
