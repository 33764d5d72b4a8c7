// fm_kcorrect.hip -- the k-mer correction of a batch of reads against a resident index.  The algorithm is fm_kcorrect.h's.
//
//   kmer_correct_kernel<WIDE>   one wavefront per read, kKcThreads / 64 reads per workgroup, which share the layout's mask table
//                               in LDS.  The lanes of the wavefront take the backward searches of a pass: two per k-mer when
//                               the read is counted, sixteen per unsolid base when substitutes are tried.  A read of up to
//                               kKcLdsBases bases keeps its edited codes, flags and counts in LDS, a longer one in its slice of
//                               a global workspace, through the same functions.  A search is dependent 64-byte loads and
//                               latency-bound: the kernel is held to the registers and the LDS of kKcWavesPerSimd wavefronts per
//                               SIMD.  The wavefronts of a workgroup never wait for one another after the table is filled.
#include "fm_kcorrect.h"
#include "fm_launch.h"

namespace lrsc {

static_assert(sizeof(KcResult) == sizeof(lrsc_kcorrect_result) && offsetof(KcResult, passes) == offsetof(lrsc_kcorrect_result, passes),
              "KcResult is lrsc_kcorrect_result");
static_assert(sizeof(KcParams) == sizeof(lrsc_kcorrect_params) && offsetof(KcParams, quality_cutoff) == offsetof(lrsc_kcorrect_params, quality_cutoff),
              "KcParams is lrsc_kcorrect_params");

constexpr uint32_t kKcWaves = kKcThreads / kKcLanes;
constexpr uint32_t kKcLdsStateWords = (kKcLdsBases * kKcStateBytesPerBase + 4 * kKcLanes) / 4;
static_assert(kKcLdsBases % 4 == 0 && kKcLanes == 64 && kKcGroup == 4, "the state's layout and the lanes of an attempt step");

template <bool WIDE>
__global__ __launch_bounds__(kKcThreads) __attribute__((amdgpu_waves_per_eu(kKcWavesPerSimd, kKcWavesPerSimd)))
void kmer_correct_kernel(StrandView<typename BlockOf<WIDE>::type> S, const uint8_t* __restrict__ codes, const uint64_t* __restrict__ read_off,
                         const uint8_t* __restrict__ phred, uint32_t n, KcParams p, uint8_t* ws, const uint64_t* __restrict__ ws_off,
                         uint8_t* __restrict__ corrected, KcResult* __restrict__ results, uint32_t* __restrict__ broken, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ __attribute__((aligned(16))) uint32_t state[kKcWaves][kKcLdsStateWords];
    fill_mask_table<B>(mtab);
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kKcLanes);
    const uint64_t read = (uint64_t)blockIdx.x * kKcWaves + wave;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0;
    if(read < n) {
        const uint64_t begin = read_off[read];
        const uint32_t len = (uint32_t)(read_off[read + 1] - begin);
        uint8_t* base = len <= kKcLdsBases ? reinterpret_cast<uint8_t*>(state[wave]) : ws + ws_off[read];
        const KcState st = kc_state_at(base, len);
        WaveExec w;
        KcResult res;
        const bool ok = kc_correct_read<B>(S, mtab, codes + begin, phred != nullptr ? phred + begin : nullptr, len, p, st, w, corrected + begin, res, n_rank, n_blk);
        if((threadIdx.x & (kKcLanes - 1)) == 0) {
            if(ok) results[read] = res;
            else *broken = 1u;
        }
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

hipError_t launch_kmer_correct(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, const uint8_t* phred, uint32_t n, const KcParams& p,
                               uint8_t* ws, const uint64_t* ws_off, uint8_t* corrected, KcResult* results, uint32_t* broken, DevCounters* ctr,
                               hipStream_t stream)
{
    const uint64_t groups = ((uint64_t)n + kKcWaves - 1) / kKcWaves;
    if(n == 0 || groups >= (1ull << 31) || p.kmer_length <= 0 || p.kmer_threshold <= 0 || p.kmer_rounds <= 0) return hipErrorInvalidValue;
    if(fm.wide)
        hipLaunchKernelGGL((kmer_correct_kernel<true>), dim3((unsigned)groups), dim3(kKcThreads), 0, stream, strand_view<Block64>(fm.strand[0]), codes, read_off,
                           phred, n, p, ws, ws_off, corrected, results, broken, ctr);
    else
        hipLaunchKernelGGL((kmer_correct_kernel<false>), dim3((unsigned)groups), dim3(kKcThreads), 0, stream, strand_view<Block32>(fm.strand[0]), codes, read_off,
                           phred, n, p, ws, ws_off, corrected, results, broken, ctr);
    return hipGetLastError();
}

} // namespace lrsc
