// fm_dup.hip -- the duplicate check of a batch of reads against a resident index.  The arithmetic is fm_dup.h's.
//
//   1. dup_chain_kernel<WIDE>   one lane per chain, four chains per read, laid out by kind: the workgroups of kind 0 (w in .bwt)
//                               first, then those of kind 1, 2, 3.  The reverse-complement chains of most reads die within a few
//                               dozen steps; laid out by kind their wavefronts retire then, and the chains that go the whole read
//                               share their wavefronts with chains that do the same.  A step is one or two 64-byte loads and
//                               popcounts against the layout's mask table in LDS.  The chain is latency-bound: the kernel is held
//                               to the registers of kDupWavesPerSimd wavefronts per SIMD.  One very long read is one lane's chain.
//   2. dup_combine_kernel       one lane per read: the four chains -> '$' intervals (two look-ups in the '$' list of .bwt),
//                               SUBSTRING / ABSENT or the canonical slot, and an atomicMin of the read's number on the slot's word
//                               of winner[]
//   3. dup_classify_kernel      one lane per read: UNIQUE when the slot's bit is clear and the read won the slot, else FULL_LENGTH
//   4. dup_commit_kernel        one lane per read: sets the slot's bit (32-bit atomic OR), winner[] back to kDupNoWinner
// The outcome is that of the reads taken one after the other in input order, whatever the order the lanes run in.
#include "fm_dup.h"
#include "fm_launch.h"

namespace lrsc {

static_assert(sizeof(DupResult) == sizeof(lrsc_dup_result) && offsetof(DupResult, cls) == offsetof(lrsc_dup_result, cls) &&
              offsetof(DupResult, rvc_lower) == offsetof(lrsc_dup_result, rvc_dollar), "DupResult is lrsc_dup_result");
static_assert(kDupUnique == LRSC_DUP_UNIQUE && kDupSubstring == LRSC_DUP_SUBSTRING && kDupFullLength == LRSC_DUP_FULL_LENGTH &&
              kDupAbsent == LRSC_DUP_ABSENT, "the classes are lrsc_dup_class");

template <bool WIDE>
__global__ __launch_bounds__(kDupThreads) __attribute__((amdgpu_waves_per_eu(kDupWavesPerSimd, kDupWavesPerSimd)))
void dup_chain_kernel(StrandView<typename BlockOf<WIDE>::type> S0, StrandView<typename BlockOf<WIDE>::type> S1, const uint32_t* __restrict__ words,
                      const uint64_t* __restrict__ read_off, uint32_t n, uint32_t groups_per_kind, DupChainOut* __restrict__ chains, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    // The table's fill and the wavefront sums below are written in place, not with fm_launch.h's fill_mask_table and wave_sum:
    // with the helpers the kernel came to 930 (Block64) and 939 (Block32) instructions against 935 and 938, at the same 61 and 52
    // VGPRs, and measured 0.4 to 1.1 % slower.
    for(uint32_t i = threadIdx.x; i < MaskTab<B>::kWords; i += blockDim.x) mtab[i] = mask_word<B>(i);
    __syncthreads();
    const uint32_t kind = blockIdx.x / groups_per_kind;           // uniform in the workgroup
    const uint64_t read = (uint64_t)(blockIdx.x - kind * groups_per_kind) * kDupThreads + threadIdx.x;
    const StrandView<B> S = select_view(dup_kind_strand(kind) != 0, S0, S1);       // the kind's strand
    uint32_t n_rank = 0, n_blk = 0;
    if(read < n) {
        const uint64_t begin = read_off[read];
        const uint32_t len = (uint32_t)(read_off[read + 1] - begin);
        chains[(uint64_t)kind * n + read] = dup_chain<B>(S, mtab, words, begin, len, kind, n_rank, n_blk);
    }
    // the wavefront's totals -> the counter shard of its workgroup (every lane of the wavefront is here)
    unsigned long long a = n_rank, b = n_blk;
#pragma unroll
    for(int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    wave_count(ctr, a, b);
}

__global__ __launch_bounds__(256) void dup_combine_kernel(DupDollars bwt, uint64_t n_rows, const DupChainOut* __restrict__ chains, uint32_t n, uint64_t n_slots,
                                                          DupResult* __restrict__ results, uint64_t* __restrict__ slots, uint32_t* __restrict__ winner,
                                                          uint32_t* __restrict__ broken)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if(i >= n) return;
    DupResult r;
    uint64_t slot;
    if(!dup_combine(bwt, n_rows, chains[i], chains[(uint64_t)n + i], chains[2ull * n + i], chains[3ull * n + i], n_slots, r, slot)) *broken = 1u;
    results[i] = r;
    slots[i] = slot;
    if(slot < n_slots) atomicMin(winner + slot, (uint32_t)i);
}

__global__ __launch_bounds__(256) void dup_classify_kernel(DupResult* __restrict__ results, const uint64_t* __restrict__ slots, uint32_t n, uint64_t n_slots,
                                                           const uint32_t* __restrict__ bits, const uint32_t* __restrict__ winner)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if(i >= n) return;
    const uint64_t slot = slots[i];
    if(slot >= n_slots) return;
    results[i].cls = dup_classify(((bits[slot >> 5] >> (uint32_t)(slot & 31u)) & 1u) != 0, winner[slot], (uint32_t)i);
}

__global__ __launch_bounds__(256) void dup_commit_kernel(const uint64_t* __restrict__ slots, uint32_t n, uint64_t n_slots, uint32_t* __restrict__ bits,
                                                         uint32_t* __restrict__ winner)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if(i >= n) return;
    const uint64_t slot = slots[i];
    if(slot >= n_slots) return;
    atomicOr(bits + (slot >> 5), 1u << (uint32_t)(slot & 31u));
    winner[slot] = kDupNoWinner;
}

hipError_t launch_dup_chains(const FmIndexDev& fm, const uint32_t* words, const uint64_t* read_off, uint32_t n, DupChainOut* chains, DevCounters* ctr,
                             hipStream_t stream)
{
    const uint64_t gpk = ((uint64_t)n + kDupThreads - 1) / kDupThreads;
    if(n == 0 || gpk * kDupKinds >= (1ull << 31)) return hipErrorInvalidValue;
    if(fm.wide)
        hipLaunchKernelGGL((dup_chain_kernel<true>), dim3((unsigned)(gpk * kDupKinds)), dim3(kDupThreads), 0, stream, strand_view<Block64>(fm.strand[0]),
                           strand_view<Block64>(fm.strand[1]), words, read_off, n, (uint32_t)gpk, chains, ctr);
    else
        hipLaunchKernelGGL((dup_chain_kernel<false>), dim3((unsigned)(gpk * kDupKinds)), dim3(kDupThreads), 0, stream, strand_view<Block32>(fm.strand[0]),
                           strand_view<Block32>(fm.strand[1]), words, read_off, n, (uint32_t)gpk, chains, ctr);
    return hipGetLastError();
}

hipError_t launch_dup_classify(const FmIndexDev& fm, const DupChainOut* chains, uint32_t n, uint64_t n_slots, DupResult* results, uint64_t* slots, uint32_t* winner,
                               uint32_t* bits, uint32_t* broken, hipStream_t stream)
{
    if(n == 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((uint64_t)n + 255) / 256)), block(256);
    const FmStrand& s0 = fm.strand[0];
    const DupDollars bwt{s0.dollars, s0.dollar_dir, s0.n_dollars, fm.wide ? Block64::kSyms : Block32::kSyms};
    hipLaunchKernelGGL(dup_combine_kernel, grid, block, 0, stream, bwt, s0.n_symbols, chains, n, n_slots, results, slots, winner, broken);
    hipError_t e = hipGetLastError();
    if(e != hipSuccess) return e;
    hipLaunchKernelGGL(dup_classify_kernel, grid, block, 0, stream, results, slots, n, n_slots, bits, winner);
    e = hipGetLastError();
    if(e != hipSuccess) return e;
    hipLaunchKernelGGL(dup_commit_kernel, grid, block, 0, stream, slots, n, n_slots, bits, winner);
    return hipGetLastError();
}

} // namespace lrsc
