// fm_fmwalk.hip -- paired-end reads merged by walking a resident index from one end to the other.  The algorithm is fm_fmwalk.h's.
//
//   fmwalk_trim_kernel<WIDE>    one wavefront per pair: both reads trimmed, lanes = (position, base, strand) probes; the pair's
//                               trimmed lengths and, when both reach min_overlap, the four strings its walks start and end with.
//   fmwalk_walk_kernel<WIDE>    one wavefront per walk, two walks per pair.  The grid is persistent: a wavefront takes the walks
//                               slot, slot + wavefronts, ... and keeps one slice of the workspace for all of them (the frontier,
//                               the append-only tree of (parent, base) nodes, the strings).  The lanes are the (leaf, base, strand)
//                               triples of a step, the (leaf, strand) chains of a refinement, the (position, strand) chains of a
//                               result's coverage.  It leaves the walk's code, leaves, coverage and string; the entry chooses
//                               between a pair's two.
//
// Both share the layout's mask table in LDS among the kFwThreads / 64 wavefronts of a workgroup, which never wait for one another
// after it is filled, and keep the two strand views there, because a lane picks its strand's.  A step is dependent 64-byte loads
// and latency-bound: the kernels are held to the registers of kFwWavesPerSimd wavefronts per SIMD.
#include "fm_fmwalk.h"
#include "fm_launch.h"

namespace lrsc {

static_assert(sizeof(FwResult) == sizeof(lrsc_fmwalk_result) && offsetof(FwResult, coverage) == offsetof(lrsc_fmwalk_result, coverage) &&
                  offsetof(FwResult, trimmed_length) == offsetof(lrsc_fmwalk_result, trimmed_length),
              "FwResult is lrsc_fmwalk_result");
static_assert(sizeof(FwParams) == sizeof(lrsc_fmwalk_params) && offsetof(FwParams, max_leaves) == offsetof(lrsc_fmwalk_params, max_leaves),
              "FwParams is lrsc_fmwalk_params");
static_assert(kFwLanes == 64 && kFwRound * 8 == kFwLanes && kFwScan * 8 == kFwLanes, "the lanes of a step and of a trim scan");
static_assert(sizeof(FwWalkOut) == 24, "no padding that a copy could leave unset");

constexpr uint32_t kFwWaves = kFwThreads / kFwLanes;

template <bool WIDE>
__global__ __launch_bounds__(kFwThreads) __attribute__((amdgpu_waves_per_eu(kFwWavesPerSimd, kFwWavesPerSimd)))
void fmwalk_trim_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, const uint8_t* __restrict__ codes, const uint64_t* __restrict__ read_off, uint32_t n_pairs,
                        FwParams p, uint8_t* __restrict__ strs, uint32_t* __restrict__ trimmed, uint32_t* __restrict__ broken, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ uint32_t att[kFwWaves][kFwLanes];
    __shared__ StrandView<B> view;                                // read where a search needs it, not held in registers
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) view = bwt;
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kFwLanes);
    const uint64_t pair = (uint64_t)blockIdx.x * kFwWaves + wave;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    if(pair < n_pairs) {
        const uint64_t b1 = read_off[2 * pair], b2 = read_off[2 * pair + 1], end = read_off[2 * pair + 2];
        const uint32_t m4 = ((uint32_t)p.min_overlap + 3u) & ~3u;
        WaveExec w;
        uint32_t t[2];
        fw_trim_pair<B>(view, mtab, codes + b1, (uint32_t)(b2 - b1), codes + b2, (uint32_t)(end - b2), p, att[wave], w, strs + pair * 4 * m4, m4, t, bad, n_rank, n_blk);
        if(WaveExec::lane() == 0) {
            trimmed[2 * pair] = t[0];
            trimmed[2 * pair + 1] = t[1];
        }
        if(bad) *broken = 1u;
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

// What a wavefront of the walk kernel needs between its phases, in LDS: a phase reads what it uses again after the fence before
// it, so none of it stays in registers through a walk.
struct FwWalkArgs {
    const uint64_t* read_off;
    const uint8_t* strs;
    const uint32_t* trimmed;
    uint8_t* best;
    FwWalkOut* outs;
    uint32_t* broken;
    uint64_t stride;
    FwParams p;
    uint32_t n_walks;
};

template <bool WIDE>
__global__ __launch_bounds__(kFwThreads) __attribute__((amdgpu_waves_per_eu(kFwWavesPerSimd, kFwWavesPerSimd)))
void fmwalk_walk_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, StrandView<typename BlockOf<WIDE>::type> rbwt, FwWalkArgs args, uint8_t* ws, uint64_t ws_slice,
                        DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ StrandView<B> views[2];                            // picked per lane
    __shared__ FwWalkArgs a;
    __shared__ FwWork work[kFwWaves];
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) {
        views[0] = bwt;
        views[1] = rbwt;
        a = args;
    }
    if(threadIdx.x < kFwWaves) work[threadIdx.x] = fw_work_at(ws + ((uint64_t)blockIdx.x * kFwWaves + threadIdx.x) * ws_slice, args.p);
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kFwLanes);
    const uint32_t slot = blockIdx.x * kFwWaves + wave, n_slots = gridDim.x * kFwWaves;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    for(uint32_t walk = slot; walk < WaveExec::uniform(a.n_walks) && !bad; walk += n_slots) {
        const uint64_t pair = walk >> 1;
        const uint32_t wk = walk & 1u, m = (uint32_t)a.p.min_overlap, m4 = work[wave].m4;
        WaveExec w;
        FwWalkOut o{0, 0u, 0u, 0u, 0ull};
        if(WaveExec::uniform(a.trimmed[2 * pair]) >= m && WaveExec::uniform(a.trimmed[2 * pair + 1]) >= m) {    // the gate
            const uint8_t* s = a.strs + pair * 4 * m4;
            const uint32_t n1 = (uint32_t)(a.read_off[2 * pair + 1] - a.read_off[2 * pair]), n2 = (uint32_t)(a.read_off[2 * pair + 2] - a.read_off[2 * pair + 1]);
            fw_walk<B>(views, mtab, s + wk * m4, s + (3 - wk) * m4, a.p, WaveExec::uniform(fw_max_overlap(a.p, n1, n2)), work[wave], w, o, bad, n_rank, n_blk);
            bad = fw_any_bad(w, bad) ? 1u : 0u;                   // the wavefront leaves the loop together
            uint8_t* to = a.best + (uint64_t)walk * a.stride;
            for(uint32_t i = WaveExec::lane(); i < o.length && i < a.stride; i += kFwLanes) to[i] = work[wave].best()[i];
        }
        if(WaveExec::lane() == 0) {
            if(!bad) a.outs[walk] = o;
            else *a.broken = 1u;
        }
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

hipError_t launch_fmwalk_trim(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, uint8_t* strs,
                              uint32_t* trimmed, uint32_t* broken, DevCounters* ctr, hipStream_t stream)
{
    const uint64_t groups = ((uint64_t)n_pairs + kFwWaves - 1) / kFwWaves;
    if(n_pairs == 0 || groups >= (1ull << 31)) return hipErrorInvalidValue;
    if(fm.wide)
        hipLaunchKernelGGL((fmwalk_trim_kernel<true>), dim3((unsigned)groups), dim3(kFwThreads), 0, stream, strand_view<Block64>(fm.strand[0]), codes, read_off, n_pairs,
                           p, strs, trimmed, broken, ctr);
    else
        hipLaunchKernelGGL((fmwalk_trim_kernel<false>), dim3((unsigned)groups), dim3(kFwThreads), 0, stream, strand_view<Block32>(fm.strand[0]), codes, read_off, n_pairs,
                           p, strs, trimmed, broken, ctr);
    return hipGetLastError();
}

hipError_t launch_fmwalk_walks(const FmIndexDev& fm, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, const uint8_t* strs, const uint32_t* trimmed,
                               uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint8_t* best, uint64_t stride, FwWalkOut* outs, uint32_t* broken, DevCounters* ctr,
                               hipStream_t stream)
{
    if(n_pairs == 0 || n_pairs >= (1u << 30) || groups == 0 || groups >= (1u << 28) || ws_slice < fw_workspace_bytes(p) || (ws_slice & 7u)) return hipErrorInvalidValue;
    const FwWalkArgs args{read_off, strs, trimmed, best, outs, broken, stride, p, 2 * n_pairs};
    if(fm.wide)
        hipLaunchKernelGGL((fmwalk_walk_kernel<true>), dim3(groups), dim3(kFwThreads), 0, stream, strand_view<Block64>(fm.strand[0]),
                           strand_view<Block64>(fm.strand[1]), args, ws, ws_slice, ctr);
    else
        hipLaunchKernelGGL((fmwalk_walk_kernel<false>), dim3(groups), dim3(kFwThreads), 0, stream, strand_view<Block32>(fm.strand[0]),
                           strand_view<Block32>(fm.strand[1]), args, ws, ws_slice, ctr);
    return hipGetLastError();
}

} // namespace lrsc
