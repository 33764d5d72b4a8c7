// fm_validate.hip -- fmwalk's validate algorithm on a resident index.  The algorithm is fm_validate.h's, the walk fm_fmwalk.h's and
// the split fm_kmerize.h's.
//
//   validate_walk_kernel<WIDE>   one wavefront per walk, two walks per read longer than min_overlap (a shorter read's two are
//                                skipped).  The grid is persistent: a wavefront takes the walks slot, slot + wavefronts, ... and
//                                keeps one slice of the workspace, sized for the longest read of the call, for all of them.  The
//                                lanes are fw_walk's: the (leaf, base, strand) triples of a step, the (leaf, strand) chains of a
//                                refinement, the (position, strand) chains of a result's coverage.  It leaves the walk's code,
//                                leaves, coverage and string; the entry decides between a read's two.
//   validate_split_kernel<WIDE>  one wavefront per read that the walks left undecided, as kmerize_split_kernel: lanes are the
//                                (position, strand) counts, 32 positions a phase, the (boundary, direction, base, strand) probes,
//                                kKmProbe boundaries a phase, then the pieces; two reductions find the main piece.
//
// As in fm_fmwalk.hip the wavefronts of a workgroup share the mask table in LDS and never wait for one another after it is filled,
// uniform state that outlives a phase stands in LDS (a walk's own parameters among it), and the kernels are held to the registers
// of kVdWavesPerSimd wavefronts.
#include "fm_validate.h"
#include "fm_launch.h"

namespace lrsc {

static_assert(sizeof(VdResult) == sizeof(lrsc_fmwalk_validate_result) && offsetof(VdResult, coverage) == offsetof(lrsc_fmwalk_validate_result, coverage) &&
                  offsetof(VdResult, chosen) == offsetof(lrsc_fmwalk_validate_result, chosen) && offsetof(VdResult, read) == offsetof(lrsc_fmwalk_validate_result, read),
              "VdResult is lrsc_fmwalk_validate_result");
static_assert(kVdLanes == 64 && kVdThreads == kFwThreads && kVdThreads == kKmThreads && kVdWavesPerSimd == kFwWavesPerSimd, "the lanes of fw_walk and km_split");

constexpr uint32_t kVdWaves = kVdThreads / kVdLanes;

// What a wavefront of the walk kernel needs between its phases, in LDS.
struct VdWalkArgs {
    const uint8_t* codes;
    const uint64_t* read_off;
    uint8_t* best;
    FwWalkOut* outs;
    uint32_t* broken;
    uint64_t stride;
    FwParams p;                                                   // max_insert: vd_depth of the call's longest read
    uint32_t n_walks;
};

template <bool WIDE>
__global__ __launch_bounds__(kVdThreads) __attribute__((amdgpu_waves_per_eu(kVdWavesPerSimd, kVdWavesPerSimd)))
void validate_walk_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, StrandView<typename BlockOf<WIDE>::type> rbwt, VdWalkArgs args, uint8_t* ws, uint64_t ws_slice,
                          DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ StrandView<B> views[2];                            // picked per lane
    __shared__ VdWalkArgs a;
    __shared__ FwWork work[kVdWaves];
    __shared__ FwParams own[kVdWaves];                            // the walk's parameters: its read's depth limit
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) {
        views[0] = bwt;
        views[1] = rbwt;
        a = args;
    }
    if(threadIdx.x < kVdWaves) work[threadIdx.x] = fw_work_at(ws + ((uint64_t)blockIdx.x * kVdWaves + threadIdx.x) * ws_slice, args.p);
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kVdLanes);
    const uint32_t slot = blockIdx.x * kVdWaves + wave, n_slots = gridDim.x * kVdWaves;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    for(uint32_t walk = slot; walk < WaveExec::uniform(a.n_walks) && !bad; walk += n_slots) {
        const uint64_t at = WaveExec::uniform64(a.read_off[walk >> 1]);
        const uint32_t n = WaveExec::uniform((uint32_t)(a.read_off[(walk >> 1) + 1] - at));
        WaveExec w;
        FwWalkOut o{0, 0u, 0u, 0u, 0ull};
        if(n > (uint32_t)a.p.min_overlap) {
            vd_walk<B>(views, mtab, a.codes + at, n, a.p, walk & 1u, own[wave], work[wave], w, o, bad, n_rank, n_blk);
            bad = fw_any_bad(w, bad) ? 1u : 0u;                   // the wavefront leaves the loop together
            uint8_t* to = a.best + (uint64_t)walk * a.stride;
            for(uint32_t i = WaveExec::lane(); !bad && i < o.length && i < a.stride; i += kVdLanes) to[i] = work[wave].best()[i];
        }
        if(WaveExec::lane() == 0) {
            if(!bad) a.outs[walk] = o;
            else *a.broken = 1u;
        }
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

struct VdSplitArgs {
    const uint8_t* codes;
    const uint64_t* read_off;
    const KmJob* jobs;
    KmPiece* pieces;
    KmJobOut* outs;
    uint32_t* broken;
    uint64_t threshold;
    uint32_t n_jobs, k;
};

template <bool WIDE>
__global__ __launch_bounds__(kVdThreads) __attribute__((amdgpu_waves_per_eu(kVdWavesPerSimd, kVdWavesPerSimd)))
void validate_split_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, VdSplitArgs args, uint8_t* ws, uint64_t ws_slice, uint32_t longest, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ uint32_t att[kVdWaves][kVdLanes];
    __shared__ StrandView<B> view;                                // read where a search needs it, not held in registers
    __shared__ VdSplitArgs a;
    __shared__ KmWork work[kVdWaves];
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) {
        view = bwt;
        a = args;
    }
    if(threadIdx.x < kVdWaves) work[threadIdx.x] = km_work_at(ws + ((uint64_t)blockIdx.x * kVdWaves + threadIdx.x) * ws_slice, longest);
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kVdLanes);
    const uint32_t slot = blockIdx.x * kVdWaves + wave, n_slots = gridDim.x * kVdWaves;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    for(uint32_t job = slot; job < WaveExec::uniform(a.n_jobs) && !bad; job += n_slots) {
        const KmJob j = a.jobs[job];
        const uint32_t len = WaveExec::uniform(j.len);
        const uint8_t* read = a.codes + WaveExec::uniform64(a.read_off[WaveExec::uniform(j.read)]) + WaveExec::uniform(j.head);
        WaveExec w;
        uint32_t n_pieces = 0;
        int32_t main_piece = -1;
        if(len >= a.k && len <= longest)
            km_split<B, WaveExec, true>(view, mtab, read, len, WaveExec::uniform(a.k), WaveExec::uniform64(a.threshold), false, work[wave], att[wave], w,
                                        a.pieces + WaveExec::uniform64(j.slot), n_pieces, main_piece, bad, n_rank, n_blk);
        else bad = 1;
        bad = fw_any_bad(w, bad) ? 1u : 0u;                       // the wavefront leaves the loop together
        if(WaveExec::lane() == 0) {
            if(!bad) a.outs[job] = KmJobOut{n_pieces, main_piece};
            else *a.broken = 1u;
        }
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

hipError_t launch_validate_walks(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_reads, const FwParams& p, uint32_t groups, uint8_t* ws,
                                 uint64_t ws_slice, uint8_t* best, uint64_t stride, FwWalkOut* outs, uint32_t* broken, DevCounters* ctr, hipStream_t stream)
{
    if(n_reads == 0 || n_reads >= (1u << 30) || groups == 0 || groups >= (1u << 28) || ws_slice < fw_workspace_bytes(p) || (ws_slice & 7u) ||
       stride < (uint64_t)p.max_insert + 1)
        return hipErrorInvalidValue;
    const VdWalkArgs args{codes, read_off, best, outs, broken, stride, p, 2 * n_reads};
    if(fm.wide)
        hipLaunchKernelGGL((validate_walk_kernel<true>), dim3(groups), dim3(kVdThreads), 0, stream, strand_view<Block64>(fm.strand[0]),
                           strand_view<Block64>(fm.strand[1]), args, ws, ws_slice, ctr);
    else
        hipLaunchKernelGGL((validate_walk_kernel<false>), dim3(groups), dim3(kVdThreads), 0, stream, strand_view<Block32>(fm.strand[0]),
                           strand_view<Block32>(fm.strand[1]), args, ws, ws_slice, ctr);
    return hipGetLastError();
}

hipError_t launch_validate_split(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, const KmJob* jobs, uint32_t n_jobs, uint32_t k, uint64_t threshold,
                                 uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint32_t longest, KmPiece* pieces, KmJobOut* outs, uint32_t* broken, DevCounters* ctr,
                                 hipStream_t stream)
{
    if(n_jobs == 0 || k == 0 || groups == 0 || groups >= (1u << 28) || ws_slice < km_workspace_bytes(longest) || (ws_slice & 7u)) return hipErrorInvalidValue;
    const VdSplitArgs args{codes, read_off, jobs, pieces, outs, broken, threshold, n_jobs, k};
    if(fm.wide)
        hipLaunchKernelGGL((validate_split_kernel<true>), dim3(groups), dim3(kVdThreads), 0, stream, strand_view<Block64>(fm.strand[0]), args, ws, ws_slice, longest, ctr);
    else
        hipLaunchKernelGGL((validate_split_kernel<false>), dim3(groups), dim3(kVdThreads), 0, stream, strand_view<Block32>(fm.strand[0]), args, ws, ws_slice, longest, ctr);
    return hipGetLastError();
}

} // namespace lrsc
