// fm_kmerize.hip -- fmwalk's hybrid and kmerize algorithms and the sampled k-mer counts on a resident index.  The algorithm is
// fm_kmerize.h's, the trim and the walk fm_fmwalk.h's.
//
//   kmerize_split_kernel<WIDE>  one wavefront per read to split.  The grid is persistent: a wavefront takes the jobs slot, slot +
//                               wavefronts, ... and keeps one slice of the workspace for all of them (a byte per position and
//                               strand, the split flags, the list of boundaries to probe).  Lanes are the (position, strand)
//                               counts, the (boundary, direction, base, strand) probes, then the pieces.
//   hybrid_gate_kernel<WIDE>    one wavefront per pair: both reads trimmed, the length gate, the repeat gate's four counts; the
//                               pair's KmGate and, when it is to be walked, the four strings its walks start and end with.
//   hybrid_walk_kernel<WIDE>    fmwalk_walk_kernel for the pairs the gate lets through, with MergeAndKmerize's maxOverlap.
//   kmer_sample_kernel<WIDE>    one lane per sample: the LF steps of extractString, the bases to the sample's workspace row, the
//                               two searches of countSequenceOccurrences.
//
// As in fm_fmwalk.hip the wavefronts of a workgroup share the mask table in LDS and never wait for one another after it is filled,
// uniform state that outlives a phase stands in LDS, and the kernels are held to the registers of kKmWavesPerSimd wavefronts.
#include "fm_kmerize.h"
#include "fm_launch.h"

namespace lrsc {

static_assert(sizeof(KmPiece) == sizeof(lrsc_fmwalk_piece) && sizeof(KmRead) == sizeof(lrsc_fmwalk_read_result) &&
                  sizeof(KmHybrid) == sizeof(lrsc_fmwalk_hybrid_result) && offsetof(KmHybrid, read) == offsetof(lrsc_fmwalk_hybrid_result, read),
              "the structs of lrsc.h");
static_assert(kKmLanes == 64 && kKmProbe * 16 == kKmLanes && kKmThreads == kFwThreads && kKmWavesPerSimd == kFwWavesPerSimd, "the lanes of a probe phase");
static_assert(sizeof(KmJob) == 24 && sizeof(KmGate) == 24 && sizeof(KmJobOut) == 8, "no padding that a copy could leave unset");

constexpr uint32_t kKmWaves = kKmThreads / kKmLanes;

struct KmSplitArgs {
    const uint8_t* codes;
    const uint64_t* read_off;
    const KmJob* jobs;
    KmPiece* pieces;
    KmJobOut* outs;
    uint32_t* broken;
    uint32_t n_jobs, k, threshold, filters;
};

template <bool WIDE>
__global__ __launch_bounds__(kKmThreads) __attribute__((amdgpu_waves_per_eu(kKmWavesPerSimd, kKmWavesPerSimd)))
void kmerize_split_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, KmSplitArgs args, uint8_t* ws, uint64_t ws_slice, uint32_t longest, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ uint32_t att[kKmWaves][kKmLanes];
    __shared__ StrandView<B> view;                                // read where a search needs it, not held in registers
    __shared__ KmSplitArgs a;
    __shared__ KmWork work[kKmWaves];
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) {
        view = bwt;
        a = args;
    }
    if(threadIdx.x < kKmWaves) work[threadIdx.x] = km_work_at(ws + ((uint64_t)blockIdx.x * kKmWaves + threadIdx.x) * ws_slice, longest);
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kKmLanes);
    const uint32_t slot = blockIdx.x * kKmWaves + wave, n_slots = gridDim.x * kKmWaves;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    for(uint32_t job = slot; job < WaveExec::uniform(a.n_jobs) && !bad; job += n_slots) {
        const KmJob j = a.jobs[job];
        const uint32_t len = WaveExec::uniform(j.len);
        const uint8_t* read = a.codes + WaveExec::uniform64(a.read_off[WaveExec::uniform(j.read)]) + WaveExec::uniform(j.head);
        WaveExec w;
        uint32_t n_pieces = 0;
        int32_t main_piece = -1;
        if(len >= a.k && len <= longest)
            km_split<B>(view, mtab, read, len, WaveExec::uniform(a.k), WaveExec::uniform(a.threshold), WaveExec::uniform(a.filters) != 0, work[wave], att[wave], w,
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

template <bool WIDE>
__global__ __launch_bounds__(kKmThreads) __attribute__((amdgpu_waves_per_eu(kKmWavesPerSimd, kKmWavesPerSimd)))
void hybrid_gate_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, const uint8_t* __restrict__ codes, const uint64_t* __restrict__ read_off, uint32_t n_pairs,
                        FwParams p, uint64_t repeat_kmer_freq, uint8_t* __restrict__ strs, KmGate* __restrict__ gates, uint32_t* __restrict__ broken, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ uint32_t att[kKmWaves][kKmLanes];
    __shared__ StrandView<B> view;
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) view = bwt;
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kKmLanes);
    const uint64_t pair = (uint64_t)blockIdx.x * kKmWaves + wave;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    if(pair < n_pairs) {
        const uint64_t b1 = read_off[2 * pair], b2 = read_off[2 * pair + 1], end = read_off[2 * pair + 2];
        const uint32_t m4 = ((uint32_t)p.min_overlap + 3u) & ~3u;
        WaveExec w;
        KmGate g;
        km_gate_pair<B>(view, mtab, codes + b1, (uint32_t)(b2 - b1), codes + b2, (uint32_t)(end - b2), p, repeat_kmer_freq, att[wave], w, strs + pair * 4 * m4, m4, g,
                        bad, n_rank, n_blk);
        if(fw_any_bad(w, bad)) *broken = 1u;
        else if(WaveExec::lane() == 0) gates[pair] = g;
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

// What a wavefront of the walk kernel needs between its phases, in LDS (fm_fmwalk.hip's FwWalkArgs with the gates).
struct KmWalkArgs {
    const uint64_t* read_off;
    const uint8_t* strs;
    const KmGate* gates;
    uint8_t* best;
    FwWalkOut* outs;
    uint32_t* broken;
    uint64_t stride;
    FwParams p;
    uint32_t n_walks;
};

template <bool WIDE>
__global__ __launch_bounds__(kKmThreads) __attribute__((amdgpu_waves_per_eu(kKmWavesPerSimd, kKmWavesPerSimd)))
void hybrid_walk_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, StrandView<typename BlockOf<WIDE>::type> rbwt, KmWalkArgs args, uint8_t* ws, uint64_t ws_slice,
                        DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ StrandView<B> views[2];                            // picked per lane
    __shared__ KmWalkArgs a;
    __shared__ FwWork work[kKmWaves];
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) {
        views[0] = bwt;
        views[1] = rbwt;
        a = args;
    }
    if(threadIdx.x < kKmWaves) work[threadIdx.x] = fw_work_at(ws + ((uint64_t)blockIdx.x * kKmWaves + threadIdx.x) * ws_slice, args.p);
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kKmLanes);
    const uint32_t slot = blockIdx.x * kKmWaves + wave, n_slots = gridDim.x * kKmWaves;     // uniform in the wavefront
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    for(uint32_t walk = slot; walk < WaveExec::uniform(a.n_walks) && !bad; walk += n_slots) {
        const uint64_t pair = walk >> 1;
        const uint32_t wk = walk & 1u, m4 = work[wave].m4;
        WaveExec w;
        FwWalkOut o{0, 0u, 0u, 0u, 0ull};
        if(WaveExec::uniform(a.gates[pair].flags) & kKmWalk) {
            const uint8_t* s = a.strs + pair * 4 * m4;
            const uint32_t n1 = (uint32_t)(a.read_off[2 * pair + 1] - a.read_off[2 * pair]), n2 = (uint32_t)(a.read_off[2 * pair + 2] - a.read_off[2 * pair + 1]);
            fw_walk<B>(views, mtab, s + wk * m4, s + (3 - wk) * m4, a.p, WaveExec::uniform(km_max_overlap(a.p, n1, n2)), work[wave], w, o, bad, n_rank, n_blk);
            bad = fw_any_bad(w, bad) ? 1u : 0u;                   // the wavefront leaves the loop together
            uint8_t* to = a.best + (uint64_t)walk * a.stride;
            for(uint32_t i = WaveExec::lane(); i < o.length && i < a.stride; i += kKmLanes) to[i] = work[wave].best()[i];
        }
        if(WaveExec::lane() == 0) {
            if(!bad) a.outs[walk] = o;
            else *a.broken = 1u;
        }
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

template <bool WIDE>
__global__ __launch_bounds__(kKmThreads) __attribute__((amdgpu_waves_per_eu(kKmWavesPerSimd, kKmWavesPerSimd)))
void kmer_sample_kernel(StrandView<typename BlockOf<WIDE>::type> rbwt, const uint64_t* __restrict__ rows, uint32_t n, uint32_t len, uint8_t* __restrict__ ws,
                        uint32_t* __restrict__ counts, uint32_t* __restrict__ broken, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    fill_mask_table<B>(mtab);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kKmThreads + threadIdx.x;
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    if(i < n) {
        const uint64_t row = rows[i];
        if(row < rbwt.n_dollars) {
            const uint64_t c = km_sample_count<B>(rbwt, mtab, row, len, ws + i * len, bad, n_rank, n_blk);
            if(!bad) counts[i] = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;
        } else bad = 1;
        if(bad) *broken = 1u;
    }
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

hipError_t launch_kmerize_split(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, const KmJob* jobs, uint32_t n_jobs, uint32_t k, uint32_t threshold,
                                bool filters, uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint32_t longest, KmPiece* pieces, KmJobOut* outs, uint32_t* broken,
                                DevCounters* ctr, hipStream_t stream)
{
    if(n_jobs == 0 || k == 0 || groups == 0 || groups >= (1u << 28) || ws_slice < km_workspace_bytes(longest) || (ws_slice & 7u)) return hipErrorInvalidValue;
    const KmSplitArgs args{codes, read_off, jobs, pieces, outs, broken, n_jobs, k, threshold, filters ? 1u : 0u};
    if(fm.wide)
        hipLaunchKernelGGL((kmerize_split_kernel<true>), dim3(groups), dim3(kKmThreads), 0, stream, strand_view<Block64>(fm.strand[0]), args, ws, ws_slice, longest, ctr);
    else
        hipLaunchKernelGGL((kmerize_split_kernel<false>), dim3(groups), dim3(kKmThreads), 0, stream, strand_view<Block32>(fm.strand[0]), args, ws, ws_slice, longest, ctr);
    return hipGetLastError();
}

hipError_t launch_hybrid_gate(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, uint64_t repeat_kmer_freq,
                              uint8_t* strs, KmGate* gates, uint32_t* broken, DevCounters* ctr, hipStream_t stream)
{
    const uint64_t groups = ((uint64_t)n_pairs + kKmWaves - 1) / kKmWaves;
    if(n_pairs == 0 || groups >= (1ull << 31)) return hipErrorInvalidValue;
    if(fm.wide)
        hipLaunchKernelGGL((hybrid_gate_kernel<true>), dim3((unsigned)groups), dim3(kKmThreads), 0, stream, strand_view<Block64>(fm.strand[0]), codes, read_off, n_pairs,
                           p, repeat_kmer_freq, strs, gates, broken, ctr);
    else
        hipLaunchKernelGGL((hybrid_gate_kernel<false>), dim3((unsigned)groups), dim3(kKmThreads), 0, stream, strand_view<Block32>(fm.strand[0]), codes, read_off, n_pairs,
                           p, repeat_kmer_freq, strs, gates, broken, ctr);
    return hipGetLastError();
}

hipError_t launch_hybrid_walks(const FmIndexDev& fm, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, const uint8_t* strs, const KmGate* gates,
                               uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint8_t* best, uint64_t stride, FwWalkOut* outs, uint32_t* broken, DevCounters* ctr,
                               hipStream_t stream)
{
    if(n_pairs == 0 || n_pairs >= (1u << 30) || groups == 0 || groups >= (1u << 28) || ws_slice < fw_workspace_bytes(p) || (ws_slice & 7u)) return hipErrorInvalidValue;
    const KmWalkArgs args{read_off, strs, gates, best, outs, broken, stride, p, 2 * n_pairs};
    if(fm.wide)
        hipLaunchKernelGGL((hybrid_walk_kernel<true>), dim3(groups), dim3(kKmThreads), 0, stream, strand_view<Block64>(fm.strand[0]),
                           strand_view<Block64>(fm.strand[1]), args, ws, ws_slice, ctr);
    else
        hipLaunchKernelGGL((hybrid_walk_kernel<false>), dim3(groups), dim3(kKmThreads), 0, stream, strand_view<Block32>(fm.strand[0]),
                           strand_view<Block32>(fm.strand[1]), args, ws, ws_slice, ctr);
    return hipGetLastError();
}

hipError_t launch_kmer_sample(const FmIndexDev& fm, const uint64_t* rows, uint32_t n, uint32_t len, uint8_t* ws, uint32_t* counts, uint32_t* broken, DevCounters* ctr,
                              hipStream_t stream)
{
    const uint64_t groups = ((uint64_t)n + kKmThreads - 1) / kKmThreads;
    if(n == 0 || len == 0 || len > kKmMaxSampleLength) return hipErrorInvalidValue;
    if(fm.wide)
        hipLaunchKernelGGL((kmer_sample_kernel<true>), dim3((unsigned)groups), dim3(kKmThreads), 0, stream, strand_view<Block64>(fm.strand[1]), rows, n, len, ws, counts,
                           broken, ctr);
    else
        hipLaunchKernelGGL((kmer_sample_kernel<false>), dim3((unsigned)groups), dim3(kKmThreads), 0, stream, strand_view<Block32>(fm.strand[1]), rows, n, len, ws, counts,
                           broken, ctr);
    return hipGetLastError();
}

} // namespace lrsc
