// fm_overlap.hip -- exact irreducible read overlaps over a resident index.  The algorithm is fm_overlap.h's.
//
//   overlap_collect_kernel<WIDE>   one lane per chain, four chains per read, sixteen reads per wavefront: the blocks of each chain in
//                                  the order of its search, and its head (count, containment block, isSubstring).
//   overlap_reduce_kernel<WIDE>    one wavefront per read: the trims, the submaximal filter, the join and the irreducible rounds of
//                                  fm_overlap.h on what the chains left; the read's final blocks go from the wavefront's slice to a
//                                  pool, at a place taken from the pool's counter.
//
// Both grids are persistent: a wavefront takes the tiles, or the reads, slot, slot + wavefronts, ...; the reduce kernel keeps one
// slice of the workspace for all of its reads.  Both share the layout's mask table in LDS among the kOvThreads / 64 wavefronts of
// a workgroup, which never wait for one another after it is filled, and keep the two strand views there, because a lane picks
// its strand's.  A step is dependent 64-byte loads and latency-bound: the kernels are held to the registers of kOvWavesPerSimd
// wavefronts per SIMD.
#include "fm_overlap.h"
#include "fm_launch.h"

namespace lrsc {

static_assert(sizeof(OvOutBlock) == sizeof(lrsc_overlap_block) && offsetof(OvOutBlock, overlap_len) == offsetof(lrsc_overlap_block, overlap_len) &&
                  offsetof(OvOutBlock, contained) == offsetof(lrsc_overlap_block, contained),
              "OvOutBlock is lrsc_overlap_block");
static_assert(sizeof(OvOutRead) == sizeof(lrsc_overlap_read) && offsetof(OvOutRead, first_block) == offsetof(lrsc_overlap_read, first_block), "OvOutRead is lrsc_overlap_read");
static_assert(kOvLanes == 64 && kOvReadsPerWave * kOvChains == kOvLanes, "the lanes of a collect tile");

constexpr uint32_t kOvWaves = kOvThreads / kOvLanes;

template <bool WIDE>
__global__ __launch_bounds__(kOvThreads) __attribute__((amdgpu_waves_per_eu(kOvWavesPerSimd, kOvWavesPerSimd)))
void overlap_collect_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, StrandView<typename BlockOf<WIDE>::type> rbwt, const uint8_t* __restrict__ codes,
                            const uint64_t* __restrict__ read_off, uint32_t n_reads, OvParams p, OvChainHead* __restrict__ heads, OvBlock* __restrict__ chain_blocks,
                            uint32_t* __restrict__ broken, DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ StrandView<B> views[2];                            // picked per lane
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) {
        views[0] = bwt;
        views[1] = rbwt;
    }
    __syncthreads();
    const uint32_t slot = blockIdx.x * kOvWaves + threadIdx.x / kOvLanes, n_slots = gridDim.x * kOvWaves;
    const uint32_t lane = threadIdx.x & (kOvLanes - 1), slots = ov_slots(p);
    const uint64_t n_tiles = ((uint64_t)n_reads + kOvReadsPerWave - 1) / kOvReadsPerWave;
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    for(uint64_t tile = slot; tile < n_tiles; tile += n_slots) {
        const uint64_t read = tile * kOvReadsPerWave + lane / kOvChains;
        if(read >= n_reads) continue;
        const uint32_t chain = lane % kOvChains;
        const uint64_t begin = read_off[read];
        const uint32_t n = (uint32_t)(read_off[read + 1] - begin);
        OvChainHead head{0u, 0u, 0u, 0u, OvBlock{OvIv{0, 0}, OvIv{0, 0}, 0u, 0u, 0u, 0u}};
        // a read longer than the call's longest has no slots to write to: the entry sized them from the same offsets
        if(n >= p.min_overlap && n <= p.max_len)
            ov_collect_chain<B>(views, mtab, codes + begin, n, p.min_overlap, chain, chain_blocks + (read * kOvChains + chain) * slots, slots, head, bad, n_rank, n_blk);
        heads[read * kOvChains + chain] = head;
    }
    if(bad) *broken = 1u;
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

// What a wavefront of the reduce kernel needs between its phases, in LDS
struct OvReduceArgs {
    const uint64_t* read_off;
    const OvChainHead* heads;
    const OvBlock* chain_blocks;
    OvOutRead* outs;
    OvOutBlock* pool;
    unsigned long long* pool_used;
    uint32_t* broken;
    uint64_t pool_cap;
    OvParams p;
    uint32_t n_reads, pad;
};

template <bool WIDE>
__global__ __launch_bounds__(kOvThreads) __attribute__((amdgpu_waves_per_eu(kOvWavesPerSimd, kOvWavesPerSimd)))
void overlap_reduce_kernel(StrandView<typename BlockOf<WIDE>::type> bwt, StrandView<typename BlockOf<WIDE>::type> rbwt, OvReduceArgs args, uint8_t* ws, uint64_t ws_slice,
                           DevCounters* ctr)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    __shared__ StrandView<B> views[2];
    __shared__ OvReduceArgs a;
    __shared__ OvWork work[kOvWaves];
    __shared__ unsigned long long place[kOvWaves];
    fill_mask_table<B>(mtab);
    if(threadIdx.x == 0) {
        views[0] = bwt;
        views[1] = rbwt;
        a = args;
    }
    if(threadIdx.x < kOvWaves) work[threadIdx.x] = ov_work_at(ws + ((uint64_t)blockIdx.x * kOvWaves + threadIdx.x) * ws_slice, args.p);
    __syncthreads();
    const uint32_t wave = WaveExec::uniform(threadIdx.x / kOvLanes);
    const uint32_t slot = blockIdx.x * kOvWaves + wave, n_slots = gridDim.x * kOvWaves;       // uniform in the wavefront
    const uint32_t slots = ov_slots(a.p);
    uint32_t n_rank = 0, n_blk = 0, bad = 0;
    for(uint32_t read = slot; read < WaveExec::uniform(a.n_reads) && !bad; read += n_slots) {
        WaveExec w;
        OvOutRead res{0u, 0u, kOvOk, 0u, 0ull};
        const uint32_t n = (uint32_t)WaveExec::uniform64(a.read_off[read + 1] - a.read_off[read]);
        ov_reduce_read<B>(views, mtab, a.heads + (uint64_t)read * kOvChains, a.chain_blocks + (uint64_t)read * kOvChains * slots, slots, n, a.p.min_overlap, work[wave], w,
                          work[wave].stage(), res, bad, n_rank, n_blk);
        bad = ov_any_bad(w, bad) ? 1u : 0u;                       // the wavefront leaves the loop together
        if(bad) break;
        if(WaveExec::lane() == 0) place[wave] = res.n_blocks ? atomicAdd(a.pool_used, (unsigned long long)res.n_blocks) : 0ull;
        WaveExec::sync();
        const uint64_t first = WaveExec::uniform64(place[wave]);
        if(first + res.n_blocks > a.pool_cap) {                   // the pool holds kOvOutCap blocks for every read: never
            res.status = kOvOverflow;
            res.n_blocks = 0;
        }
        for(uint32_t i = WaveExec::lane(); i < res.n_blocks; i += kOvLanes) a.pool[first + i] = work[wave].stage()[i];
        res.first_block = first;
        if(WaveExec::lane() == 0) a.outs[read] = res;
    }
    if(bad && WaveExec::lane() == 0) *a.broken = 1u;
    wave_count(ctr, wave_sum(n_rank), wave_sum(n_blk));
}

hipError_t launch_overlap_collect(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_reads, const OvParams& p, uint32_t groups,
                                  OvChainHead* heads, OvBlock* chain_blocks, uint32_t* broken, DevCounters* ctr, hipStream_t stream)
{
    if(n_reads == 0 || groups == 0 || groups >= (1u << 28)) return hipErrorInvalidValue;
    if(fm.wide)
        hipLaunchKernelGGL((overlap_collect_kernel<true>), dim3(groups), dim3(kOvThreads), 0, stream, strand_view<Block64>(fm.strand[0]), strand_view<Block64>(fm.strand[1]),
                           codes, read_off, n_reads, p, heads, chain_blocks, broken, ctr);
    else
        hipLaunchKernelGGL((overlap_collect_kernel<false>), dim3(groups), dim3(kOvThreads), 0, stream, strand_view<Block32>(fm.strand[0]), strand_view<Block32>(fm.strand[1]),
                           codes, read_off, n_reads, p, heads, chain_blocks, broken, ctr);
    return hipGetLastError();
}

hipError_t launch_overlap_reduce(const FmIndexDev& fm, const uint64_t* read_off, uint32_t n_reads, const OvParams& p, const OvChainHead* heads, const OvBlock* chain_blocks,
                                 uint32_t groups, uint8_t* ws, uint64_t ws_slice, OvOutRead* outs, OvOutBlock* pool, uint64_t pool_cap, unsigned long long* pool_used,
                                 uint32_t* broken, DevCounters* ctr, hipStream_t stream)
{
    if(n_reads == 0 || groups == 0 || groups >= (1u << 28) || ws_slice < ov_workspace_bytes(p) || (ws_slice & 7u)) return hipErrorInvalidValue;
    const OvReduceArgs args{read_off, heads, chain_blocks, outs, pool, pool_used, broken, pool_cap, p, n_reads, 0u};
    if(fm.wide)
        hipLaunchKernelGGL((overlap_reduce_kernel<true>), dim3(groups), dim3(kOvThreads), 0, stream, strand_view<Block64>(fm.strand[0]), strand_view<Block64>(fm.strand[1]),
                           args, ws, ws_slice, ctr);
    else
        hipLaunchKernelGGL((overlap_reduce_kernel<false>), dim3(groups), dim3(kOvThreads), 0, stream, strand_view<Block32>(fm.strand[0]), strand_view<Block32>(fm.strand[1]),
                           args, ws, ws_slice, ctr);
    return hipGetLastError();
}

} // namespace lrsc
