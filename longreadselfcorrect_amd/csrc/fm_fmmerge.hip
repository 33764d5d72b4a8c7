// fm_fmmerge.hip -- unambiguous read merging over a resident index.  The algorithm is fm_fmmerge.h's; every kernel is one of its
// functions a lane per item.
//
//   fmmerge_links_kernel      a lane per read of a chunk, after the overlap's collect and reduce of that chunk: the read's final
//                             blocks in the pool -> its two links; the read's words of the state are set.
//   fmmerge_init_kernel       a lane per node: the node before the first round.
//   fmmerge_round_kernel      a lane per node: one round of pointer doubling from one buffer into the other.
//   fmmerge_cut_kernel        a lane per node, after the first ranking: the cycles' cuts, the dropped reads.
//   fmmerge_place_kernel      a lane per read, after the second ranking: root, key, strand and offset; the root enters the sequence.
//   fmmerge_scan_*_kernel     the exclusive prefix sums over the keys (sequences and bases) in three launches: tile sums, the
//                             sums' own scan by one workgroup, the tiles' scans.
//   fmmerge_finish_kernel     a lane per read: lrsc_fmmerge_read, and from the root lrsc_fmmerge_seq.
//   fmmerge_assemble_kernel   kFmmAssembleLanes lanes per read: the bases it owns, as characters, a byte per store.
//
// A round is a dependent 24-byte gather per lane with nothing to hide it but other wavefronts: the kernels hold few registers
// (kFmmWavesPerSimd wavefronts per SIMD fit) and the grids cover all items at once.
#include "fm_fmmerge.h"
#include "fm_launch.h"

namespace lrsc {

static_assert(sizeof(FmmOutRead) == sizeof(lrsc_fmmerge_read) && offsetof(FmmOutRead, offset) == offsetof(lrsc_fmmerge_read, offset), "FmmOutRead is lrsc_fmmerge_read");
static_assert(sizeof(FmmOutSeq) == sizeof(lrsc_fmmerge_seq) && offsetof(FmmOutSeq, n_reads) == offsetof(lrsc_fmmerge_seq, n_reads) &&
                  offsetof(FmmOutSeq, circular) == offsetof(lrsc_fmmerge_seq, circular),
              "FmmOutSeq is lrsc_fmmerge_seq");
static_assert(kFmmReversed == LRSC_FMMERGE_REVERSED && kFmmDropped == LRSC_FMMERGE_DROPPED && kFmmSelfLink == LRSC_FMMERGE_SELF_LINK, "the flags that lrsc.h states");

constexpr uint32_t kFmmWaves = kFmmThreads / kWaveLanes;

__device__ __forceinline__ uint64_t fmm_item() { return (uint64_t)blockIdx.x * kFmmThreads + threadIdx.x; }

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_links_kernel(FmmState s, uint32_t first, uint32_t n_chunk, uint32_t min_overlap, const OvOutRead* __restrict__ outs, const OvOutBlock* __restrict__ pool,
                          const unsigned long long* __restrict__ pool_used, const OvChainHead* __restrict__ heads, const uint32_t* order0, const uint32_t* order1,
                          uint32_t* first_bad)
{
    const uint64_t i = fmm_item();
    if(i >= n_chunk) return;
    const uint32_t r = first + (uint32_t)i;
    const uint32_t* order[2] = {order0, order1};
    FmmLink l[2];
    fmm_link_read(r, s.n, fmm_len(s, r), min_overlap, outs[i], pool, *pool_used, heads[i * kOvChains], order, l, first_bad);
    s.links[2 * r] = l[0];
    s.links[2 * r + 1] = l[1];
    s.cut[2 * r] = 0u;
    s.cut[2 * r + 1] = 0u;
    s.seed[r] = r;
    s.mark[r] = 0u;
    s.aux[r] = kFmmNone;
    s.key_len[r] = 0ull;
    s.key_reads[r] = 0u;
}

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_init_kernel(FmmState s, FmmNode* __restrict__ nodes)
{
    const uint64_t x = fmm_item();
    if(x < 2ull * s.n) nodes[x] = fmm_node_init(s, (uint32_t)x);
}

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_round_kernel(const FmmNode* __restrict__ in, FmmNode* __restrict__ out, uint64_t n_nodes)
{
    const uint64_t x = fmm_item();
    if(x < n_nodes) out[x] = fmm_node_round(in, (uint32_t)x);
}

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_cut_kernel(FmmState s, const FmmNode* __restrict__ nodes)
{
    const uint64_t x = fmm_item();
    if(x < 2ull * s.n) fmm_cut(s, nodes, (uint32_t)x);
}

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_place_kernel(FmmState s, const FmmNode* __restrict__ nodes)
{
    const uint64_t r = fmm_item();
    if(r < s.n) fmm_place_read(s, nodes, (uint32_t)r);
}

// The exclusive prefix sums of (c, v) over the workgroup's lanes, and the workgroup's totals.  Every lane has to be here.
__device__ __forceinline__ void fmm_block_scan(uint32_t c, unsigned long long v, uint32_t& before_c, unsigned long long& before_v, uint32_t& total_c,
                                               unsigned long long& total_v)
{
    __shared__ uint32_t wave_c[kFmmWaves];
    __shared__ unsigned long long wave_v[kFmmWaves];
    const uint32_t lane = threadIdx.x & (kWaveLanes - 1), wave = threadIdx.x / kWaveLanes;
    uint32_t ic = c;
    unsigned long long iv = v;
#pragma unroll
    for(int o = 1; o < 64; o <<= 1) {
        const uint32_t uc = (uint32_t)__shfl_up((int)ic, o, 64);
        const unsigned long long uv = __shfl_up(iv, o, 64);
        ic += lane >= (uint32_t)o ? uc : 0u;
        iv += lane >= (uint32_t)o ? uv : 0ull;
    }
    __syncthreads();                                              // the table is free again
    if(lane == kWaveLanes - 1) {
        wave_c[wave] = ic;
        wave_v[wave] = iv;
    }
    __syncthreads();
    before_c = ic - c;
    before_v = iv - v;
    total_c = 0;
    total_v = 0;
#pragma unroll
    for(uint32_t w = 0; w < kFmmWaves; ++w) {
        before_c += w < wave ? wave_c[w] : 0u;
        before_v += w < wave ? wave_v[w] : 0ull;
        total_c += wave_c[w];
        total_v += wave_v[w];
    }
}

// tile_seqs[b], tile_bases[b] = the sequences and bases under the keys of tile b
__global__ __launch_bounds__(kFmmThreads)
void fmmerge_scan_tiles_kernel(FmmState s, uint32_t* __restrict__ tile_seqs, unsigned long long* __restrict__ tile_bases)
{
    const uint64_t k = fmm_item();
    const unsigned long long v = k < s.n ? s.key_len[k] : 0ull;
    uint32_t bc, tc;
    unsigned long long bv, tv;
    fmm_block_scan(v ? 1u : 0u, v, bc, bv, tc, tv);
    if(threadIdx.x == 0) {
        tile_seqs[blockIdx.x] = tc;
        tile_bases[blockIdx.x] = tv;
    }
}

// one workgroup: the tiles' sums -> their exclusive prefix sums, in place; totals[0] = sequences, totals[1] = bases
__global__ __launch_bounds__(kFmmThreads)
void fmmerge_scan_top_kernel(uint32_t* __restrict__ tile_seqs, unsigned long long* __restrict__ tile_bases, uint32_t n_tiles, unsigned long long* __restrict__ totals)
{
    uint32_t carry_c = 0;
    unsigned long long carry_v = 0;
    for(uint32_t t0 = 0; t0 < n_tiles; t0 += kFmmThreads) {       // uniform in the workgroup
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = t < n_tiles ? tile_seqs[t] : 0u;
        const unsigned long long v = t < n_tiles ? tile_bases[t] : 0ull;
        uint32_t bc, tc;
        unsigned long long bv, tv;
        fmm_block_scan(c, v, bc, bv, tc, tv);
        if(t < n_tiles) {
            tile_seqs[t] = carry_c + bc;
            tile_bases[t] = carry_v + bv;
        }
        carry_c += tc;
        carry_v += tv;
    }
    if(threadIdx.x == 0) {
        totals[0] = carry_c;
        totals[1] = carry_v;
    }
}

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_scan_apply_kernel(FmmState s, const uint32_t* __restrict__ tile_seqs, const unsigned long long* __restrict__ tile_bases)
{
    const uint64_t k = fmm_item();
    const unsigned long long v = k < s.n ? s.key_len[k] : 0ull;
    uint32_t bc, tc;
    unsigned long long bv, tv;
    fmm_block_scan(v ? 1u : 0u, v, bc, bv, tc, tv);
    if(k < s.n) {
        s.key_seq[k] = tile_seqs[blockIdx.x] + bc;
        s.key_off[k] = tile_bases[blockIdx.x] + bv;
    }
}

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_finish_kernel(FmmState s, FmmOutRead* __restrict__ per_read, FmmOutSeq* __restrict__ seqs)
{
    const uint64_t r = fmm_item();
    if(r < s.n) fmm_finish_read(s, (uint32_t)r, per_read, seqs);
}

__global__ __launch_bounds__(kFmmThreads)
void fmmerge_assemble_kernel(FmmState s, const uint8_t* __restrict__ codes, char* __restrict__ bases, uint64_t n_bases)
{
    const uint64_t item = fmm_item(), r = item / kFmmAssembleLanes;
    if(r >= s.n) return;
    uint32_t first = 0;
    uint64_t at = 0;
    bool reversed = false;
    if(!fmm_assemble_plan(s, (uint32_t)r, first, at, reversed)) return;
    const uint32_t len = fmm_len(s, (uint32_t)r);
    const uint8_t* mine = codes + s.read_off[r];
    for(uint32_t j = first + (uint32_t)(item % kFmmAssembleLanes); j < len; j += kFmmAssembleLanes)
        if(at + j < n_bases) bases[at + j] = fmm_assemble_base(mine, len, j, reversed);
}

static uint32_t fmm_groups(uint64_t items) { return (uint32_t)((items + kFmmThreads - 1) / kFmmThreads); }
static bool fmm_ok(const FmmState& s) { return s.n != 0 && s.n <= kFmmMaxReads; }

hipError_t launch_fmmerge_links(const FmmState& s, uint32_t first, uint32_t n_chunk, uint32_t min_overlap, const OvOutRead* outs, const OvOutBlock* pool,
                                const unsigned long long* pool_used, const OvChainHead* heads, const uint32_t* order0, const uint32_t* order1, uint32_t* first_bad,
                                hipStream_t stream)
{
    if(!fmm_ok(s) || n_chunk == 0 || (uint64_t)first + n_chunk > s.n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmmerge_links_kernel, dim3(fmm_groups(n_chunk)), dim3(kFmmThreads), 0, stream, s, first, n_chunk, min_overlap, outs, pool, pool_used, heads, order0,
                       order1, first_bad);
    return hipGetLastError();
}

hipError_t launch_fmmerge_init(const FmmState& s, FmmNode* nodes, hipStream_t stream)
{
    if(!fmm_ok(s)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmmerge_init_kernel, dim3(fmm_groups(2ull * s.n)), dim3(kFmmThreads), 0, stream, s, nodes);
    return hipGetLastError();
}

hipError_t launch_fmmerge_round(const FmmState& s, const FmmNode* in, FmmNode* out, hipStream_t stream)
{
    if(!fmm_ok(s) || in == out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmmerge_round_kernel, dim3(fmm_groups(2ull * s.n)), dim3(kFmmThreads), 0, stream, in, out, 2ull * s.n);
    return hipGetLastError();
}

hipError_t launch_fmmerge_cut(const FmmState& s, const FmmNode* nodes, hipStream_t stream)
{
    if(!fmm_ok(s)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmmerge_cut_kernel, dim3(fmm_groups(2ull * s.n)), dim3(kFmmThreads), 0, stream, s, nodes);
    return hipGetLastError();
}

hipError_t launch_fmmerge_place(const FmmState& s, const FmmNode* nodes, hipStream_t stream)
{
    if(!fmm_ok(s)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmmerge_place_kernel, dim3(fmm_groups(s.n)), dim3(kFmmThreads), 0, stream, s, nodes);
    return hipGetLastError();
}

uint32_t fmmerge_scan_tiles(uint32_t n) { return fmm_groups(n); }

hipError_t launch_fmmerge_scan(const FmmState& s, int step, uint32_t* tile_seqs, unsigned long long* tile_bases, unsigned long long* totals, hipStream_t stream)
{
    if(!fmm_ok(s)) return hipErrorInvalidValue;
    const uint32_t tiles = fmm_groups(s.n);
    if(step == 0) hipLaunchKernelGGL(fmmerge_scan_tiles_kernel, dim3(tiles), dim3(kFmmThreads), 0, stream, s, tile_seqs, tile_bases);
    else if(step == 1) hipLaunchKernelGGL(fmmerge_scan_top_kernel, dim3(1), dim3(kFmmThreads), 0, stream, tile_seqs, tile_bases, tiles, totals);
    else hipLaunchKernelGGL(fmmerge_scan_apply_kernel, dim3(tiles), dim3(kFmmThreads), 0, stream, s, tile_seqs, tile_bases);
    return hipGetLastError();
}

hipError_t launch_fmmerge_finish(const FmmState& s, FmmOutRead* per_read, FmmOutSeq* seqs, hipStream_t stream)
{
    if(!fmm_ok(s)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmmerge_finish_kernel, dim3(fmm_groups(s.n)), dim3(kFmmThreads), 0, stream, s, per_read, seqs);
    return hipGetLastError();
}

hipError_t launch_fmmerge_assemble(const FmmState& s, const uint8_t* codes, char* bases, uint64_t n_bases, hipStream_t stream)
{
    if(!fmm_ok(s)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmmerge_assemble_kernel, dim3(fmm_groups((uint64_t)s.n * kFmmAssembleLanes)), dim3(kFmmThreads), 0, stream, s, codes, bases, n_bases);
    return hipGetLastError();
}

} // namespace lrsc
