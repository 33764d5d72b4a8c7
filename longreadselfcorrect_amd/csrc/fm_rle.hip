// fm_rle.hip -- run-length encodes a device-resident BWT into the reference's RL units (one byte each: code << 5 | run, run <= 31,
// BWTWriterBinary::writeBWChar's rule) without a host pass: what the loop in lrsc_build_bwt made on the host, byte for byte.
//
//   1. rle_summary_kernel  per tile: first and last symbol, length of the last run modulo 31, one single run or not
//   2. hipCUB InclusiveScan over the tiles with rle_combine: entry t - 1 tells tile t how far into a run it starts
//   3. rle_count_kernel    per tile: units that start in it; hipCUB ExclusiveSum gives every tile's offset and the total,
//                          and the output is allocated at exactly that size
//   4. rle_emit_kernel     per tile: its units, staged in LDS at the output's 16-byte phase and stored 16 bytes per lane
//
// A tile is kRleTile symbols in LDS, one stretch of kRleChunks x 16 per lane (fm_rle.h).  The symbols come from the
// byte-per-symbol BWT of build_bwt_resident (SrcBytes: 16-byte coalesced loads) or from the rank blocks of an index copy
// (SrcBlocks: one lane unpacks one 64-byte block with decode_block, looking its '$' rows up once through the directory).  Within a tile the lanes'
// summaries are joined by a block scan with the same operator; the unit that a tile's last symbols open may run on for at most
// 30 symbols, so the emit kernel loads a halo past the tile's end and no tile waits for another.  No atomics anywhere.
#include <hipcub/hipcub.hpp>

#include "fm_launch.h"
#include "fm_rle.h"

namespace lrsc {

static constexpr uint32_t kTileChunks = kRleTile / 16;
// the tile, then room for the halo: two Sym16 from the byte BWT, one whole rank block (at most 12 Sym16) from the blocks
static constexpr uint32_t kSymRows = kTileChunks + Block32::kSyms / 16;
static constexpr uint32_t kStageRows = kTileChunks + 1;          // a tile's units at any 16-byte phase

struct SrcBytes {
    const uint8_t* bwt;
    uint64_t N;
};
template <class Block>
struct SrcBlocks {
    const Block* blocks;
    const uint64_t* dollars;
    const uint32_t* dollar_dir;
    uint64_t n_dollars, n_blocks, N;
};

// symbols [tile * kRleTile, + kRleTile (+ kRleHalo)) -> syms; what lies at and beyond N is never looked at
__device__ __forceinline__ void load_tile(const SrcBytes& src, uint64_t tile, bool halo, Sym16* syms)
{
    const uint64_t base = tile * kRleTile;
    const uint32_t rows = kTileChunks + (halo ? kRleHalo / 16 : 0);
    for(uint32_t q = threadIdx.x; q < rows; q += kRleLanes) {
        const uint64_t p = base + 16ull * q;
        Sym16 v{{0u, 0u, 0u, 0u}};
        if(p + 16 <= src.N) v = *reinterpret_cast<const Sym16*>(src.bwt + p);
        else if(p < src.N) {                                      // the ragged end: the last symbol stands in for those beyond it
#pragma unroll
            for(uint32_t i = 0; i < 16; ++i) v.w[i >> 2] |= (uint32_t)src.bwt[std::min<uint64_t>(p + i, src.N - 1)] << (8 * (i & 3));
        }
        syms[q] = v;
    }
    __syncthreads();
}
template <class Block>
__device__ __forceinline__ void load_tile(const SrcBlocks<Block>& src, uint64_t tile, bool halo, Sym16* syms)
{
    constexpr uint32_t kBlocks = kRleTile / Block::kSyms;
    static_assert(kBlocks + 1 <= kRleLanes, "one lane per block, and one for the halo");
    const uint64_t g = tile * kBlocks + threadIdx.x;
    if(threadIdx.x < kBlocks + (halo ? 1u : 0u) && g < src.n_blocks) decode_block<Block>(src, g, syms + threadIdx.x * (Block::kSyms / 16));
    __syncthreads();
}

// the lane's stretch, how much of it exists, and what the lanes before it in the tile add up to after `seed`
struct Stretch {
    const Sym16* s;
    uint64_t base;
    uint32_t n_valid;
};
__device__ __forceinline__ Stretch my_stretch(const Sym16* syms, uint64_t tile, uint64_t N)
{
    Stretch st;
    st.s = syms + threadIdx.x * kRleChunks;
    st.base = tile * kRleTile + (uint64_t)threadIdx.x * (kRleChunks * 16);
    st.n_valid = st.base >= N ? 0u : (uint32_t)std::min<uint64_t>(N - st.base, kRleChunks * 16);
    return st;
}

using SummaryScan = hipcub::BlockScan<RunSummary, kRleLanes>;
using CountScan = hipcub::BlockScan<uint32_t, kRleLanes>;
using CountReduce = hipcub::BlockReduce<uint32_t, kRleLanes>;

template <class Src>
__global__ __launch_bounds__(kRleLanes) void rle_summary_kernel(Src src, RunSummary* __restrict__ sum)
{
    __shared__ Sym16 syms[kSymRows];
    __shared__ typename SummaryScan::TempStorage tmp;
    const uint64_t tile = blockIdx.x;
    load_tile(src, tile, false, syms);
    const Stretch st = my_stretch(syms, tile, src.N);
    const RunSummary mine = stretch_summary<kRleChunks>(st.s, st.n_valid);
    RunSummary incl, total;
    SummaryScan(tmp).InclusiveScan(mine, incl, RleCombine{}, total);
    if(threadIdx.x == 0) sum[tile] = total;
}

// incl: the inclusive scan of the tiles' summaries.  cnt[tile] = units that start in the tile.
template <class Src>
__global__ __launch_bounds__(kRleLanes) void rle_count_kernel(Src src, const RunSummary* __restrict__ incl, uint64_t* __restrict__ cnt)
{
    __shared__ Sym16 syms[kSymRows];
    __shared__ union { typename SummaryScan::TempStorage scan; typename CountReduce::TempStorage red; } tmp;
    const uint64_t tile = blockIdx.x;
    load_tile(src, tile, false, syms);
    const Stretch st = my_stretch(syms, tile, src.N);
    const RunSummary seed = tile ? incl[tile - 1] : RunSummary{0, 0, 0, 0};
    RunSummary before;
    SummaryScan(tmp.scan).ExclusiveScan(stretch_summary<kRleChunks>(st.s, st.n_valid), before, seed, RleCombine{});
    const uint32_t n = stretch_count<kRleChunks>(st.s, st.n_valid, before);
    __syncthreads();
    const uint32_t total = CountReduce(tmp.red).Sum(n);
    if(threadIdx.x == 0) cnt[tile] = total;
}

// off: the exclusive sum of cnt.  Writes units [off[tile], off[tile + 1]) of out, which is 16-byte aligned.
template <class Src>
__global__ __launch_bounds__(kRleLanes) void rle_emit_kernel(Src src, const RunSummary* __restrict__ incl, const uint64_t* __restrict__ off,
                                                             uint8_t* __restrict__ out)
{
    __shared__ Sym16 syms[kSymRows];
    __shared__ Sym16 stage[kStageRows];
    __shared__ union { typename SummaryScan::TempStorage scan; typename CountScan::TempStorage sum; } tmp;
    const uint64_t tile = blockIdx.x;
    load_tile(src, tile, true, syms);
    const Stretch st = my_stretch(syms, tile, src.N);
    const RunSummary seed = tile ? incl[tile - 1] : RunSummary{0, 0, 0, 0};
    RunSummary before;
    SummaryScan(tmp.scan).ExclusiveScan(stretch_summary<kRleChunks>(st.s, st.n_valid), before, seed, RleCombine{});
    const uint32_t n = stretch_count<kRleChunks>(st.s, st.n_valid, before);
    __syncthreads();
    uint32_t first = 0, total = 0;
    CountScan(tmp.sum).ExclusiveSum(n, first, total);
    // the units take the place in the staging rows that they have in the output's 16-byte rows
    const uint64_t o = off[tile];
    const uint32_t phase = (uint32_t)(o & 15);
    const uint64_t end = st.base + kRleChunks * 16;
    const uint32_t n_after = end < src.N ? (uint32_t)std::min<uint64_t>(src.N - end, kRleMaxRun - 1) : 0u;
    if(n) stretch_emit<kRleChunks>(st.s, st.n_valid, before, n_after, reinterpret_cast<uint8_t*>(stage) + phase + first);
    __syncthreads();
    uint8_t* row0 = out + (o - phase);
    const uint32_t stop = phase + total;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
    for(uint32_t q = threadIdx.x; 16 * q < stop; q += kRleLanes) {
        const uint32_t lo = 16 * q;
        if(lo >= phase && lo + 16 <= stop) *reinterpret_cast<Sym16*>(row0 + lo) = stage[q];
        else
            for(uint32_t k = std::max(lo, phase); k < std::min(lo + 16, stop); ++k) row0[k] = sb[k];
    }
}

constexpr int kOomStatus = LRSC_ERR_DEVICE;                      // what DEV_TRY answers when device memory runs out

template <class Src>
static int rle_t(const Src& src, uint8_t** d_units, uint64_t* n_units, std::string& err)
{
    hipStream_t st = nullptr;
    *d_units = nullptr;
    *n_units = 0;
    const uint64_t n_tiles = (src.N + kRleTile - 1) / kRleTile;
    if(n_tiles == 0) return LRSC_OK;
    if(n_tiles >= (1ull << 31)) { err = "RL encoder: more than 2^31 tiles"; return LRSC_ERR_UNSUPPORTED; }
    const unsigned grid = (unsigned)n_tiles;
    Owned d;
    RunSummary *d_sum = nullptr, *d_incl = nullptr;
    uint64_t* d_cnt = nullptr;
    DEV_TRY(d.alloc(&d_sum, n_tiles));
    DEV_TRY(d.alloc(&d_incl, n_tiles));
    DEV_TRY(d.alloc(&d_cnt, n_tiles + 1));
    hipLaunchKernelGGL(rle_summary_kernel<Src>, dim3(grid), dim3(kRleLanes), 0, st, src, d_sum);
    DEV_TRY(hipGetLastError());
    size_t need_a = 0, need_b = 0;
    DEV_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, need_a, d_sum, d_incl, RleCombine{}, (int)n_tiles, st));
    DEV_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need_b, d_cnt, d_cnt, (int)(n_tiles + 1), st));
    uint8_t* d_tmp = nullptr;
    size_t need = std::max(need_a, need_b);
    DEV_TRY(d.alloc(&d_tmp, need));
    DEV_TRY(hipcub::DeviceScan::InclusiveScan(d_tmp, need, d_sum, d_incl, RleCombine{}, (int)n_tiles, st));
    // entry n_tiles is 0 and becomes the total in the scan
    DEV_TRY(hipMemsetAsync(d_cnt + n_tiles, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(rle_count_kernel<Src>, dim3(grid), dim3(kRleLanes), 0, st, src, d_incl, d_cnt);
    DEV_TRY(hipGetLastError());
    need = std::max(need_a, need_b);
    DEV_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, need, d_cnt, d_cnt, (int)(n_tiles + 1), st));
    uint64_t total = 0;
    DEV_TRY(hipMemcpy(&total, d_cnt + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if(total == 0 || total > src.N) { err = "RL encoder: unit count out of range"; return LRSC_ERR_DEVICE; }
    uint8_t* d_out = nullptr;
    DEV_TRY(d.alloc(&d_out, total));
    hipLaunchKernelGGL(rle_emit_kernel<Src>, dim3(grid), dim3(kRleLanes), 0, st, src, d_incl, d_cnt, d_out);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipDeviceSynchronize());
    d.keep(d_out);
    *d_units = d_out;
    *n_units = total;
    return LRSC_OK;
}

int rle_bwt_device(const uint8_t* d_bwt, uint64_t N, uint8_t** d_units, uint64_t* n_units, std::string& err)
{
    return rle_t(SrcBytes{d_bwt, N}, d_units, n_units, err);
}

template <class Block>
static int rle_strand_t(const FmStrand& s, uint8_t** d_units, uint64_t* n_units, std::string& err)
{
    if(s.n_blocks != s.n_symbols / Block::kSyms + 1) { err = "RL encoder: block count does not fit the symbol count"; return LRSC_ERR_ARG; }
    return rle_t(SrcBlocks<Block>{static_cast<const Block*>(s.blocks), s.dollars, s.dollar_dir, s.n_dollars, s.n_blocks, s.n_symbols}, d_units,
                 n_units, err);
}

int rle_strand_device(const FmStrand& strand, bool wide, uint8_t** d_units, uint64_t* n_units, std::string& err)
{
    return wide ? rle_strand_t<Block64>(strand, d_units, n_units, err) : rle_strand_t<Block32>(strand, d_units, n_units, err);
}

} // namespace lrsc
