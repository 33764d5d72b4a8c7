// fm_remove.hip -- takes reads out of an index copy that lies on the device: the byte-per-symbol BWT of the kept reads, which
// fm_pack.hip then packs as it packs a sorted or a merged BWT.  The arithmetic is fm_remove.h's.
//
//   1. remove_mark_kernel<WIDE>      one lane per dropped read: the backward walk from the read's sentinel row to its '$' row, a
//                                    bit per visited row (32-bit atomic OR: the rows of one word belong to different walks).  A step
//                                    is one 64-byte load and popcounts against the layout's mask table in LDS.  The chain is
//                                    latency-bound: the kernel is held to the registers of kRemoveWalkWavesPerSimd wavefronts per
//                                    SIMD.  One very long read is one lane's chain.
//   2. remove_count_kernel           one wavefront per tile of kRemoveTile rows: the rows whose bit is clear; a hipCUB exclusive
//                                    scan turns the counts into the tiles' offsets in the output
//   3. remove_compact_kernel<WIDE>   per tile: its rank blocks go to LDS decoded, one lane per block; every lane copies the kept
//                                    ones of its 16 rows to the stage at the workgroup prefix sum of the kept counts; the stage
//                                    leaves with 16-byte stores where the tile owns the whole chunk
#include <hipcub/hipcub.hpp>

#include <chrono>

#include "fm_launch.h"
#include "fm_remove.h"

namespace lrsc {

struct RemoveAtomicMark {
    uint32_t* bitmap;
    __device__ __forceinline__ void operator()(uint64_t row) const { atomicOr(bitmap + (row >> 5), 1u << (uint32_t)(row & 31u)); }
};

template <bool WIDE>
__global__ __launch_bounds__(kRemoveWalkThreads) __attribute__((amdgpu_waves_per_eu(kRemoveWalkWavesPerSimd, kRemoveWalkWavesPerSimd)))
void remove_mark_kernel(StrandView<typename BlockOf<WIDE>::type> S, const uint32_t* __restrict__ ids, uint64_t n_drop, uint32_t* __restrict__ bitmap,
                        unsigned long long* __restrict__ rows_total, uint32_t* __restrict__ broken)
{
    using B = typename BlockOf<WIDE>::type;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTab<B>::kWords];
    // The table's fill and the wavefront sum below are written in place, not with fm_launch.h's fill_mask_table and wave_sum: with
    // the helpers the kernel's instruction stream was not the one measured before (other register names, one operand order).
    for(uint32_t i = threadIdx.x; i < MaskTab<B>::kWords; i += blockDim.x) mtab[i] = mask_word<B>(i);
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kRemoveWalkThreads + threadIdx.x;
    uint64_t rows = 0;
    if(k < n_drop) {
        const uint32_t read = ids[k];
        if(read >= S.n_dollars || remove_mark_read<B>(S, mtab, read, RemoveAtomicMark{bitmap}, rows) != kWalkOk) *broken = 1u;
    }
    // rows of the wavefront's walks -> one atomic (every lane of the wavefront is here)
    unsigned long long total = rows;
#pragma unroll
    for(int o = 32; o > 0; o >>= 1) total += __shfl_down(total, o, 64);
    if((threadIdx.x & 63) == 0 && total) atomicAdd(rows_total, total);
}

// kept[t] = rows of tile t whose bit is clear, t in [0, n_tiles); kept[n_tiles] = 0
__global__ __launch_bounds__(256) void remove_count_kernel(const uint32_t* __restrict__ bitmap, uint64_t N, uint64_t n_tiles, uint64_t* __restrict__ kept)
{
    constexpr uint32_t kWords = kRemoveTile / 32, kPerLane = (kWords + 63) / 64;
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    uint32_t marked = 0;
    if(t < n_tiles) {
        const uint32_t w = lane * kPerLane;
        if(w < kWords) marked = remove_words_marked(bitmap, t * kWords + w, std::min(kPerLane, kWords - w));
    }
#pragma unroll
    for(int o = 32; o > 0; o >>= 1) marked += __shfl_down(marked, o, 64);
    if(lane == 0 && t <= n_tiles) kept[t] = t < n_tiles ? std::min<uint64_t>(kRemoveTile, N - t * kRemoveTile) - marked : 0;
}

template <bool WIDE>
__global__ __launch_bounds__(kRemoveLanes) void remove_compact_kernel(StrandView<typename BlockOf<WIDE>::type> S, const uint32_t* __restrict__ bitmap,
                                                                      const uint64_t* __restrict__ tile_off, uint8_t* __restrict__ out)
{
    using B = typename BlockOf<WIDE>::type;
    constexpr uint32_t kChunks = B::kSyms / 16, kWaves = kRemoveLanes / 64;
    __shared__ Sym16 sym[kRemoveTile / 16];
    __shared__ Sym16 stage[RemoveStage<kRemoveTile>::kRows];
    __shared__ uint32_t wave_total[kWaves];
    const uint64_t p0 = (uint64_t)blockIdx.x * kRemoveTile;
    const uint32_t n_valid = (uint32_t)std::min<uint64_t>(kRemoveTile, S.N - p0);
    const uint64_t off = tile_off[blockIdx.x];
    const uint64_t n_kept64 = tile_off[blockIdx.x + 1] - off;
    if(n_kept64 > n_valid) return;                                // never with offsets scanned from this bitmap
    const uint32_t n_kept = (uint32_t)n_kept64;
    if(n_kept == 0) return;
    const uint64_t first_block = p0 / B::kSyms;
    const uint32_t n_blk = (n_valid + B::kSyms - 1) / B::kSyms;
    for(uint32_t u = threadIdx.x; u < n_blk; u += kRemoveLanes) decode_block<B>(S, first_block + u, sym + u * kChunks);
    const uint32_t keep = remove_keep16(bitmap, p0, threadIdx.x, n_valid);
    const uint32_t cnt = (uint32_t)__builtin_popcount(keep);
    uint32_t incl = cnt;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for(int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        incl += lane >= (uint32_t)o ? v : 0u;
    }
    if(lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = incl - cnt;
#pragma unroll
    for(uint32_t w = 0; w < kWaves; ++w) before += w < wave ? wave_total[w] : 0u;
    const uint32_t shift = (uint32_t)(off & 15u);
    // before + cnt <= n_kept <= kRemoveTile by the offsets' construction; the check keeps a foreign bitmap inside the stage
    if(keep && before + cnt <= kRemoveTile) remove_scatter16(sym, threadIdx.x, keep, reinterpret_cast<uint8_t*>(stage) + shift + before);
    __syncthreads();
    uint8_t* out16 = out + (off - shift);
    for(uint32_t c = threadIdx.x; 16 * c < shift + n_kept; c += kRemoveLanes) remove_store_chunk(stage, shift, n_kept, c, out16);
}

constexpr int kOomStatus = LRSC_ERR_NOMEM;                       // what DEV_TRY answers when device memory runs out

template <bool WIDE>
static int remove_strand_t(const FmStrand& s, const uint32_t* ids, uint64_t n_drop, uint8_t** d_bwt_out, uint64_t* n_out, double ms[2], std::string& err)
{
    using B = typename BlockOf<WIDE>::type;
    using clk = std::chrono::steady_clock;
    hipStream_t st = nullptr;
    const uint64_t N = s.n_symbols;
    if(s.n_blocks != N / B::kSyms + 1) { err = "index remove: block count does not fit the symbol count"; return LRSC_ERR_FORMAT; }
    if(s.n_dollars == 0 || s.n_dollars > N || s.n_dollars >= (1ull << 32)) { err = "index remove: an index without reads, or with 2^32 or more"; return LRSC_ERR_UNSUPPORTED; }
    const uint64_t n_tiles = (N + kRemoveTile - 1) / kRemoveTile;
    const uint64_t walk_groups = (n_drop + kRemoveWalkThreads - 1) / kRemoveWalkThreads;
    if(n_tiles >= (1ull << 31) - 1 || walk_groups >= (1ull << 31)) { err = "index remove: more than 2^31 tiles"; return LRSC_ERR_UNSUPPORTED; }
    const StrandView<B> S = strand_view<B>(s);
    const uint64_t n_words = remove_bitmap_words(N, kRemoveTile);
    Owned d;
    uint32_t *d_bitmap = nullptr, *d_ids = nullptr, *d_broken = nullptr;
    unsigned long long* d_rows = nullptr;
    uint64_t* d_kept = nullptr;
    uint8_t *d_tmp = nullptr, *d_bwt = nullptr;
    DEV_TRY(d.alloc(&d_bitmap, n_words));
    DEV_TRY(d.alloc(&d_ids, n_drop));
    DEV_TRY(d.alloc(&d_broken, 1));
    DEV_TRY(d.alloc(&d_rows, 1));
    DEV_TRY(d.alloc(&d_kept, n_tiles + 1));
    DEV_TRY(hipMemsetAsync(d_bitmap, 0, n_words * sizeof(uint32_t), st));
    DEV_TRY(hipMemsetAsync(d_broken, 0, sizeof(uint32_t), st));
    DEV_TRY(hipMemsetAsync(d_rows, 0, sizeof(unsigned long long), st));
    if(n_drop) DEV_TRY(hipMemcpyAsync(d_ids, ids, n_drop * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    DEV_TRY(hipDeviceSynchronize());
    const auto t0 = clk::now();
    if(n_drop) {
        hipLaunchKernelGGL((remove_mark_kernel<WIDE>), dim3((unsigned)walk_groups), dim3(kRemoveWalkThreads), 0, st, S, d_ids, n_drop, d_bitmap, d_rows, d_broken);
        DEV_TRY(hipGetLastError());
    }
    uint32_t broken = 0;
    unsigned long long rows = 0;
    DEV_TRY(hipMemcpy(&broken, d_broken, sizeof(uint32_t), hipMemcpyDeviceToHost));
    DEV_TRY(hipMemcpy(&rows, d_rows, sizeof(rows), hipMemcpyDeviceToHost));
    const auto t1 = clk::now();
    if(broken) { err = "index remove: a backward walk from a sentinel row does not end at a '$' row (the index is no BWT of a string set)"; return LRSC_ERR_FORMAT; }
    hipLaunchKernelGGL(remove_count_kernel, dim3((unsigned)((n_tiles + 1 + 3) / 4)), dim3(256), 0, st, d_bitmap, N, n_tiles, d_kept);
    DEV_TRY(hipGetLastError());
    size_t need = 0;
    DEV_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, d_kept, d_kept, (int)(n_tiles + 1), st));
    DEV_TRY(d.alloc(&d_tmp, need));
    DEV_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, need, d_kept, d_kept, (int)(n_tiles + 1), st));
    uint64_t total = 0;
    DEV_TRY(hipMemcpy(&total, d_kept + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if(total > N || N - total != rows) {
        err = "index remove: the marked rows are not the rows of the dropped reads (walks of two reads met: the index is no BWT of a string set)";
        return LRSC_ERR_FORMAT;
    }
    if(total == 0) { err = "index remove: nothing is kept"; return LRSC_ERR_ARG; }
    const uint64_t cap = (total + 15) / 16 * 16;
    DEV_TRY(d.alloc(&d_bwt, cap));
    DEV_TRY(hipMemsetAsync(d_bwt + cap - 16, 0, 16, st));           // the packer reads whole 16-byte rows
    hipLaunchKernelGGL((remove_compact_kernel<WIDE>), dim3((unsigned)n_tiles), dim3(kRemoveLanes), 0, st, S, d_bitmap, d_kept, d_bwt);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipDeviceSynchronize());
    ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms[1] += std::chrono::duration<double, std::milli>(clk::now() - t1).count();
    d.keep(d_bwt);
    *d_bwt_out = d_bwt;
    *n_out = total;
    return LRSC_OK;
}

int remove_strand_device(const FmStrand& s, bool wide, const uint32_t* ids, uint64_t n_drop, uint8_t** d_bwt, uint64_t* n_out, double ms[2],
                         std::string& err)
{
    *d_bwt = nullptr;
    *n_out = 0;
    return wide ? remove_strand_t<true>(s, ids, n_drop, d_bwt, n_out, ms, err) : remove_strand_t<false>(s, ids, n_drop, d_bwt, n_out, ms, err);
}

} // namespace lrsc
