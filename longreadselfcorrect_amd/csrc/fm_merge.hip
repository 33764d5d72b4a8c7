// fm_merge.hip -- merges two index copies that lie on one device into the byte-per-symbol BWT of their union (A's reads
// followed by B's), which fm_pack.hip then packs as it packs a sorted BWT.  The arithmetic is fm_merge.h's.
//
//   1. merge_rank_kernel<WIDE_A, WIDE_B>   one lane per read of B: the backward walk through both indexes, rank[i] for every row
//                                          of B.  A step is two independent 64-byte loads (B's block of row i, A's block of
//                                          prefix r), both issued before either is used, then popcounts against the LDS mask
//                                          table of either layout.  The chain is latency-bound: the kernel is held to the
//                                          registers of kMergeWalkWavesPerSimd wavefronts per SIMD.
//   2. merge_tile_kernel                   one lane per tile edge: the first B row at or beyond it (binary search in j + rank[j])
//   3. merge_interleave_kernel<WA, WB>     per tile of kMergeTile merged positions: the tile's B positions (coalesced reads of
//                                          rank[]) and the rank blocks of both inputs that hold its rows go to LDS, one lane
//                                          decoding one block; then every lane fills 16 positions and stores them with one
//                                          16-byte access.  No atomics anywhere.
//   4. merge_origin_kernel                 one lane per '$' row of B: where it falls among the union's
#include <chrono>

#include "fm_launch.h"
#include "fm_merge.h"

namespace lrsc {

template <bool WIDE_A, bool WIDE_B>
__global__ __launch_bounds__(kMergeWalkThreads) __attribute__((amdgpu_waves_per_eu(kMergeWalkWavesPerSimd, kMergeWalkWavesPerSimd)))
void merge_rank_kernel(StrandView<typename BlockOf<WIDE_A>::type> A, StrandView<typename BlockOf<WIDE_B>::type> B, uint64_t n_reads_a,
                       uint64_t n_reads_b, uint64_t* __restrict__ rank)
{
    using BA = typename BlockOf<WIDE_A>::type;
    using BB = typename BlockOf<WIDE_B>::type;
    // one table serves both inputs when their layouts agree
    __shared__ __attribute__((aligned(16))) uint32_t mtab_b[MaskTab<BB>::kWords];
    __shared__ __attribute__((aligned(16))) uint32_t mtab_other[WIDE_A == WIDE_B ? 1 : MaskTab<BA>::kWords];
    fill_mask_table<BB>(mtab_b);
    if(WIDE_A != WIDE_B) fill_mask_table<BA>(mtab_other);
    __syncthreads();
    const uint32_t* mtab_a = WIDE_A == WIDE_B ? mtab_b : mtab_other;
    const uint64_t read = (uint64_t)blockIdx.x * kMergeWalkThreads + threadIdx.x;
    if(read >= n_reads_b) return;
    MergeWalk<BA, BB> w = merge_walk_start<BA, BB>(read, n_reads_a);
    // a read has fewer symbols than B has rows and never leaves either index: the bound and the range check only end the walk
    // through an index that is no BWT of a string set
    for(uint64_t step = 0; step < B.N; ++step) {
        if(w.i >= B.N || w.r > A.N) break;
        rank[w.i] = w.r;
        const BB bb = B.blocks[block_of<BB>(w.i)];
        const BA ba = A.blocks[block_of<BA>(w.r)];
        if(!merge_walk_step(A, B, ba, bb, mtab_a, mtab_b, w)) break;
    }
}

// tile_row[t] = first B row at or beyond merged position min(t * kMergeTile, N), t in [0, n_tiles]
__global__ __launch_bounds__(256) void merge_tile_kernel(const uint64_t* __restrict__ rank, uint64_t n_b, uint64_t N, uint64_t n_tiles,
                                                         uint64_t* __restrict__ tile_row)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if(t > n_tiles) return;
    tile_row[t] = merge_tile_search(rank, n_b, std::min<uint64_t>(t * kMergeTile, N));
}

template <bool WIDE_A, bool WIDE_B>
__global__ __launch_bounds__(kMergeLanes) void merge_interleave_kernel(StrandView<typename BlockOf<WIDE_A>::type> A,
                                                                       StrandView<typename BlockOf<WIDE_B>::type> B,
                                                                       const uint64_t* __restrict__ rank, const uint64_t* __restrict__ tile_row,
                                                                       uint8_t* __restrict__ out)
{
    using BA = typename BlockOf<WIDE_A>::type;
    using BB = typename BlockOf<WIDE_B>::type;
    using SA = MergeStage<BA, kMergeTile>;
    using SB = MergeStage<BB, kMergeTile>;
    __shared__ Sym16 sym_a[SA::kRows];
    __shared__ Sym16 sym_b[SB::kRows];
    __shared__ uint16_t pos_b[kMergeTile];
    const uint64_t N = A.N + B.N;
    const uint64_t p0 = (uint64_t)blockIdx.x * kMergeTile;
    const uint64_t p1 = std::min<uint64_t>(p0 + kMergeTile, N);
    const uint64_t j0 = tile_row[blockIdx.x], j1 = tile_row[blockIdx.x + 1];
    if(j0 > p0 || j1 < j0 || j1 - j0 > p1 - p0) return;         // never with rank[] of a walk: it is non-decreasing
    const uint32_t n_bt = (uint32_t)(j1 - j0);
    const MergeSpan span_a = merge_span<BA>(p0 - j0, p1 - j1);
    const MergeSpan span_b = merge_span<BB>(j0, j1);
    for(uint32_t k = threadIdx.x; k < n_bt; k += kMergeLanes) pos_b[k] = (uint16_t)(j0 + k + rank[j0 + k] - p0);
    for(uint32_t u = threadIdx.x; u < span_a.n_blocks + span_b.n_blocks; u += kMergeLanes) {
        if(u < span_a.n_blocks) decode_block<BA>(A, span_a.first_block + u, sym_a + u * SA::kChunks);
        else decode_block<BB>(B, span_b.first_block + (u - span_a.n_blocks), sym_b + (u - span_a.n_blocks) * SB::kChunks);
    }
    __syncthreads();
    const uint32_t q = threadIdx.x * 16;
    const uint32_t n_valid = (uint32_t)(p1 - p0);
    if(q < n_valid)                                               // out is whole 16-byte rows: the last one is written in full
        *reinterpret_cast<Sym16*>(out + p0 + q) = merge_fill16(pos_b, n_bt, sym_a, span_a.skip, sym_b, span_b.skip, q, n_valid);
}

__global__ __launch_bounds__(256) void merge_origin_kernel(const uint64_t* __restrict__ dollars_a, uint64_t n_a, const uint64_t* __restrict__ dollars_b,
                                                           uint64_t n_b, uint64_t rows_b, const uint64_t* __restrict__ rank, uint8_t* __restrict__ origin)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if(k >= n_b) return;
    const uint64_t d = dollars_b[k];
    if(d < rows_b) origin[merge_origin_slot(dollars_a, n_a, rank[d], k)] = 1;
}

constexpr int kOomStatus = LRSC_ERR_DEVICE;                      // what DEV_TRY answers when device memory runs out

template <bool WIDE_A, bool WIDE_B>
static int merge_strand_t(const FmStrand& a, const FmStrand& b, uint8_t** d_bwt_out, uint64_t** d_rank_out, double ms[2], std::string& err)
{
    using BA = typename BlockOf<WIDE_A>::type;
    using BB = typename BlockOf<WIDE_B>::type;
    using clk = std::chrono::steady_clock;
    hipStream_t st = nullptr;
    if(a.n_blocks != a.n_symbols / BA::kSyms + 1 || b.n_blocks != b.n_symbols / BB::kSyms + 1) {
        err = "index merge: block count does not fit the symbol count";
        return LRSC_ERR_ARG;
    }
    if(b.n_dollars == 0 || b.n_dollars > b.n_symbols) { err = "index merge: an index without reads"; return LRSC_ERR_ARG; }
    const uint64_t N = a.n_symbols + b.n_symbols;
    const uint64_t n_tiles = (N + kMergeTile - 1) / kMergeTile;
    const uint64_t walk_groups = (b.n_dollars + kMergeWalkThreads - 1) / kMergeWalkThreads;
    if(n_tiles >= (1ull << 31) || walk_groups >= (1ull << 31)) { err = "index merge: more than 2^31 tiles"; return LRSC_ERR_UNSUPPORTED; }
    const StrandView<BA> A = strand_view<BA>(a);
    const StrandView<BB> B = strand_view<BB>(b);
    Owned d;
    uint64_t *d_rank = nullptr, *d_tile = nullptr;
    uint8_t* d_bwt = nullptr;
    DEV_TRY(d.alloc(&d_rank, b.n_symbols));
    const auto t0 = clk::now();
    hipLaunchKernelGGL((merge_rank_kernel<WIDE_A, WIDE_B>), dim3((unsigned)walk_groups), dim3(kMergeWalkThreads), 0, st, A, B, a.n_dollars,
                       b.n_dollars, d_rank);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipDeviceSynchronize());
    const auto t1 = clk::now();
    DEV_TRY(d.alloc(&d_tile, n_tiles + 1));
    DEV_TRY(d.alloc(&d_bwt, (N + 15) / 16 * 16));
    hipLaunchKernelGGL(merge_tile_kernel, dim3((unsigned)((n_tiles + 256) / 256)), dim3(256), 0, st, d_rank, b.n_symbols, N, n_tiles, d_tile);
    DEV_TRY(hipGetLastError());
    hipLaunchKernelGGL((merge_interleave_kernel<WIDE_A, WIDE_B>), dim3((unsigned)n_tiles), dim3(kMergeLanes), 0, st, A, B, d_rank, d_tile, d_bwt);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipDeviceSynchronize());
    ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms[1] += std::chrono::duration<double, std::milli>(clk::now() - t1).count();
    d.keep(d_rank); d.keep(d_bwt);
    *d_rank_out = d_rank;
    *d_bwt_out = d_bwt;
    return LRSC_OK;
}

int merge_strand_device(const FmStrand& a, bool wide_a, const FmStrand& b, bool wide_b, uint8_t** d_bwt, uint64_t** d_rank, double ms[2],
                        std::string& err)
{
    *d_bwt = nullptr;
    *d_rank = nullptr;
    if(wide_a) return wide_b ? merge_strand_t<true, true>(a, b, d_bwt, d_rank, ms, err) : merge_strand_t<true, false>(a, b, d_bwt, d_rank, ms, err);
    return wide_b ? merge_strand_t<false, true>(a, b, d_bwt, d_rank, ms, err) : merge_strand_t<false, false>(a, b, d_bwt, d_rank, ms, err);
}

int merge_origin_device(const FmStrand& a, const FmStrand& b, const uint64_t* d_rank, uint8_t* origin, std::string& err)
{
    hipStream_t st = nullptr;
    const uint64_t n = a.n_dollars + b.n_dollars;
    Owned d;
    uint8_t* d_origin = nullptr;
    DEV_TRY(d.alloc(&d_origin, n));
    DEV_TRY(hipMemsetAsync(d_origin, 0, n, st));
    hipLaunchKernelGGL(merge_origin_kernel, dim3((unsigned)((b.n_dollars + 255) / 256)), dim3(256), 0, st, a.dollars, a.n_dollars, b.dollars, b.n_dollars,
                       b.n_symbols, d_rank, d_origin);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipMemcpy(origin, d_origin, n, hipMemcpyDeviceToHost));
    return LRSC_OK;
}

} // namespace lrsc
