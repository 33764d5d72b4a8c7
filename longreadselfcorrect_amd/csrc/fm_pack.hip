// fm_pack.hip -- packs a device-resident BWT (one code per byte, as bwt_build.hip leaves it) into the rank-block image of
// fm_device.h without a host round trip: what build_strand_image (fm_layout.cpp) makes from the RL units of the same BWT,
// byte for byte.
//
//   1. pack_hist_kernel    per block: A,C,G,T and '$' among its symbols          (reads N bytes)
//   2. hipCUB ExclusiveSum over the blocks, one per symbol: the counts before every block; entry n_blocks holds the totals
//   3. pack_blocks_kernel  per block: counts + '$' flag + the two bit planes      (reads N bytes, writes n_blocks x 64)
//   4. hipCUB Select::If over the positions: the sorted '$' list (a stable compaction keeps position order)
//   5. dollar_dir_kernel   '$' rows before every group of blocks, from the scanned '$' counts
//
// Both streaming kernels move the symbols of kPackThreads blocks through LDS: the workgroup loads them with one 16-byte access per
// lane (consecutive lanes, consecutive addresses), then every thread packs the block of its own LDS row with the functions
// of fm_pack.h.  pack_blocks_kernel sends the finished blocks back through LDS so that they leave as full 16-byte-per-lane
// stores as well, every 64-byte block written once.  No atomics anywhere.
#include <hipcub/hipcub.hpp>

#include "fm_launch.h"
#include "fm_pack.h"

namespace lrsc {

// symbols of blocks [first_block, first_block + kPackThreads) -> rows; bytes at and beyond N read as 0
template <class Block>
__device__ __forceinline__ void stage_tile(const uint8_t* __restrict__ bwt, uint64_t N, uint64_t first_block, Sym16* rows)
{
    constexpr uint32_t kChunks = PackTile<Block>::kChunks;
    const uint64_t base = first_block * Block::kSyms;
    for(uint32_t q = threadIdx.x; q < kPackThreads * kChunks; q += kPackThreads) {
        const uint64_t p = base + 16ull * q;
        Sym16 v{{0u, 0u, 0u, 0u}};
        if(p + 16 <= N) v = *reinterpret_cast<const Sym16*>(bwt + p);
        else if(p < N) {
#pragma unroll
            for(uint32_t i = 0; i < 16; ++i)
                if(p + i < N) v.w[i >> 2] |= (uint32_t)bwt[p + i] << (8 * (i & 3));
        }
        rows[(q / kChunks) * PackTile<Block>::kRow + q % kChunks] = v;
    }
    __syncthreads();
}

// cnt: five arrays (A,C,G,T,'$') of n_blocks + 1 entries; entry n_blocks is 0 and becomes the total in the scan
template <class Block>
__global__ __launch_bounds__(kPackThreads) void pack_hist_kernel(const uint8_t* __restrict__ bwt, uint64_t N, uint64_t n_blocks,
                                                                 uint64_t* __restrict__ cnt)
{
    __shared__ Sym16 rows[kPackThreads * PackTile<Block>::kRow];
    const uint64_t first = (uint64_t)blockIdx.x * kPackThreads;
    stage_tile<Block>(bwt, N, first, rows);
    const uint64_t b = first + threadIdx.x;
    if(b > n_blocks) return;
    uint32_t c[5] = {0, 0, 0, 0, 0};
    if(b < n_blocks) {
        const uint64_t left = N - b * Block::kSyms;
        block_hist<Block>(rows + threadIdx.x * PackTile<Block>::kRow, (uint32_t)(left < Block::kSyms ? left : Block::kSyms), c);
    }
#pragma unroll
    for(uint32_t k = 0; k < 5; ++k) cnt[k * (n_blocks + 1) + b] = c[k];
}

template <class Block>
__global__ __launch_bounds__(kPackThreads) void pack_blocks_kernel(const uint8_t* __restrict__ bwt, uint64_t N, uint64_t n_blocks,
                                                                   const uint64_t* __restrict__ before, Block* __restrict__ out)
{
    __shared__ Sym16 rows[kPackThreads * PackTile<Block>::kRow];
    const uint64_t first = (uint64_t)blockIdx.x * kPackThreads;
    stage_tile<Block>(bwt, N, first, rows);
    const uint64_t b = first + threadIdx.x;
    Sym16 piece[4] = {};
    if(b < n_blocks) {
        uint64_t bef[4];
#pragma unroll
        for(uint32_t k = 0; k < 4; ++k) bef[k] = before[k * (n_blocks + 1) + b];
        const uint64_t left = N - b * Block::kSyms;
        const Block blk = pack_block<Block>(rows + threadIdx.x * PackTile<Block>::kRow, (uint32_t)(left < Block::kSyms ? left : Block::kSyms), bef);
        __builtin_memcpy(piece, &blk, sizeof(Block));
    }
    __syncthreads();                                   // every row has been read: the finished blocks take their place
#pragma unroll
    for(uint32_t j = 0; j < 4; ++j) rows[threadIdx.x * PackTile<Block>::kOutRow + j] = piece[j];
    __syncthreads();
    Sym16* dst = reinterpret_cast<Sym16*>(out + first);
    for(uint32_t q = threadIdx.x; q < kPackThreads * 4; q += kPackThreads)
        if(first + (q >> 2) < n_blocks) dst[q] = rows[(q >> 2) * PackTile<Block>::kOutRow + (q & 3)];
}

__global__ __launch_bounds__(256) void dollar_dir_kernel(const uint64_t* __restrict__ dollars_before, uint64_t n_blocks, uint64_t n_dir,
                                                         uint32_t* __restrict__ dir)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if(g < n_dir) dir[g] = dollar_dir_entry(dollars_before, n_blocks, g);
}

struct IsDollar {
    const uint8_t* bwt;
    __host__ __device__ __forceinline__ bool operator()(const uint64_t& pos) const { return bwt[pos] == 0; }
};

constexpr int kOomStatus = LRSC_ERR_DEVICE;                      // what DEV_TRY answers when device memory runs out

template <class Block>
static int pack_strand_t(const uint8_t* d_bwt, uint64_t N, PackedStrand& out, std::string& err)
{
    hipStream_t st = nullptr;
    const uint64_t n_blocks = N / Block::kSyms + 1;
    const uint64_t n1 = n_blocks + 1;
    if(n1 >= (1ull << 31)) { err = "index packer: more than 2^31 rank blocks"; return LRSC_ERR_UNSUPPORTED; }
    const unsigned tiles = (unsigned)((n1 + kPackThreads - 1) / kPackThreads);
    Owned d;
    uint64_t* d_cnt = nullptr;
    DEV_TRY(d.alloc(&d_cnt, 5 * n1));
    hipLaunchKernelGGL(pack_hist_kernel<Block>, dim3(tiles), dim3(kPackThreads), 0, st, d_bwt, N, n_blocks, d_cnt);
    DEV_TRY(hipGetLastError());
    size_t need = 0;
    DEV_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, d_cnt, d_cnt, (int)n1, st));
    uint8_t* d_tmp = nullptr;
    DEV_TRY(d.alloc(&d_tmp, need));
    for(uint32_t k = 0; k < 5; ++k) DEV_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, need, d_cnt + k * n1, d_cnt + k * n1, (int)n1, st));
    uint64_t tot[5];
    for(uint32_t k = 0; k < 5; ++k) DEV_TRY(hipMemcpy(&tot[k], d_cnt + k * n1 + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if(tot[4] >= (1ull << 32)) { err = "more than 2^32 reads"; return LRSC_ERR_UNSUPPORTED; }
    if(tot[0] + tot[1] + tot[2] + tot[3] + tot[4] != N) { err = "index packer: a BWT code outside $ACGT"; return LRSC_ERR_DEVICE; }

    Block* d_blocks = nullptr;
    DEV_TRY(d.alloc(&d_blocks, n_blocks));
    hipLaunchKernelGGL(pack_blocks_kernel<Block>, dim3(tiles), dim3(kPackThreads), 0, st, d_bwt, N, n_blocks, d_cnt, d_blocks);
    DEV_TRY(hipGetLastError());

    // the '$' rows in position order, 2^30 positions per call (hipCUB counts in int)
    uint64_t* d_dollars = nullptr;
    uint64_t* d_nsel = nullptr;
    DEV_TRY(d.alloc(&d_dollars, tot[4]));
    DEV_TRY(d.alloc(&d_nsel, 1));
    const uint64_t chunk = 1ull << 30;
    uint8_t* d_sel_tmp = nullptr;
    DEV_TRY(hipcub::DeviceSelect::If(nullptr, need, hipcub::CountingInputIterator<uint64_t>(0), d_dollars, d_nsel, (int)std::min(chunk, N), IsDollar{d_bwt}, st));
    DEV_TRY(d.alloc(&d_sel_tmp, need));
    uint64_t got = 0;
    for(uint64_t base = 0; base < N; base += chunk) {
        size_t n2 = need;
        DEV_TRY(hipcub::DeviceSelect::If(d_sel_tmp, n2, hipcub::CountingInputIterator<uint64_t>(base), d_dollars + got, d_nsel,
                                        (int)std::min(chunk, N - base), IsDollar{d_bwt}, st));
        uint64_t n_sel = 0;
        DEV_TRY(hipMemcpy(&n_sel, d_nsel, sizeof(uint64_t), hipMemcpyDeviceToHost));
        got += n_sel;
        if(got > tot[4]) break;
    }
    if(got != tot[4]) { err = "index packer: '$' list and '$' counts disagree"; return LRSC_ERR_DEVICE; }

    const uint64_t n_dir = (n_blocks >> kDollarDirShift) + 2;
    uint32_t* d_dir = nullptr;
    DEV_TRY(d.alloc(&d_dir, n_dir));
    hipLaunchKernelGGL(dollar_dir_kernel, dim3((unsigned)((n_dir + 255) / 256)), dim3(256), 0, st, d_cnt + 4 * n1, n_blocks, n_dir, d_dir);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipDeviceSynchronize());

    d.keep(d_blocks); d.keep(d_dollars); d.keep(d_dir);
    out.blocks = d_blocks;
    out.dollars = d_dollars;
    out.dollar_dir = d_dir;
    out.n_blocks = n_blocks;
    out.n_dollars = tot[4];
    out.n_dir = n_dir;
    out.pred[0] = 0;
    out.pred[1] = tot[4];
    out.pred[2] = out.pred[1] + tot[0];
    out.pred[3] = out.pred[2] + tot[1];
    out.pred[4] = out.pred[3] + tot[2];
    return LRSC_OK;
}

int pack_strand_device(const uint8_t* d_bwt, uint64_t N, bool wide, PackedStrand& out, std::string& err)
{
    if(!wide) {
        if(N >= (1ull << 31)) { err = "Block32 layout needs < 2^31 symbols"; return LRSC_ERR_ARG; }
        return pack_strand_t<Block32>(d_bwt, N, out, err);
    }
    return pack_strand_t<Block64>(d_bwt, N, out, err);
}

} // namespace lrsc
