// fm_unrle.hip -- packs the RL units of a saved index (the .bwt/.rbwt payload, one byte per run) into the rank-block image of
// fm_device.h on the device: what build_strand_image (fm_layout.cpp) makes of the same units on one host thread, byte for
// byte, without the byte-per-symbol BWT in between.
//
//   1. unrle_tile_kernel   per unit tile: symbols per code, symbols in all, first invalid unit      (reads the units once)
//   2. hipCUB ExclusiveSum over the unit tiles, one per code and one for the positions: where every unit tile starts, the
//      totals in entry n_tiles; hipCUB Min over the invalid-unit indexes.  The host looks at the totals here and launches
//      nothing more unless every unit is valid and the runs add up to N.
//   3. unrle_pack_kernel   per symbol tile of kUnrleBlocks rank blocks: seek, expand, pack, '$' list and directory
//                          (reads the units once more, writes n_blocks x 64 bytes)
//
// The pack kernel's workgroup finds the unit tile that holds its first symbol by a binary search of the scanned positions and
// loads it as its first chunk: kUnrleLanes lanes x 16 units in LDS, the lanes' run sums scanned into `starts`.  The counts
// before the symbol tile are the unit tile's plus what units16_before finds ahead of the first symbol.  Then, chunk after
// chunk, every lane takes Sym16 pieces of the tile that the chunk covers completely, finds each piece's first unit through
// `starts` and writes the piece whole (expand_sym16).  The next chunk begins at the lane that holds the first symbol not yet
// written, so a piece never has to be put together from two chunks.  With the rows filled the kernel is the packer's
// (block_hist, a workgroup scan, pack_block, the blocks out through LDS); the thread of a block also writes that block's '$'
// positions and, for the first block of a group, the directory entry.  No atomics anywhere.
#include <hipcub/hipcub.hpp>

#include "fm_launch.h"
#include "fm_unrle.h"

namespace lrsc {

static_assert(kUnrleBlocks == kPackThreads, "the symbol tile is the packer's");
static_assert(kUnrleBlocks <= kUnrleLanes, "one thread per rank block");
// a chunk that is not the stream's last holds (kUnrleLanes - 1) x 16 symbols or more after its first lane: more than the 15
// that may stay unwritten, so the next chunk begins at a later lane
static_assert(kUnrleLanes >= 2, "the chunks advance");

constexpr uint32_t kNoBad = 0xFFFFFFFFu;
constexpr uint64_t kNoBad64 = ~0ull;

// units [first, first + 16) of the stream, n of which exist; the others read as 0
__device__ __forceinline__ Sym16 load_units16(const uint8_t* __restrict__ units, uint64_t n_units, uint64_t first, uint32_t& n)
{
    Sym16 v{{0u, 0u, 0u, 0u}};
    n = first >= n_units ? 0u : (uint32_t)std::min<uint64_t>(n_units - first, 16);
    if(n == 16) v = *reinterpret_cast<const Sym16*>(units + first);
    else {
#pragma unroll
        for(uint32_t i = 0; i < 16; ++i)
            if(i < n) v.w[i >> 2] |= (uint32_t)units[first + i] << (8 * (i & 3));
    }
    return v;
}

struct SumsJoin {
    __device__ __forceinline__ UnitSums operator()(const UnitSums& a, const UnitSums& b) const
    {
        UnitSums r;
#pragma unroll
        for(uint32_t k = 0; k < 5; ++k) r.c[k] = a.c[k] + b.c[k];
        r.bad = a.bad < b.bad ? a.bad : b.bad;
        return r;
    }
};
struct Cnt5 {
    uint32_t c[5];
};
struct Cnt5Add {
    __device__ __forceinline__ Cnt5 operator()(const Cnt5& a, const Cnt5& b) const
    {
        Cnt5 r;
#pragma unroll
        for(uint32_t k = 0; k < 5; ++k) r.c[k] = a.c[k] + b.c[k];
        return r;
    }
};

using SumsReduce = hipcub::BlockReduce<UnitSums, kUnrleLanes>;
using RunScan = hipcub::BlockScan<uint32_t, kUnrleLanes>;
using Cnt5Reduce = hipcub::BlockReduce<Cnt5, kUnrleLanes>;
using CntScan = hipcub::BlockScan<uint64_t, kUnrleLanes>;

// sums: six arrays of n_tiles + 1 entries (A,C,G,T,'$', all symbols); entry n_tiles is 0 and becomes the total in the scan.
// bad[t]: index in the stream of the tile's first invalid unit, or kNoBad64.
__global__ __launch_bounds__(kUnrleLanes) void unrle_tile_kernel(const uint8_t* __restrict__ units, uint64_t n_units, uint64_t n_tiles,
                                                                 uint64_t* __restrict__ sums, uint64_t* __restrict__ bad)
{
    __shared__ typename SumsReduce::TempStorage tmp;
    const uint64_t tile = blockIdx.x;
    uint32_t n;
    const Sym16 v = load_units16(units, n_units, tile * kUnrleTile + 16ull * threadIdx.x, n);
    UnitSums mine = units16_sums(v, n);
    mine.bad = mine.bad == kUnrleNone ? kNoBad : 16 * threadIdx.x + mine.bad;
    const UnitSums all = SumsReduce(tmp).Reduce(mine, SumsJoin{});
    if(threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for(uint32_t k = 0; k < 5; ++k) {
            sums[k * (n_tiles + 1) + tile] = all.c[k];
            total += all.c[k];
        }
        sums[5 * (n_tiles + 1) + tile] = total;
        bad[tile] = all.bad == kNoBad ? kNoBad64 : tile * kUnrleTile + all.bad;
    }
}

// Wavefronts per SIMD that the pack kernel's LDS lets a CU hold (160 KiB, four wavefronts per workgroup, four SIMDs): the
// register allocator is held to the same number, so that LDS stays the limit.
template <class Block> struct UnrleOcc;
template <> struct UnrleOcc<Block32> { static constexpr uint32_t kWaves = 4; };
template <> struct UnrleOcc<Block64> { static constexpr uint32_t kWaves = 6; };

// scan: the exclusive sums of the tile kernel's six arrays.  Every unit is valid, scan[5][n_tiles] = N and scan[4][n_tiles] =
// n_dollars: the host has seen to that.  out has n_blocks = N / kSyms + 1 blocks, dir has n_dir entries.
template <class Block>
__global__ __launch_bounds__(kUnrleLanes, UnrleOcc<Block>::kWaves) void unrle_pack_kernel(const uint8_t* __restrict__ units, uint64_t n_units, uint64_t N, uint64_t n_blocks,
                                                                 uint64_t n_tiles, const uint64_t* __restrict__ scan, uint64_t n_dollars,
                                                                 Block* __restrict__ out, uint64_t* __restrict__ dollars,
                                                                 uint32_t* __restrict__ dir, uint64_t n_dir)
{
    using Tile = PackTile<Block>;
    constexpr uint32_t kTileSyms = kUnrleBlocks * Block::kSyms;
    __shared__ Sym16 rows[kUnrleBlocks * Tile::kRow];
    __shared__ Sym16 chunk[kUnrleLanes];
    __shared__ uint32_t starts[kUnrleLanes + 1];
    __shared__ uint64_t seed[5];                                   // A,C,G,T,'$' before the tile's first symbol
    __shared__ union {
        typename RunScan::TempStorage run;
        typename Cnt5Reduce::TempStorage red;
        typename CntScan::TempStorage cnt;
    } tmp;
    const uint32_t lane = threadIdx.x;
    const uint64_t n1 = n_tiles + 1;
    const uint64_t first = (uint64_t)blockIdx.x * kUnrleBlocks;    // < n_blocks: first * kSyms <= N
    const uint64_t p = first * Block::kSyms;
    const uint32_t n_syms = (uint32_t)std::min<uint64_t>(N - p, kTileSyms);
    const uint32_t n_q = (n_syms + 15) / 16;

    if(n_syms == 0) {                                              // the terminal block alone: everything lies before it
        if(lane < 5) seed[lane] = scan[lane * n1 + n_tiles];
    } else {
        const uint64_t* pos = scan + 5 * n1;
        const uint64_t t = unrle_seek_tile(pos, n_tiles, p);
        uint64_t cb = t * kUnrleTile;                              // the chunk's first unit, and the position of that unit's first symbol
        uint64_t cpos = pos[t];
        uint32_t q_done = 0;
        for(bool seek = true;; seek = false) {
            uint32_t n;
            const Sym16 v = load_units16(units, n_units, cb + 16ull * lane, n);
            chunk[lane] = v;
            uint32_t before, total;
            RunScan(tmp.run).ExclusiveSum(units16_total(v, n), before, total);
            starts[lane] = before;
            if(lane == 0) starts[kUnrleLanes] = total;
            __syncthreads();
            if(seek) {
                Cnt5 c;
                units16_before(v, n, before, (uint32_t)(p - cpos), c.c);
                const Cnt5 all = Cnt5Reduce(tmp.red).Reduce(c, Cnt5Add{});
                if(lane == 0) {
#pragma unroll
                    for(uint32_t k = 0; k < 5; ++k) seed[k] = scan[k * n1 + t] + all.c[k];
                }
            }
            // pieces that this chunk and the ones before it cover whole; the tile's last piece may be a short one
            const uint64_t cover = cpos + total - p;
            const uint32_t q_end = cover >= n_syms ? n_q : (uint32_t)(cover >> 4);
            for(uint32_t q = q_done + lane; q < q_end; q += kUnrleLanes) {
                const uint32_t x = (uint32_t)(p + 16ull * q - cpos);
                rows[(q / Tile::kChunks) * Tile::kRow + q % Tile::kChunks] =
                    expand_sym16(reinterpret_cast<const uint8_t*>(chunk), starts, kUnrleLanes, x, std::min(16u, n_syms - 16 * q));
            }
            q_done = q_end;
            if(q_done == n_q) break;
            const uint32_t l = unrle_find_lane(starts, kUnrleLanes, (uint32_t)(p + 16ull * q_done - cpos));
            if(l == 0) break;                                      // not with valid units (see the static_assert): never turn in place
            cb += 16ull * l;
            cpos += starts[l];
            __syncthreads();                                       // every lane is done with the chunk before the next one replaces it
        }
    }
    __syncthreads();

    // From here on the packer, one thread per rank block.  The block is packed ahead of the scan with nothing before it, and
    // the scanned counts are added to its counters afterwards (they stay below the '$' flag's bit): its row is read once,
    // and only the finished planes stay in registers across the scan.
    using CountT = decltype(Block::cnt[0] + 0);
    const uint64_t b = first + lane;
    const bool mine = lane < kUnrleBlocks && b < n_blocks;
    const Sym16* row = rows + (lane < kUnrleBlocks ? lane : 0u) * Tile::kRow;
    uint32_t n_valid = 0;
    uint32_t h[5] = {0, 0, 0, 0, 0};
    Block blk{};
    if(mine) {
        const uint64_t left = N - b * Block::kSyms;
        const uint64_t none[4] = {0, 0, 0, 0};
        n_valid = (uint32_t)(left < Block::kSyms ? left : Block::kSyms);
        block_hist<Block>(row, n_valid, h);
        blk = pack_block<Block>(row, n_valid, none);
    }
    // a tile holds fewer than 2^16 symbols: the four base counts share one 64-bit scan, 16 bits each
    static_assert(kTileSyms < (1u << 16), "packed counts");
    uint64_t ex_acgt;
    uint32_t ex_dollar;
    CntScan(tmp.cnt).ExclusiveSum((uint64_t)h[0] | (uint64_t)h[1] << 16 | (uint64_t)h[2] << 32 | (uint64_t)h[3] << 48, ex_acgt);
    __syncthreads();
    RunScan(tmp.run).ExclusiveSum(h[4], ex_dollar);
    if(mine) {
#pragma unroll
        for(uint32_t k = 0; k < 4; ++k) blk.cnt[k] += (CountT)(seed[k] + ((ex_acgt >> (16 * k)) & 0xFFFFu));
        uint64_t d = seed[4] + ex_dollar;                          // '$' rows before this block
        if((b & ((1u << kDollarDirShift) - 1)) == 0) dir[b >> kDollarDirShift] = (uint32_t)d;
        if(h[4]) {
#pragma unroll 1
            for(uint32_t wi = 0; wi < Block::kWords; ++wi)
                for(uint32_t m = sym_bits32(row, wi, n_valid).dollar; m; m &= m - 1, ++d)
                    if(d < n_dollars) dollars[d] = b * Block::kSyms + 32 * wi + (uint32_t)__builtin_ctz(m);
        }
        // the groups that begin at or beyond n_blocks hold the total (dollar_dir_entry)
        if(b == n_blocks - 1)
            for(uint64_t g = (b >> kDollarDirShift) + 1; g < n_dir; ++g) dir[g] = (uint32_t)n_dollars;
    }
    Sym16 piece[4];
    __builtin_memcpy(piece, &blk, sizeof(Block));
    __syncthreads();                                               // every row has been read: the finished blocks take their place
    if(lane < kUnrleBlocks) {
#pragma unroll
        for(uint32_t j = 0; j < 4; ++j) rows[lane * Tile::kOutRow + j] = piece[j];
    }
    __syncthreads();
    Sym16* dst = reinterpret_cast<Sym16*>(out + first);
    for(uint32_t q = lane; q < kUnrleBlocks * 4; q += kUnrleLanes)
        if(first + (q >> 2) < n_blocks) dst[q] = rows[(q >> 2) * Tile::kOutRow + (q & 3)];
}

constexpr int kOomStatus = LRSC_ERR_DEVICE;                      // what DEV_TRY answers when device memory runs out

template <class Block>
static int unrle_t(const uint8_t* d_units, uint64_t n_units, uint64_t N, PackedStrand& out, uint64_t* first_bad, std::string& err)
{
    hipStream_t st = nullptr;
    if(first_bad) *first_bad = kNoBad64;
    if(N == 0) { err = "RL decoder: no symbols"; return LRSC_ERR_ARG; }
    if(n_units == 0) { err = "BWT runs do not add up to the symbol count in the header"; return LRSC_ERR_FORMAT; }
    const uint64_t n_blocks = N / Block::kSyms + 1;
    if(n_blocks + 1 >= (1ull << 31)) { err = "index packer: more than 2^31 rank blocks"; return LRSC_ERR_UNSUPPORTED; }
    const uint64_t n_tiles = (n_units + kUnrleTile - 1) / kUnrleTile;
    const uint64_t n1 = n_tiles + 1;
    if(n1 >= (1ull << 31)) { err = "RL decoder: more than 2^31 unit tiles"; return LRSC_ERR_UNSUPPORTED; }
    Owned d;
    uint64_t *d_scan = nullptr, *d_bad = nullptr, *d_first = nullptr;
    DEV_TRY(d.alloc(&d_scan, 6 * n1));
    DEV_TRY(d.alloc(&d_bad, n_tiles));
    DEV_TRY(d.alloc(&d_first, 1));
    for(uint32_t k = 0; k < 6; ++k) DEV_TRY(hipMemsetAsync(d_scan + k * n1 + n_tiles, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(unrle_tile_kernel, dim3((unsigned)n_tiles), dim3(kUnrleLanes), 0, st, d_units, n_units, n_tiles, d_scan, d_bad);
    DEV_TRY(hipGetLastError());
    size_t need_a = 0, need_b = 0;
    DEV_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need_a, d_scan, d_scan, (int)n1, st));
    DEV_TRY(hipcub::DeviceReduce::Min(nullptr, need_b, d_bad, d_first, (int)n_tiles, st));
    uint8_t* d_tmp = nullptr;
    DEV_TRY(d.alloc(&d_tmp, std::max(need_a, need_b)));
    for(uint32_t k = 0; k < 6; ++k) {
        size_t need = need_a;
        DEV_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, need, d_scan + k * n1, d_scan + k * n1, (int)n1, st));
    }
    DEV_TRY(hipcub::DeviceReduce::Min(d_tmp, need_b, d_bad, d_first, (int)n_tiles, st));
    uint64_t tot[6], bad = kNoBad64;
    for(uint32_t k = 0; k < 6; ++k) DEV_TRY(hipMemcpy(&tot[k], d_scan + k * n1 + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost));
    DEV_TRY(hipMemcpy(&bad, d_first, sizeof(uint64_t), hipMemcpyDeviceToHost));
    // build_strand_image's checks and texts; past them every position that the pack kernel forms lies inside its array
    if(first_bad) *first_bad = bad;
    if(bad != kNoBad64) { err = "corrupt RL unit in BWT"; return LRSC_ERR_FORMAT; }
    if(tot[5] > N) { err = "BWT runs exceed the symbol count in the header"; return LRSC_ERR_FORMAT; }
    if(tot[5] < N) { err = "BWT runs do not add up to the symbol count in the header"; return LRSC_ERR_FORMAT; }
    if(tot[4] >= (1ull << 32)) { err = "more than 2^32 reads"; return LRSC_ERR_UNSUPPORTED; }

    const uint64_t n_dir = (n_blocks >> kDollarDirShift) + 2;
    Block* d_blocks = nullptr;
    uint64_t* d_dollars = nullptr;
    uint32_t* d_dir = nullptr;
    DEV_TRY(d.alloc(&d_blocks, n_blocks));
    DEV_TRY(d.alloc(&d_dollars, tot[4]));
    DEV_TRY(d.alloc(&d_dir, n_dir));
    const unsigned grid = (unsigned)((n_blocks + kUnrleBlocks - 1) / kUnrleBlocks);
    hipLaunchKernelGGL(unrle_pack_kernel<Block>, dim3(grid), dim3(kUnrleLanes), 0, st, d_units, n_units, N, n_blocks, n_tiles, d_scan, tot[4],
                       d_blocks, d_dollars, d_dir, n_dir);
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

int pack_units_device(const uint8_t* d_units, uint64_t n_units, uint64_t N, bool wide, PackedStrand& out, uint64_t* first_bad,
                      std::string& err)
{
    if(!wide) {
        if(N >= (1ull << 31)) { err = "Block32 layout needs < 2^31 symbols"; return LRSC_ERR_ARG; }
        return unrle_t<Block32>(d_units, n_units, N, out, first_bad, err);
    }
    return unrle_t<Block64>(d_units, n_units, N, out, first_bad, err);
}

} // namespace lrsc
