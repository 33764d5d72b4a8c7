// fm_merge.h -- two FM-indexes -> the BWT of their union (A's reads followed by B's), the per-lane arithmetic of the device
// merge (fm_merge.hip).
//
// A strand of an index is the BWT of a string set whose sentinels sort in input order.  In the union every sentinel of A sorts
// before every sentinel of B, so of two equal suffixes A's comes first.  The merge needs one number per row of B: rank[j], how
// many suffixes of A are smaller than the suffix of B's row j.
//
//   walk        One lane per read b of B walks it backwards through both indexes: it starts at B row i = b (the suffix that is
//               the read's sentinel alone) with r = n_A (every sentinel of A is smaller, nothing else is), and while
//               c = BWT_B[i] is no '$' steps i <- C_B[c] + Occ_B(c, i), r <- C_A[c] + Occ_A(c, r).  Every row visited, the first
//               and the one that holds the '$' included, gets rank[i] = r.  The walks of all reads visit every row of B once.
//               BWT_B[i] and Occ_B(c, i) come from one rank block of B and Occ_A(c, r) from one of A, whichever c is: the caller
//               loads both before merge_walk_step looks at either.  B's side of the step is fm_strand.h's lf_step.
//   interleave  rank[] is non-decreasing in the row, so B row j lands at merged position j + rank[j], strictly increasing, and
//               A's rows fill the gaps in order.  A tile of merged positions [p0, p1) finds its first B row by a binary search
//               of p0 in j + rank[j] (merge_tile_search): rows [j0, j1) of B and [p0 - j0, p1 - j1) of A make the tile.  Both
//               are decoded from their rank blocks with decode_block, and every lane fills 16 consecutive positions
//               (merge_fill16) from the two decoded stretches and the tile's list of B positions.
//   origin      B's k-th '$' row, row d of B, is preceded in the union by B's k earlier ones and by the '$' rows of A that lie
//               among A's first rank[d] rows (merge_origin_slot).
//
// All functions here are LRSC_HD and free of HIP types: the kernels call them, and tests/host_tools/merge_driver.cpp compiles
// the same source for the CPU and holds it against a suffix sort of the union.
#pragma once
#include <stdint.h>

#include <string>

#include "fm_strand.h"

namespace lrsc {

constexpr uint32_t kMergeWalkThreads = 128;                       // lanes, one read of B each, per workgroup of the walk
// Wavefronts per SIMD that the walk's launch is sized for: the chain of dependent block loads is latency-bound, so the kernel
// has to stay within 512 / kMergeWalkWavesPerSimd VGPRs (two 64-byte blocks in flight are 32 of them).
constexpr uint32_t kMergeWalkWavesPerSimd = 8;
constexpr uint32_t kMergeLanes = 256;                             // threads per interleave tile, 16 merged positions each
constexpr uint32_t kMergeTile = kMergeLanes * 16;                 // merged positions per tile
static_assert(kMergeTile <= 65536, "a tile's B positions are kept as 16-bit offsets");

// ---- the walk ----
template <class BlockA, class BlockB>
struct MergeWalk {
    typename BlockLay<BlockB>::pos_t i;                           // row of B
    typename BlockLay<BlockA>::pos_t r;                           // suffixes of A smaller than that row's
};
template <class BlockA, class BlockB>
LRSC_HD MergeWalk<BlockA, BlockB> merge_walk_start(uint64_t read_of_b, uint64_t n_reads_a)
{
    MergeWalk<BlockA, BlockB> w;
    w.i = (typename BlockLay<BlockB>::pos_t)read_of_b;
    w.r = (typename BlockLay<BlockA>::pos_t)n_reads_a;
    return w;
}

// One step.  bb is B's block block_of(w.i), ba is A's block block_of(w.r).  Returns false, w unchanged, when BWT_B[w.i] is
// '$': the read is done.
template <class BlockA, class BlockB>
LRSC_HD bool merge_walk_step(const StrandView<BlockA>& A, const StrandView<BlockB>& B, const BlockA& ba, const BlockB& bb,
                             const uint32_t* mtab_a, const uint32_t* mtab_b, MergeWalk<BlockA, BlockB>& w)
{
    using PA = typename BlockLay<BlockA>::pos_t;
    using PB = typename BlockLay<BlockB>::pos_t;
    const PB gb = w.i / BlockB::kSyms;
    const PA ga = w.r / BlockA::kSyms;
    const uint32_t ob = (uint32_t)(w.i - gb * BlockB::kSyms), oa = (uint32_t)(w.r - ga * BlockA::kSyms);
    const uint32_t code = block_symbol(bb, ob);
    uint64_t cb = block_base_count(bb, code) + block_prefix_count(bb, code, mtab_b + ob * BlockLay<BlockB>::kRow);
    uint64_t ca = block_base_count(ba, code) + block_prefix_count(ba, code, mtab_a + oa * BlockLay<BlockA>::kRow);
    if(code == 0) {                                               // '$' is stored as A: only flagged blocks pay for the list
        bool at = false;
        uint64_t j = 0;                                           // the rows' ranks among the '$' rows: not needed here
        if(has_dollar_flag(bb)) {
            cb -= dollars_before(B, (uint64_t)gb, (uint64_t)gb * BlockB::kSyms, (uint64_t)w.i, at, j);
            if(at) return false;
        }
        if(oa != 0 && has_dollar_flag(ba)) ca -= dollars_before(A, (uint64_t)ga, (uint64_t)ga * BlockA::kSyms, (uint64_t)w.r, at, j);
    }
    w.i = strand_pred(B, code) + (PB)cb;
    w.r = strand_pred(A, code) + (PA)ca;
    return true;
}

// ---- the interleave ----
// first row j of B, in [0, n_b], whose merged position j + rank[j] is at or beyond p
LRSC_HD uint64_t merge_tile_search(const uint64_t* rank, uint64_t n_b, uint64_t p)
{
    uint64_t lo = 0, hi = n_b;
    while(lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if(m + rank[m] < p) lo = m + 1; else hi = m;
    }
    return lo;
}

// What a tile of kTile merged positions decodes of one input: whole rank blocks from the one that holds the tile's first row on.
template <class Block, uint32_t kTile>
struct MergeStage {
    static constexpr uint32_t kBlocks = kTile / Block::kSyms + 2;             // a tile's rows, begun anywhere in a block
    static constexpr uint32_t kChunks = Block::kSyms / 16;
    static constexpr uint32_t kRows = kBlocks * kChunks;                      // Sym16 rows; more than kTile + kSyms symbols
    static_assert(kBlocks * Block::kSyms > kTile + Block::kSyms, "a lane may look one symbol past its input's last row of the tile");
};
struct MergeSpan {
    uint64_t first_block;                                         // first block to decode
    uint32_t n_blocks;                                            // blocks to decode (0: the tile holds no row of this input)
    uint32_t skip;                                                // the tile's first row, counted from the first decoded symbol
};
template <class Block>
LRSC_HD MergeSpan merge_span(uint64_t row0, uint64_t row1)
{
    MergeSpan s;
    s.first_block = row0 / Block::kSyms;
    s.skip = (uint32_t)(row0 - s.first_block * Block::kSyms);
    s.n_blocks = row1 > row0 ? (uint32_t)((row1 - 1) / Block::kSyms - s.first_block + 1) : 0u;
    return s;
}
// Merged positions [q, q + 16) of a tile, of which those below n_valid exist (the others read 0).  pos_b[0 .. n_bt) are the
// tile's B rows as positions in the tile, ascending; sym_a / sym_b the decoded stretches, the tile's first row at skip_a / skip_b.
LRSC_HD Sym16 merge_fill16(const uint16_t* pos_b, uint32_t n_bt, const Sym16* sym_a, uint32_t skip_a, const Sym16* sym_b, uint32_t skip_b,
                           uint32_t q, uint32_t n_valid)
{
    uint32_t lo = 0, hi = n_bt;                                   // B rows of the tile before q
    while(lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if(pos_b[m] < q) lo = m + 1; else hi = m;
    }
    uint32_t k = lo;
    Sym16 v{{0u, 0u, 0u, 0u}};
    LRSC_UNROLL
    for(uint32_t t = 0; t < 16; ++t) {
        const uint32_t p = q + t;
        if(p < n_valid) {
            const bool from_b = k < n_bt && pos_b[k] == p;
            const uint32_t c = from_b ? sym_at(sym_b, skip_b + k) : sym_at(sym_a, skip_a + p - k);
            k += from_b ? 1u : 0u;
            v.w[t >> 2] |= c << (8 * (t & 3));
        }
    }
    return v;
}

// ---- the origin of the union's '$' rows ----
// index, among the union's '$' rows, of B's k-th, whose row has rank rank_d: the '$' rows of A that lie among A's first rank_d
// rows come before it
LRSC_HD uint64_t merge_origin_slot(const uint64_t* dollars_a, uint64_t n_a, uint64_t rank_d, uint64_t k)
{
    uint64_t lo = 0, hi = n_a;
    while(lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if(dollars_a[m] < rank_d) lo = m + 1; else hi = m;
    }
    return lo + k;
}

// ---- the device merge (fm_merge.hip) ----
// One strand: a and b are copies on the current device.  *d_bwt (hipFree) gets the union's BWT, a.n_symbols + b.n_symbols codes
// 0..4 in a buffer rounded up to 16 bytes, *d_rank (hipFree) rank[] of b's rows.  ms[0] += the walk, ms[1] += the interleave.
// Returns an lrsc_status; on an error nothing stays allocated.
int merge_strand_device(const FmStrand& a, bool wide_a, const FmStrand& b, bool wide_b, uint8_t** d_bwt, uint64_t** d_rank, double ms[2],
                        std::string& err);
// origin[k] = 1 when the k-th '$' row of the union is a row of b, else 0; n_dollars of a plus n_dollars of b bytes on the host
int merge_origin_device(const FmStrand& a, const FmStrand& b, const uint64_t* d_rank, uint8_t* origin, std::string& err);

} // namespace lrsc
