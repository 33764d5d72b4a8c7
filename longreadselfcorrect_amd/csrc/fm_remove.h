// fm_remove.h -- an FM-index without some of its reads: the per-lane arithmetic of the device removal (fm_remove.hip).
//
// A strand of an index is the BWT of a string set whose sentinels sort in input order.  Deleting every row that belongs to a
// read (its sentinel row, the rows of its suffixes, its '$' row) leaves the other suffixes in their order and their preceding
// symbols as they were: what is left is the BWT of the remaining reads, the mirror image of fm_merge.h's union.
//
//   mark     One lane per dropped read i walks it backwards from row i (the suffix that is the read's sentinel alone) with
//            fm_strand.h's LF step until the row's symbol is '$', and sets the bit of every row it visits, the first and the
//            '$' row included.  The walks of different reads visit different rows; the bits of 32 rows share a word, so a bit is
//            set with a 32-bit atomic OR.  The bitmap takes num_symbols / 8 bytes.
//   count    rows of a tile of kRemoveTile whose bit is clear (remove_tile_kept); an exclusive scan gives every tile's offset
//            in the output.
//   compact  Per tile: its rank blocks are decoded (decode_block), every lane takes 16 rows and copies the kept ones
//            (remove_keep16, remove_scatter16) to a stage at the lane's offset, the sum of the kept rows of the lanes before
//            it.  The stage is laid out congruent to the output modulo 16, so the tile leaves with 16-byte stores except for
//            the bytes of the two 16-byte chunks it shares with its neighbours (remove_store_chunk).
//
// Every walk ends on any input (remove_mark_read is fm_strand.h's walk_read_back).  All functions here are LRSC_HD and free of
// HIP types: the kernels call them, and tests/host_tools/remove_driver.cpp compiles the same source for the CPU and holds it
// against a suffix sort of the kept reads.
#pragma once
#include <stdint.h>

#include <string>

#include "fm_strand.h"

namespace lrsc {

constexpr uint32_t kRemoveWalkThreads = 128;                      // lanes, one dropped read each, per workgroup of the mark walk
// Wavefronts per SIMD that the walk's launch is sized for: as the locate walks, a chain of dependent 64-byte loads
constexpr uint32_t kRemoveWalkWavesPerSimd = 8;
constexpr uint32_t kRemoveLanes = 192;                            // threads per compaction tile, 16 rows each
constexpr uint32_t kRemoveTile = kRemoveLanes * 16;               // rows per tile: 16 Block32 or 24 Block64
static_assert(kRemoveTile % Block32::kSyms == 0 && kRemoveTile % Block64::kSyms == 0, "a tile is whole rank blocks of either layout");
static_assert(kRemoveTile % 32 == 0, "a tile is whole bitmap words");

LRSC_HD uint64_t remove_bitmap_words(uint64_t n_symbols, uint32_t tile) { return (n_symbols + tile - 1) / tile * (tile / 32); }

// ---- mark: the walk of one dropped read ----
// mark(row) is called for every row of the read; rows += their number.  Returns kWalkOk when the walk ended at a '$' row.
template <class Block, class Mark>
LRSC_HD uint32_t remove_mark_read(const StrandView<Block>& S, const uint32_t* mtab, uint32_t read, Mark&& mark, uint64_t& rows)
{
    uint64_t k = 0, t = 0;
    return walk_read_back(S, mtab, read, [&](typename BlockLay<Block>::pos_t i, uint64_t) {
        mark((uint64_t)i);
        ++rows;
    }, k, t);
}

// ---- count: kept rows of a tile, from words [w0, w0 + n_words) of the bitmap that one lane looks at ----
LRSC_HD uint32_t remove_words_marked(const uint32_t* bitmap, uint64_t w0, uint32_t n_words)
{
    uint32_t n = 0;
    for(uint32_t w = 0; w < n_words; ++w) n += (uint32_t)__builtin_popcount(bitmap[w0 + w]);
    return n;
}

// ---- compact ----
// bit t set: row p0 + 16 * lane + t of the tile that starts at row p0 exists (there are n_valid rows in the tile) and is kept
LRSC_HD uint32_t remove_keep16(const uint32_t* bitmap, uint64_t p0, uint32_t lane, uint32_t n_valid)
{
    const uint32_t q = lane * 16;
    if(q >= n_valid) return 0u;
    const uint32_t word = bitmap[(p0 + q) >> 5];
    const uint32_t marked = (word >> (q & 16u)) & 0xFFFFu;
    const uint32_t exist = n_valid - q >= 16 ? 0xFFFFu : ((1u << (n_valid - q)) - 1u);
    return ~marked & exist;
}
// the kept rows of a lane, from the decoded tile to dst[0 .. popcount(keep))
LRSC_HD void remove_scatter16(const Sym16* sym, uint32_t lane, uint32_t keep, uint8_t* dst)
{
    const Sym16 v = sym[lane];
    uint32_t n = 0;
    LRSC_UNROLL
    for(uint32_t t = 0; t < 16; ++t) {
        if((keep >> t) & 1u) dst[n++] = (uint8_t)((v.w[t >> 2] >> (8 * (t & 3))) & 0xFFu);
    }
}
// The tile's n_kept symbols lie in the stage from byte `shift` on, shift = (the tile's offset in the output) % 16, and
// out16 = the output at that offset - shift, a 16-byte boundary.  Chunk c is bytes [16c, 16c + 16) of both.  A chunk that the tile
// fills alone leaves with one 16-byte store; of a chunk shared with a neighbour only the tile's own bytes are written.
LRSC_HD void remove_store_chunk(const Sym16* stage, uint32_t shift, uint32_t n_kept, uint32_t c, uint8_t* out16)
{
    const uint32_t lo = 16 * c, hi = lo + 16, end = shift + n_kept;
    if(lo >= end || hi <= shift) return;
    if(lo >= shift && hi <= end) {
        *reinterpret_cast<Sym16*>(out16 + lo) = stage[c];
        return;
    }
    for(uint32_t i = lo < shift ? shift : lo; i < (hi < end ? hi : end); ++i) out16[i] = (uint8_t)sym_at(stage, i);
}
template <uint32_t kTile> struct RemoveStage { static constexpr uint32_t kRows = kTile / 16 + 1; };   // Sym16 rows: a tile shifted by up to 15 bytes

// ---- the device removal (fm_remove.hip) ----
// One strand: s is a copy on the current device, ids[0 .. n_drop) the dropped reads, ascending.  *d_bwt (hipFree) gets the BWT
// of the kept reads, *n_out codes 0..4 in a buffer rounded up to 16 bytes.  ms[0] += the walk, ms[1] += count, scan and compaction.
// Returns an lrsc_status; on an error nothing stays allocated.  LRSC_ERR_FORMAT when a walk does not end at a '$' row or the
// marked rows are not as many as the walks visited.
int remove_strand_device(const FmStrand& s, bool wide, const uint32_t* ids, uint64_t n_drop, uint8_t** d_bwt, uint64_t* n_out, double ms[2],
                         std::string& err);

} // namespace lrsc
