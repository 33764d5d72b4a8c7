// fm_strand.h -- one strand of a resident index as a lane sees it: what the device index tools (RL encode, merge, locate,
// duplicate check, removal, k-mer correction, paired-end walk, overlap) share of the rank-block layout of fm_device.h.
//
// A strand of an index is the BWT of a string set whose sentinels sort in input order: row i < n is the suffix that is read
// i's sentinel alone.  Its image is the rank blocks (Block32 or Block64: the A,C,G,T counts before the block and two bit planes,
// '$' stored as A), the sorted list of the '$' rows, and a directory of that list with one entry per group of blocks.
//
//   view      StrandView<Block>: the three arrays, their sizes and C[] as a kernel argument (strand_view, strand_pred,
//             select_view); BlockLay / MaskTab / mask_word: the layout's position type and its table of partial-word masks
//   block     One rank block held in registers: its symbol at an offset (block_symbol), the counts before it and within it
//             (block_base_count, block_prefix_count), and the whole block as codes (unpack_block, decode_block: the inverse of
//             fm_pack.h's pack_block)
//   '$' list  dollars_before: the '$' rows of a block before a position, through the directory entry of the block's group and
//             the few list entries of the group; dollar_rank: the '$' rows of the strand before a position
//   LF        lf_step: i <- C[c] + Occ(c, i) with c = BWT[i], both from the one rank block of row i; walk_read_back: the steps
//             from a read's sentinel row to its '$' row, which ends on any input
//   search    block_occ: Occ(c, p) from the rank block of p; search_first, search_step: the interval of a one-base string, and
//             the interval [lo, hi1) narrowed by one more base.  The loop around them, how it reads its bases and what it makes
//             of an empty interval is each tool's own.
//   counts    OccAll, block_occ_all, interval_occ_all: Occ of every symbol at the ends of an interval, with search_step's loads, for
//             the step that keeps the same string's interval in the other strand too (fm_overlap.h)
//
// All functions here are LRSC_HD and free of HIP types: the kernels call them, and the drivers under tests/host_tools compile
// the same source for the CPU.
#pragma once
#include <stdint.h>

#include "fm_device.h"
#include "fm_pack.h"

namespace lrsc {

// position type and mask-table row of a layout (rank_device.h's Lay<WIDE>, without HIP types)
template <class Block> struct BlockLay;
template <> struct BlockLay<Block32> { using pos_t = uint32_t; static constexpr uint32_t kRow = 8; };
template <> struct BlockLay<Block64> { using pos_t = uint64_t; static constexpr uint32_t kRow = 4; };
// Row `off` of the table holds the kWords partial-word masks of "the first off symbols of a block".
template <class Block> struct MaskTab { static constexpr uint32_t kWords = (Block::kSyms + 1) * BlockLay<Block>::kRow; };
template <class Block>
LRSC_HD uint32_t mask_word(uint32_t i)
{
    const uint32_t off = i / BlockLay<Block>::kRow, w = i % BlockLay<Block>::kRow;
    return w < Block::kWords ? low_mask((int32_t)off - 32 * (int32_t)w) : 0u;
}

// One strand as a kernel reads it.  C[] as four scalars: indexing a by-value kernel argument dynamically would put it in scratch.
template <class Block>
struct StrandView {
    using pos_t = typename BlockLay<Block>::pos_t;
    const Block* blocks;
    const uint64_t* dollars;
    const uint32_t* dollar_dir;
    uint64_t n_dollars, n_blocks, N;
    pos_t c1, c2, c3, c4;                                         // C[A], C[C], C[G], C[T]
};
template <class Block>
LRSC_HD StrandView<Block> strand_view(const FmStrand& s)
{
    using P = typename BlockLay<Block>::pos_t;
    StrandView<Block> m;
    m.blocks = static_cast<const Block*>(s.blocks); m.dollars = s.dollars; m.dollar_dir = s.dollar_dir;
    m.n_dollars = s.n_dollars; m.n_blocks = s.n_blocks; m.N = s.n_symbols;
    m.c1 = (P)s.pred[1]; m.c2 = (P)s.pred[2]; m.c3 = (P)s.pred[3]; m.c4 = (P)s.pred[4];
    return m;
}
template <class Block>
LRSC_HD typename BlockLay<Block>::pos_t strand_pred(const StrandView<Block>& s, uint32_t code)
{
    typename BlockLay<Block>::pos_t v = s.c1;
    v += code >= 1 ? (s.c2 - s.c1) : 0;
    v += code >= 2 ? (s.c3 - s.c2) : 0;
    v += code >= 3 ? (s.c4 - s.c3) : 0;
    return v;
}
// b when `second`, else a, member by member: a by-value argument picked by a run-time index would be copied to scratch
template <class Block>
LRSC_HD StrandView<Block> select_view(bool second, const StrandView<Block>& a, const StrandView<Block>& b)
{
    StrandView<Block> S;
    S.blocks = second ? b.blocks : a.blocks; S.dollars = second ? b.dollars : a.dollars; S.dollar_dir = second ? b.dollar_dir : a.dollar_dir;
    S.n_dollars = second ? b.n_dollars : a.n_dollars; S.n_blocks = second ? b.n_blocks : a.n_blocks; S.N = second ? b.N : a.N;
    S.c1 = second ? b.c1 : a.c1; S.c2 = second ? b.c2 : a.c2; S.c3 = second ? b.c3 : a.c3; S.c4 = second ? b.c4 : a.c4;
    return S;
}
template <class Block> LRSC_HD uint64_t block_of(typename BlockLay<Block>::pos_t p) { return (uint64_t)(p / Block::kSyms); }

// ---- one rank block, held in registers: every index into it is a constant after unrolling ----
LRSC_HD uint32_t plane_lo(const Block32& b, uint32_t wi) { return b.w[Block32::lo_index(wi)]; }
LRSC_HD uint32_t plane_hi(const Block32& b, uint32_t wi) { return b.w[Block32::hi_index(wi)]; }
LRSC_HD uint32_t plane_lo(const Block64& b, uint32_t wi) { return b.lo[wi]; }
LRSC_HD uint32_t plane_hi(const Block64& b, uint32_t wi) { return b.hi[wi]; }
LRSC_HD bool has_dollar_flag(const Block32& b) { return (b.cnt[0] & kFlag32) != 0; }
LRSC_HD bool has_dollar_flag(const Block64& b) { return (b.cnt[0] & kFlag64) != 0; }

LRSC_HD uint64_t pick4(uint32_t code, uint64_t a, uint64_t b, uint64_t c, uint64_t d)
{
    return (code & 2u) ? ((code & 1u) ? d : c) : ((code & 1u) ? b : a);       // by the code's bits, never an equality chain (rank_device.h)
}
LRSC_HD uint64_t block_base_count(const Block32& b, uint32_t code) { return pick4(code, b.cnt[0] & ~kFlag32, b.cnt[1], b.cnt[2], b.cnt[3]); }
LRSC_HD uint64_t block_base_count(const Block64& b, uint32_t code) { return pick4(code, b.cnt[0] & ~kFlag64, b.cnt[1], b.cnt[2], b.cnt[3]); }

// code (A=0 .. T=3, '$' reads as A) of symbol `off` of the block
template <class Block>
LRSC_HD uint32_t block_symbol(const Block& b, uint32_t off)
{
    uint32_t l = 0, h = 0;
    LRSC_UNROLL
    for(uint32_t wi = 0; wi < Block::kWords; ++wi) {
        l = (off >> 5) == wi ? plane_lo(b, wi) : l;
        h = (off >> 5) == wi ? plane_hi(b, wi) : h;
    }
    return ((l >> (off & 31u)) & 1u) | (((h >> (off & 31u)) & 1u) << 1);
}
// symbols with that code among the first symbols of the block, mrow being their row of the mask table ('$' rows count as A)
template <class Block>
LRSC_HD uint32_t block_prefix_count(const Block& b, uint32_t code, const uint32_t* mrow)
{
    const uint32_t L = (code & 1u) ? 0u : 0xFFFFFFFFu;
    const uint32_t H = (code & 2u) ? 0u : 0xFFFFFFFFu;
    uint32_t c = 0;
    LRSC_UNROLL
    for(uint32_t wi = 0; wi < Block::kWords; ++wi) c += (uint32_t)__builtin_popcount((plane_lo(b, wi) ^ L) & (plane_hi(b, wi) ^ H) & mrow[wi]);
    return c;
}

// ---- the '$' list ----
// '$' rows of block g (which starts at symbol base) before position pos, and whether pos itself is one (at_pos): the directory
// entry of the block's group, then the few list entries of the group.  j is the number of '$' rows of the whole strand before
// pos, the rank of pos among them when it is one itself.
template <class Block>
LRSC_HD uint32_t dollars_before(const StrandView<Block>& s, uint64_t g, uint64_t base, uint64_t pos, bool& at_pos, uint64_t& j)
{
    j = s.dollar_dir[g >> kDollarDirShift];
    uint32_t n = 0;
    uint64_t d = ~0ull;
    for(; j < s.n_dollars; ++j) {
        d = s.dollars[j];
        if(d >= pos) break;
        n += d >= base ? 1u : 0u;
    }
    at_pos = j < s.n_dollars && d == pos;
    return n;
}
// '$' rows of the strand before row pos <= N, pos being a row of block g: the index of the first entry >= pos of the sorted list
LRSC_HD uint64_t dollar_rank(const uint64_t* dollars, uint64_t n_dollars, const uint32_t* dollar_dir, uint64_t g, uint64_t pos)
{
    uint64_t j = dollar_dir[g >> kDollarDirShift];
    while(j < n_dollars && dollars[j] < pos) ++j;
    return j;
}

// ---- rank block -> codes: the inverse of pack_block ----
// bits 0..3 of x -> bit 0 of each of four bytes
LRSC_HD uint32_t spread_byte_bits(uint32_t x) { return ((x & 0xFu) * 0x00204081u) & 0x01010101u; }

// The kSyms codes ($ACGT = 0..4) of block b, which starts at symbol `base` and of which the first n_valid symbols exist, to
// out[0 .. kSyms/16); codes at and beyond n_valid are 0.  d[0..n_d) are the sorted '$' positions from the block's first one
// on (dollar_rank of base; entries beyond the block are ignored, and an unflagged block is given none).
template <class Block>
LRSC_HD void unpack_block(const Block& b, uint64_t base, const uint64_t* d, uint64_t n_d, uint32_t n_valid, Sym16* out)
{
    uint64_t j = 0;
    LRSC_UNROLL
    for(uint32_t wi = 0; wi < Block::kWords; ++wi) {
        uint32_t dollar = 0;
        for(; j < n_d && d[j] - base < 32ull * (wi + 1); ++j) dollar |= 1u << ((uint32_t)(d[j] - base) & 31u);
        const uint32_t v = low_mask((int32_t)n_valid - (int32_t)(32 * wi)) & ~dollar;
        const uint32_t lo = plane_lo(b, wi) & v, hi = plane_hi(b, wi) & v;
        LRSC_UNROLL
        for(uint32_t q = 0; q < 8; ++q)
            out[2 * wi + (q >> 2)].w[q & 3] = spread_byte_bits(v >> (4 * q)) + spread_byte_bits(lo >> (4 * q)) + (spread_byte_bits(hi >> (4 * q)) << 1);
    }
}
// block g of a strand -> its codes at out[0 .. kSyms/16).  Strand is anything with a view's blocks, '$' list and N.
template <class Block, class Strand>
LRSC_HD void decode_block(const Strand& s, uint64_t g, Sym16* out)
{
    const Block b = s.blocks[g];
    const uint64_t base = g * Block::kSyms;
    const uint64_t left = s.N - base;                             // n_blocks = N / kSyms + 1: base <= N
    uint64_t j = s.n_dollars;
    if(has_dollar_flag(b)) j = dollar_rank(s.dollars, s.n_dollars, s.dollar_dir, g, base);
    unpack_block<Block>(b, base, s.dollars + j, s.n_dollars - j, (uint32_t)(left < Block::kSyms ? left : Block::kSyms), out);
}

// ---- the LF step and the walk of one read ----
// One LF step from row i < S.N, b being its block i / kSyms.  Returns false, i unchanged, when BWT[i] is '$': k is then the
// rank of the row among the strand's '$' rows.
template <class Block>
LRSC_HD bool lf_step(const StrandView<Block>& S, const Block& b, const uint32_t* mtab, typename BlockLay<Block>::pos_t& i, uint64_t& k)
{
    using P = typename BlockLay<Block>::pos_t;
    const P g = i / Block::kSyms;
    const uint32_t o = (uint32_t)(i - g * Block::kSyms);
    const uint32_t code = block_symbol(b, o);
    uint64_t c = block_base_count(b, code) + block_prefix_count(b, code, mtab + o * BlockLay<Block>::kRow);
    if(code == 0 && has_dollar_flag(b)) {                         // '$' is stored as A: only flagged blocks pay for the list
        bool at = false;
        const uint32_t n = dollars_before(S, (uint64_t)g, (uint64_t)g * Block::kSyms, (uint64_t)i, at, k);
        if(at) return false;
        c -= n;
    }
    i = strand_pred(S, code) + (P)c;
    return true;
}

// What a lane reports of a walk: 0, or that it was cut short.  An index made by this library never gives the latter.
enum : uint32_t { kWalkOk = 0, kWalkBroken = 1 };

// Read `read` backwards from its sentinel row to its '$' row.  visit(row, t) sees every row of the read, the first and the '$'
// row included, t being the steps taken to it.  Returns kWalkOk with k = the rank of the '$' row among the strand's '$' rows
// (k < n_dollars: dollars_before found the row in the list) and t = the read's length.
template <class Block, class Visit>
LRSC_HD uint32_t walk_read_back(const StrandView<Block>& S, const uint32_t* mtab, uint32_t read, Visit&& visit, uint64_t& k_out, uint64_t& t_out)
{
    using P = typename BlockLay<Block>::pos_t;
    P i = (P)read;
    // a read has fewer symbols than the strand has rows and never leaves it: the bound and the range check only end the walk
    // through an index that is no BWT of a string set
    for(uint64_t t = 0; t < S.N; ++t) {
        if(i >= S.N) return kWalkBroken;
        visit(i, t);
        const Block b = S.blocks[block_of<Block>(i)];
        uint64_t k = 0;
        if(!lf_step(S, b, mtab, i, k)) {
            k_out = k;
            t_out = t;
            return kWalkOk;
        }
    }
    return kWalkBroken;
}

// ---- the backward search: an interval of rows [lo, hi1), narrowed one base at a time ----
// Occ over the first `off` symbols of block g, held in b, plus the block's base count ('$' rows are stored as A and taken out)
template <class Block>
LRSC_HD uint64_t block_occ(const StrandView<Block>& S, const Block& b, uint64_t g, uint32_t off, uint32_t code, const uint32_t* mtab)
{
    uint64_t c = block_base_count(b, code) + block_prefix_count(b, code, mtab + off * BlockLay<Block>::kRow);
    if(code == 0 && off != 0 && has_dollar_flag(b)) {
        bool at = false;
        uint64_t j = 0;
        c -= dollars_before(S, g, g * Block::kSyms, g * Block::kSyms + off, at, j);
    }
    return c;
}
// Pos below is the type in which the caller holds its interval and in which the step adds: pos_t, or 64 bits whatever the
// layout.  pred = strand_pred(S, code), which the caller has at hand.
// the interval of the one-base string `code`
template <class Block, class Pos>
LRSC_HD void search_first(const StrandView<Block>& S, uint32_t code, typename BlockLay<Block>::pos_t pred, Pos& lo, Pos& hi1)
{
    lo = (Pos)pred;
    hi1 = code == 3u ? (Pos)S.N : (Pos)strand_pred(S, code + 1);
}
// One step with `code` from an interval of the strand, lo <= hi1 <= S.N: two Occ queries, one rank block when both ends lie in
// one block.  n_rank += the Occ queries, n_blk += the block loads.  Whether the new interval is empty, or one of the strand at
// all (it always is with the BWT of a string set), is the caller's to ask.
template <class Block, class Pos>
LRSC_HD void search_step(const StrandView<Block>& S, const uint32_t* mtab, uint32_t code, typename BlockLay<Block>::pos_t pred, Pos& lo, Pos& hi1,
                         uint32_t& n_rank, uint32_t& n_blk)
{
    using P = typename BlockLay<Block>::pos_t;
    const uint64_t gl = block_of<Block>((P)lo), gu = block_of<Block>((P)hi1);
    const Block bl = S.blocks[gl];
    const uint64_t ca = block_occ(S, bl, gl, (uint32_t)((P)lo - (P)(gl * Block::kSyms)), code, mtab);
    uint64_t cb;
    if(gu == gl) cb = block_occ(S, bl, gl, (uint32_t)((P)hi1 - (P)(gl * Block::kSyms)), code, mtab);
    else {
        const Block bu = S.blocks[gu];
        cb = block_occ(S, bu, gu, (uint32_t)((P)hi1 - (P)(gu * Block::kSyms)), code, mtab);
    }
    lo = (Pos)pred + (Pos)ca;
    hi1 = (Pos)pred + (Pos)cb;
    n_rank += 2;
    n_blk += gu == gl ? 1u : 2u;
}

// ---- the counts of every symbol: what a step needs that keeps the same string's interval in the other strand too ----
// Occ of '$', A, C, G, T before a position, members and not an array: an index that is known only at run time would put it in
// scratch.  k below is a symbol's rank, '$' = 0, A..T = 1..4.
struct OccAll {
    uint64_t d, a, c, g, t;
};
LRSC_HD uint64_t occ_get(const OccAll& o, uint32_t k) { return k == 0 ? o.d : pick4(k - 1, o.a, o.c, o.g, o.t); }
LRSC_HD uint64_t occ_less_than(const OccAll& o, uint32_t k)
{
    return (k > 0 ? o.d : 0) + (k > 1 ? o.a : 0) + (k > 2 ? o.c : 0) + (k > 3 ? o.g : 0);
}
LRSC_HD OccAll occ_diff(const OccAll& u, const OccAll& l) { return OccAll{u.d - l.d, u.a - l.a, u.c - l.c, u.g - l.g, u.t - l.t}; }
// the counts before offset `off` of block g, held in b: block_occ of the four bases and dollar_rank
template <class Block>
LRSC_HD OccAll block_occ_all(const StrandView<Block>& S, const Block& b, uint64_t g, uint32_t off, const uint32_t* mtab)
{
    OccAll o;
    o.d = dollar_rank(S.dollars, S.n_dollars, S.dollar_dir, g, g * Block::kSyms + off);
    o.a = block_occ(S, b, g, off, 0u, mtab);
    o.c = block_occ(S, b, g, off, 1u, mtab);
    o.g = block_occ(S, b, g, off, 2u, mtab);
    o.t = block_occ(S, b, g, off, 3u, mtab);
    return o;
}
// The counts at both ends of an interval of the strand, lo <= hi1 <= S.N, with search_step's loads: one rank block when both
// ends lie in one.  search_step's new interval with `code` is strand_pred(S, code) + the base's member of l and of u.
template <class Block>
LRSC_HD void interval_occ_all(const StrandView<Block>& S, const uint32_t* mtab, uint64_t lo, uint64_t hi1, OccAll& l, OccAll& u, uint32_t& n_rank, uint32_t& n_blk)
{
    using P = typename BlockLay<Block>::pos_t;
    const uint64_t gl = block_of<Block>((P)lo), gu = block_of<Block>((P)hi1);
    const Block bl = S.blocks[gl];
    l = block_occ_all(S, bl, gl, (uint32_t)((P)lo - (P)(gl * Block::kSyms)), mtab);
    if(gu == gl) u = block_occ_all(S, bl, gl, (uint32_t)((P)hi1 - (P)(gl * Block::kSyms)), mtab);
    else {
        const Block bu = S.blocks[gu];
        u = block_occ_all(S, bu, gu, (uint32_t)((P)hi1 - (P)(gu * Block::kSyms)), mtab);
    }
    n_rank += 2;
    n_blk += gu == gl ? 1u : 2u;
}

} // namespace lrsc
