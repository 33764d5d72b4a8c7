// fm_pack.h -- BWT codes -> rank blocks (fm_device.h), the per-block arithmetic of the device packer (fm_pack.hip).
//
// The device BWT build leaves the BWT in HBM as one code per byte ($=0 A=1 C=2 G=3 T=4).  The packer turns that stream into
// exactly what build_strand_image (fm_layout.cpp) makes from the RL units of the same BWT: a histogram pass gives every
// block's symbol counts (block_hist), an exclusive scan turns them into the counts before the block, and a second pass writes
// each 64-byte block once (pack_block).  Both functions are LRSC_HD and free of HIP types: the kernels call them, and
// tests/host_tools/pack_driver.cpp compiles the same source for the CPU and holds it against build_strand_image.
#pragma once
#include <stdint.h>

#include <string>

#include "fm_device.h"

#ifdef __HIPCC__
#define LRSC_UNROLL _Pragma("unroll")
#else
#define LRSC_UNROLL
#endif

namespace lrsc {

// 16 consecutive BWT codes as the packer moves them (one 16-byte access): symbol i is byte i, little-endian words
struct alignas(16) Sym16 {
    uint32_t w[4];
};
// symbol i of the stretch at s
LRSC_HD uint32_t sym_at(const Sym16* s, uint32_t i) { return (s[i >> 4].w[(i >> 2) & 3] >> (8 * (i & 3))) & 0xFFu; }

// 32 symbols of a block as bit masks (bit i = symbol i): the two code planes (A=0 C=1 G=2 T=3; '$' is stored as A),
// the '$' rows and the positions that exist (< n_valid).  All four are zero at positions >= n_valid.
struct SymBits {
    uint32_t lo, hi, dollar, valid;
};

// bit 0 of each of the four bytes of x -> bits 0..3
LRSC_HD uint32_t gather_byte_bits(uint32_t x) { return ((x * 0x01020408u) >> 24) & 0xFu; }

// symbols [32*wi, 32*wi + 32) of the block that starts at s
LRSC_HD SymBits sym_bits32(const Sym16* s, uint32_t wi, uint32_t n_valid)
{
    const uint32_t k1 = 0x01010101u;
    uint32_t lo = 0, hi = 0, any = 0;
    LRSC_UNROLL
    for(uint32_t q = 0; q < 8; ++q) {
        const uint32_t x = s[2 * wi + (q >> 2)].w[q & 3];
        const uint32_t b0 = x & k1, b1 = (x >> 1) & k1, b2 = (x >> 2) & k1;
        // code - 1 for A,C,G,T = 1..4: low bit set for C (010) and T (100), high bit for G (011) and T
        lo |= gather_byte_bits(b2 | (b1 & ~b0)) << (4 * q);
        hi |= gather_byte_bits(b2 | (b1 & b0)) << (4 * q);
        any |= gather_byte_bits(b0 | b1 | b2) << (4 * q);
    }
    const uint32_t m = low_mask((int32_t)n_valid - (int32_t)(32 * wi));
    return SymBits{lo & m, hi & m, ~any & m, m};
}

// cnt[0..3] = A,C,G,T among the first n_valid symbols of the block at s, cnt[4] = its '$' rows
template <class Block>
LRSC_HD void block_hist(const Sym16* s, uint32_t n_valid, uint32_t cnt[5])
{
    for(int c = 0; c < 5; ++c) cnt[c] = 0;
    LRSC_UNROLL
    for(uint32_t wi = 0; wi < Block::kWords; ++wi) {
        const SymBits b = sym_bits32(s, wi, n_valid);
        const uint32_t d = (uint32_t)__builtin_popcount(b.dollar);
        cnt[0] += (uint32_t)__builtin_popcount(b.valid & ~b.lo & ~b.hi) - d;
        cnt[1] += (uint32_t)__builtin_popcount(b.lo & ~b.hi);
        cnt[2] += (uint32_t)__builtin_popcount(b.hi & ~b.lo);
        cnt[3] += (uint32_t)__builtin_popcount(b.lo & b.hi);
        cnt[4] += d;
    }
}

LRSC_HD void set_planes(Block32& b, uint32_t wi, uint32_t lo, uint32_t hi)
{
    b.w[Block32::lo_index(wi)] = lo;
    b.w[Block32::hi_index(wi)] = hi;
}
LRSC_HD void set_planes(Block64& b, uint32_t wi, uint32_t lo, uint32_t hi)
{
    b.lo[wi] = lo;
    b.hi[wi] = hi;
}
LRSC_HD void set_dollar_flag(Block32& b) { b.cnt[0] |= kFlag32; }
LRSC_HD void set_dollar_flag(Block64& b) { b.cnt[0] |= kFlag64; }

// The rank block of the kSyms symbols at s, of which the first n_valid exist (0 for the terminal block of an index whose
// length is a multiple of kSyms); before[c] = A,C,G,T in the BWT ahead of the block.
template <class Block>
LRSC_HD Block pack_block(const Sym16* s, uint32_t n_valid, const uint64_t before[4])
{
    using CountT = decltype(Block::cnt[0] + 0);
    Block b;
    for(int c = 0; c < 4; ++c) b.cnt[c] = (CountT)before[c];
    uint32_t dollar = 0;
    LRSC_UNROLL
    for(uint32_t wi = 0; wi < Block::kWords; ++wi) {
        const SymBits sb = sym_bits32(s, wi, n_valid);
        set_planes(b, wi, sb.lo, sb.hi);
        dollar |= sb.dollar;
    }
    if(dollar) set_dollar_flag(b);
    return b;
}

// dollar_dir[g]: '$' rows before block g << kDollarDirShift; dollars_before has n_blocks + 1 entries, the last one the total
LRSC_HD uint32_t dollar_dir_entry(const uint64_t* dollars_before, uint64_t n_blocks, uint64_t g)
{
    const uint64_t b = g << kDollarDirShift;
    return (uint32_t)dollars_before[b < n_blocks ? b : n_blocks];
}

// ---- the tile of the streaming kernels (fm_pack.hip, fm_unrle.hip) ----
constexpr uint32_t kPackThreads = 128;          // rank blocks per workgroup, one thread each in the packer

// An LDS row holds one block's symbols plus 16 bytes, a block's output 64 + 16 bytes: with these strides the 16-byte accesses
// of the lanes of a wave, one row each, fall on different banks.
template <class Block>
struct PackTile {
    static constexpr uint32_t kChunks = Block::kSyms / 16;
    static constexpr uint32_t kRow = kChunks + 1;
    static constexpr uint32_t kOutRow = 5;
    static_assert(kRow >= kOutRow, "the finished blocks reuse the symbol rows");
};

// ---- the device packer (fm_pack.hip) ----
// One strand's image in device memory, as lrsc_index_upload would have left it.
struct PackedStrand {
    void* blocks = nullptr;          // n_blocks x 64 bytes
    uint64_t* dollars = nullptr;     // max(n_dollars, 1) entries
    uint32_t* dollar_dir = nullptr;  // n_dir entries
    uint64_t n_blocks = 0, n_dollars = 0, n_dir = 0;
    uint64_t pred[5] = {0, 0, 0, 0, 0};
};

// Packs d_bwt[0..N) (codes 0..4, on the current device) into Block64 (wide) or Block32 blocks.  Returns an lrsc_status; on an
// error nothing stays allocated.  Otherwise the three arrays of `out` are the caller's (hipFree).
int pack_strand_device(const uint8_t* d_bwt, uint64_t N, bool wide, PackedStrand& out, std::string& err);

} // namespace lrsc
