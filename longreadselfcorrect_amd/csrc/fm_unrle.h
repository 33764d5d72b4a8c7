// fm_unrle.h -- RL units (the reference's .bwt/.rbwt payload) -> rank blocks, the per-lane arithmetic of the device decoder
// (fm_unrle.hip).
//
// A unit is one byte, (code << 5) | run with code $ACGT = 0..4 and run in 1..31 (SuffixTools/RLBWT.cpp:23-32 reads them, one
// after the other, into the run string).  The decoder never makes the byte-per-symbol BWT: a workgroup that packs a tile of rank
// blocks finds the units that cover the tile's symbols, expands exactly those into the Sym16 rows of the packer (fm_pack.h) in
// LDS and packs them with block_hist / pack_block.  Two tilings meet here:
//
//   unit tile    kUnrleTile consecutive units, kUnrleLanes lanes x 16 units (one Sym16 load per lane).  Its symbol count and
//                its per-code sums are scanned over the tiles, so every unit tile knows the symbol position and the A,C,G,T,'$'
//                counts at which it starts.
//   symbol tile  the packer's: kUnrleBlocks rank blocks.  Its first symbol lies in the unit tile that unrle_seek_tile finds
//                in the scanned positions; from there on the units are taken a chunk (again kUnrleLanes x 16 units) at a time.
//
// Inside a chunk the lanes' run sums are scanned into `starts` (entry l: symbols of the chunk before lane l's units, entry
// n_lanes: the chunk's total), and everything else is a look-up in that table: unrle_find_lane, unrle_locate, expand_sym16.
// All functions here are LRSC_HD and free of HIP types: the kernels call them, and tests/host_tools/unrle_driver.cpp compiles
// the same source for the CPU and holds it against build_strand_image.
#pragma once
#include <stdint.h>

#include <string>

#include "fm_device.h"
#include "fm_pack.h"

namespace lrsc {

constexpr uint32_t kUnrleLanes = 256;                             // threads per workgroup; lanes of a unit tile and of a chunk
constexpr uint32_t kUnrleTile = kUnrleLanes * 16;                 // units per unit tile
constexpr uint32_t kUnrleBlocks = 128;                            // rank blocks per symbol tile (the packer's kPackThreads)
constexpr uint32_t kUnrleNone = 16;                               // UnitSums::bad of sixteen valid units

LRSC_HD uint32_t unit_at(const Sym16& v, uint32_t i) { return (v.w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }
LRSC_HD uint32_t unit_code(uint32_t u) { return u >> 5; }
LRSC_HD uint32_t unit_run(uint32_t u) { return u & 31u; }
// the host decoder's test (fm_layout.cpp): a code outside $ACGT or an empty run is a corrupt unit
LRSC_HD bool unit_ok(uint32_t u) { return unit_code(u) <= 4 && unit_run(u) != 0; }
// where a code's symbols are counted: A,C,G,T = 0..3 as in a rank block, '$' = 4
LRSC_HD uint32_t unit_slot(uint32_t code) { return code == 0 ? 4u : code - 1; }

// Symbols per slot among the first n of sixteen units, and the index of the first invalid one among them (kUnrleNone: none).
// An invalid unit counts for nothing.
struct UnitSums {
    uint32_t c[5];
    uint32_t bad;
};
LRSC_HD UnitSums units16_sums(const Sym16& v, uint32_t n)
{
    UnitSums s{{0, 0, 0, 0, 0}, kUnrleNone};
    LRSC_UNROLL
    for(uint32_t i = 0; i < 16; ++i) {
        const uint32_t u = unit_at(v, i);
        const bool in = i < n, ok = unit_ok(u);
        const uint32_t run = in && ok ? unit_run(u) : 0u;
        LRSC_UNROLL
        for(uint32_t k = 0; k < 5; ++k) s.c[k] += unit_slot(unit_code(u)) == k ? run : 0u;
        if(in && !ok && s.bad == kUnrleNone) s.bad = i;
    }
    return s;
}

// symbols of the first n of sixteen valid units
LRSC_HD uint32_t units16_total(const Sym16& v, uint32_t n)
{
    uint32_t t = 0;
    LRSC_UNROLL
    for(uint32_t i = 0; i < 16; ++i) t += i < n ? unit_run(unit_at(v, i)) : 0u;
    return t;
}

// The seek's first half.  pos[0 .. n_tiles] are the scanned symbol positions of the unit tiles, strictly ascending (every unit
// has a symbol), pos[n_tiles] = N.  Returns the unit tile that holds symbol p < N: the last t with pos[t] <= p.
LRSC_HD uint64_t unrle_seek_tile(const uint64_t* pos, uint64_t n_tiles, uint64_t p)
{
    uint64_t a = 0, b = n_tiles;                                   // pos[a] <= p < pos[b]
    while(b - a > 1) {
        const uint64_t m = a + ((b - a) >> 1);
        if(pos[m] <= p) a = m; else b = m;
    }
    return a;
}

// The seek's second half, a lane's share: of the symbols of its first n units, which start `start` symbols into the tile, those
// that lie before the tile's symbol `rel`, per slot.  Summed over the lanes this is what the tile holds ahead of `rel`.
LRSC_HD void units16_before(const Sym16& v, uint32_t n, uint32_t start, uint32_t rel, uint32_t cnt[5])
{
    for(uint32_t k = 0; k < 5; ++k) cnt[k] = 0;
    uint32_t at = start;
    LRSC_UNROLL
    for(uint32_t i = 0; i < 16; ++i) {
        const uint32_t u = unit_at(v, i);
        const uint32_t run = i < n ? unit_run(u) : 0u;
        const uint32_t left = rel > at ? rel - at : 0u;
        const uint32_t take = run < left ? run : left;
        LRSC_UNROLL
        for(uint32_t k = 0; k < 5; ++k) cnt[k] += unit_slot(unit_code(u)) == k ? take : 0u;
        at += run;
    }
}

// the last lane l in [0, n_lanes] with starts[l] <= x; starts[0] = 0, so there is one
LRSC_HD uint32_t unrle_find_lane(const uint32_t* starts, uint32_t n_lanes, uint32_t x)
{
    uint32_t a = 0, b = n_lanes + 1;                               // starts[a] <= x, and starts[b] > x or b is the end
    while(b - a > 1) {
        const uint32_t m = (a + b) >> 1;
        if(starts[m] <= x) a = m; else b = m;
    }
    return a;
}

// The unit of the chunk that holds the chunk's symbol x < starts[n_lanes], as its index among the chunk's units, and how many
// of its symbols lie before x.
struct UnitAt {
    uint32_t unit, off;
};
LRSC_HD UnitAt unrle_locate(const uint8_t* units, const uint32_t* starts, uint32_t n_lanes, uint32_t x)
{
    uint32_t l = unrle_find_lane(starts, n_lanes - 1, x);
    uint32_t i = 16 * l, at = starts[l];
    // x < starts[l + 1]: the lane's sixteen units reach beyond x, so the walk ends inside them
    for(uint32_t run = unit_run(units[i]); at + run <= x; run = unit_run(units[i])) {
        at += run;
        ++i;
    }
    return UnitAt{i, x - at};
}

// Symbols [x, x + n_syms) of the chunk, n_syms <= 16 and x + n_syms <= starts[n_lanes], as codes; the rest of the Sym16 is 0.
LRSC_HD Sym16 expand_sym16(const uint8_t* units, const uint32_t* starts, uint32_t n_lanes, uint32_t x, uint32_t n_syms)
{
    Sym16 v{{0u, 0u, 0u, 0u}};
    if(n_syms == 0) return v;
    const UnitAt f = unrle_locate(units, starts, n_lanes, x);
    uint32_t i = f.unit;
    uint32_t code = unit_code(units[i]), left = unit_run(units[i]) - f.off;
    LRSC_UNROLL
    for(uint32_t j = 0; j < 16; ++j) {
        if(j < n_syms) {
            if(left == 0) {                                        // j < n_syms: symbol x + j exists, and so does the unit that holds it
                ++i;
                code = unit_code(units[i]);
                left = unit_run(units[i]);
            }
            v.w[j >> 2] |= code << (8 * (j & 3));
            --left;
        }
    }
    return v;
}

// ---- the device decoder (fm_unrle.hip) ----
// Packs the N symbols that d_units[0..n_units) encode (on the current device, 16-byte aligned as hipMalloc returns it) into
// Block64 (wide) or Block32 blocks: what build_strand_image makes of the same units, and what pack_strand_device makes of the
// decoded bytes.  Returns an lrsc_status; on an error nothing stays allocated.  A corrupt unit, or runs that do not add up to
// N, give LRSC_ERR_FORMAT with build_strand_image's text and no kernel has indexed anything by them; *first_bad (optional) is
// the index of the first corrupt unit, or ~0 when there is none.  Otherwise the three arrays of `out` are the caller's (hipFree).
int pack_units_device(const uint8_t* d_units, uint64_t n_units, uint64_t N, bool wide, PackedStrand& out, uint64_t* first_bad,
                      std::string& err);

} // namespace lrsc
