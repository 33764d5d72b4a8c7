// fm_rle.h -- BWT codes -> RL units (the reference's .bwt/.rbwt payload), the per-lane arithmetic of the device encoder
// (fm_rle.hip).
//
// A unit is one byte, (code << 5) | run with run in 1..31, and the rule is BWTWriterBinary::writeBWChar's: the same symbol and
// a run below 31 extends the unit, anything else opens a new one.  So position i opens a unit when its symbol differs from the
// one before it, or when its distance from the head of its run is a multiple of 31.  That distance is the only thing that
// reaches back further than one symbol, and only its value modulo 31 matters: RunSummary carries it, rle_combine is the
// associative operator that joins the summaries of two adjacent stretches, and everything else is local to a stretch.
//
// The encoder works on tiles of kRleTile symbols; a tile is kRleLanes stretches of kRleChunks x 16 symbols, one per lane, in
// the Sym16 form of fm_pack.h.  The symbols come from the byte-per-symbol BWT, or from the rank blocks of a resident index
// copy through fm_strand.h's decode_block, the inverse of pack_block.  All functions here are LRSC_HD and free of HIP types:
// the kernels call them, and tests/host_tools/rle_driver.cpp compiles the same source for the CPU and holds it against the
// sequential rule.
#pragma once
#include <stdint.h>

#include <string>

#include "fm_strand.h"

#ifdef __HIPCC__
#define LRSC_ROLLED _Pragma("unroll 1")
#else
#define LRSC_ROLLED
#endif

namespace lrsc {

constexpr uint32_t kRleMaxRun = 31;                               // longest run one unit holds
constexpr uint32_t kRleLanes = 256;                               // stretches, and threads, per tile
constexpr uint32_t kRleChunks = 3;                                // Sym16 per stretch: odd, so the lanes' 16-byte LDS reads spread over the banks
constexpr uint32_t kRleTile = kRleLanes * kRleChunks * 16;        // 12288 symbols = 64 Block32 = 96 Block64
constexpr uint32_t kRleHalo = 32;                                 // symbols past a tile's end that its last unit may cover (30) rounded to Sym16
static_assert(kRleTile % Block32::kSyms == 0 && kRleTile % Block64::kSyms == 0, "a tile is whole rank blocks of either layout");
static_assert(kRleHalo >= kRleMaxRun - 1 && kRleHalo % 16 == 0, "halo");

// What a stretch of symbols tells the stretches after it.
struct alignas(4) RunSummary {
    uint8_t tail;    // length of its last run, modulo 31 (the run may have begun before the stretch once summaries are joined)
    uint8_t first;   // its first symbol
    uint8_t last;    // its last symbol
    uint8_t flags;   // kRleSome: not empty; kRleSingle: one single run
};
constexpr uint8_t kRleSome = 1, kRleSingle = 2;

// summary of a followed by b; associative, with the empty summary {0,0,0,0} as its identity
LRSC_HD RunSummary rle_combine(const RunSummary& a, const RunSummary& b)
{
    if(!(b.flags & kRleSome)) return a;
    if(!(a.flags & kRleSome)) return b;
    RunSummary r;
    r.first = a.first;
    r.last = b.last;
    if((b.flags & kRleSingle) && b.first == a.last) {             // b only prolongs a's last run
        const uint32_t t = (uint32_t)a.tail + b.tail;
        r.tail = (uint8_t)(t >= kRleMaxRun ? t - kRleMaxRun : t);
        r.flags = (uint8_t)(kRleSome | (a.flags & kRleSingle));
    } else {
        r.tail = b.tail;
        r.flags = kRleSome;
    }
    return r;
}
struct RleCombine {
    LRSC_HD RunSummary operator()(const RunSummary& a, const RunSummary& b) const { return rle_combine(a, b); }
};

// The walk over a stretch that all three phases share.  `in` summarises everything before the stretch (empty at the start of
// the BWT); f(i, c, opens) sees symbol c at i and whether it opens a unit.
template <uint32_t kChunks, class F>
LRSC_HD void rle_walk(const Sym16* s, uint32_t n_valid, const RunSummary& in, F&& f)
{
    uint32_t prev = (in.flags & kRleSome) ? in.last : 0xFFu;
    uint32_t r = in.tail;                                         // symbols of the current run so far, modulo 31
    // one Sym16 per turn of a rolled loop, and no way out of it but its end: unrolled with an exit per symbol, the kernels would
    // keep an execution mask for each of them
    LRSC_ROLLED
    for(uint32_t q = 0; q < kChunks && 16 * q < n_valid; ++q) {
        const Sym16 v = s[q];
        LRSC_UNROLL
        for(uint32_t j = 0; j < 16; ++j) {
            const uint32_t i = 16 * q + j;
            if(i < n_valid) {
                const uint32_t c = (v.w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                const bool opens = c != prev || r == 0;
                r = c != prev ? 1u : (r + 1 == kRleMaxRun ? 0u : r + 1);
                prev = c;
                f(i, c, opens);
            }
        }
    }
}

// phase 1: the summary of the first n_valid symbols of a stretch
template <uint32_t kChunks>
LRSC_HD RunSummary stretch_summary(const Sym16* s, uint32_t n_valid)
{
    RunSummary r{0, 0, 0, 0};
    if(n_valid == 0) return r;
    uint32_t run = 0, changes = 0, last = 0;
    rle_walk<kChunks>(s, n_valid, r, [&](uint32_t, uint32_t c, bool) {
        const bool same = run != 0 && c == last;
        changes += (run != 0 && !same) ? 1u : 0u;
        run = same ? run + 1 : 1u;
        last = c;
    });
    r.tail = (uint8_t)(run % kRleMaxRun);
    r.first = (uint8_t)sym_at(s, 0);
    r.last = (uint8_t)last;
    r.flags = (uint8_t)(kRleSome | (changes == 0 ? kRleSingle : 0));
    return r;
}

// phase 3: units that start in the stretch
template <uint32_t kChunks>
LRSC_HD uint32_t stretch_count(const Sym16* s, uint32_t n_valid, const RunSummary& in)
{
    uint32_t n = 0;
    rle_walk<kChunks>(s, n_valid, in, [&](uint32_t, uint32_t, bool opens) { n += opens ? 1u : 0u; });
    return n;
}

// phase 4: writes the stretch_count units that start in the stretch to out.  The last of them may run on past the stretch:
// s[kChunks...] holds the symbols that follow, of which n_after (at most kRleMaxRun - 1 are looked at) exist.
template <uint32_t kChunks>
LRSC_HD void stretch_emit(const Sym16* s, uint32_t n_valid, const RunSummary& in, uint32_t n_after, uint8_t* out)
{
    uint32_t n = 0, len = 0, code = 0;                            // len == 0: the unit that is open began before the stretch
    rle_walk<kChunks>(s, n_valid, in, [&](uint32_t, uint32_t c, bool opens) {
        if(opens) {
            if(len) out[n++] = (uint8_t)((code << 5) | len);
            code = c;
            len = 1;
        } else if(len) ++len;
    });
    if(!len) return;
    for(uint32_t i = kChunks * 16; len < kRleMaxRun && i < kChunks * 16 + n_after && sym_at(s, i) == code; ++i) ++len;
    out[n] = (uint8_t)((code << 5) | len);
}

// ---- the device encoder (fm_rle.hip) ----
// RL units of d_bwt[0..N) (codes 0..4, one per byte, on the current device).  Returns an lrsc_status; on an error nothing stays
// allocated.  Otherwise *d_units (hipFree) holds *n_units bytes on the device, allocated at that size.
int rle_bwt_device(const uint8_t* d_bwt, uint64_t N, uint8_t** d_units, uint64_t* n_units, std::string& err);
// The same for one strand of an index copy on the current device, decoded from its rank blocks and '$' list.
int rle_strand_device(const FmStrand& strand, bool wide, uint8_t** d_units, uint64_t* n_units, std::string& err);

} // namespace lrsc
