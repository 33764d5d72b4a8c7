// fm_dup.h -- is a read a duplicate, or contained in another read: the per-lane arithmetic of the device duplicate check
// (fm_dup.hip), the reference's QCProcess::performDuplicateCheck (Algorithm/QCProcess.cpp:206-265) on the rank-block layout.
//
// The reference looks a read w and its reverse complement rc up with the synchronised update of an interval pair.  What it uses
// of the result are four plain intervals, each a backward search of its own:
//
//   kind 0   w               in .bwt    consumes w[L-1], w[L-2], ... w[0]
//   kind 1   reverse(w)      in .rbwt   consumes w[0], w[1], ... w[L-1]
//   kind 2   rc              in .bwt    consumes comp(w[0]), comp(w[1]), ...
//   kind 3   complement(w)   in .rbwt   consumes comp(w[L-1]), comp(w[L-2]), ...
//
// A chain (dup_chain) is one lane's: a step (fm_strand.h's search_step) is one base and two Occ queries, one rank block when both
// ends of the interval lie in one block (the rule once the interval has narrowed), and a chain whose interval becomes empty ends there, as findIntervalPair
// does.  The bases are read a 32-bit word, four codes, at a time.  A chain that lives to its end reports its lower end, D(lower)
// and D(upper + 1), D(p) being the '$' rows of the strand before row p: D(upper + 1) - D(lower) rows of the interval have '$' as
// their preceding symbol, every other row is an extension by a base.
//
// dup_combine joins the four chains of a read: SUBSTRING when an interval holds an extension by a base, ABSENT when neither w
// nor rc is a read, else the canonical slot, the smaller valid lower of the two '$' intervals.  In .bwt the interval of a string s
// begins with its occurrences at the end of a read, suffix "s$", in read order; there are as many as the interval of reverse(s)
// in .rbwt has rows preceded by '$', E of them.  Those of the first E rows that are preceded by '$' themselves are the reads equal
// to s, so their ranks among the sorted reads are [D(lower), D(lower + E) - 1]: interval[0] after updateBothL(.., '$'), which
// for a read that is no SUBSTRING has no other row.  Of the reads of one call that share a slot the first in input order owns
// it (a minimum of read numbers), and it is UNIQUE when the slot's bit was clear before the call (dup_classify).  Nothing
// depends on the order in which lanes run.
//
// Every chain ends on any input: its steps are the read's bases, and an interval that leaves the strand reports kDupBroken.
// All functions here are LRSC_HD and free of HIP types: the kernels call them, and tests/host_tools/dup_driver.cpp compiles
// the same source for the CPU and holds it against the plain definition.
#pragma once
#include <stdint.h>

#include "fm_strand.h"

namespace lrsc {

constexpr uint32_t kDupThreads = 128;                             // lanes, one chain each, per workgroup; a workgroup holds chains of one kind
// Wavefronts per SIMD that the launch is sized for: a chain is dependent 64-byte loads and latency-bound, so the kernel has to
// stay within 512 / kDupWavesPerSimd VGPRs.
constexpr uint32_t kDupWavesPerSimd = 8;
constexpr uint32_t kDupKinds = 4;
constexpr uint32_t kDupNoWinner = 0xFFFFFFFFu;                    // a slot no read of the call has claimed

enum : uint32_t { kDupDead = 0, kDupLive = 1, kDupBroken = 2 };   // how a chain ended
// lrsc_dup_class
enum : int32_t { kDupUnique = 0, kDupSubstring = 1, kDupFullLength = 2, kDupAbsent = 3 };

struct DupChainOut {
    uint64_t lo;                                                  // lower of a live chain
    uint64_t d_lo, d_hi1;                                         // D(lower), D(upper + 1) of a live chain
    uint32_t state;
    uint32_t extended;                                            // the interval holds a row whose preceding symbol is a base
};
struct DupResult {                                                // lrsc_dup_result
    int64_t fwd_lower, fwd_upper, rvc_lower, rvc_upper;
    int32_t cls;
    uint32_t pad;
};

// strand of a kind (0 = .bwt, 1 = .rbwt), direction through the read, complement
LRSC_HD uint32_t dup_kind_strand(uint32_t kind) { return kind & 1u; }
LRSC_HD bool dup_kind_forward(uint32_t kind) { return kind == 1u || kind == 2u; }
LRSC_HD uint32_t dup_kind_flip(uint32_t kind) { return kind >= 2u ? 3u : 0u; }

// the codes of the reads, one per byte, as 32-bit words; a lane keeps the word it read last
struct DupReader {
    uint64_t at;
    uint32_t word;
};
LRSC_HD uint32_t dup_code(const uint32_t* words, uint64_t pos, DupReader& r)
{
    const uint64_t w = pos >> 2;
    if(w != r.at) { r.word = words[w]; r.at = w; }
    return (r.word >> (8 * (uint32_t)(pos & 3u))) & 3u;
}

// The '$' list of a strand without its rank blocks.
struct DupDollars {
    const uint64_t* dollars;
    const uint32_t* dollar_dir;
    uint64_t n_dollars;
    uint32_t block_syms;
};
template <class Block>
LRSC_HD DupDollars dup_dollars(const StrandView<Block>& S) { return DupDollars{S.dollars, S.dollar_dir, S.n_dollars, Block::kSyms}; }
// D(pos): '$' rows of the strand before row pos <= N
LRSC_HD uint64_t dup_d(const DupDollars& d, uint64_t pos) { return dollar_rank(d.dollars, d.n_dollars, d.dollar_dir, pos / d.block_syms, pos); }

// The chain of `kind` for the read at words[begin .. begin + len), len >= 1.  n_rank += the Occ queries, n_blk += the block loads.
template <class Block>
LRSC_HD DupChainOut dup_chain(const StrandView<Block>& S, const uint32_t* mtab, const uint32_t* words, uint64_t begin, uint32_t len, uint32_t kind,
                              uint32_t& n_rank, uint32_t& n_blk)
{
    using P = typename BlockLay<Block>::pos_t;
    const bool forward = dup_kind_forward(kind);
    const uint32_t flip = dup_kind_flip(kind);
    DupChainOut out{0, 0, 0, kDupDead, 0};
    DupReader rd{~0ull, 0};
    P lo = 0, hi1 = 0;                                            // the interval's rows are [lo, hi1)
    for(uint32_t t = 0; t < len; ++t) {
        const uint32_t code = dup_code(words, forward ? begin + t : begin + (len - 1 - t), rd) ^ flip;
        const P pred = strand_pred(S, code);
        if(t == 0) search_first(S, code, pred, lo, hi1);
        else search_step(S, mtab, code, pred, lo, hi1, n_rank, n_blk);
        if(hi1 > S.N || lo > hi1) { out.state = kDupBroken; return out; }     // never with the BWT of a string set
        if(lo == hi1) return out;                                 // the search string does not occur
    }
    out.state = kDupLive;
    const DupDollars dd = dup_dollars(S);
    out.lo = (uint64_t)lo;
    out.d_lo = dup_d(dd, (uint64_t)lo);
    out.d_hi1 = dup_d(dd, (uint64_t)hi1);
    out.extended = (uint64_t)(hi1 - lo) > out.d_hi1 - out.d_lo ? 1u : 0u;
    return out;
}

// the reads equal to the string of a .bwt chain, `in_bwt`, whose reversal is the .rbwt chain `in_rbwt`: true, with their ranks
// among the sorted reads in [lower, upper], when there are any
LRSC_HD bool dup_equal_reads(const DupDollars& bwt, uint64_t n_rows, const DupChainOut& in_bwt, const DupChainOut& in_rbwt, int64_t& lower, int64_t& upper)
{
    if(in_bwt.state != kDupLive || in_rbwt.state != kDupLive) return false;
    const uint64_t at_end = in_rbwt.d_hi1 - in_rbwt.d_lo;         // E
    if(at_end == 0 || at_end > n_rows || in_bwt.lo > n_rows - at_end) return false;
    const uint64_t d_end = dup_d(bwt, in_bwt.lo + at_end);
    if(d_end <= in_bwt.d_lo) return false;
    lower = (int64_t)in_bwt.d_lo;
    upper = (int64_t)d_end - 1;
    return true;
}

// The four chains of a read -> its '$' intervals and SUBSTRING / ABSENT, or a class still to be decided (kDupUnique) with the
// read's canonical slot.  bwt = the '$' list of .bwt, a strand of n_rows rows.  Returns false when a chain was broken.
LRSC_HD bool dup_combine(const DupDollars& bwt, uint64_t n_rows, const DupChainOut& c0, const DupChainOut& c1, const DupChainOut& c2, const DupChainOut& c3,
                         uint64_t n_slots, DupResult& r, uint64_t& slot)
{
    r = DupResult{0, -1, 0, -1, kDupAbsent, 0u};
    slot = ~0ull;
    if(c0.state == kDupBroken || c1.state == kDupBroken || c2.state == kDupBroken || c3.state == kDupBroken) return false;
    const bool fwd = dup_equal_reads(bwt, n_rows, c0, c1, r.fwd_lower, r.fwd_upper);
    const bool rvc = dup_equal_reads(bwt, n_rows, c2, c3, r.rvc_lower, r.rvc_upper);
    const uint32_t ext = (c0.state == kDupLive ? c0.extended : 0u) | (c1.state == kDupLive ? c1.extended : 0u) |
                         (c2.state == kDupLive ? c2.extended : 0u) | (c3.state == kDupLive ? c3.extended : 0u);
    if(ext) { r.cls = kDupSubstring; return true; }
    if(!fwd && !rvc) return true;
    slot = (uint64_t)(fwd && (!rvc || r.fwd_lower <= r.rvc_lower) ? r.fwd_lower : r.rvc_lower);
    if(slot >= n_slots) { slot = ~0ull; return false; }
    r.cls = kDupUnique;
    return true;
}
// the class of a read that claimed `slot`: winner = the smallest read number of the call that claimed it, bit = the slot's
// bit before the call
LRSC_HD int32_t dup_classify(bool bit, uint32_t winner, uint32_t read) { return !bit && winner == read ? kDupUnique : kDupFullLength; }

} // namespace lrsc
