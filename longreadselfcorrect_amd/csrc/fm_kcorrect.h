// fm_kcorrect.h -- k-mer read correction against a resident index: the per-lane and per-read code of the device corrector
// (fm_kcorrect.hip), the reference's ErrorCorrectProcess::kmerCorrection and attemptKmerCorrection
// (Algorithm/ErrorCorrectProcess.cpp:287-438, 488-544) on the rank-block layout.
//
// count(w) is the interval of w in .bwt plus that of revcomp(w) in .bwt, each a backward search of its own (kc_chain, on
// fm_strand.h's search_step): the forward chain consumes w[k-1] .. w[0], the other comp(w[0]) .. comp(w[k-1]).  A chain can be
// told to read one base of the read as another: the substitutions of an attempt are counted without touching the read.
//
// One wavefront owns a read (kc_correct_read).  Its state is the edited codes seq[n], a flag byte per base and the two counts
// per k-mer; `W` is fm_wave.h's wavefront, of which this uses each, min_over, sum_over and uniform.  A pass:
//
//   count     lanes take chains, k-mer by k-mer a forward and a reverse-complement one.  The first pass counts all nk k-mers, a
//             later one only those that cover the base the pass before changed: a count is a function of the k-mer's string.
//   solid     a k-mer is good when its count reaches the support of its lowest phred (kc_support); a base is solid when a good
//             k-mer covers it.  All solid: the read is done, kmer_qc = 1.
//   attempts  the unsolid bases from the left, kKcGroup at a time: 4 substitutes x 2 strands x (leftmost, rightmost covering
//             k-mer) = 16 chains per base fill the wavefront.  The decisions (kc_attempt) are taken in (base, left before right)
//             order and the first success ends the scan, so the result is that of one base at a time.
//
// Every loop is bounded by the read's length and by kmer_rounds + 2 passes on any input; an interval that leaves the strand
// (kKcBroken) ends the read.  All functions here are LRSC_HD and free of HIP types: the kernels call them, and
// tests/host_tools/kcorrect_driver.cpp compiles the same source for the CPU.
#pragma once
#include <stdint.h>

#include "fm_strand.h"
#include "fm_wave.h"

namespace lrsc {

constexpr uint32_t kKcLanes = kWaveLanes;                         // a wavefront: one read
constexpr uint32_t kKcThreads = 256;                              // four reads per workgroup, one mask table
// Wavefronts per SIMD that the launch is sized for: a chain is dependent 64-byte loads and latency-bound, so the kernel has to
// stay within 512 / kKcWavesPerSimd VGPRs (allocated in eights: 80) and a workgroup within 160 KiB / (4 * kKcWavesPerSimd /
// (kKcThreads / 64)) of LDS.  Six, not the duplicate check's eight: held to 64 VGPRs the pass loop spilled.
constexpr uint32_t kKcWavesPerSimd = 6;
// Reads up to this many bases keep their state in LDS (10 bytes per base and 256), longer ones in a global workspace.
constexpr uint32_t kKcLdsBases = 256;
constexpr uint32_t kKcGroup = 4;                                  // unsolid bases whose attempts share a wavefront step
constexpr uint32_t kKcChainsPerBase = kKcLanes / kKcGroup;        // 16
constexpr uint32_t kKcStateBytesPerBase = 10;                     // code, flag, two 32-bit counts

constexpr uint64_t kKcBroken = ~0ull;                             // a chain whose interval left the strand
constexpr uint32_t kKcNone = kWaveNone;
constexpr uint32_t kKcCountMax = 0x7FFFFFFFu;                     // a count is held as the reference holds it, in 31 bits

enum : uint8_t { kKcSolid = 1, kKcLowBase = 2, kKcLowKmer = 4, kKcGoodKmer = 8 };    // the flag byte of a base / of the k-mer that starts there

struct KcParams {                                                 // lrsc_kcorrect_params
    int32_t kmer_length, kmer_threshold, kmer_rounds, quality_cutoff;
};
struct KcResult {                                                 // lrsc_kcorrect_result
    uint32_t kmer_qc, n_changed, passes, pad;
};
// The state of one read, in LDS or in the workspace, the same code either way: two 32-bit counts per base (of the k-mer that
// starts there and of its reverse complement), the kKcLanes counts of an attempt step, the edited codes, a flag byte per base.
struct KcState {
    uint8_t* base;
    uint32_t n4;                                                  // the read's length, rounded up to a multiple of 4
    LRSC_HD uint32_t* cnt_fwd() const { return reinterpret_cast<uint32_t*>(base); }
    LRSC_HD uint32_t* cnt_rvc() const { return reinterpret_cast<uint32_t*>(base) + n4; }
    LRSC_HD uint32_t* att() const { return reinterpret_cast<uint32_t*>(base) + 2 * (uint64_t)n4; }
    LRSC_HD uint8_t* seq() const { return base + 8 * (uint64_t)n4 + 4 * kKcLanes; }
    LRSC_HD uint8_t* flag() const { return base + 9 * (uint64_t)n4 + 4 * kKcLanes; }
};
// bytes of the state of a read of n bases, a multiple of 4
LRSC_HD uint64_t kc_workspace_bytes(uint64_t n) { return ((n + 3) & ~3ull) * kKcStateBytesPerBase + 4 * kKcLanes; }
LRSC_HD KcState kc_state_at(uint8_t* base, uint32_t n) { return KcState{base, (n + 3u) & ~3u}; }

// required support of a phred score (Util/CorrectionThresholds.cpp): x at or above the cutoff, else x + 1
LRSC_HD uint32_t kc_support(bool low, const KcParams& p) { return (uint32_t)p.kmer_threshold + (low ? 1u : 0u); }

// The occurrences in strand S of the k-mer at seq[start .. start + k), or of its reverse complement (rvc), base ov_pos of the
// read taken as ov_code (ov_pos = kKcNone: none).  kKcBroken when the interval leaves the strand.  n_rank += the Occ queries,
// n_blk += the block loads.
template <class Block>
LRSC_HD uint64_t kc_chain(const StrandView<Block>& S, const uint32_t* mtab, const uint8_t* seq, uint32_t start, uint32_t k, bool rvc, uint32_t ov_pos,
                          uint32_t ov_code, uint32_t& n_rank, uint32_t& n_blk)
{
    using P = typename BlockLay<Block>::pos_t;
    P lo = 0, hi1 = 0;                                            // the interval's rows are [lo, hi1)
    for(uint32_t t = 0; t < k; ++t) {
        const uint32_t pos = rvc ? start + t : start + (k - 1 - t);
        uint32_t code = pos == ov_pos ? ov_code : (uint32_t)seq[pos];
        code = (code & 3u) ^ (rvc ? 3u : 0u);
        const P pred = strand_pred(S, code);
        if(t == 0) search_first(S, code, pred, lo, hi1);
        else search_step(S, mtab, code, pred, lo, hi1, n_rank, n_blk);
        if(hi1 > S.N || lo > hi1) return kKcBroken;               // never with the BWT of a string set
        if(lo == hi1) return 0;                                   // the k-mer does not occur
    }
    return (uint64_t)(hi1 - lo);
}
LRSC_HD uint32_t kc_clamp(uint64_t count) { return count > kKcCountMax ? kKcCountMax : (uint32_t)count; }
LRSC_HD uint32_t kc_count(const KcState& st, uint32_t i)
{
    const uint64_t c = (uint64_t)st.cnt_fwd()[i] + st.cnt_rvc()[i];
    return kc_clamp(c);
}

// the k-mers that cover base i of a read of n >= k bases: the leftmost and the rightmost
LRSC_HD uint32_t kc_left_kmer(uint32_t i, uint32_t k) { return i + 1 >= k ? i + 1 - k : 0u; }
LRSC_HD uint32_t kc_right_kmer(uint32_t i, uint32_t n, uint32_t k) { return i < n - k ? i : n - k; }

// attemptKmerCorrection's decision: c[b] the count of the k-mer with base b at the position, min_count, the base there now.
// Every base with c >= 2 * min_count replaces the best so far (the last one wins, not the largest); the correction is made when
// there is one and it differs from the original.  Returns the new base, or kKcNone.
LRSC_HD uint32_t kc_attempt(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t min_count, uint32_t original)
{
    const uint64_t need = 2ull * min_count;
    uint32_t best = kKcNone;
    best = c0 >= need ? 0u : best;
    best = c1 >= need ? 1u : best;
    best = c2 >= need ? 2u : best;
    best = c3 >= need ? 3u : best;
    return best == original ? kKcNone : best;
}

// what lane `lane` of an attempt step counts: group (which unsolid base), side (0 = leftmost, 1 = rightmost covering k-mer),
// substitute, strand
LRSC_HD uint32_t kc_lane_group(uint32_t lane) { return lane / kKcChainsPerBase; }
LRSC_HD uint32_t kc_lane_side(uint32_t lane) { return (lane >> 3) & 1u; }
LRSC_HD uint32_t kc_lane_code(uint32_t lane) { return (lane >> 1) & 3u; }
LRSC_HD bool kc_lane_rvc(uint32_t lane) { return (lane & 1u) != 0; }
LRSC_HD uint32_t kc_pick_group(uint32_t g, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3)
{
    return (g & 2u) ? ((g & 1u) ? b3 : b2) : ((g & 1u) ? b1 : b0);
}

// One read: orig[0 .. n) its codes, phred[0 .. n) its scores or nullptr (15 everywhere), st its state, out[0 .. n) the corrected
// codes.  Returns false when a chain was broken (out and res are then not written).  n_rank, n_blk: the caller's lane totals,
// as kc_chain counts them (on the CPU the totals of the read).
template <class Block, class W>
LRSC_HD bool kc_correct_read(const StrandView<Block>& S, const uint32_t* mtab, const uint8_t* orig, const uint8_t* phred, uint32_t n, const KcParams& p,
                             const KcState& st, W& w, uint8_t* out, KcResult& res, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t k = (uint32_t)p.kmer_length;
    if(n < k) {                                                   // nothing can be done: returned as it is
        w.each([&](uint32_t lane) {
            for(uint32_t j = lane; j < n; j += kKcLanes) out[j] = orig[j];
        });
        res = KcResult{0u, 0u, 0u, 0u};
        return true;
    }
    const uint32_t nk = n - k + 1;
    w.each([&](uint32_t lane) {
        for(uint32_t j = lane; j < n; j += kKcLanes) {
            st.seq()[j] = orig[j];
            st.flag()[j] = (phred != nullptr ? (int32_t)phred[j] : 15) < p.quality_cutoff ? kKcLowBase : 0;
        }
    });
    w.each([&](uint32_t lane) {                                   // the lowest phred of a k-mer decides its support
        for(uint32_t i = lane; i < nk; i += kKcLanes) {
            uint8_t low = 0;
            for(uint32_t j = i; j < i + k && !low; ++j) low = st.flag()[j] & kKcLowBase;
            if(low) st.flag()[i] |= kKcLowKmer;
        }
    });

    uint32_t from = 0, to = nk, passes = 0;
    bool solid = false, broken = false;
    const uint32_t max_passes = (uint32_t)p.kmer_rounds + 2;      // `if(rounds++ > maxAttempts) break;`
    while(passes < max_passes) {
        // ---- count the k-mers [from, to)
        const uint32_t n_chains = 2 * (to - from);
        const uint32_t bad = w.min_over([&](uint32_t lane) -> uint32_t {
            uint32_t r = kKcNone;
            for(uint32_t c = lane; c < n_chains; c += kKcLanes) {
                const uint32_t i = from + (c >> 1);
                const uint64_t v = kc_chain<Block>(S, mtab, st.seq(), i, k, (c & 1u) != 0, kKcNone, 0u, n_rank, n_blk);
                if(v == kKcBroken) r = 0;
                ((c & 1u) ? st.cnt_rvc() : st.cnt_fwd())[i] = kc_clamp(v);
            }
            return r;
        });
        ++passes;
        if(bad != kKcNone) { broken = true; break; }
        // ---- good k-mers, solid bases
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < nk; i += kKcLanes) {
                const uint8_t f = st.flag()[i];
                const bool good = kc_count(st, i) >= kc_support((f & kKcLowKmer) != 0, p);
                st.flag()[i] = good ? (uint8_t)(f | kKcGoodKmer) : (uint8_t)(f & ~kKcGoodKmer);
            }
        });
        const uint32_t first = w.min_over([&](uint32_t lane) -> uint32_t {
            uint32_t r = kKcNone;
            for(uint32_t j = lane; j < n; j += kKcLanes) {
                const uint32_t a = kc_left_kmer(j, k), b = kc_right_kmer(j, n, k);
                uint8_t good = 0;
                for(uint32_t i = a; i <= b && !good; ++i) good = st.flag()[i] & kKcGoodKmer;
                const uint8_t f = st.flag()[j];
                st.flag()[j] = good ? (uint8_t)(f | kKcSolid) : (uint8_t)(f & ~kKcSolid);
                if(!good && r == kKcNone) r = j;
            }
            return r;
        });
        if(first == kKcNone) { solid = true; break; }
        if(passes == max_passes) break;
        // ---- the attempts of the unsolid bases, kKcGroup at a time, until one succeeds
        bool corrected = false;
        uint32_t pos = first;
        while(pos < n && !corrected && !broken) {
            uint32_t b0 = kKcNone, b1 = kKcNone, b2 = kKcNone, b3 = kKcNone, found = 0;
            for(; pos < n && found < kKcGroup; ++pos)
                if(!(w.uniform(st.flag()[pos]) & kKcSolid)) {
                    b0 = found == 0 ? pos : b0;
                    b1 = found == 1 ? pos : b1;
                    b2 = found == 2 ? pos : b2;
                    b3 = found == 3 ? pos : b3;
                    ++found;
                }
            if(found == 0) break;
            const uint32_t bad_att = w.min_over([&](uint32_t lane) -> uint32_t {
                const uint32_t i = kc_pick_group(kc_lane_group(lane), b0, b1, b2, b3);
                uint64_t v = 0;
                if(i != kKcNone) {
                    const uint32_t at = kc_lane_side(lane) ? kc_right_kmer(i, n, k) : kc_left_kmer(i, k);
                    v = kc_chain<Block>(S, mtab, st.seq(), at, k, kc_lane_rvc(lane), i, kc_lane_code(lane), n_rank, n_blk);
                }
                st.att()[lane] = kc_clamp(v);
                return v == kKcBroken ? 0u : kKcNone;
            });
            if(bad_att != kKcNone) { broken = true; break; }
            for(uint32_t g = 0; g < found && !corrected; ++g) {
                const uint32_t i = kc_pick_group(g, b0, b1, b2, b3);
                const uint32_t t = kc_support((w.uniform(st.flag()[i]) & kKcLowBase) != 0, p);
                for(uint32_t side = 0; side < 2 && !corrected; ++side) {
                    const uint32_t at = side ? kc_right_kmer(i, n, k) : kc_left_kmer(i, k);
                    const uint32_t have = w.uniform(kc_count(st, at));
                    const uint32_t* a = st.att() + g * kKcChainsPerBase + side * 8;
                    const uint32_t best = w.uniform(kc_attempt(kc_clamp((uint64_t)a[0] + a[1]), kc_clamp((uint64_t)a[2] + a[3]), kc_clamp((uint64_t)a[4] + a[5]),
                                                               kc_clamp((uint64_t)a[6] + a[7]), have > t ? have : t, st.seq()[i]));
                    if(best != kKcNone) {
                        corrected = true;
                        from = kc_left_kmer(i, k);
                        to = kc_right_kmer(i, n, k) + 1;
                        w.each([&](uint32_t lane) {
                            if(lane == 0) st.seq()[i] = (uint8_t)best;
                        });
                    }
                }
            }
        }
        if(broken || !corrected) break;
    }
    if(broken) return false;
    // a read that is not all solid is returned unedited
    const uint32_t changed = w.sum_over([&](uint32_t lane) -> uint32_t {
        uint32_t d = 0;
        for(uint32_t j = lane; j < n; j += kKcLanes) {
            const uint8_t c = solid ? st.seq()[j] : orig[j];
            d += c != orig[j] ? 1u : 0u;
            out[j] = c;
        }
        return d;
    });
    res = KcResult{solid ? 1u : 0u, changed, passes, 0u};
    return true;
}

} // namespace lrsc
