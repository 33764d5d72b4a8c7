// fm_kmerize.h -- a read cut at its unreliable k-mers, a pair merged or cut, and the sampled k-mer counts: the per-lane, per-read
// and per-pair code of fm_kmerize.hip, the reference's FMIndexWalkProcess::MergeAndKmerize, KmerizeReads, splitRead(KmerContext&),
// isSimple, numNextKmer, isLowComplexity and maxCon (FMIndexWalk/FMIndexWalkProcess.cpp:29-150, 229-267, 394-477, 555-609, 855-881),
// KmerContext (FMIndexWalkProcess.h:61-130) and BWTAlgorithms::sampleKmerCounts without its rand() (SuffixTools/BWTAlgorithms.cpp:
// 135-141, 396-402, 454-469, 527-539) on the rank-block layout.  The trim, the walk and the counts are fm_fmwalk.h's, unchanged.
//
// One wavefront owns a read's split (km_split), a pair's gate (km_gate_pair) and, as in fm_fmwalk.h, one walk.
//
//   split     the two single-strand counts of every k-mer in .bwt, lanes = (position, strand), 32 positions a phase; what they
//             leave is one byte per (position, strand): is the count at the threshold or above.  A scan lists the boundaries p
//             where the k-mers p - 1 and p are not both solid on both strands, and only those are probed: kKmProbe boundaries a
//             phase, lanes = (boundary, direction, base, strand), the trim's probe.  A boundary splits unless exactly one base
//             extends k-mer p - 1 to the right and exactly one extends k-mer p to the left.  A scan over the split flags numbers
//             the pieces in read order; a lane per piece then has its length, whether it holds a k-mer solid on both strands,
//             and (hybrid) its two filters.  The main piece is the first of those with the greatest span among the pieces that
//             hold such a k-mer, a span of 0 never: two reductions.
//   gate      both reads trimmed (fw_trim), the [k, m] length gate, the early return, and isSuitableForFMWalk: four counts of the
//             first m-mers, lanes = (read, strand).
//   sample    one lane per sample: up to len LF steps from a '$' row of .rbwt, the bases to a workspace row, then the two
//             searches of countSequenceOccurrences in .rbwt.
//
// The per-position flags and lists of a split live in one slice of a global workspace (KmWork), sized from the longest read of
// the call: a read's length is bounded by the ABI's 32 bits alone.  Nothing is indexed before its range was checked; an interval
// that leaves the strand sets `bad`.  All functions here are LRSC_HD and free of HIP types: the kernels call them, and
// tests/host_tools/fmwalk_hybrid_driver.cpp compiles the same source for the CPU.
#pragma once
#include <stdint.h>

#include "fm_fmwalk.h"

namespace lrsc {

constexpr uint32_t kKmLanes = kWaveLanes;
constexpr uint32_t kKmThreads = 256;                              // four wavefronts per workgroup, one mask table
constexpr uint32_t kKmWavesPerSimd = 4;                           // as kFwWavesPerSimd: a lane holds a rank block, an interval and a view
constexpr uint32_t kKmProbe = 4;                                  // boundaries of an isSimple phase: 4 x 2 directions x 4 bases x 2 strands
constexpr uint32_t kKmMaxSampleLength = 4096;                     // lrsc_kmer_sample_counts' len (LRSC_ERR_UNSUPPORTED above it)
constexpr uint32_t kKmWalkThreshold = 3;                          // SAIntervalTree's default SA_threshold: MergeAndKmerize passes none

struct KmPiece {                                                  // lrsc_fmwalk_piece
    uint32_t start, length, kept;
};
struct KmRead {                                                   // lrsc_fmwalk_read_result
    uint32_t kmerize;
    int32_t head;
    uint32_t length, n_pieces;
    int32_t main_piece;
    uint32_t whole;
};
struct KmHybrid {                                                 // lrsc_fmwalk_hybrid_result
    FwResult walk;
    KmRead read[2];
};
// a split to run: read[head .. head + len) of the staged reads, len >= k, its pieces from `slot` on
struct KmJob {
    uint32_t read, head, len, pad;
    uint64_t slot;
};
struct KmJobOut {
    uint32_t n_pieces;
    int32_t main_piece;
};
// what the gate leaves of a pair
enum : uint32_t { kKmGate = 1u, kKmReturned = 2u, kKmWalk = 4u };
struct KmGate {
    int32_t head[2];
    uint32_t trimmed[2];
    uint32_t flags, pad;
};

// One wavefront's slice of the split's workspace, for reads of up to `cap` k-mers.
struct KmWork {
    uint8_t* base;
    uint32_t cap;                                                 // a multiple of 8
    LRSC_HD uint8_t* solid() const { return base; }                                                           // 2 cap: (position, strand)
    LRSC_HD uint8_t* split() const { return base + 2ull * cap; }                                              // cap
    LRSC_HD uint32_t* list() const { return reinterpret_cast<uint32_t*>(base + 4ull * cap); }                  // cap: boundaries, then the pieces' keys
};
LRSC_HD KmWork km_work_at(uint8_t* base, uint32_t longest)
{
    KmWork w;
    w.base = base;
    w.cap = (longest + 7u) & ~7u;
    return w;
}
LRSC_HD uint64_t km_workspace_bytes(uint32_t longest)            // a multiple of 8
{
    const uint64_t cap = ((uint64_t)longest + 7u) & ~7ull;
    return 8ull * cap;
}

// isLowComplexity of s[0 .. len), len >= 1: the reference's float quotient held against the double 0.9, so that exactly nine
// tenths is not low
LRSC_HD bool km_low_complexity(const uint8_t* s, uint32_t len)
{
    uint32_t a = 0, c = 0, g = 0, t = 0;
    for(uint32_t i = 0; i < len; ++i) {
        const uint32_t code = s[i] & 3u;
        a += code == 0u ? 1u : 0u;
        c += code == 1u ? 1u : 0u;
        g += code == 2u ? 1u : 0u;
        t += code == 3u ? 1u : 0u;
    }
    const float n = (float)len;
    return (double)((float)a / n) >= 0.9 || (double)((float)t / n) >= 0.9 || (double)((float)c / n) >= 0.9 || (double)((float)g / n) >= 0.9;
}
// maxCon as written, the last position's own branch included (no N stands among codes)
LRSC_HD uint64_t km_max_con(const uint8_t* s, uint32_t len)
{
    uint64_t c = 1, max = 1;
    for(uint32_t i = 1; i < len; ++i) {
        if(s[i] != s[i - 1]) {
            if(c > max) max = c;
            c = 1;
        } else {
            ++c;
            if(i == len - 1) {
                if(c > max) max = c;
            } else if(s[i] != s[i + 1]) {
                if(c > max) max = c;
            }
        }
    }
    return max;
}

// splitRead(KmerContext(read[0 .. n), k)), n >= k, with MergeAndKmerize's filters when `filters`: pieces[0 .. n_pieces) in read
// order (start within read[], length, kept), main_piece = mainSeedIdx.  att: kKmLanes words.
//
// VALIDATE is splitRead(std::string&) (613-722), ValidateReads' split, which differs in three places.  A k-mer qualifies by the sum
// of its two counts: both of its bytes in solid() then say so, and the boundaries to probe are found as above.  The reference takes
// that sum from an interval that grows along the read and restarts at k bases when it falls below the threshold; a string occurs no
// more often than its last k bases, so this is the k-mer's own sum at every position.  A threshold of 2^32 or more is never met
// (ValidateReads' `threshold - 1` of 0 is one).  The only filter is isLowComplexity, and the main piece needs no solid k-mer.
template <class Block, class W, bool VALIDATE = false>
LRSC_HD void km_split(const StrandView<Block>& bwt, const uint32_t* mtab, const uint8_t* read, uint32_t n, uint32_t k, uint64_t threshold, bool filters,
                      const KmWork& ws, uint32_t* att, W& w, KmPiece* pieces, uint32_t& n_pieces, int32_t& main_piece, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t nk = n - k + 1;
    n_pieces = 0;
    main_piece = -1;
    if(nk > ws.cap) { bad = 1; return; }
    // ---- KmerContext: kmerFreqs_same and kmerFreqs_revc against the threshold
    for(uint32_t p0 = 0; p0 < nk; p0 += kKmLanes / 2) {
        w.each([&](uint32_t lane) {
            const uint32_t p = p0 + (lane >> 1);
            if(VALIDATE) att[lane] = 0;
            if(p >= nk) return;
            const uint64_t c = fw_count<Block>(bwt, mtab, k, (lane & 1u) != 0, [&](uint32_t i) -> uint32_t { return (uint32_t)read[p + i]; }, bad, n_rank, n_blk);
            if(VALIDATE) att[lane] = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;      // the sum still says whether a threshold below 2^32 is met
            else ws.solid()[2ull * p + (lane & 1u)] = c >= threshold ? 1 : 0;
        });
        if(VALIDATE) w.each([&](uint32_t lane) {
            const uint32_t p = p0 + (lane >> 1);
            if(p < nk) ws.solid()[2ull * p + (lane & 1u)] = threshold <= 0xFFFFFFFFull && (uint64_t)att[lane] + att[lane ^ 1u] >= threshold ? 1 : 0;
        });
    }
    if(fw_any_bad(w, bad)) return;
    // ---- the boundaries that isSimple is asked about
    uint32_t n_list = 0;
    for(uint32_t p0 = 0; p0 < nk; p0 += kKmLanes) {
        n_list += w.scan([&](uint32_t lane) -> uint32_t {
            const uint32_t p = p0 + lane;
            if(p >= nk) return 0u;
            ws.split()[p] = 0;
            if(p == 0) return 0u;
            const uint8_t* s = ws.solid() + 2ull * p;
            return s[-2] + s[-1] == 2 && s[0] + s[1] == 2 ? 0u : 1u;
        }, [&](uint32_t lane, uint32_t before, uint32_t mine) {
            if(mine) ws.list()[n_list + before] = p0 + lane;
        });
    }
    for(uint32_t j0 = 0; j0 < n_list; j0 += kKmProbe) {
        w.each([&](uint32_t lane) {
            const uint32_t j = j0 + (lane >> 4);
            uint32_t hit = 0;
            if(j < n_list) {
                const uint32_t p = ws.list()[j], base = (lane >> 1) & 3u;
                const bool start = ((lane >> 3) & 1u) != 0;       // NK_START of k-mer p; else NK_END of k-mer p - 1
                const uint64_t c = fw_count<Block>(bwt, mtab, k, (lane & 1u) != 0, [&](uint32_t i) -> uint32_t {
                    if(start) return i == 0 ? base : (uint32_t)read[p + i - 1];
                    return i == k - 1 ? base : (uint32_t)read[p + i];
                }, bad, n_rank, n_blk);
                hit = c ? 1u : 0u;
            }
            att[lane] = hit;
        });
        w.each([&](uint32_t lane) {
            if(lane < kKmProbe && j0 + lane < n_list)
                ws.split()[ws.list()[j0 + lane]] = fw_branches(att, 2 * lane) == 1 && fw_branches(att, 2 * lane + 1) == 1 ? 0 : 1;
        });
    }
    if(fw_any_bad(w, bad)) return;
    // ---- the intervals in read order
    uint32_t np = 0;
    for(uint32_t p0 = 0; p0 < nk; p0 += kKmLanes) {
        np += w.scan([&](uint32_t lane) -> uint32_t {
            const uint32_t p = p0 + lane;
            return p < nk && (p == 0 || ws.split()[p]) ? 1u : 0u;
        }, [&](uint32_t lane, uint32_t before, uint32_t mine) {
            if(mine) pieces[np + before].start = p0 + lane;
        });
    }
    // ---- a piece's length, its filters, and its key: second - first when it holds a k-mer solid on both strands, else 0
    for(uint32_t i0 = 0; i0 < np; i0 += kKmLanes) {
        w.each([&](uint32_t lane) {
            const uint32_t i = i0 + lane;
            if(i >= np) return;
            const uint32_t first = pieces[i].start, last = i + 1 < np ? pieces[i + 1].start - 1 : nk - 1, len = last - first + k;
            bool strong = VALIDATE;
            for(uint32_t p = first; !VALIDATE && p <= last; ++p) strong = strong || ws.solid()[2ull * p] + ws.solid()[2ull * p + 1] == 2;
            uint32_t kept = 1;
            if(VALIDATE ? km_low_complexity(read + first, len) : filters && (km_low_complexity(read + first, len) || km_max_con(read + first, len) * 3 > (uint64_t)len))
                kept = 0;
            pieces[i].length = len;
            pieces[i].kept = kept;
            ws.list()[i] = strong ? last - first : 0u;
        });
    }
    // ---- mainSeedIdx: the first piece with the strictly greatest key, none when every key is 0
    const uint32_t best = ~w.min_over([&](uint32_t lane) -> uint32_t {
        uint32_t r = kWaveNone;
        for(uint32_t i = lane; i < np; i += kKmLanes) r = ~ws.list()[i] < r ? ~ws.list()[i] : r;
        return r;
    });
    if(best != 0) {
        main_piece = (int32_t)w.min_over([&](uint32_t lane) -> uint32_t {
            for(uint32_t i = lane; i < np; i += kKmLanes)
                if(ws.list()[i] == best) return i;
            return kWaveNone;
        });
    }
    n_pieces = np;
}

// MergeAndKmerize up to its walks, of one pair, r1[0 .. n1) and r2[0 .. n2) its reads' codes: the trims (a read shorter than k,
// on which the reference throws, counts as trimmed to nothing), the [k, m] gate, the return when a trimmed read is shorter than
// k, and isSuitableForFMWalk with the given repeat_kmer_freq.  When the pair is to be walked the walks' strings a, b, rc(a),
// rc(b) stand at strs + 0, m4, 2 m4, 3 m4 as fw_trim_pair leaves them.  att: kKmLanes words.
template <class Block, class W>
LRSC_HD void km_gate_pair(const StrandView<Block>& bwt, const uint32_t* mtab, const uint8_t* r1, uint32_t n1, const uint8_t* r2, uint32_t n2, const FwParams& p,
                          uint64_t repeat_kmer_freq, uint32_t* att, W& w, uint8_t* strs, uint32_t m4, KmGate& g, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t k = (uint32_t)p.kmer_length, m = (uint32_t)p.min_overlap;
    g = KmGate{{0, 0}, {0u, 0u}, 0u, 0u};
    LRSC_FW_NOUNROLL
    for(uint32_t r = 0; r < 2; ++r) {
        const uint32_t n = r ? n2 : n1;
        if(n < k) continue;
        int32_t head = 0, tail = 0;
        fw_trim<Block>(bwt, mtab, r ? r2 : r1, n, k, att, w, head, tail, bad, n_rank, n_blk);
        g.head[r] = head > tail ? 0 : head;
        g.trimmed[r] = head > tail ? 0u : (uint32_t)(tail - head) + k;
    }
    if(fw_any_bad(w, bad)) return;
    const uint32_t t1 = g.trimmed[0], t2 = g.trimmed[1];
    if((t1 <= m && t1 >= k) || (t2 <= m && t2 >= k)) g.flags |= kKmGate;
    else if(t1 < k || t2 < k) {
        g.flags |= kKmReturned;
        return;
    }
    if(t1 < m || t2 < m) return;                                  // isBothReadLengthSufficient
    uint64_t freq[2];
    LRSC_FW_NOUNROLL
    for(uint32_t r = 0; r < 2; ++r) {
        const uint8_t* s = (r ? r2 : r1) + (uint32_t)g.head[r];
        freq[r] = w.sum64_over([&](uint32_t lane) -> uint64_t {
            if(lane >= 2) return 0ull;
            return fw_count<Block>(bwt, mtab, m, (lane & 1u) != 0, [&](uint32_t i) -> uint32_t { return (uint32_t)s[i]; }, bad, n_rank, n_blk);
        });
    }
    if(fw_any_bad(w, bad)) return;
    if(!(freq[0] < repeat_kmer_freq && freq[1] < repeat_kmer_freq)) return;
    g.flags |= kKmWalk;
    w.each([&](uint32_t lane) {
        for(uint32_t i = lane; i < m; i += kKmLanes) {
            const uint8_t a = r1[(uint32_t)g.head[0] + i] & 3u, b = r2[(uint32_t)g.head[1] + i] & 3u;
            strs[i] = a;
            strs[m4 + i] = b;
            strs[2 * m4 + m - 1 - i] = a ^ 3u;
            strs[3 * m4 + m - 1 - i] = b ^ 3u;
        }
    });
}
// ((len1 + len2) / 2) * 0.95, of the untrimmed lengths, as the reference's size_t <- double
LRSC_HD uint32_t km_max_overlap(const FwParams& p, uint32_t n1, uint32_t n2)
{
    return p.max_overlap != -1 ? (uint32_t)p.max_overlap : (uint32_t)((double)(((uint64_t)n1 + n2) / 2) * 0.95);
}
// MergeAndKmerize's three accept rules (FMIndexWalkProcess.cpp:77-103): 0, 1, or kFwNone.  same = mergedseq1 == rc(mergedseq2).
LRSC_HD uint32_t km_choose(const FwWalkOut& w0, const FwWalkOut& w1, bool same)
{
    const bool few = w0.max_used <= 1 && w1.max_used <= 1;
    if(w0.length != 0 && w1.length == 0 && few) return 0;
    if(w0.length == 0 && w1.length != 0 && few) return 1;
    if(w0.length != 0 && w1.length != 0 && same) return w0.coverage > w1.coverage ? 0u : 1u;
    return kFwNone;
}

// One pair, start to end, as the kernels and the entry do it between them: the gate (hybrid_gate_kernel), the two walks with the
// constructor's threshold (hybrid_walk_kernel), the choice and, for a pair that is not merged, the splits of its trimmed reads
// with the filters (kmerize_split_kernel), their pieces' starts within the untrimmed reads (lrsc_fmwalk_hybrid).  pieces[e]:
// the slots of read e, n_e - k + 1 of them.  merged[0 .. res.walk.length) = the merged string's codes when res.walk.merged.
template <class Block, class W>
LRSC_HD void km_hybrid_pair(const StrandView<Block>* views, const uint32_t* mtab, const uint8_t* r1, uint32_t n1, const uint8_t* r2, uint32_t n2, const FwParams& p,
                            uint64_t repeat_kmer_freq, const FwWork& ws, const KmWork& kws, W& w, uint8_t* merged, KmHybrid& res, KmPiece* const pieces[2],
                            uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t k = (uint32_t)p.kmer_length;
    KmGate g;
    km_gate_pair<Block>(views[0], mtab, r1, n1, r2, n2, p, repeat_kmer_freq, ws.att(), w, ws.str(0), ws.m4, g, bad, n_rank, n_blk);
    if(fw_any_bad(w, bad)) return;
    const uint32_t gate = (g.flags & kKmGate) ? 1u : 0u;
    res.walk = FwResult{0u, 0u, {0, 0}, {0u, 0u}, {0ull, 0ull}, {g.trimmed[0], g.trimmed[1]}};
    for(uint32_t e = 0; e < 2; ++e) res.read[e] = KmRead{gate, g.head[e], g.trimmed[e], 0u, -1, gate};
    if(g.flags & kKmWalk) {
        FwParams wp = p;
        wp.kmer_threshold = (int32_t)kKmWalkThreshold;
        FwWalkOut o[2] = {FwWalkOut{0, 0u, 0u, 0u, 0ull}, FwWalkOut{0, 0u, 0u, 0u, 0ull}};
        for(uint32_t wk = 0; wk < 2; ++wk) {
            fw_walk<Block>(views, mtab, ws.str(wk), ws.str(3 - wk), wp, km_max_overlap(wp, n1, n2), ws, w, o[wk], bad, n_rank, n_blk);
            if(fw_any_bad(w, bad)) return;
            w.each([&](uint32_t lane) {
                for(uint32_t i = lane; i < o[wk].length; i += kKmLanes) ws.kept(wk)[i] = ws.best()[i];
            });
        }
        const bool same = o[0].length != 0 && o[0].length == o[1].length && w.min_over([&](uint32_t lane) -> uint32_t {
            for(uint32_t i = lane; i < o[0].length; i += kKmLanes)
                if(ws.kept(0)[i] != (ws.kept(1)[o[0].length - 1 - i] ^ 3u)) return 0u;
            return kWaveNone;
        }) == kWaveNone;
        const uint32_t pick = km_choose(o[0], o[1], same);
        res.walk.status[0] = o[0].status; res.walk.status[1] = o[1].status;
        res.walk.max_used_leaves[0] = o[0].max_used; res.walk.max_used_leaves[1] = o[1].max_used;
        res.walk.coverage[0] = o[0].coverage; res.walk.coverage[1] = o[1].coverage;
        if(pick != kFwNone) {
            res.walk.merged = 1;
            res.walk.length = o[pick].length;
            w.each([&](uint32_t lane) {
                for(uint32_t i = lane; i < res.walk.length; i += kKmLanes) merged[i] = ws.kept(pick)[i];
            });
            return;
        }
    }
    if(g.flags & kKmReturned) return;
    for(uint32_t e = 0; e < 2; ++e) {
        if(g.trimmed[e] < k) continue;
        const uint32_t head = (uint32_t)g.head[e];
        KmPiece* to = pieces[e];
        km_split<Block>(views[0], mtab, (e ? r2 : r1) + head, g.trimmed[e], k, (uint32_t)p.kmer_threshold, true, kws, ws.att(), w, to, res.read[e].n_pieces,
                        res.read[e].main_piece, bad, n_rank, n_blk);
        if(fw_any_bad(w, bad)) return;
        res.read[e].kmerize = 1;
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < res.read[e].n_pieces; i += kKmLanes) to[i].start += head;
        });
    }
}

// One sample of sampleKmerCounts: extractString(rbwt, row, len), its bases in the order the LF steps give them to out[0 .. len),
// then countSequenceOccurrences of the string in .rbwt.  row < the strand's '$' rows.
template <class Block>
LRSC_HD uint64_t km_sample_count(const StrandView<Block>& rbwt, const uint32_t* mtab, uint64_t row, uint32_t len, uint8_t* out, uint32_t& bad, uint32_t& n_rank,
                                 uint32_t& n_blk)
{
    using P = typename BlockLay<Block>::pos_t;
    P i = (P)row;
    uint32_t n = 0;
    while(n < len) {
        if((uint64_t)i >= rbwt.N) { bad = 1; return 0; }
        const uint64_t g = block_of<Block>(i);
        const Block b = rbwt.blocks[g];
        const uint32_t code = block_symbol(b, (uint32_t)(i - (P)(g * Block::kSyms)));
        uint64_t rank = 0;
        n_rank += 1;
        n_blk += 1;
        if(!lf_step(rbwt, b, mtab, i, rank)) break;               // '$'
        out[n++] = (uint8_t)code;
    }
    if(n == 0) return 0;
    // the string is reverse(out): a backward search of it reads out[] from its front, one of its reverse complement from its end
    uint64_t c = 0;
    FwIv v;
    if(!fw_search<Block>(rbwt, mtab, n, [&](uint32_t t) -> uint32_t { return out[t]; }, v, n_rank, n_blk)) { bad = 1; return 0; }
    c += fw_size(v);
    if(!fw_search<Block>(rbwt, mtab, n, [&](uint32_t t) -> uint32_t { return (uint32_t)out[n - 1 - t] ^ 3u; }, v, n_rank, n_blk)) { bad = 1; return 0; }
    c += fw_size(v);
    return c;
}

} // namespace lrsc
