// fm_validate.h -- a single read validated by walks inside it: the per-lane and per-read code of fm_validate.hip, the reference's
// FMIndexWalkProcess::ValidateReads (FMIndexWalk/FMIndexWalkProcess.cpp:269-391) with SAIntervalTree's single-read constructor and
// validate() (FMIndexWalk/SAIntervalTree.cpp:59-94, 173-237) and splitRead(std::string&) (FMIndexWalkProcess.cpp:613-722) on the
// rank-block layout.  The walk is fm_fmwalk.h's fw_walk without isTwoReadsOverlap, the split fm_kmerize.h's km_split in its
// VALIDATE form, the low-complexity filter km_low_complexity; nothing of them is restated here.
//
// One wavefront owns one of a read's two walks (vd_walk), and one wavefront the split of a read whose walks decide nothing.
//
//   walks     of a read of n > min_overlap bases.  Walk 0 goes from the read's first min_overlap bases to its last, walk 1 the same
//             on the read's reverse complement.  The depth limit is (size_t)(n * 1.1), max_overlap -1 stands for (size_t)(n * 0.9),
//             both in double arithmetic; the threshold is kmer_threshold, the reference's `threshold`, as in lrsc_fmwalk_merge.
//   decision  vd_decide (FMIndexWalkProcess.cpp:318-352): one string and the other walk did not run out of depth, or two strings:
//             the read is merged, and its sequence is the first of walk 0's and walk 1's strings that is no shorter than the
//             read, else the read itself.  Walk 1's string reads on the other strand and is given as it is.
//   split     everything else, with the threshold (size_t)kmer_threshold - 1, unsigned: 0 when kmer_threshold is 1, so that every
//             k-mer qualifies, and 2^64 - 1 when it is 0, so that none does (vd_split_threshold).
//
// A wavefront's workspace is FwWork, sized for the longest read of the call: max_insert = vd_depth(longest).  A walk's own depth
// limit is its read's.  All functions here are LRSC_HD and free of HIP types: the kernels call them, and
// tests/host_tools/fmwalk_validate_driver.cpp compiles the same source for the CPU.
#pragma once
#include <stdint.h>

#include "fm_kmerize.h"

namespace lrsc {

constexpr uint32_t kVdLanes = kWaveLanes;
constexpr uint32_t kVdThreads = 256;                              // four wavefronts per workgroup, one mask table
constexpr uint32_t kVdWavesPerSimd = 4;                           // as kFwWavesPerSimd

struct VdResult {                                                 // lrsc_fmwalk_validate_result
    uint32_t merged, length;
    int32_t status[2];
    uint32_t max_used_leaves[2];
    uint64_t coverage[2];
    uint32_t walk_length[2];
    int32_t chosen;
    KmRead read;
};

// maxSearchDepth and maxOverlap of a read of n bases, as the reference's size_t <- double
LRSC_HD uint32_t vd_depth(uint32_t n) { return (uint32_t)((double)n * 1.1); }
LRSC_HD uint32_t vd_max_overlap(const FwParams& p, uint32_t n) { return p.max_overlap != -1 ? (uint32_t)p.max_overlap : (uint32_t)((double)n * 0.9); }
// `threshold - 1` of ValidateReads' size_t
LRSC_HD uint64_t vd_split_threshold(int32_t kmer_threshold) { return (uint64_t)(int64_t)kmer_threshold - 1ull; }

// The first and the last m bases of the read (walk 0) or of its reverse complement (walk 1), to q[0 .. m) and e[0 .. m); n >= m.
template <class W>
LRSC_HD void vd_ends(const uint8_t* read, uint32_t n, uint32_t m, uint32_t walk, uint8_t* q, uint8_t* e, W& w)
{
    w.each([&](uint32_t lane) {
        for(uint32_t i = lane; i < m; i += kVdLanes) {
            q[i] = walk ? (read[n - 1 - i] & 3u) ^ 3u : read[i] & 3u;
            e[i] = walk ? (read[m - 1 - i] & 3u) ^ 3u : read[n - m + i] & 3u;
        }
    });
}

// SAIntervalTree(&s, m, maxOverlap, maxSearchDepth, L, indices, threshold).validate of s = the read or its reverse complement,
// n > m: the string to ws.best()[0 .. out.length).  p.max_insert is the call's (the workspace's); wp is p with the read's own.
template <class Block, class W>
LRSC_HD void vd_walk(const StrandView<Block>* views, const uint32_t* mtab, const uint8_t* read, uint32_t n, const FwParams& p, uint32_t walk, FwParams& wp,
                     const FwWork& ws, W& w, FwWalkOut& out, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t depth = vd_depth(n);
    if(n <= (uint32_t)p.min_overlap || depth > (uint32_t)p.max_insert) { bad = 1; return; }
    wp = p;
    wp.max_insert = (int32_t)depth;
    vd_ends(read, n, (uint32_t)p.min_overlap, walk, ws.str(0), ws.str(1), w);
    fw_walk<Block, W, false>(views, mtab, ws.str(0), ws.str(1), wp, w.uniform(vd_max_overlap(p, n)), ws, w, out, bad, n_rank, n_blk);
}

// FMIndexWalkProcess.cpp:318-352 of a read of n bases: is it merged, and whose string is its sequence (0, 1, or -1: the read's own)
LRSC_HD bool vd_decide(uint32_t n, const FwWalkOut& w0, const FwWalkOut& w1, int32_t& chosen, uint32_t& length)
{
    const bool s0 = w0.length != 0, s1 = w1.length != 0;
    const bool long0 = (double)w0.length / (double)n >= 1, long1 = (double)w1.length / (double)n >= 1;
    chosen = -1;
    length = 0;
    if(s0 && !s1 && w1.status != -2) chosen = long0 ? 0 : -1;
    else if(s1 && !s0 && w0.status != -2) chosen = long1 ? 1 : -1;
    else if(s0 && s1) chosen = long0 ? 0 : (long1 ? 1 : -1);
    else return false;
    length = chosen < 0 ? n : (chosen ? w1.length : w0.length);
    return true;
}
LRSC_HD VdResult vd_result(uint32_t n, const FwWalkOut& w0, const FwWalkOut& w1)
{
    VdResult r{0u, 0u, {w0.status, w1.status}, {w0.max_used, w1.max_used}, {w0.coverage, w1.coverage}, {w0.length, w1.length}, -1, KmRead{0u, 0, n, 0u, -1, 0u}};
    r.merged = vd_decide(n, w0, w1, r.chosen, r.length) ? 1u : 0u;
    return r;
}

// One read, start to end, as the kernels and the entry do it between them: the short read (lrsc_fmwalk_validate), the two walks
// (validate_walk_kernel, a wavefront each), the decision (the entry) and the split (validate_split_kernel).  seq[0 .. res.length)
// = the sequence's codes when res.merged; pieces: n - k + 1 slots when n >= k.
template <class Block, class W>
LRSC_HD void vd_read(const StrandView<Block>* views, const uint32_t* mtab, const uint8_t* read, uint32_t n, const FwParams& p, const FwWork& ws, const KmWork& kws, W& w,
                     uint8_t* seq, VdResult& res, KmPiece* pieces, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t k = (uint32_t)p.kmer_length;
    const FwWalkOut none{0, 0u, 0u, 0u, 0ull};
    if(n <= (uint32_t)p.min_overlap) {                            // correctSequence is the read; kmerize unless it is of low complexity
        res = vd_result(n, none, none);
        res.read.whole = 1;
        res.read.kmerize = km_low_complexity(read, n) ? 0u : 1u;
        return;
    }
    FwWalkOut o[2] = {none, none};
    for(uint32_t wk = 0; wk < 2; ++wk) {
        FwParams wp;
        vd_walk<Block>(views, mtab, read, n, p, wk, wp, ws, w, o[wk], bad, n_rank, n_blk);
        if(fw_any_bad(w, bad)) return;
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < o[wk].length; i += kVdLanes) ws.kept(wk)[i] = ws.best()[i];
        });
    }
    res = vd_result(n, o[0], o[1]);
    if(res.merged) {
        const uint8_t* from = res.chosen < 0 ? read : ws.kept((uint32_t)res.chosen);
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < res.length; i += kVdLanes) seq[i] = from[i] & 3u;
        });
        return;
    }
    if(n < k) return;                                             // the reference asserts: neither merged nor kmerized, nothing left
    km_split<Block, W, true>(views[0], mtab, read, n, k, vd_split_threshold(p.kmer_threshold), false, kws, ws.att(), w, pieces, res.read.n_pieces, res.read.main_piece,
                             bad, n_rank, n_blk);
    if(fw_any_bad(w, bad)) return;
    res.read.kmerize = 1;                                         // kmerReads is not empty
}

} // namespace lrsc
