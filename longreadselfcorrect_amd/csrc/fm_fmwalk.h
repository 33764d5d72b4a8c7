// fm_fmwalk.h -- paired-end reads merged by an FM-index walk: the per-lane and per-pair code of the device walk (fm_fmwalk.hip),
// the reference's FMIndexWalkProcess::MergePairedReads and trimRead (FMIndexWalk/FMIndexWalkProcess.cpp:153-226, 825-870) with
// SAIntervalTree::mergeTwoReads and what it calls (FMIndexWalk/SAIntervalTree.cpp:20-56, 103-170, 248-449, 494-507) on the
// rank-block layout.
//
// An interval is held as its rows [lo, hi1); it is valid when lo < hi1.  A backward-search step (fw_update) is fm_strand.h's
// search_step of an interval that is one of the strand.  A search (fw_search) ends where findInterval ends: at the first empty
// interval after the first step, whose rows it keeps, because isTwoReadsOverlap compares intervals whether they are valid or not.
//
// One wavefront owns a pair's trim (fw_trim_pair) and one each of its two walks (fw_walk); fw_merge_pair is the whole of a pair.
// `W` is fm_wave.h's wavefront, of which this uses each, min_over, sum64_over, scan, uniform and uniform64.
//
// views[0] is .bwt and views[1] is .rbwt; a lane picks its strand's by index, so the kernel keeps the two in LDS.
//
//   trim      fw_trim: the head and the tail k-mer first, 16 searches of k steps, one lane each; only when one is a dead end the
//             scan, kFwScan positions x 8 searches a step, of which the first position with two or more branches is taken: the
//             serial scan's result whatever the step.
//   walk      fw_walk: the frontier is an array of leaves (two intervals and a node of the tree) in frontier order.  A step takes
//             kFwRound leaves at a time, lane = (leaf, base, strand): the lane updates that strand's interval with the base, a
//             scan over the keep flags of the (leaf, base) pairs places the kept ones in leaf and then base order.  Every kept
//             extension is a new node (parent, base) of an append-only tree: the leaves' strings are never copied.  Refinement
//             (refineSAInterval) and the searches of the root and terminal intervals are chains, lane = (leaf, strand), over the
//             last min_overlap bases of the leaf, which a lane first reads back from the tree.
//   coverage  calculateKmerCoverage of every result in frontier order, lanes over (position, strand); the strictly greatest wins.
//
// All of a pair's state lives in one slice of a global workspace (FwWork): the tree does not fit LDS at the limits below (64
// leaves x 2000 steps), and every step loads rank blocks from memory anyway.  Every loop is bounded by the parameters; an
// interval that leaves the strand, or a tree that would outgrow its slice, sets `bad` and ends the pair (kernel: *broken = 1), and
// nothing is indexed before its range was checked.  All functions here are LRSC_HD and free of HIP types: the kernels call them,
// and tests/host_tools/fmwalk_driver.cpp compiles the same source for the CPU.
#pragma once
#include <stdint.h>

#include "fm_strand.h"
#include "fm_wave.h"

#if defined(__clang__)
#define LRSC_FW_NOUNROLL _Pragma("nounroll")
#else
#define LRSC_FW_NOUNROLL
#endif

namespace lrsc {

constexpr uint32_t kFwLanes = kWaveLanes;                         // a wavefront: one pair's trim, or one walk
constexpr uint32_t kFwThreads = 256;                              // four wavefronts per workgroup, one mask table
// Wavefronts per SIMD that the launch is sized for: a walk is dependent 64-byte loads and latency-bound, so more wavefronts hide
// more of it.  Four: 512 / 4 = 128 VGPRs hold a lane's rank block, interval and strand view (104 with 64-bit positions), which
// 512 / 5 rounded down to eights, 96, do not.  The walk kernel's grid is persistent, resident_waves(kFwWavesPerSimd) wavefronts that take walks in turn, so the
// workspace is one slice per wavefront.
constexpr uint32_t kFwWavesPerSimd = 4;
// the limits of lrsc_fmwalk_merge (LRSC_ERR_UNSUPPORTED above them)
constexpr uint32_t kFwMaxLeaves = 64;
constexpr uint32_t kFwMaxInsert = 2000;
constexpr uint32_t kFwMaxOverlap = 255;
constexpr uint32_t kFwMaxKmer = 255;
constexpr uint32_t kFwRound = 8;                                  // leaves of a step that share the wavefront: 8 x 4 bases x 2 strands
constexpr uint32_t kFwScan = 8;                                   // positions of a trim scan step: 8 x 4 bases x 2 strands
constexpr uint32_t kFwChainLeaves = kFwLanes / 2;                 // leaves whose refinement chains share the wavefront
constexpr uint32_t kFwNone = kWaveNone;

struct FwParams {                                                 // lrsc_fmwalk_params
    int32_t kmer_length, kmer_threshold, min_overlap, max_overlap, max_insert, max_leaves;
};
struct FwResult {                                                 // lrsc_fmwalk_result
    uint32_t merged, length;
    int32_t status[2];
    uint32_t max_used_leaves[2];
    uint64_t coverage[2];
    uint32_t trimmed_length[2];
};
struct FwIv {
    uint64_t lo, hi1;
};
struct FwLeaf {
    FwIv fwd, rvc;                                                // of reverse(s) in .rbwt, of revcomp(s) in .bwt, s the leaf's last kmerSize bases
    uint32_t node, pad;
};
LRSC_HD bool fw_valid(const FwIv& v) { return v.lo < v.hi1; }
LRSC_HD uint64_t fw_size(const FwIv& v) { return v.lo < v.hi1 ? v.hi1 - v.lo : 0ull; }
LRSC_HD bool fw_within(const FwIv& v, const FwIv& t) { return v.lo < v.hi1 && v.lo >= t.lo && v.hi1 <= t.hi1; }

// One wavefront's slice of the workspace.  A node of the tree is (parent << 2) | base; node 0 is the query.
struct FwWork {
    uint8_t* base;
    uint32_t m4, len8, max_front, tree_cap;
    LRSC_HD FwLeaf* front(uint32_t which) const { return reinterpret_cast<FwLeaf*>(base) + (uint64_t)which * max_front; }
    LRSC_HD FwIv* probe() const { return reinterpret_cast<FwIv*>(front(2)); }                                // kFwLanes
    LRSC_HD FwIv* term() const { return probe() + kFwLanes; }                                                  // the terminal fwd, rvc
    LRSC_HD uint32_t* tree() const { return reinterpret_cast<uint32_t*>(term() + 2); }                         // tree_cap, even
    LRSC_HD uint32_t* att() const { return tree() + tree_cap; }                                               // kFwLanes
    LRSC_HD uint8_t* str(uint32_t i) const { return reinterpret_cast<uint8_t*>(att() + kFwLanes) + (uint64_t)i * m4; }   // a, b, rc(a), rc(b)
    LRSC_HD uint8_t* q() const { return str(4); }                                                             // the walk's query and target
    LRSC_HD uint8_t* e() const { return str(5); }
    LRSC_HD uint8_t* sfx(uint32_t i) const { return str(6 + i); }                                             // kFwChainLeaves
    LRSC_HD uint8_t* cand() const { return str(6 + kFwChainLeaves); }
    LRSC_HD uint8_t* best() const { return cand() + len8; }                                                   // the walk's string
    LRSC_HD uint8_t* kept(uint32_t walk) const { return cand() + (uint64_t)(2 + walk) * len8; }               // fw_merge_pair's copies
    LRSC_HD uint8_t* result_flag() const { return cand() + 4ull * len8; }                                     // max_front
};
LRSC_HD FwWork fw_work_at(uint8_t* base, const FwParams& p)
{
    const uint32_t m = (uint32_t)p.min_overlap, I = (uint32_t)p.max_insert, L = (uint32_t)p.max_leaves;
    FwWork w;
    w.base = base;
    w.m4 = (m + 3u) & ~3u;
    w.len8 = ((I + 1 > m ? I + 1 : m) + 7u) & ~7u;
    w.max_front = 4 * L;
    // a step adds at most L nodes and the loop goes on, or up to 4 L and it ends; there are at most I + 1 steps
    w.tree_cap = (L * (I + 2) + 4 * L + 2u) & ~1u;
    return w;
}
LRSC_HD uint64_t fw_workspace_bytes(const FwParams& p)           // a multiple of 8
{
    const FwWork w = fw_work_at(nullptr, p);
    const uint64_t b = 2ull * w.max_front * sizeof(FwLeaf) + (kFwLanes + 2) * sizeof(FwIv) + 4ull * w.tree_cap + 4ull * kFwLanes +
                       (6ull + kFwChainLeaves) * w.m4 + 4ull * w.len8 + w.max_front;
    return (b + 7ull) & ~7ull;
}

// One backward-search step of [lo, hi1) with `code`.  False, nothing loaded, when the interval is not one of the strand.
template <class Block>
LRSC_HD bool fw_update(const StrandView<Block>& S, const uint32_t* mtab, uint32_t code, FwIv& v, uint32_t& n_rank, uint32_t& n_blk)
{
    if(v.hi1 > S.N || v.lo > v.hi1) return false;
    search_step(S, mtab, code, strand_pred(S, code), v.lo, v.hi1, n_rank, n_blk);
    return v.hi1 <= S.N && v.lo <= v.hi1;
}
// findInterval of the string whose bases, in the order the search consumes them, are code_at(0 .. len), len >= 1
template <class Block, class CodeAt>
LRSC_HD bool fw_search(const StrandView<Block>& S, const uint32_t* mtab, uint32_t len, CodeAt&& code_at, FwIv& v, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t first = code_at(0u) & 3u;
    search_first(S, first, strand_pred(S, first), v.lo, v.hi1);
    if(v.hi1 > S.N || v.lo > v.hi1) return false;
    for(uint32_t t = 1; t < len; ++t) {
        if(!fw_update<Block>(S, mtab, code_at(t) & 3u, v, n_rank, n_blk)) return false;
        if(v.lo == v.hi1) break;
    }
    return true;
}
// the occurrences in .bwt of the string w[0 .. len) = at(0 .. len), or of its reverse complement
template <class Block, class At>
LRSC_HD uint64_t fw_count(const StrandView<Block>& bwt, const uint32_t* mtab, uint32_t len, bool rvc, At&& at, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    FwIv v;
    if(!fw_search<Block>(bwt, mtab, len, [&](uint32_t t) -> uint32_t { return rvc ? at(t) ^ 3u : at(len - 1 - t); }, v, n_rank, n_blk)) {
        bad = 1;
        return 0;
    }
    return fw_size(v);
}

// every lane's `bad`, agreed on
template <class W>
LRSC_HD bool fw_any_bad(W& w, const uint32_t& bad)
{
    return w.min_over([&](uint32_t) -> uint32_t { return bad ? 0u : kFwNone; }) != kFwNone;
}

// the bases (of A,T,C,G) with which the k-mer at `slot` of the probes in att() occurs, a probe being (base, strand)
LRSC_HD uint32_t fw_branches(const uint32_t* att, uint32_t slot)
{
    uint32_t n = 0;
    for(uint32_t b = 0; b < 4; ++b) n += (att[slot * 8 + 2 * b] | att[slot * 8 + 2 * b + 1]) ? 1u : 0u;
    return n;
}

// trimRead of read[0 .. n), n >= k: head and tail as the reference leaves them (the trimmed read is empty when head > tail, else
// read[head .. tail + k)).
template <class Block, class W>
LRSC_HD void fw_trim(const StrandView<Block>& bwt, const uint32_t* mtab, const uint8_t* read, uint32_t n, uint32_t k, uint32_t* att, W& w, int32_t& head_out,
                     int32_t& tail_out, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const int32_t tail0 = (int32_t)(n - k);
    // does the k-mer `base + read[pos .. pos + k - 1)` (START) or `read[pos + 1 .. pos + k) + base` (END) occur on this strand?
    auto probe = [&](uint32_t lane, int32_t pos, bool end) -> uint32_t {
        const uint32_t base = (lane >> 1) & 3u;
        const uint64_t c = fw_count<Block>(bwt, mtab, k, (lane & 1u) != 0, [&](uint32_t i) -> uint32_t {
            if(end) return i == k - 1 ? base : (uint32_t)read[(uint32_t)pos + 1 + i];
            return i == 0 ? base : (uint32_t)read[(uint32_t)pos + i - 1];
        }, bad, n_rank, n_blk);
        return c ? 1u : 0u;
    };
    w.each([&](uint32_t lane) {
        att[lane] = lane < 16 ? probe(lane, (lane >> 3) ? tail0 : 0, (lane >> 3) != 0) : 0u;
    });
    const uint32_t at_head = w.uniform(fw_branches(att, 0)), at_tail = w.uniform(fw_branches(att, 1));
    int32_t head = 0, tail = tail0;
    if(at_head == 0) {
        head = tail0 + 1;
        for(int32_t g = 1; g <= tail0; g += (int32_t)kFwScan) {
            w.each([&](uint32_t lane) {
                const int32_t pos = g + (int32_t)(lane >> 3);
                att[lane] = pos <= tail0 ? probe(lane, pos, false) : 0u;
            });
            const uint32_t first = w.min_over([&](uint32_t lane) -> uint32_t {
                return lane < kFwScan && g + (int32_t)lane <= tail0 && fw_branches(att, lane) >= 2 ? lane : kFwNone;
            });
            if(first != kFwNone) { head = g + (int32_t)first; break; }
        }
    }
    if(at_tail == 0) {
        tail = head - 1;
        for(int32_t g = tail0 - 1; g >= head; g -= (int32_t)kFwScan) {
            w.each([&](uint32_t lane) {
                const int32_t pos = g - (int32_t)(lane >> 3);
                att[lane] = pos >= head ? probe(lane, pos, true) : 0u;
            });
            const uint32_t first = w.min_over([&](uint32_t lane) -> uint32_t {
                return lane < kFwScan && g - (int32_t)lane >= head && fw_branches(att, lane) >= 2 ? lane : kFwNone;
            });
            if(first != kFwNone) { tail = g - (int32_t)first; break; }
        }
    }
    head_out = head;
    tail_out = tail;
}

// The last m bases of the string of the leaf at `node`, `depth` steps below the query q[0 .. qlen), qlen >= m, to out[0 .. m).
// False when a parent is no node yet.
LRSC_HD bool fw_suffix(const uint32_t* tree, uint32_t tree_n, uint32_t node, uint32_t depth, const uint8_t* q, uint32_t qlen, uint32_t m, uint8_t* out)
{
    for(uint32_t i = m; i-- > 0;) {
        const uint32_t at = qlen + depth - m + i;                 // of the whole string
        if(at >= qlen) {
            if(node == 0 || node >= tree_n) return false;
            const uint32_t e = tree[node];
            out[i] = (uint8_t)(e & 3u);
            node = e >> 2;
        } else out[i] = q[at];
    }
    return true;
}

struct FwWalkOut {
    int32_t status;
    uint32_t length, max_used, pad;
    uint64_t coverage;
};

// SAIntervalTree(q, m, max_overlap, I, L, indices, e, threshold).mergeTwoReads: q and e are m bases each (MergePairedReads gives
// it nothing else), so the string is never longer than I + 1 and the rest of e that the reference appends is empty.  The merged
// string goes to ws.best()[0 .. out.length); out.length = 0 is the reference's empty string.  The walk keeps q and e in its
// workspace and reads the parameters where it uses them: what it holds in registers between its phases is its counters.
// SHORTCUT = false is SAIntervalTree::validate (SAIntervalTree.cpp:173-237): the same walk without isTwoReadsOverlap, so that the
// terminal is looked for only after the first extension, also when q == e.
#define FW_M ((uint32_t)p.min_overlap)
template <class Block, class W, bool SHORTCUT = true>
LRSC_HD void fw_walk(const StrandView<Block>* views, const uint32_t* mtab, const uint8_t* q_from, const uint8_t* e_from, const FwParams& p,
                     uint32_t max_overlap, const FwWork& ws, W& w, FwWalkOut& out, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    out = FwWalkOut{-4, 0u, 0u, 0u, 0ull};
    w.each([&](uint32_t lane) {
        for(uint32_t i = lane; i < FW_M; i += kFwLanes) {
            ws.q()[i] = q_from[i];
            ws.e()[i] = e_from[i];
        }
    });

    // ---- the root's and the terminal intervals: four chains
    w.each([&](uint32_t lane) {
        if(lane < 4) {
            const bool rvc = (lane & 1u) != 0;
            const uint8_t* s = (lane >> 1) ? ws.e() : ws.q();
            const StrandView<Block>& S = views[rvc ? 0 : 1];
            FwIv v{0, 0};
            if(!fw_search<Block>(S, mtab, FW_M, [&](uint32_t t) -> uint32_t { return (uint32_t)s[t] ^ (rvc ? 3u : 0u); }, v, n_rank, n_blk)) bad = 1;
            ws.probe()[lane] = v;
        }
    });
    // ---- isTwoReadsOverlap.  Case 1 compares the intervals as they are, valid or not.  Cases 2 and 3 look for the first m bases
    // of one string in the other: with m bases each the only place is 0 and the overlap is the whole string, so both say q == e.
    bool overlap = SHORTCUT && w.uniform64(ws.probe()[0].lo) == w.uniform64(ws.probe()[2].lo) && w.uniform64(ws.probe()[0].hi1) == w.uniform64(ws.probe()[2].hi1);
    if(SHORTCUT && !overlap) overlap = w.min_over([&](uint32_t lane) -> uint32_t {
        uint32_t r = kFwNone;
        for(uint32_t i = lane; i < FW_M; i += kFwLanes) r = ws.q()[i] != ws.e()[i] ? 0u : r;
        return r;
    }) == kFwNone;
    if(overlap) {
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < FW_M; i += kFwLanes) ws.best()[i] = ws.q()[i];
        });
        out.status = 1;
        out.length = FW_M;
        return;
    }
    w.each([&](uint32_t lane) {
        if(lane == 0) ws.front(0)[0] = FwLeaf{ws.probe()[0], ws.probe()[1], 0u, 0u};
        if(lane == 1 || lane == 2) ws.term()[lane - 1] = ws.probe()[lane + 1];
    });

    uint32_t cur = 0, n_front = 1, cur_len = FW_M, kmer = FW_M, tree_n = 1, n_res = 0;
    // attempToExtend: front(cur)[0 .. n_front) -> front(1 - cur), the new nodes from tree_n on; returns the new frontier's size
    auto extend = [&]() -> uint32_t {
        const FwLeaf* from = ws.front(cur);
        FwLeaf* to = ws.front(1 - cur);
        uint32_t n_new = 0;
        for(uint32_t j0 = 0; j0 < n_front; j0 += kFwRound) {
            w.each([&](uint32_t lane) {
                const uint32_t j = j0 + (lane >> 3), base = (lane >> 1) & 3u;
                const bool rvc = (lane & 1u) != 0;
                FwIv v{0, 0};
                if(j < n_front) {
                    v = rvc ? from[j].rvc : from[j].fwd;
                    if(fw_valid(v)) {                             // an invalid interval stays as it is
                        const StrandView<Block>& S = views[rvc ? 0 : 1];
                        if(!fw_update<Block>(S, mtab, rvc ? base ^ 3u : base, v, n_rank, n_blk)) bad = 1;
                    }
                }
                ws.probe()[lane] = v;
            });
            n_new += w.scan([&](uint32_t lane) -> uint32_t {
                const uint32_t j = j0 + (lane >> 3);
                return (lane & 1u) == 0 && j < n_front && fw_size(ws.probe()[lane]) + fw_size(ws.probe()[lane + 1]) >= (uint64_t)p.kmer_threshold ? 1u : 0u;
            }, [&](uint32_t lane, uint32_t before, uint32_t keep) {
                if(!keep) return;
                const uint32_t at = n_new + before, node = tree_n + at;
                if(at >= ws.max_front || node >= ws.tree_cap) { bad = 1; return; }
                ws.tree()[node] = (from[j0 + (lane >> 3)].node << 2) | ((lane >> 1) & 3u);
                to[at] = FwLeaf{ws.probe()[lane], ws.probe()[lane + 1], node, 0u};
            });
        }
        return n_new;
    };
    // refineSAInterval(m) of front(which)[0 .. n), depth steps below the query
    auto refine = [&](uint32_t which, uint32_t n, uint32_t depth) {
        FwLeaf* leaves = ws.front(which);
        for(uint32_t j0 = 0; j0 < n; j0 += kFwChainLeaves) {
            w.each([&](uint32_t lane) {
                const uint32_t j = j0 + (lane >> 1);
                if((lane & 1u) == 0 && j < n && !fw_suffix(ws.tree(), tree_n, leaves[j].node, depth, ws.q(), FW_M, FW_M, ws.sfx(lane >> 1))) bad = 1;
            });
            if(fw_any_bad(w, bad)) return;                        // a suffix that was not written is not searched
            w.each([&](uint32_t lane) {
                const uint32_t j = j0 + (lane >> 1);
                if(j >= n) return;
                const bool rvc = (lane & 1u) != 0;
                const uint8_t* s = ws.sfx(lane >> 1);
                const StrandView<Block>& S = views[rvc ? 0 : 1];
                FwIv v{0, 0};
                if(!fw_search<Block>(S, mtab, FW_M, [&](uint32_t t) -> uint32_t { return (uint32_t)s[t] ^ (rvc ? 3u : 0u); }, v, n_rank, n_blk)) bad = 1;
                if(rvc) leaves[j].rvc = v;
                else leaves[j].fwd = v;
            });
        }
    };

    // extendLeaves and isTerminated.  `retry` is extendLeaves' second attempt, after the refinement of the leaves that found no
    // extension: it comes round the loop again so that the step and the refinement stand here once.
    bool retry = false;
    while(retry || (n_front != 0 && n_front <= (uint32_t)p.max_leaves && cur_len <= (uint32_t)p.max_insert)) {
        const uint32_t n_new = extend();
        bool again = false;
        if(n_new == 0 && !retry) again = true;                    // the k-mer may have outgrown the index's reads
        else {
            if(n_new != 0) {
                ++kmer;
                ++cur_len;
                tree_n += n_new;
            }
            cur ^= 1u;
            n_front = n_new;
        }
        retry = again;
        if(retry || (n_front != 0 && kmer >= max_overlap)) {
            refine(cur, n_front, cur_len - FW_M);
            kmer = FW_M;
        }
        if(fw_any_bad(w, bad)) return;
        if(retry) continue;
        out.max_used = n_front > out.max_used ? n_front : out.max_used;
        // ---- isTerminated
        const FwLeaf* leaves = ws.front(cur);
        n_res = (uint32_t)w.sum64_over([&](uint32_t lane) -> uint64_t {
            uint64_t r = 0;
            for(uint32_t j = lane; j < n_front; j += kFwLanes) {
                const bool hit = fw_within(leaves[j].fwd, ws.term()[0]) || fw_within(leaves[j].rvc, ws.term()[1]);
                ws.result_flag()[j] = hit ? 1 : 0;
                r += hit ? 1u : 0u;
            }
            return r;
        });
        if(n_res != 0) break;
    }
    if(n_res == 0) {
        out.status = n_front == 0 ? -1 : (cur_len > (uint32_t)p.max_insert ? -2 : (n_front > (uint32_t)p.max_leaves ? -3 : -4));
        return;
    }
    // ---- the results in frontier order: the string with the strictly greatest k-mer coverage
    out.status = 1;
    const FwLeaf* leaves = ws.front(cur);
    const uint32_t half = FW_M / 2;
    uint8_t* cand = ws.cand();
    for(uint32_t j = 0; j < n_front; ++j) {
        if(!w.uniform(ws.result_flag()[j])) continue;
        w.each([&](uint32_t lane) {
            if(lane == 0) {                                       // the path, read back from the leaf
                uint32_t node = leaves[j].node;
                for(uint32_t i = cur_len; i-- > FW_M;) {
                    if(node == 0 || node >= tree_n) { bad = 1; break; }
                    const uint32_t t = ws.tree()[node];
                    cand[i] = (uint8_t)(t & 3u);
                    node = t >> 2;
                }
            } else
                for(uint32_t i = lane - 1; i < FW_M; i += kFwLanes - 1) cand[i] = ws.q()[i];
        });
        if(fw_any_bad(w, bad)) return;
        const uint32_t n_chains = 2 * ((cur_len - FW_M) / half + 1);
        const uint64_t cov = w.sum64_over([&](uint32_t lane) -> uint64_t {
            uint64_t c = 0;
            for(uint32_t ch = lane; ch < n_chains; ch += kFwLanes) {
                const uint8_t* s = cand + (ch >> 1) * half;
                c += fw_count<Block>(views[0], mtab, FW_M, (ch & 1u) != 0, [&](uint32_t i) -> uint32_t { return s[i]; }, bad, n_rank, n_blk);
            }
            return c;
        });
        if(cov > out.coverage) {
            out.coverage = cov;
            out.length = cur_len;
            w.each([&](uint32_t lane) {
                for(uint32_t i = lane; i < cur_len; i += kFwLanes) ws.best()[i] = cand[i];
            });
        }
    }
}
#undef FW_M

// The trim and the gate of one pair, r1[0 .. n1) and r2[0 .. n2) its reads' codes: trimmed[] = the trimmed lengths (0 for a read
// shorter than k, on which the reference throws), and when both reach m the walks' strings a, b, rc(a), rc(b), the first m bases
// of the trimmed reads, at strs + 0, m4, 2 m4, 3 m4.  att: kFwLanes words.  Returns whether the pair is to be walked.
template <class Block, class W>
LRSC_HD bool fw_trim_pair(const StrandView<Block>& bwt, const uint32_t* mtab, const uint8_t* r1, uint32_t n1, const uint8_t* r2, uint32_t n2, const FwParams& p,
                          uint32_t* att, W& w, uint8_t* strs, uint32_t m4, uint32_t trimmed[2], uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t k = (uint32_t)p.kmer_length, m = (uint32_t)p.min_overlap;
    int32_t head[2] = {0, 0};
    LRSC_FW_NOUNROLL
    for(uint32_t r = 0; r < 2; ++r) {
        const uint32_t n = r ? n2 : n1;
        trimmed[r] = 0;
        if(n < k) continue;
        int32_t tail = 0;
        fw_trim<Block>(bwt, mtab, r ? r2 : r1, n, k, att, w, head[r], tail, bad, n_rank, n_blk);
        trimmed[r] = head[r] > tail ? 0u : (uint32_t)(tail - head[r]) + k;
    }
    if(fw_any_bad(w, bad) || trimmed[0] < m || trimmed[1] < m) return false;
    w.each([&](uint32_t lane) {
        for(uint32_t i = lane; i < m; i += kFwLanes) {
            const uint8_t a = r1[(uint32_t)head[0] + i] & 3u, b = r2[(uint32_t)head[1] + i] & 3u;
            strs[i] = a;
            strs[m4 + i] = b;
            strs[2 * m4 + m - 1 - i] = a ^ 3u;
            strs[3 * m4 + m - 1 - i] = b ^ 3u;
        }
    });
    return true;
}
// ((len1 + len2) / 2) * 0.9, of the untrimmed lengths, as the reference's size_t <- double
LRSC_HD uint32_t fw_max_overlap(const FwParams& p, uint32_t n1, uint32_t n2)
{
    return p.max_overlap != -1 ? (uint32_t)p.max_overlap : (uint32_t)((double)(((uint64_t)n1 + n2) / 2) * 0.9);
}
// MergePairedReads' choice between the walks' strings: 0, 1, or kFwNone when the pair is not merged
LRSC_HD uint32_t fw_choose(const FwWalkOut& w0, const FwWalkOut& w1)
{
    if(w0.length != 0 && w1.length == 0) return 0;
    if(w0.length == 0 && w1.length != 0) return 1;
    if(w0.length != 0 && w0.length == w1.length) return w0.coverage > w1.coverage ? 0u : 1u;
    return kFwNone;
}
LRSC_HD FwResult fw_result(bool walked, const uint32_t trimmed[2], const FwWalkOut& w0, const FwWalkOut& w1)
{
    FwResult res{0u, 0u, {0, 0}, {0u, 0u}, {0ull, 0ull}, {trimmed[0], trimmed[1]}};
    if(!walked) return res;
    const uint32_t pick = fw_choose(w0, w1);
    res.merged = pick != kFwNone ? 1u : 0u;
    res.length = pick == kFwNone ? 0u : (pick ? w1.length : w0.length);
    res.status[0] = w0.status; res.status[1] = w1.status;
    res.max_used_leaves[0] = w0.max_used; res.max_used_leaves[1] = w1.max_used;
    res.coverage[0] = w0.coverage; res.coverage[1] = w1.coverage;
    return res;
}

// One pair, start to end, as the kernels and the entry do it between them: the trim (fmwalk_trim_kernel), walk 0 from a to rc(b)
// and walk 1 from b to rc(a) (fmwalk_walk_kernel, a wavefront each), the choice (lrsc_fmwalk_merge).  merged[0 .. res.length) =
// the merged string's codes when res.merged.  `bad` is set when an interval left the strand (merged and res are then not to be
// used).
template <class Block, class W>
LRSC_HD void fw_merge_pair(const StrandView<Block>* views, const uint32_t* mtab, const uint8_t* r1, uint32_t n1, const uint8_t* r2, uint32_t n2, const FwParams& p,
                           const FwWork& ws, W& w, uint8_t* merged, FwResult& res, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    uint32_t trimmed[2];
    FwWalkOut o[2] = {FwWalkOut{0, 0u, 0u, 0u, 0ull}, FwWalkOut{0, 0u, 0u, 0u, 0ull}};
    const bool walked = fw_trim_pair<Block>(views[0], mtab, r1, n1, r2, n2, p, ws.att(), w, ws.str(0), ws.m4, trimmed, bad, n_rank, n_blk);
    if(fw_any_bad(w, bad)) return;
    for(uint32_t wk = 0; walked && wk < 2; ++wk) {
        fw_walk<Block>(views, mtab, ws.str(wk), ws.str(3 - wk), p, fw_max_overlap(p, n1, n2), ws, w, o[wk], bad, n_rank, n_blk);
        if(fw_any_bad(w, bad)) return;
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < o[wk].length; i += kFwLanes) ws.kept(wk)[i] = ws.best()[i];
        });
    }
    res = fw_result(walked, trimmed, o[0], o[1]);
    if(!res.merged) return;
    const uint8_t* s = ws.kept(fw_choose(o[0], o[1]));
    w.each([&](uint32_t lane) {
        for(uint32_t i = lane; i < res.length; i += kFwLanes) merged[i] = s[i];
    });
}

} // namespace lrsc
