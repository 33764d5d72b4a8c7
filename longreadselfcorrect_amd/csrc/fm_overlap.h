// fm_overlap.h -- exact irreducible read overlaps over a resident index: the per-chain and per-read code of the device overlap
// (fm_overlap.hip), the reference's OverlapAlgorithm::overlapReadExact with what it calls (Algorithm/OverlapAlgorithm.cpp:22-44,
// 270-389, 419-487, 1043-1193, 1423-1444; Algorithm/OverlapBlock.cpp:40-70, 182-360) and BWTAlgorithms::initIntervalPair,
// updateBothL, updateBothR and getExtCount, on the rank-block layout.
//
// An interval pair (OvBlock's a, b) is the rows [lo, hi1) of a string in the strand that is searched and of the same string in
// the other strand.  A step to the left (updateBothL) takes the counts of every symbol at both ends of a (fm_strand.h's
// interval_occ_all, the loads of one search_step): a's new rows are search_step's, b narrows by the symbols below the base.  A
// step to the right (updateBothR) is the same on the other strand with a and b swapped.
//
//   collect   ov_collect_chain, one lane per chain, four chains per read (findOverlapBlocksExact of seq in .bwt, complement(seq)
//             in .rbwt, reverseComplement(seq) in .bwt, reverse(seq) in .rbwt): a block wherever the overlap reaches min_overlap
//             and the '$' probe is valid, in the order of the search; at full length the extension counts of both sides
//             (isSubstring) or the containment block.  The counts of an end serve the '$' probe and the next base alike.
//   reduce    ov_reduce_read, one wavefront per read: TrimOBLInterval of each chain's list (the stable descending sort of a list
//             that the search left ascending is its reverse; the walk from the back is a prefix sum over the lanes), the
//             containment blocks appended, removeSubMaximalBlocks (a stable rank sort by interval[0].lower over the lanes; the
//             restarting resolution only where neighbours intersect, by one lane), removeContainmentBlocks, the lists joined, the
//             containments first to the output, computeIrreducibleBlocks of both joined lists.  A round of it takes the
//             extension counts of every (group, block) over the lanes, one lane reads the groups in list order and writes the
//             plan (what ends and is output, what is popped again, which block goes on with which base into which new group,
//             kept groups before branched ones), the right updates of the plan are the lanes' again, and a prefix sum drops the
//             blocks that became invalid.  A group is a run of blocks with one group number.
//
// isTargetSubstring of a block is 0: the reference leaves it uninitialised on this path and never sets it, and what it reads
// there decides whether OverlapProcess::process skips the block.
//
// All of a read's state lives in one wavefront's slice of a global workspace (OvWork), sized from the parameters; nothing is
// indexed before its range was checked.  A read whose blocks, plan or output would outgrow the slice gets status kOvOverflow and
// no blocks.  An interval that leaves the strand sets `bad` (kernel: *broken = 1).  All functions here are LRSC_HD and free of
// HIP types: the kernels call them, and tests/host_tools/overlap_driver.cpp compiles the same source for the CPU.
#pragma once
#include <stdint.h>

#include "fm_strand.h"
#include "fm_wave.h"

namespace lrsc {

constexpr uint32_t kOvLanes = kWaveLanes;
constexpr uint32_t kOvThreads = 256;                              // four wavefronts per workgroup, one mask table
// Wavefronts per SIMD that the launches are sized for.  Both kernels are chains of dependent 64-byte loads and latency-bound, so
// more wavefronts hide more of it (fm_fmwalk.h).  Four: a lane holds two rank blocks' worth of counts (two OccAll, 20 registers),
// a rank block, an interval pair and a strand view, within 512 / 4 = 128 VGPRs but not within the 96 of five.
constexpr uint32_t kOvWavesPerSimd = 4;
constexpr uint32_t kOvChains = 4;
constexpr uint32_t kOvReadsPerWave = kOvLanes / kOvChains;        // collect: one lane per chain
// the limits of lrsc_overlap_exact (LRSC_ERR_UNSUPPORTED above them)
constexpr uint32_t kOvMaxRead = 2000;
constexpr uint32_t kOvMaxMinOverlap = 2000;
constexpr uint32_t kOvTrimSum = 128;                              // TrimOBLInterval's cumulative interval size
constexpr uint32_t kOvOutCap = 256;                               // final blocks of a read
constexpr uint32_t kOvMinBlocks = 512;                            // a slice's lists hold this many blocks at least
constexpr uint32_t kOvNone = kWaveNone;
enum : uint32_t { kOvOk = 0, kOvOverflow = 1 };

struct OvIv {
    uint64_t lo, hi1;
};
// flags: bit 0 isTargetRev, bit 1 isQueryRev, bit 2 isQueryComp
struct OvBlock {
    OvIv a, b;                                                    // ranges.interval[0], [1]
    uint32_t len, flags, gid, pad;
};
struct OvChainHead {                                              // what a chain leaves beside its blocks
    uint32_t n_blocks, has_contain, is_substring, pad;
    OvBlock contain;
};
struct OvOutBlock {                                               // lrsc_overlap_block
    int64_t lower, upper;
    uint32_t overlap_len;
    uint8_t target_rev, query_rev, query_comp, contained;
};
struct OvOutRead {                                                // lrsc_overlap_read
    uint32_t is_substring, n_blocks, status, pad;
    uint64_t first_block;
};
struct OvOcc {
    OccAll l, u;
};
LRSC_HD uint64_t ov_size(const OvIv& v) { return v.lo < v.hi1 ? v.hi1 - v.lo : 0ull; }
// AlignFlags of a chain: sufPre, prePre, sufSuf, preSuf
LRSC_HD uint32_t ov_chain_flags(uint32_t chain) { return (chain & 1u) | ((chain >> 1) << 1) | (((chain & 1u) ^ (chain >> 1)) << 2); }

struct OvParams {
    uint32_t min_overlap, max_len;                                // of the call: the longest read
};
// blocks a chain can emit: the overlap lengths min_overlap .. max_len - 1
LRSC_HD uint32_t ov_slots(const OvParams& p) { return p.max_len > p.min_overlap ? p.max_len - p.min_overlap : 0u; }
LRSC_HD uint32_t ov_list_cap(const OvParams& p)
{
    const uint32_t c = 4 * ov_slots(p) + 8;                       // the four lists and their containments, joined
    return c < kOvMinBlocks ? kOvMinBlocks : c;
}

// One wavefront's slice of the reduce workspace: three block lists, the counts, masks and plan of a round, the control words,
// the final blocks of the read it has in hand
struct OvWork {
    uint8_t* base;
    uint32_t cap, pad;
    LRSC_HD OvBlock* list(uint32_t which) const { return reinterpret_cast<OvBlock*>(base) + (uint64_t)which * cap; }   // 0 cur, 1 tmp, 2 joined
    LRSC_HD OvOcc* occ() const { return reinterpret_cast<OvOcc*>(list(3)); }
    LRSC_HD uint32_t* mask() const { return reinterpret_cast<uint32_t*>(occ() + cap); }
    LRSC_HD uint32_t* plan_src() const { return mask() + cap; }
    LRSC_HD uint32_t* plan_code() const { return plan_src() + cap; }
    LRSC_HD uint32_t* plan_gid() const { return plan_code() + cap; }
    LRSC_HD uint32_t* att() const { return plan_gid() + cap; }                                                          // kOvLanes
    LRSC_HD uint32_t* ctl() const { return att() + kOvLanes; }                                                          // 8
    LRSC_HD OvOutBlock* stage() const { return reinterpret_cast<OvOutBlock*>(ctl() + 8); }                              // kOvOutCap: the read's final blocks
};
LRSC_HD OvWork ov_work_at(uint8_t* base, const OvParams& p)
{
    OvWork w;
    w.base = base;
    w.cap = ov_list_cap(p);
    w.pad = 0;
    return w;
}
LRSC_HD uint64_t ov_workspace_bytes(const OvParams& p)            // a multiple of 8
{
    const uint64_t cap = ov_list_cap(p);
    return cap * (3 * sizeof(OvBlock) + sizeof(OvOcc) + 4 * sizeof(uint32_t)) + (kOvLanes + 8) * sizeof(uint32_t) + kOvOutCap * sizeof(OvOutBlock);
}
static_assert(sizeof(OvBlock) == 48 && sizeof(OvOcc) == 80 && sizeof(OvOutBlock) == 24 && sizeof(OvOutRead) == 24 && sizeof(OvChainHead) == 64, "the slices' strides");

// The counts at both ends of v in S.  False, nothing loaded, when v is no interval of the strand.
template <class Block>
LRSC_HD bool ov_counts(const StrandView<Block>& S, const uint32_t* mtab, const OvIv& v, OccAll& l, OccAll& u, uint32_t& n_rank, uint32_t& n_blk)
{
    if(v.hi1 > S.N || v.lo > v.hi1) return false;
    interval_occ_all(S, mtab, v.lo, v.hi1, l, u, n_rank, n_blk);
    return true;
}
// updateBothL / updateBothR with the symbol of rank k, l and u being the counts at the ends of `direct` in the strand whose C[]
// pred is of: direct <- C[k] + the symbol's counts, other narrows by the symbols below k
LRSC_HD void ov_update(OvIv& direct, OvIv& other, uint32_t k, uint64_t pred, const OccAll& l, const OccAll& u)
{
    const OccAll diff = occ_diff(u, l);
    other.lo += occ_less_than(diff, k);
    other.hi1 = other.lo + occ_get(diff, k);
    direct.lo = pred + occ_get(l, k);
    direct.hi1 = pred + occ_get(u, k);
}
template <class Block>
LRSC_HD uint64_t ov_pred(const StrandView<Block>& S, uint32_t k) { return k == 0 ? 0ull : (uint64_t)strand_pred(S, k - 1); }

// findOverlapBlocksExact of chain `chain` of seq[0 .. n), n >= m >= 2: its blocks to out[0 .. head.n_blocks), n_blocks <= slots.
template <class Block>
LRSC_HD void ov_collect_chain(const StrandView<Block>* views, const uint32_t* mtab, const uint8_t* seq, uint32_t n, uint32_t m, uint32_t chain, OvBlock* out, uint32_t slots,
                              OvChainHead& head, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const StrandView<Block>& S = views[chain & 1u];
    const StrandView<Block>& R = views[(chain & 1u) ^ 1u];
    const uint32_t flags = ov_chain_flags(chain), flip = (chain == 1 || chain == 2) ? 3u : 0u;
    // the base that the search takes at step t: w[n - 1 - t] of seq, complement(seq), reverseComplement(seq), reverse(seq)
    auto code_at = [&](uint32_t t) -> uint32_t { return ((uint32_t)seq[(chain >> 1) ? t : n - 1 - t] & 3u) ^ flip; };
    head.n_blocks = 0; head.has_contain = 0; head.is_substring = 0; head.pad = 0;
    OvIv a, b;
    const uint32_t first = code_at(0);
    search_first(S, first, strand_pred(S, first), a.lo, a.hi1);
    search_first(R, first, strand_pred(R, first), b.lo, b.hi1);
    uint32_t count = 0;
    OccAll l, u;
    for(uint32_t t = 1; t < n; ++t) {                             // a, b: the pair of the last t bases
        if(!ov_counts<Block>(S, mtab, a, l, u, n_rank, n_blk)) { bad = 1; return; }
        if(t >= m && u.d > l.d) {                                 // the probe with '$': the reads that start with these bases
            if(count >= slots) { bad = 1; return; }
            out[count++] = OvBlock{OvIv{l.d, u.d}, OvIv{b.lo, b.lo + (u.d - l.d)}, t, flags, 0u, 0u};
        }
        const uint32_t k = code_at(t) + 1;
        ov_update(a, b, k, ov_pred(S, k), l, u);
    }
    head.n_blocks = count;
    OccAll rl, ru;
    if(!ov_counts<Block>(S, mtab, a, l, u, n_rank, n_blk) || !ov_counts<Block>(R, mtab, b, rl, ru, n_rank, n_blk)) { bad = 1; return; }
    const OccAll left = occ_diff(u, l), right = occ_diff(ru, rl);
    if((left.a | left.c | left.g | left.t | right.a | right.c | right.g | right.t) != 0) {
        head.is_substring = 1;
        return;
    }
    if(a.lo < a.hi1 && b.lo < b.hi1 && u.d > l.d) {                // probe.isValid() after its '$' on the left
        OvIv pa{l.d, u.d}, pb{b.lo, b.lo + (u.d - l.d)};
        if(!ov_counts<Block>(R, mtab, pb, rl, ru, n_rank, n_blk)) { bad = 1; return; }
        ov_update(pb, pa, 0u, 0ull, rl, ru);                      // and its '$' on the right
        head.has_contain = 1;
        head.contain = OvBlock{pa, pb, n, flags, 0u, 0u};
    }
}

// every lane's `bad`, agreed on
template <class W>
LRSC_HD bool ov_any_bad(W& w, const uint32_t& bad)
{
    return w.min_over([&](uint32_t) -> uint32_t { return bad ? 0u : kOvNone; }) != kOvNone;
}

// from[0 .. n) -> to[0 .. n) in the order of a stable sort: descending overlap length, or ascending interval[0].lower
template <class W>
LRSC_HD void ov_rank_sort(W& w, const OvBlock* from, OvBlock* to, uint32_t n, bool by_lower)
{
    w.each([&](uint32_t lane) {
        for(uint32_t i = lane; i < n; i += kOvLanes) {
            const OvBlock x = from[i];
            uint32_t rank = 0;
            for(uint32_t j = 0; j < n; ++j) {
                const bool before = by_lower ? from[j].a.lo < x.a.lo : from[j].len > x.len;
                const bool same = by_lower ? from[j].a.lo == x.a.lo : from[j].len == x.len;
                rank += before || (same && j < i) ? 1u : 0u;
            }
            to[rank] = x;
        }
    });
}

// y when `second`, else x, member by member: a choice between two structs is one between their addresses and keeps both in scratch
LRSC_HD OvBlock ov_pick(bool second, const OvBlock& x, const OvBlock& y)
{
    return OvBlock{OvIv{second ? y.a.lo : x.a.lo, second ? y.a.hi1 : x.a.hi1}, OvIv{second ? y.b.lo : x.b.lo, second ? y.b.hi1 : x.b.hi1}, second ? y.len : x.len,
                   second ? y.flags : x.flags, second ? y.gid : x.gid, 0u};
}

// removeSubMaximalBlocks' loop over a[0 .. n), sorted by interval[0].lower, as one lane runs it; returns the new n (never above
// the old: a resolution takes two blocks and gives back one or two)
LRSC_HD uint32_t ov_resolve_serial(OvBlock* a, uint32_t n)
{
    uint32_t i = 0;
    while(i + 1 < n) {
        const OvBlock p = a[i], q = a[i + 1];
        if(q.a.lo >= p.a.hi1 || p.a.lo >= q.a.hi1) { ++i; continue; }
        // resolveOverlap: numDiff is 0 on both, so the longer overlap is the better block
        const bool p_better = p.len > q.len;
        const OvBlock better = ov_pick(!p_better, p, q);
        OvBlock worse = ov_pick(p_better, p, q);
        const uint64_t top = better.a.hi1 < worse.a.hi1 ? better.a.hi1 : worse.a.hi1, bottom = better.a.lo > worse.a.lo ? better.a.lo : worse.a.lo;
        const uint64_t dup = top - bottom;
        bool two = false;
        if(better.a.hi1 - better.a.lo != dup) {
            if(better.a.lo < worse.a.lo) worse.a.lo += dup;
            else worse.a.hi1 -= dup;
            two = worse.a.lo < worse.a.hi1;
        }
        for(uint32_t k = i + 2; k < n; ++k) a[k - 2] = a[k];
        n -= 2;
        // the resolved list sorted by lower (stable), merged in: a block of the list stands before an equal one merged in
        const bool swap = two && worse.a.lo < better.a.lo;
        const OvBlock r0 = ov_pick(swap, better, worse), r1 = ov_pick(swap, worse, better);
        for(uint32_t r = 0; r < (two ? 2u : 1u); ++r) {
            const OvBlock x = ov_pick(r != 0, r0, r1);
            uint32_t at = 0;
            while(at < n && a[at].a.lo <= x.a.lo) ++at;
            for(uint32_t k = n; k > at; --k) a[k] = a[k - 1];
            a[at] = x;
            ++n;
        }
        i = 0;
    }
    return n;
}

// the symbols (bit k: rank k) that extend the block to the right, in the query's representation (getCanonicalExtCount)
LRSC_HD uint32_t ov_ext_mask(const OvOcc& o, uint32_t flags)
{
    const OccAll d = occ_diff(o.u, o.l);
    const bool comp = (flags & 4u) != 0;
    return (d.d ? 1u : 0u) | ((comp ? d.t : d.a) ? 2u : 0u) | ((comp ? d.g : d.c) ? 4u : 0u) | ((comp ? d.c : d.g) ? 8u : 0u) | ((comp ? d.a : d.t) ? 16u : 0u);
}

// What one lane makes of the groups of a round, cur[0 .. n) with their masks: what _processIrreducibleBlocksExactIterative's
// inner loop decides.  TLBs that end go to out (n_out), the rest into the plan: (block, base code, new group), kept groups first.
// Returns the plan's size, kOvNone when plan or output would overflow or a group has no base to go on with.
LRSC_HD uint32_t ov_plan_round(const OvWork& ws, const OvBlock* cur, uint32_t n, OvOutBlock* out, uint32_t& n_out, uint32_t read_len)
{
    const uint32_t* mask = ws.mask();
    uint32_t n_plan = 0, gid = 0;
    for(uint32_t pass = 0; pass < 2; ++pass) {
        for(uint32_t s = 0; s < n;) {
            uint32_t e = s + 1;
            while(e < n && cur[e].gid == cur[s].gid) ++e;
            const uint32_t top = cur[s].len;
            uint32_t tl = s, ext = 0;
            while(tl < e && cur[tl].len == top) ext |= mask[tl++];
            bool go_on = true;
            if(ext & 1u) {
                uint32_t t = s;
                while(t < tl && (mask[t] & 1u)) ++t;
                if(t == tl) {                                     // every top-length block ends: output them, the group is done
                    go_on = false;
                    for(uint32_t i = s; pass == 0 && i < tl; ++i) {
                        if(n_out >= kOvOutCap) return kOvNone;
                        const OvOcc& o = ws.occ()[i];             // the final updateBothR('$')
                        const uint64_t lower = cur[i].a.lo, size = o.u.d - o.l.d;
                        out[n_out++] = OvOutBlock{(int64_t)lower, (int64_t)(lower + size) - 1, cur[i].len, (uint8_t)(cur[i].flags & 1u), (uint8_t)((cur[i].flags >> 1) & 1u),
                                                  (uint8_t)((cur[i].flags >> 2) & 1u), (uint8_t)(cur[i].len == read_len ? 1 : 0)};
                    }
                }                                                 // else: what was pushed is popped again, goto SARightExtension
            }
            if(go_on) {
                for(uint32_t i = tl; i < e; ++i) ext |= mask[i];
                const uint32_t dna = ext >> 1;
                if(dna == 0) return kOvNone;
                const bool unique = (dna & (dna - 1)) == 0;
                if(unique == (pass == 0)) {
                    for(uint32_t base = 0; base < 4; ++base) {    // ALPHABET order
                        if(!((dna >> base) & 1u)) continue;
                        for(uint32_t i = s; i < e; ++i) {
                            if(n_plan >= ws.cap) return kOvNone;
                            ws.plan_src()[n_plan] = i;
                            ws.plan_code()[n_plan] = base;
                            ws.plan_gid()[n_plan++] = gid;
                        }
                        ++gid;
                    }
                }
            }
            s = e;
        }
    }
    return n_plan;
}

// computeIrreducibleBlocks of from[0 .. n): the final blocks appended to out.  False on overflow.
template <class Block, class W>
LRSC_HD bool ov_irreducible(const StrandView<Block>* views, const uint32_t* mtab, const OvWork& ws, W& w, const OvBlock* from, uint32_t n, uint32_t read_len, OvOutBlock* out,
                            uint32_t& n_out, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    OvBlock* cur = ws.list(0);
    OvBlock* tmp = ws.list(1);
    ov_rank_sort(w, from, cur, n, false);
    w.each([&](uint32_t lane) {
        for(uint32_t i = lane; i < n; i += kOvLanes) cur[i].gid = 0;
    });
    // a round extends every group by a base: no read of the index is longer than the strand
    for(uint64_t round = 0; n != 0; ++round) {
        if(round > views[0].N) { bad = 1; return true; }
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < n; i += kOvLanes) {
                const OvBlock x = cur[i];
                OvOcc o{};
                if(!ov_counts<Block>(views[(x.flags & 1u) ? 0 : 1], mtab, x.b, o.l, o.u, n_rank, n_blk)) bad = 1;
                ws.occ()[i] = o;
                ws.mask()[i] = ov_ext_mask(o, x.flags);
            }
        });
        if(ov_any_bad(w, bad)) return true;
        w.each([&](uint32_t lane) {
            if(lane != 0) return;
            uint32_t k = n_out;
            ws.ctl()[0] = ov_plan_round(ws, cur, n, out, k, read_len);
            ws.ctl()[1] = k;
        });
        const uint32_t n_plan = w.uniform(ws.ctl()[0]);
        if(n_plan == kOvNone) return false;
        n_out = w.uniform(ws.ctl()[1]);
        w.each([&](uint32_t lane) {
            for(uint32_t j = lane; j < n_plan; j += kOvLanes) {
                const uint32_t src = ws.plan_src()[j];
                OvBlock x = cur[src];
                const OvOcc o = ws.occ()[src];
                const uint32_t k = (ws.plan_code()[j] ^ ((x.flags & 4u) ? 3u : 0u)) + 1;
                uint64_t pred = ov_pred(views[0], k);
                if(!(x.flags & 1u)) pred = ov_pred(views[1], k);
                ov_update(x.b, x.a, k, pred, o.l, o.u);
                x.gid = ws.plan_gid()[j];
                tmp[j] = x;
            }
        });
        uint32_t kept = 0;
        for(uint32_t j0 = 0; j0 < n_plan; j0 += kOvLanes)
            kept += w.scan([&](uint32_t lane) -> uint32_t { return j0 + lane < n_plan && tmp[j0 + lane].a.lo < tmp[j0 + lane].a.hi1 ? 1u : 0u; },
                           [&](uint32_t lane, uint32_t before, uint32_t keep) {
                               if(keep) cur[kept + before] = tmp[j0 + lane];
                           });
        n = kept;
    }
    return true;
}

// overlapReadExact of one read of read_len bases from what its four chains left: heads[0 .. 4) and chain c's blocks at
// blocks + c * slots.  The final blocks to out[0 .. res.n_blocks), at most kOvOutCap.
template <class Block, class W>
LRSC_HD void ov_reduce_read(const StrandView<Block>* views, const uint32_t* mtab, const OvChainHead* heads, const OvBlock* blocks, uint32_t slots, uint32_t read_len,
                            uint32_t min_overlap, const OvWork& ws, W& w, OvOutBlock* out, OvOutRead& res, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    res = OvOutRead{0u, 0u, kOvOk, 0u, 0ull};
    if(read_len < min_overlap) return;
    res.is_substring = (w.uniform(heads[0].is_substring) | w.uniform(heads[1].is_substring) | w.uniform(heads[2].is_substring) | w.uniform(heads[3].is_substring)) ? 1u : 0u;
    OvBlock* joined = ws.list(2);
    uint32_t n_joined = 0, n_suffix = 0;
    bool fits = true;
    // the lists in the order of the join: suffixFwd, suffixRev, prefixFwd, prefixRev = the chains 0, 1, 2, 3
    for(uint32_t chain = 0; chain < kOvChains && fits; ++chain) {
        const OvBlock* src = blocks + (uint64_t)chain * slots;
        const uint32_t n = w.uniform(heads[chain].n_blocks);
        if(n > slots) { bad = 1; return; }
        // ---- TrimOBLInterval.  Sorted descending, the list is src reversed; the walk from the back takes src[0], src[1], ...
        // and never the front, src[n - 1]; where the sum reaches 128 at src[s], src[s .. n) is erased.
        uint32_t kept = n, acc = 0;
        for(uint32_t s0 = 0; s0 < n; s0 += kOvLanes) {
            const uint32_t total = w.scan(
                [&](uint32_t lane) -> uint32_t {
                    const uint32_t s = s0 + lane;
                    const uint64_t size = s < n ? ov_size(src[s].b) : 0ull;
                    return size < kOvTrimSum ? (uint32_t)size : kOvTrimSum;
                },
                [&](uint32_t lane, uint32_t before, uint32_t mine) {
                    const uint32_t s = s0 + lane;
                    // longestOverlap is the back's, the shortest: this difference is never positive
                    const bool far = s < n && 2 * ((int64_t)src[0].len - (int64_t)src[s].len) >= (int64_t)read_len;
                    ws.att()[lane] = s + 1 < n && (acc + before + mine >= kOvTrimSum || far) ? s : kOvNone;
                });
            const uint32_t hit = w.min_over([&](uint32_t lane) -> uint32_t { return ws.att()[lane]; });
            if(hit != kOvNone) { kept = hit; break; }
            acc = acc + total < kOvTrimSum ? acc + total : kOvTrimSum;
        }
        // ---- the containment blocks of this strand appended: fwd = those of chains 0 and 2, rev = of chains 1 and 3
        const uint32_t c0 = chain & 1u, c1 = c0 + 2;
        const uint32_t has0 = w.uniform(heads[c0].has_contain), has1 = w.uniform(heads[c1].has_contain);
        uint32_t n_list = kept + has0 + has1;
        if(n_list > ws.cap || n_joined + n_list > ws.cap) { fits = false; break; }
        OvBlock* first = ws.list(0);
        OvBlock* sorted = ws.list(1);
        w.each([&](uint32_t lane) {
            for(uint32_t i = lane; i < kept; i += kOvLanes) first[i] = src[kept - 1 - i];
            if(lane == 0 && has0) first[kept] = heads[c0].contain;
            if(lane == 1 && has1) first[kept + has0] = heads[c1].contain;
        });
        // ---- removeSubMaximalBlocks
        ov_rank_sort(w, first, sorted, n_list, true);
        const uint32_t crossing = w.min_over([&](uint32_t lane) -> uint32_t {
            uint32_t r = kOvNone;
            for(uint32_t i = lane; i + 1 < n_list; i += kOvLanes) r = sorted[i + 1].a.lo < sorted[i].a.hi1 && sorted[i].a.lo < sorted[i + 1].a.hi1 ? 0u : r;
            return r;
        });
        if(crossing != kOvNone) {
            w.each([&](uint32_t lane) {
                if(lane == 0) ws.ctl()[0] = ov_resolve_serial(sorted, n_list);
            });
            n_list = w.uniform(ws.ctl()[0]);
        }
        // ---- removeContainmentBlocks, and the join
        for(uint32_t i0 = 0; i0 < n_list; i0 += kOvLanes)
            n_joined += w.scan([&](uint32_t lane) -> uint32_t { return i0 + lane < n_list && sorted[i0 + lane].len != read_len ? 1u : 0u; },
                               [&](uint32_t lane, uint32_t before, uint32_t keep) {
                                   if(keep) joined[n_joined + before] = sorted[i0 + lane];
                               });
        if(chain == 1) n_suffix = n_joined;
    }
    uint32_t n_out = 0;
    if(fits) {
        // ---- the containments to the output first: oblFwdContain, then oblRevContain
        w.each([&](uint32_t lane) {
            if(lane != 0) return;
            uint32_t k = 0;
            for(uint32_t i = 0; i < kOvChains; ++i) {
                const uint32_t c = (i >> 1) + 2 * (i & 1u);           // 0, 2, 1, 3
                if(!heads[c].has_contain) continue;
                const OvBlock x = heads[c].contain;
                out[k++] = OvOutBlock{(int64_t)x.a.lo, (int64_t)x.a.hi1 - 1, x.len, (uint8_t)(x.flags & 1u), (uint8_t)((x.flags >> 1) & 1u), (uint8_t)((x.flags >> 2) & 1u), 1};
            }
            ws.ctl()[2] = k;
        });
        n_out = w.uniform(ws.ctl()[2]);
        fits = ov_irreducible<Block>(views, mtab, ws, w, joined, n_suffix, read_len, out, n_out, bad, n_rank, n_blk);
        if(fits && !ov_any_bad(w, bad)) fits = ov_irreducible<Block>(views, mtab, ws, w, joined + n_suffix, n_joined - n_suffix, read_len, out, n_out, bad, n_rank, n_blk);
    }
    res.status = fits ? kOvOk : kOvOverflow;
    res.n_blocks = fits ? n_out : 0u;
}

// One read start to end, as the kernels do it between them: the four chains (overlap_collect_kernel, a lane each), then the
// reduction (overlap_reduce_kernel, a wavefront).  heads: 4, chain_blocks: 4 * slots.
template <class Block, class W>
LRSC_HD void ov_overlap_read(const StrandView<Block>* views, const uint32_t* mtab, const uint8_t* seq, uint32_t n, const OvParams& p, OvChainHead* heads, OvBlock* chain_blocks,
                             const OvWork& ws, W& w, OvOutBlock* out, OvOutRead& res, uint32_t& bad, uint32_t& n_rank, uint32_t& n_blk)
{
    const uint32_t slots = ov_slots(p);
    w.each([&](uint32_t lane) {
        if(lane < kOvChains) {
            heads[lane] = OvChainHead{0u, 0u, 0u, 0u, OvBlock{OvIv{0, 0}, OvIv{0, 0}, 0u, 0u, 0u, 0u}};
            if(n >= p.min_overlap) ov_collect_chain<Block>(views, mtab, seq, n, p.min_overlap, lane, chain_blocks + (uint64_t)lane * slots, slots, heads[lane], bad, n_rank, n_blk);
        }
    });
    if(ov_any_bad(w, bad)) return;
    ov_reduce_read<Block>(views, mtab, heads, chain_blocks, slots, n, p.min_overlap, ws, w, out, res, bad, n_rank, n_blk);
}

} // namespace lrsc
