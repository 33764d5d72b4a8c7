// fm_fmmerge.h -- unambiguous read merging over a resident index: what the device fm-merge (fm_fmmerge.hip) does per read and per
// node after the exact overlap of fm_overlap.h, the reference's FMMergeProcess::process with what it calls
// (Algorithm/FMMergeProcess.cpp:30-230 process, 233-251 checkCandidate, 253-310 addCandidates; Algorithm/OverlapBlock.cpp:119-160
// getEdgeDir and toOverlap; Bigraph/Bigraph.cpp:162-220 merge, 452-524 simplify; Bigraph/Vertex.cpp:30-75 Vertex::merge), for an
// index without duplicates and contained reads, in which every block is one row.
//
//   links     fmm_link_read, one lane per read: the read's final blocks, still in the overlap's pool, become one FmmLink per end
//             (end 0 = ED_SENSE, query_rev == 0; end 1 = ED_ANTISENSE).  Containment blocks are dropped (removeContainmentBlocks).
//             An end with exactly one block has a link (addCandidates' numSense / numAnti == 1): its target is the read of the
//             block's row through the strand's lexicographic order, the target's end is the twin direction of toOverlap (a
//             target that is not reversed is met at its prefix, its antisense end), the relative strand is isReverseComplement.
//             A read whose only block on an end is itself (the reference asserts) has no link there and is flagged.
//   chains    A node is (read, exit end), 2 * read + end.  The successor of a node whose link is mutual (the target's end has
//             exactly one block, checkCandidate, and that block leads back) is (target, the target's other end); a node without
//             one is terminal and its own successor.  Every node has at most one successor and one predecessor, so the nodes
//             form directed paths and cycles, each with its mirror image: the mirror of node x is x ^ 1, and the predecessor of
//             x is the mirror of the successor of x ^ 1.  fmm_node_init and fmm_rounds(n) rounds of fmm_node_round (pointer
//             doubling, ping-pong) give every node the node it reaches, the bases (64 bits), the steps and the lowest read
//             number on the way.  The strand needs no parity of its own: a link's relative strand is (end == target end), so
//             which of a read's two nodes lies on the root's forward traversal says whether the read is reversed.
//   cut       fmm_cut, after the first ranking.  A node whose jump target is not terminal lies on a cycle and its minimum is the
//             cycle's root: the link that enters the root at its antisense end is cut, so the cycle becomes the path that starts
//             with the root and runs towards its sense end.  A terminal node (P, e) whose link is not mutual because the
//             target's end (Q, A) has another number of blocks than one is what checkCandidate refuses: the candidate is
//             coloured red and never uncoloured (FMMergeProcess.cpp:87-117).  Where Q is the other end of P's own chain (a cycle
//             with a read leading into it at Q) the other arm of the search had accepted Q: it is marked used, swept and absent
//             from the output.  Q is cut off and flagged dropped, and its neighbour's order key takes Q's number.  Then the
//             nodes are ranked again: all chains are paths now.
//   place     fmm_place_read: the chain's root is its lowest-numbered read that is in the sequence, the sequence reads on the
//             root's forward strand, a read's offset is the bases that the mirror of its node has ahead.  The root enters the
//             sequence's length, root and reads under the chain's key, its lowest-numbered used read; a prefix sum over the keys
//             gives the sequences' numbers (merged-0, merged-1, ...) and offsets.
//   assemble  fmm_assemble_base: every read writes its bases beyond the overlap with its predecessor, the first read whole, a
//             reversed read complemented.
//
// Every function is LRSC_HD and free of HIP types: the kernels call them a lane per item, and tests/host_tools/fmmerge_driver.cpp
// runs the same source on the CPU, item by item.  Nothing walks a chain link by link.
#pragma once
#include <stdint.h>

#include "fm_overlap.h"

namespace lrsc {

constexpr uint32_t kFmmThreads = 256;
// Wavefronts per SIMD the launches are sized for: a round is one dependent 24-byte gather per lane and latency-bound, and a
// lane holds two nodes, so the kernels stay far below 512 / 8 VGPRs.
constexpr uint32_t kFmmWavesPerSimd = 8;
constexpr uint32_t kFmmNone = 0xFFFFFFFFu;
constexpr uint32_t kFmmAssembleLanes = 16;                        // lanes that write one read's bases
// lrsc_fmmerge refuses more reads: a node number is 2 * read + end in 32 bits
constexpr uint32_t kFmmMaxReads = 0x7FFFFFFFu;

// FmmLink::flags
enum : uint32_t {
    kFmmLink = 1u,                                                // exactly one block on this end, and not the read itself
    kFmmTargetEnd = 2u,                                           // the end of the target that the link arrives at
    kFmmRc = 4u,                                                  // the target is on the other strand
    kFmmSelf = 8u,                                                // the only block on this end is the read itself
};
// what lrsc_fmmerge refuses, by the lowest read that shows it: first_bad[kFmmBad...]
enum : uint32_t { kFmmBadOverflow = 0, kFmmBadFilter = 1, kFmmBadOwnRow = 2, kFmmBadPool = 3, kFmmBadCount = 4 };
// lrsc_fmmerge_read::flags
enum : uint32_t { kFmmReversed = 1u, kFmmDropped = 2u, kFmmSelfLink = 4u };

struct FmmLink {
    uint32_t target, overlap, flags, count;                       // count: the blocks on this end
};
struct FmmNode {
    uint32_t jump, min_read, min_key, steps;                      // over the jump, its target included
    uint64_t dist;                                                // the bases the jump adds behind this node's read
};
struct FmmOutRead {                                               // lrsc_fmmerge_read
    uint32_t seq, flags;
    uint64_t offset;
};
struct FmmOutSeq {                                                // lrsc_fmmerge_seq
    uint64_t offset, length;
    uint32_t n_reads, root, circular, pad;
};
static_assert(sizeof(FmmLink) == 16 && sizeof(FmmNode) == 24 && sizeof(FmmOutRead) == 16 && sizeof(FmmOutSeq) == 32, "the records' strides");

// The state of a call, O(reads): every array on the device, or the driver's.
struct FmmState {
    const uint64_t* read_off;                                     // n + 1
    uint32_t n, pad;
    FmmLink* links;                                               // 2 n
    uint32_t* cut;                                                // 2 n: the link of this node was cut
    uint32_t* seed;                                               // n: the read's order key, its own number or a dropped neighbour's
    uint32_t* mark;                                               // n: kFmmDropped, bit 31: the root of a cycle
    uint32_t* aux;                                                // n: a dropped read's neighbour
    uint32_t* key_of;                                             // n: the read's chain key
    uint32_t* root_of;                                            // n
    uint64_t* off_in_seq;                                         // n
    uint64_t* key_len;                                            // n: under a key, the sequence's length (0: no sequence)
    uint32_t* key_reads;                                          // n: its reads
    uint32_t* key_seq;                                            // n: exclusive prefix sum of (key_len != 0)
    uint64_t* key_off;                                            // n: exclusive prefix sum of key_len
};
constexpr uint32_t kFmmCycleRoot = 0x80000000u;

LRSC_HD uint32_t fmm_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// rounds of doubling after which a node of a path has reached its end: 2^rounds >= 2 n
LRSC_HD uint32_t fmm_rounds(uint32_t n)
{
    uint32_t r = 0;
    while(((uint64_t)1 << r) < 2ull * n) ++r;
    return r;
}

LRSC_HD void fmm_note_bad(uint32_t* first_bad, uint32_t which, uint32_t read)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_min(first_bad + which, read, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the compiler's own: no HIP header here
#else
    first_bad[which] = fmm_min(first_bad[which], read);
#endif
}

// ---- links: one read.  res and pool are the overlap's (pool + res.first_block = the read's final blocks), head0 is chain 0's
// head, order[s] the lexicographic order of strand s.  The read's two links to out[0 .. 2).
LRSC_HD void fmm_link_read(uint32_t read, uint32_t n_reads, uint32_t read_len, uint32_t min_overlap, const OvOutRead& res, const OvOutBlock* pool, uint64_t pool_size,
                           const OvChainHead& head0, const uint32_t* const* order, FmmLink* out, uint32_t* first_bad)
{
    FmmLink l[2] = {FmmLink{kFmmNone, 0u, 0u, 0u}, FmmLink{kFmmNone, 0u, 0u, 0u}};
    if(res.status != kOvOk) fmm_note_bad(first_bad, kFmmBadOverflow, read);
    if(res.is_substring) fmm_note_bad(first_bad, kFmmBadFilter, read);
    else if(read_len >= min_overlap) {
        // findInterval of the read and its '$' (FMMergeProcess.cpp:33-41): one row, the read's own
        const OvIv own = head0.contain.a;
        if(!head0.has_contain || own.lo >= n_reads || own.hi1 <= own.lo) fmm_note_bad(first_bad, kFmmBadOwnRow, read);
        else if(own.hi1 - own.lo != 1) fmm_note_bad(first_bad, kFmmBadFilter, read);
        else if(order[0][own.lo] != read) fmm_note_bad(first_bad, kFmmBadOwnRow, read);
    }
    // blocks that are not in the pool: the read must not become a singleton (lrsc_overlap_exact refuses the same)
    const bool in_pool = res.n_blocks <= kOvOutCap && res.first_block <= pool_size && res.n_blocks <= pool_size - res.first_block;
    if(res.status == kOvOk && !in_pool) fmm_note_bad(first_bad, kFmmBadPool, read);
    const uint32_t n_blocks = res.status == kOvOk && in_pool ? res.n_blocks : 0u;
    for(uint32_t i = 0; i < n_blocks; ++i) {
        const OvOutBlock b = pool[res.first_block + i];
        if(b.contained) continue;
        if(b.upper != b.lower) fmm_note_bad(first_bad, kFmmBadFilter, read);
        if(b.lower < 0 || (uint64_t)b.lower >= n_reads) { fmm_note_bad(first_bad, kFmmBadOwnRow, read); continue; }
        FmmLink& e = l[b.query_rev ? 1 : 0];
        if(e.count++ == 0) {
            e.target = order[b.target_rev ? 1 : 0][b.lower];
            e.overlap = b.overlap_len;
            e.flags = (b.target_rev ? 0u : kFmmTargetEnd) | (b.target_rev != b.query_rev ? kFmmRc : 0u);
        }
    }
    for(uint32_t e = 0; e < 2; ++e) {
        if(l[e].count != 1 || l[e].target >= n_reads) l[e] = FmmLink{kFmmNone, 0u, 0u, l[e].count};
        else if(l[e].target == read) l[e] = FmmLink{kFmmNone, 0u, kFmmSelf, 1u};
        else l[e].flags |= kFmmLink;
        out[e] = l[e];
    }
}

// ---- chains
LRSC_HD uint32_t fmm_len(const FmmState& s, uint32_t read) { return (uint32_t)(s.read_off[read + 1] - s.read_off[read]); }
LRSC_HD uint32_t fmm_arrival(const FmmLink& l) { return 2 * l.target + ((l.flags & kFmmTargetEnd) ? 1u : 0u); }
// the link of node x leads to an end whose one link leads back
LRSC_HD bool fmm_mutual(const FmmState& s, uint32_t x)
{
    const FmmLink l = s.links[x];
    if(!(l.flags & kFmmLink)) return false;
    const FmmLink back = s.links[fmm_arrival(l)];
    return (back.flags & kFmmLink) && fmm_arrival(back) == x;
}
// the successor of node x, x itself when it is terminal
LRSC_HD uint32_t fmm_succ(const FmmState& s, uint32_t x)
{
    if(s.cut[x] || !fmm_mutual(s, x)) return x;
    return fmm_arrival(s.links[x]) ^ 1u;
}
LRSC_HD FmmNode fmm_node_init(const FmmState& s, uint32_t x)
{
    const uint32_t y = fmm_succ(s, x), r = x >> 1, t = y >> 1;
    if(y == x) return FmmNode{x, r, s.seed[r], 0u, 0ull};
    return FmmNode{y, fmm_min(r, t), fmm_min(s.seed[r], s.seed[t]), 1u, (uint64_t)(fmm_len(s, t) - s.links[x].overlap)};
}
// one round of doubling: a terminal node is its own jump target and adds nothing
LRSC_HD FmmNode fmm_node_round(const FmmNode* in, uint32_t x)
{
    const FmmNode a = in[x], b = in[a.jump];
    return FmmNode{b.jump, fmm_min(a.min_read, b.min_read), fmm_min(a.min_key, b.min_key), a.steps + b.steps, a.dist + b.dist};
}
// after the first ranking: the cycles' cuts and the dropped reads.  Whether a node lies on a cycle, or is a path's end, is read from
// links and nodes alone, never from cut.  cut, seed, mark and aux of other nodes than x are written, and seed and mark are read
// where they are written (a minimum, an or).  That is safe because every word has one writer in the launch: a cycle has one
// root, whose node (root, antisense) alone cuts it and marks it; a path has one end whose link can be refused, and that end's
// node alone cuts off Q, marks it and lowers its neighbour's seed; the reads of different chains are different words.
LRSC_HD void fmm_cut(const FmmState& s, const FmmNode* nodes, uint32_t x)
{
    const FmmNode a = nodes[x];
    const uint32_t r = x >> 1;
    if(fmm_mutual(s, a.jump)) {                                   // the jump target is not terminal (nothing is cut yet): on a cycle
        if(a.min_read == r && (x & 1u)) {
            s.cut[x] = 1u;
            s.cut[fmm_arrival(s.links[x])] = 1u;
            s.mark[r] |= kFmmCycleRoot;
        }
        return;
    }
    const FmmLink l = s.links[x];
    if(a.jump != x || !(l.flags & kFmmLink) || fmm_mutual(s, x)) return;
    const uint32_t qa = fmm_arrival(l), q = l.target;
    if(s.links[qa].count == 1 || nodes[x ^ 1u].jump != qa) return;    // accepted, or a read of another chain: red, swept, not used
    const uint32_t qb = qa ^ 1u;                                  // Q's node towards the chain
    if(!fmm_mutual(s, qb)) return;
    const uint32_t sa = fmm_arrival(s.links[qb]), nb = sa >> 1;
    s.cut[qb] = 1u;
    s.cut[sa] = 1u;
    s.mark[q] |= kFmmDropped;
    s.aux[q] = nb;
    s.seed[nb] = fmm_min(s.seed[nb], q);
}

// ---- place: one read, after the second ranking
LRSC_HD void fmm_place_read(const FmmState& s, const FmmNode* nodes, uint32_t r)
{
    if(s.mark[r] & kFmmDropped) return;
    const FmmNode a = nodes[2 * r], b = nodes[2 * r + 1];
    const uint32_t root = fmm_min(a.min_read, b.min_read), key = fmm_min(a.min_key, b.min_key);
    const uint32_t end = nodes[2 * root].jump;                    // where the root's forward traversal ends
    const bool forward = a.jump == end;
    s.root_of[r] = root | (forward ? 0u : kFmmCycleRoot);
    s.key_of[r] = key;
    s.off_in_seq[r] = forward ? b.dist : a.dist;
    if(r == root) {
        s.key_len[key] = nodes[end ^ 1u].dist + fmm_len(s, end >> 1);
        s.key_reads[key] = a.steps + b.steps + 1;
    }
}
// the records of one read, after the prefix sums over the keys
LRSC_HD void fmm_finish_read(const FmmState& s, uint32_t r, FmmOutRead* per_read, FmmOutSeq* seqs)
{
    const uint32_t self = ((s.links[2 * r].flags | s.links[2 * r + 1].flags) & kFmmSelf) ? kFmmSelfLink : 0u;
    if(s.mark[r] & kFmmDropped) {
        per_read[r] = FmmOutRead{s.key_seq[s.key_of[s.aux[r]]], kFmmDropped | self, 0ull};
        return;
    }
    const uint32_t key = s.key_of[r], root = s.root_of[r] & ~kFmmCycleRoot;
    per_read[r] = FmmOutRead{s.key_seq[key], ((s.root_of[r] & kFmmCycleRoot) ? kFmmReversed : 0u) | self, s.off_in_seq[r]};
    if(r == root) seqs[s.key_seq[key]] = FmmOutSeq{s.key_off[key], s.key_len[key], s.key_reads[key], root, (s.mark[r] & kFmmCycleRoot) ? 1u : 0u, 0u};
}

// ---- assemble: what read r writes.  first: the first of its bases, in the sequence's direction, that it writes (its overlap
// with its predecessor, 0 for the first read); at: where base 0 of it stands among all bases.  False for a dropped read.
LRSC_HD bool fmm_assemble_plan(const FmmState& s, uint32_t r, uint32_t& first, uint64_t& at, bool& reversed)
{
    if(s.mark[r] & kFmmDropped) return false;
    reversed = (s.root_of[r] & kFmmCycleRoot) != 0;
    const uint32_t entry = 2 * r + (reversed ? 0u : 1u);          // the mirror of the read's node: towards its predecessor
    first = fmm_succ(s, entry) != entry ? s.links[entry].overlap : 0u;
    at = s.key_off[s.key_of[r]] + s.off_in_seq[r];
    return true;
}
// base j of read r as the sequence reads it, from the read's codes
LRSC_HD char fmm_assemble_base(const uint8_t* codes, uint32_t len, uint32_t j, bool reversed)
{
    const uint32_t c = reversed ? 3u - (codes[len - 1 - j] & 3u) : (codes[j] & 3u);
    return (char)(c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : 'T');
}

} // namespace lrsc
