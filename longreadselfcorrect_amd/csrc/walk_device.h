// walk_device.h -- the device-side LongReadSelfCorrectByOverlap state machine (Leaf, Walk) shared by the
// per-walk kernel (extend.hip) and the walk-parallel correction flow (wp.hip).
// Reference: PacBio/LongReadCorrectByOverlap.cpp:17-878, FMIndexWalk/SAINode.cpp:166-189.
#pragma once
#include <hip/hip_runtime.h>

#include "extend.h"
#include "introsort_emul.h"
#include "rank_device.h"

// The big sequential pieces of the walk are calls, not inline copies (code size; register budget per piece).  An experiment build can
// define this empty (-DLRSC_WALK_NOINLINE=) to let a kernel's launch bounds govern the whole call tree.
#ifndef LRSC_WALK_NOINLINE
#define LRSC_WALK_NOINLINE __noinline__
#endif
// Device code in the product.  tests/host_walk compiles this header with LRSC_WALK_FN = __host__ __device__ to run the very same
// walk on the CPU against the oracle (test infrastructure: nothing in the product calls the host versions).
#ifndef LRSC_WALK_FN
#define LRSC_WALK_FN __device__
#endif
// Test hook: tests/host_walk_groups defines LRSC_WALK_TRACE(kind, a, b) to learn which shapes of the general step its inputs have
// reached (kind 0: a step with a leaves; 1: extendLeaves made a children; 2: the threshold retry taken for leaf a of b; 3:
// SelectFreqsOfrange over a leaves; 4: the children overflowed; 5 / 6: extendLeaves' level-1 / level-2 retry over a leaves; 7: the
// isInsufficientFreqs refine of a children; 8: the trim removed a leaves; 9: a further child of parent a gets ring and path copies;
// 10: the overflow branch with a survivors; 11: a hit stored in result slot a).  tests/host_walk_deal uses it too.  Empty in the
// product and in every other build.
#ifndef LRSC_WALK_TRACE
#define LRSC_WALK_TRACE(kind, a, b)
#endif

namespace lrsc {

constexpr uint64_t kNoKey = ~0ull;

// The bulk part of the constructor for ONE offset i of m_query (LongReadCorrectByOverlap.cpp:82-94,127-152):
// bi-intervals of the 5-mer, the idmer (9-mer) and, inside the target seed, the minOverlap-mer starting at i,
// each with findInterval's early exit; k-mer tables short-cut whole searches when a table of that size exists.
template <bool WIDE>
LRSC_WALK_FN __forceinline__ void prepare_offset(const FmIndexDev& fm, const StrandC<typename Lay<WIDE>::pos_t>& sf,
                                               const StrandC<typename Lay<WIDE>::pos_t>& sr, const uint32_t* __restrict__ mtab,
                                               const uint8_t* __restrict__ q, uint32_t i, uint32_t Lq, uint32_t trg0,
                                               uint32_t seedk, uint32_t mink, SortItem* it9f, SortItem* it9r, uint8_t* flags5,
                                               typename Lay<WIDE>::pos_t* term, uint32_t& n_rank, uint32_t& n_blk)
{
    using P = typename Lay<WIDE>::pos_t;
    const bool want_term = i >= trg0 && i + mink <= Lq;
    uint32_t kmax = 0;
    if(i + 5 <= Lq) kmax = 5;
    if(i + seedk <= Lq) kmax = seedk;
    if(want_term) kmax = mink > kmax ? mink : kmax;
    WalkState<P> st = walk_init<P>();
    for(uint32_t s = 0; s < kmax;) {
        const uint32_t next_emit = s < 5 ? 5u : s < seedk ? seedk : mink;
        bool jumped = false;
        if(next_emit <= kmax) {
            WalkState<P> ts = walk_init<P>();
            const uint32_t tk = table_start<WIDE>(fm, [&](uint32_t t) { return (uint32_t)q[i + t]; }, next_emit, ts);
            if(tk == next_emit) { n_rank += st.n_rank; n_blk += st.n_blk; st = ts; st.n_rank = 0; st.n_blk = 0; s = tk; jumped = true; }
        }
        if(!jumped) { st = walk_step<WIDE>(sf, sr, q[i + s], 1u << 30, st, mtab); ++s; }
        if(st.size == 5) flags5[i] = (uint8_t)((st.fwd.lo <= st.fwd.hi ? 1 : 0) | (st.rvc.lo <= st.rvc.hi ? 2 : 0));
        if(st.size == seedk) {
            // pad carries the idmer's 2-bit code through the sort: the hit chains compare it instead of re-reading m_query
            uint32_t code = 0;
            for(uint32_t t = 0; t < seedk; ++t) code = (code << 2) | q[i + t];
            it9f[i].key = st.fwd.lo <= st.fwd.hi ? (uint64_t)st.fwd.lo : kNoKey; it9f[i].val = i; it9f[i].pad = code;
            it9r[i].key = st.rvc.lo <= st.rvc.hi ? (uint64_t)st.rvc.lo : kNoKey; it9r[i].val = i; it9r[i].pad = code;
        }
        if(st.size == mink && want_term) {
            P* t = term + (uint64_t)(i - trg0) * 4;
            t[0] = st.fwd.lo; t[1] = st.fwd.hi; t[2] = st.rvc.lo; t[3] = st.rvc.hi;
        }
    }
    n_rank += st.n_rank; n_blk += st.n_blk;
}

// The same for every offset of m_query at once, when k-mer tables of exactly the three emitted sizes exist (the normal
// configuration: 5, idmer = 9, minOverlap = 13): every emit is one table entry, so a rolling 2-bit window supplies the three
// table indexes from ONE character load per offset (the generic path re-reads 5 + 9 + 13 characters per offset).
template <bool WIDE>
LRSC_WALK_FN __forceinline__ int ktab_of(const FmIndexDev& fm, uint32_t k)
{
    int t = -1;
    if(fm.ktab[0].k == k) t = 0;
    if(fm.ktab[1].k == k) t = 1;
    if(fm.ktab[2].k == k) t = 2;
    if(fm.ktab[3].k == k) t = 3;
    if(fm.ktab[4].k == k) t = 4;
    return t;
}
template <bool WIDE>
LRSC_WALK_FN __forceinline__ void ktab_entry(const FmIndexDev& fm, int t, uint32_t code, typename Lay<WIDE>::pos_t e[4])
{
    using P = typename Lay<WIDE>::pos_t;
    const void* tabv = t == 0 ? fm.ktab[0].entries : t == 1 ? fm.ktab[1].entries : t == 2 ? fm.ktab[2].entries
                     : t == 3 ? fm.ktab[3].entries : fm.ktab[4].entries;
    if(WIDE) {
        const uint4* tp = reinterpret_cast<const uint4*>(tabv) + (uint64_t)code * 2;
        const uint4 a = tp[0], b = tp[1];
        e[0] = (P)(((uint64_t)a.y << 32) | a.x); e[1] = (P)(((uint64_t)a.w << 32) | a.z);
        e[2] = (P)(((uint64_t)b.y << 32) | b.x); e[3] = (P)(((uint64_t)b.w << 32) | b.z);
    } else {
        const uint4 a = reinterpret_cast<const uint4*>(tabv)[code];
        e[0] = (P)a.x; e[1] = (P)a.y; e[2] = (P)a.z; e[3] = (P)a.w;
    }
}
template <bool WIDE>
LRSC_WALK_FN LRSC_WALK_NOINLINE bool prepare_all_from_tables(const FmIndexDev& fm, const uint8_t* __restrict__ q, uint32_t Lq, uint32_t trg0, uint32_t seedk,
                                                     uint32_t mink, SortItem* it9f, SortItem* it9r, uint8_t* flags5, typename Lay<WIDE>::pos_t* term)
{
    using P = typename Lay<WIDE>::pos_t;
    if(seedk <= 5 || mink <= seedk || mink > 16) return false;
    const int t5 = ktab_of<WIDE>(fm, 5), t9 = ktab_of<WIDE>(fm, seedk), tm = ktab_of<WIDE>(fm, mink);
    if(t5 < 0 || t9 < 0 || tm < 0) return false;
    const uint32_t m5 = (1u << 10) - 1u, m9 = (1u << (2 * seedk)) - 1u, mm = mink >= 16 ? 0xFFFFFFFFu : (1u << (2 * mink)) - 1u;
    // window = characters [i, i + mink) of m_query, newest in the low bits (zeros past the end)
    uint32_t win = 0;
    for(uint32_t t = 0; t + 1 < mink; ++t) win = (win << 2) | (t < Lq ? (uint32_t)q[t] : 0u);
    for(uint32_t i = 0; i < Lq; ++i) {
        win = ((win << 2) | (i + mink - 1 < Lq ? (uint32_t)q[i + mink - 1] : 0u)) & mm;
        P e[4];
        if(i + 5 <= Lq) {
            ktab_entry<WIDE>(fm, t5, (win >> (2 * (mink - 5))) & m5, e);
            flags5[i] = (uint8_t)((e[0] <= e[1] ? 1 : 0) | (e[2] <= e[3] ? 2 : 0));
        }
        if(i + seedk <= Lq) {
            const uint32_t code = (win >> (2 * (mink - seedk))) & m9;
            ktab_entry<WIDE>(fm, t9, code, e);
            it9f[i].key = e[0] <= e[1] ? (uint64_t)e[0] : kNoKey; it9f[i].val = i; it9f[i].pad = code;
            it9r[i].key = e[2] <= e[3] ? (uint64_t)e[2] : kNoKey; it9r[i].val = i; it9r[i].pad = code;
        }
        if(i >= trg0 && i + mink <= Lq) {
            ktab_entry<WIDE>(fm, tm, win, e);
            P* t = term + (uint64_t)(i - trg0) * 4;
            t[0] = e[0]; t[1] = e[1]; t[2] = e[2]; t[3] = e[3];
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------
// 2. the walk
// ---------------------------------------------------------------------------------------
template <class P>
struct alignas(16) Leaf {             // SAIOverlapNode3 + leafInfo, flattened; 16-byte aligned: leaf copies are dwordx4 moves
    P flo, fhi, rlo, rhi;             // fwdInterval (rbwt), rvcInterval (bwt)
    P tflo, tfhi, trlo, trhi;         // SelectFreqsOfrange's per-leaf scratch intervals (maxKmerArray)
    uint64_t suf_lo, suf_hi;          // last 64 characters of the path, 2 bits each, newest in the low bits
    uint64_t lastSeedIdx, lastOverlapLen, totalSeeds, currOverlapLen, numOfErrors, queryOverlapLen;
    double numRedeemSeed, localErr, globalErr;
    uint32_t hist_size;               // GlobalErrorRateRecord.size()
    int32_t lastSeedIdxOffset;
    int32_t res_first, res_second;    // resultindex
    int32_t kmerFrequency;            // leafInfo::kmerFrequency
    int32_t tmpFreq;                  // SelectFreqsOfrange: FMidx::kmerFrequency
    uint32_t tailLetter, tailLetterCount;
    uint32_t path_len;
    uint16_t ring, path;              // slot ids (materialised leaves only)
    uint16_t parent;                  // children: index of the parent in cur[]
    uint8_t ext, alive;               // children: extension code; survival flag
};

template <class P> __host__ __device__ __forceinline__ int64_t isize(P lo, P hi) { return (int64_t)hi - (int64_t)lo + 1; }

// ---- block moves between DISJOINT slots of a walk's workspace (rings, paths, leaves) --------------------------------------
// Written as `dst[k] = src[k]` the compiler cannot tell that the slots are disjoint, so each store orders the next load behind
// it: one memory round trip per element for a lane that has nothing else in flight.  Here a chunk of independent loads is
// issued back to back into registers and stored after one wait.  The chunk sizes are small on purpose: the lane-per-walk
// kernel is compiled at its register limit, and a chunk that spills gives back what it saves.
// 16-byte units through a type that may alias any other (the slots are read as doubles / Leaf fields elsewhere)
typedef uint32_t CopyU4 __attribute__((ext_vector_type(4), may_alias, aligned(16)));
typedef uint32_t CopyU1 __attribute__((may_alias));
constexpr uint32_t kCopyChunk16 = 5;      // 16-byte units per burst (20 registers): divides a ring row's 50
constexpr uint32_t kCopyChunk4 = 8;       // dwords per burst where only 4-byte alignment holds (path rows)

// nb bursts of kCopyChunk16 16-byte units each, both pointers 16-byte aligned
__host__ __device__ __forceinline__ void burst_copy16(void* dst_, const void* src_, uint32_t nb)
{
#if defined(__HIP_DEVICE_COMPILE__)
    CopyU4* dst = reinterpret_cast<CopyU4*>(dst_);
    const CopyU4* src = reinterpret_cast<const CopyU4*>(src_);
    for(uint32_t k = 0; k < nb * kCopyChunk16; k += kCopyChunk16) {
        CopyU4 t[kCopyChunk16];
#pragma unroll
        for(uint32_t j = 0; j < kCopyChunk16; ++j) t[j] = src[k + j];
#pragma unroll
        for(uint32_t j = 0; j < kCopyChunk16; ++j) dst[k + j] = t[j];
    }
#else
    __builtin_memcpy(dst_, src_, (size_t)nb * kCopyChunk16 * 16);
#endif
}
// n dwords, 4-byte alignment.  A tail shorter than a chunk loads its last dword again instead of branching around each load (a
// guarded load would wait for itself alone), and guards the stores.
__host__ __device__ __forceinline__ void burst_copy4(uint32_t* dst_, const uint32_t* src_, uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    CopyU1* dst = reinterpret_cast<CopyU1*>(dst_);
    const CopyU1* src = reinterpret_cast<const CopyU1*>(src_);
    uint32_t k = 0;
    for(; k + kCopyChunk4 <= n; k += kCopyChunk4) {
        uint32_t t[kCopyChunk4];
#pragma unroll
        for(uint32_t j = 0; j < kCopyChunk4; ++j) t[j] = src[k + j];
#pragma unroll
        for(uint32_t j = 0; j < kCopyChunk4; ++j) dst[k + j] = t[j];
    }
    if(k < n) {
        uint32_t t[kCopyChunk4 - 1];
#pragma unroll
        for(uint32_t j = 0; j < kCopyChunk4 - 1; ++j) t[j] = src[k + j < n ? k + j : n - 1];
#pragma unroll
        for(uint32_t j = 0; j < kCopyChunk4 - 1; ++j) if(k + j < n) dst[k + j] = t[j];
    }
#else
    __builtin_memcpy(dst_, src_, (size_t)n * 4);
#endif
}
// one leaf to another slot (dst != src): the whole leaf in, then out
template <class P> __host__ __device__ __forceinline__ void leaf_move(Leaf<P>* dst, const Leaf<P>* src)
{
    static_assert(sizeof(Leaf<P>) % 16 == 0 && alignof(Leaf<P>) == 16, "a leaf moves as 16-byte units");
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr uint32_t N = (uint32_t)(sizeof(Leaf<P>) / 16);
    CopyU4 t[N];
#pragma unroll
    for(uint32_t j = 0; j < N; ++j) t[j] = reinterpret_cast<const CopyU4*>(src)[j];
#pragma unroll
    for(uint32_t j = 0; j < N; ++j) reinterpret_cast<CopyU4*>(dst)[j] = t[j];
#else
    __builtin_memcpy(static_cast<void*>(dst), static_cast<const void*>(src), sizeof(Leaf<P>));
#endif
}

// character `t` (0 = oldest) of the suffix of length l of a leaf's path
template <class P> __host__ __device__ __forceinline__ uint32_t suf_char(const Leaf<P>& lf, uint32_t l, uint32_t t)
{
    const uint32_t back = l - 1 - t;                     // distance from the newest character
    return back < 32 ? (uint32_t)(lf.suf_lo >> (2 * back)) & 3u : (uint32_t)(lf.suf_hi >> (2 * (back - 32))) & 3u;
}
template <class P> __host__ __device__ __forceinline__ void suf_push(Leaf<P>& lf, uint32_t c)
{
    lf.suf_hi = (lf.suf_hi << 2) | (lf.suf_lo >> 62);
    lf.suf_lo = (lf.suf_lo << 2) | c;
}

__host__ __device__ __forceinline__ uint32_t path_get(const uint32_t* p, uint32_t i) { return (p[i >> 4] >> (2 * (i & 15))) & 3u; }
__host__ __device__ __forceinline__ void path_set(uint32_t* p, uint32_t i, uint32_t c)
{
    const uint32_t sh = 2 * (i & 15);
    p[i >> 4] = (p[i >> 4] & ~(3u << sh)) | (c << sh);
}

// Bitsets of the frontier's slot masks when they outgrow a register (Walk<WIDE, true>): bit i of word i >> 6
__host__ __device__ __forceinline__ uint32_t bits_words(uint32_t n) { return (n + 63u) >> 6; }
__host__ __device__ __forceinline__ void bits_set(uint64_t* b, uint32_t i) { b[i >> 6] |= 1ull << (i & 63u); }
__host__ __device__ __forceinline__ bool bits_get(const uint64_t* b, uint32_t i) { return ((b[i >> 6] >> (i & 63u)) & 1ull) != 0; }
__host__ __device__ __forceinline__ void bits_clear_all(uint64_t* b, uint32_t n) { for(uint32_t w = 0; w < bits_words(n); ++w) b[w] = 0; }
// the lowest set bit, cleared (the set is never empty where it is called)
__host__ __device__ __forceinline__ uint32_t bits_take_lowest(uint64_t* b, uint32_t n)
{
    for(uint32_t w = 0; w < bits_words(n); ++w)
        if(b[w]) { const uint32_t s = (uint32_t)__builtin_ctzll(b[w]); b[w] &= b[w] - 1ull; return w * 64u + s; }
    return 0;
}

// The frontier's capacity.  Walk<WIDE> (BIG = false) is the 32-leaf walk: 32 ring / path slots with their masks in 32-bit words,
// kMaxChildren children, kMaxResults result slots.  Walk<WIDE, true> takes its capacity from `cap` at run time -- cap leaves, ring
// and path slots, 4 cap children, cap_results >= 5 cap result slots -- and keeps its slot masks as bitsets in memory.
template <bool BIG> struct WalkCap {};
template <> struct WalkCap<true> {
    uint32_t cap, cap_children, cap_results;
    uint64_t* ring_bits;              // bit s: ring slot s is free              [bits_words(cap)]
    uint64_t* path_bits;              // bit s: path slot s is free              [bits_words(cap)]
    uint64_t* alive_bits;             // PrunedBySeedSupport: child c survived   [bits_words(cap_children)]
    uint64_t* child_bits;             // ... leaf i of cur[] has a surviving child [bits_words(cap)]
    uint64_t* seen_bits;              // the commit: parent i has had its first child [bits_words(cap)]
};

template <bool WIDE, bool BIG = false>
struct Walk : WalkCap<BIG> {
    using P = typename Lay<WIDE>::pos_t;
    // index
    StrandC<P> sF, sR;
    const FmIndexDev* fm;
    const uint32_t* mtab;
    // inputs
    const uint8_t* q;                 // m_query codes
    uint32_t Lq, initk, path_len, trg_len;
    int32_t dis;
    // parameters
    uint32_t seedSize, minOverlap, maxOverlap, maxLeaves;
    uint64_t min_SA_threshold;
    uint64_t PBcoverage;
    double PacBioErrorRate, errorRate;
    uint64_t localK;                  // m_localSimilarlykmerSize (100)
    const double* freqsOfKmerSize;    // [101]
    // derived
    uint64_t maxIndelSize, maxLength, minLength, currentLength, currentKmerSize;
    // workspace
    SortItem *it9f, *it9r;
    uint32_t n9f, n9r;
    uint16_t *next9f, *next9r, *head9f, *head9r;      // chains of equal-code entries in post-sort order, 256 hash buckets
    uint16_t *next5, *head5;                          // 5-mer chains by code (1024 heads), flags5 tells strand validity
    const uint8_t* flags5;
    const P* term;
    uint32_t n_term;
    uint64_t tmask0, tmask1;          // 128-bit filter over the target seed's minOverlap-mers (hash of their last <= 16 characters)
    Leaf<P>* cur;  uint32_t n_cur;
    Leaf<P>* leaf_small;              // the small_cap()-slot leaf buffer (the other one holds max_children()); cur / nxt swap between them
    Leaf<P>* nxt;  uint32_t n_nxt;
    double* rings;                    // [32][100]
    uint32_t* paths;  uint32_t pathw; // [32][pathw]
    uint32_t* rpaths;                 // [kMaxResults][pathw]
    WalkResultRec* results; uint32_t n_results;
    uint32_t ring_free, path_free;    // bit s: ring / path slot s is free (slot 0 belongs to the root's lineage)
    uint32_t n_rank, n_blk;
    uint64_t alive_lo, alive_hi;      // PrunedBySeedSupport: bit c = child c survived (kMaxChildren = 128)
    uint32_t has_child;               // ... bit i = leaf i of cur[] has a surviving child
    uint32_t n_highfreq;              // children of the last attempToExtend whose k-mer frequency is above isInsufficientFreqs' threshold
    uint64_t steps;
    uint32_t leaf_steps;              // frontier leaves summed over the steps (profiling)
    uint32_t max_front;               // widest frontier of the walk (profiling)
    uint64_t cyc_setup, cyc_loop;     // profiling: ticks spent building the trees/root and in the extension loop
    uint64_t* prof;                   // profiling: ReadOut::cyc_step of the read, or nullptr
    LRSC_WALK_FN __forceinline__ uint64_t tick() const { return prof ? __builtin_readcyclecounter() : 0; }
    LRSC_WALK_FN __forceinline__ void tock(int k, uint64_t t0) { if(prof) prof[k] += __builtin_readcyclecounter() - t0; }
    int error;

    LRSC_WALK_FN __forceinline__ IvT<P> upd(const StrandC<P>& s, uint32_t c, IvT<P> iv) { n_rank += 2; return update_interval<WIDE>(s, c, iv, mtab, n_blk); }

    // findInterval of the leaf's suffix of length l on both strands (initialRootNode / refineSAInterval):
    // fwd = reverse(kmer) in the rbwt, rvc = revcomp(kmer) in the bwt; both consume kmer[0], kmer[1], ... in order
    LRSC_WALK_FN __forceinline__ void find_suffix_v(uint64_t slo, uint64_t shi, uint32_t l, P& flo, P& fhi, P& rlo, P& rhi)
    {
        auto ch = [&](uint32_t t) -> uint32_t {
            const uint32_t back = l - 1 - t;
            return back < 32 ? (uint32_t)(slo >> (2 * back)) & 3u : (uint32_t)(shi >> (2 * (back - 32))) & 3u;
        };
        WalkState<P> st = walk_init<P>();
        const uint32_t t0 = table_start<WIDE>(*fm, ch, l, st);
        for(uint32_t t = t0; t < l; ++t) {
            if(st.fwd_broken && st.rvc_broken) break;
            st = walk_step<WIDE>(sF, sR, ch(t), 1u << 30, st, mtab);
        }
        n_rank += st.n_rank; n_blk += st.n_blk;
        flo = st.fwd.lo; fhi = st.fwd.hi; rlo = st.rvc.lo; rhi = st.rvc.hi;
    }
    LRSC_WALK_FN LRSC_WALK_NOINLINE void find_suffix(Leaf<P>& lf, uint32_t l)
    {
        P a, b, c, d;
        find_suffix_v(lf.suf_lo, lf.suf_hi, l, a, b, c, d);
        lf.flo = a; lf.fhi = b; lf.rlo = c; lf.rhi = d;
    }

    // refineSAInterval (.cpp:355-369).  The leaves' searches are independent: four run side by side, so that a dependent rank step
    // of one leaf waits together with those of three others (a lane walks its frontier leaf by leaf otherwise)
    LRSC_WALK_FN LRSC_WALK_NOINLINE void refineSAInterval(Leaf<P>* leaves, uint32_t n, uint64_t newKmerSize)
    {
        const uint32_t l = (uint32_t)newKmerSize;
        for(uint32_t i0 = 0; i0 < n; i0 += 4) {
            const uint32_t g = n - i0 < 4 ? n - i0 : 4;
            uint64_t slo[4], shi[4];
            WalkState<P> st[4];
            uint32_t t0[4];
#pragma unroll
            for(uint32_t j = 0; j < 4; ++j) {
                const uint32_t i = i0 + (j < g ? j : 0);
                slo[j] = leaves[i].suf_lo; shi[j] = leaves[i].suf_hi;
            }
#pragma unroll
            for(uint32_t j = 0; j < 4; ++j) {
                st[j] = walk_init<P>();
                const uint64_t a = slo[j], b = shi[j];
                t0[j] = table_start<WIDE>(*fm, [&](uint32_t t) -> uint32_t {
                    const uint32_t back = l - 1 - t;
                    return back < 32 ? (uint32_t)(a >> (2 * back)) & 3u : (uint32_t)(b >> (2 * (back - 32))) & 3u; }, l, st[j]);
            }
            // every chain starts from the same table size (or from nothing): one shared loop counter
            for(uint32_t t = t0[0]; t < l; ++t) {
                bool any = false;
#pragma unroll
                for(uint32_t j = 0; j < 4; ++j) {
                    if(j < g && !(st[j].fwd_broken && st[j].rvc_broken)) {
                        const uint32_t back = l - 1 - t;
                        const uint32_t c = back < 32 ? (uint32_t)(slo[j] >> (2 * back)) & 3u : (uint32_t)(shi[j] >> (2 * (back - 32))) & 3u;
                        st[j] = walk_step<WIDE>(sF, sR, c, 1u << 30, st[j], mtab);
                        any = true;
                    }
                }
                if(!any) break;
            }
#pragma unroll
            for(uint32_t j = 0; j < 4; ++j) {
                if(j < g) {
                    Leaf<P>& lf = leaves[i0 + j];
                    n_rank += st[j].n_rank; n_blk += st[j].n_blk;
                    lf.flo = st[j].fwd.lo; lf.fhi = st[j].fwd.hi; lf.rlo = st[j].rvc.lo; lf.rhi = st[j].rvc.hi;
                }
            }
        }
        currentKmerSize = newKmerSize;
    }

    // ---- SelectFreqsOfrange (.cpp:281-331) ---------------------------------------------------------
    // startkmer = last Lw chars of the suffix of length U; Fwd = findInterval(BWT, startkmer) walks it from
    // its last character backwards; Rvc = findInterval(RBWT, complement(startkmer)) likewise.
    // The pair is findBiInterval of x = revcomp(startkmer) with the strands' roles swapped (f walks the bwt with c, r the
    // rbwt with 3 - c, both from the k-mer's last character backwards), so a k-mer table entry of x's first characters
    // -- same early-exit semantics per strand -- replaces that many dependent rank steps.
    LRSC_WALK_FN __forceinline__ void select_first(uint64_t slo, uint64_t shi, uint32_t U, uint32_t Lw, IvT<P>& f, IvT<P>& r)
    {
        auto sc = [&](uint32_t t) -> uint32_t {                 // suf_char(lf, U, t)
            const uint32_t back = U - 1 - t;
            return back < 32 ? (uint32_t)(slo >> (2 * back)) & 3u : (uint32_t)(shi >> (2 * (back - 32))) & 3u;
        };
        bool fb = false, rb = false;
        uint32_t t1 = 1;
        {
            WalkState<P> ts = walk_init<P>();
            const uint32_t tk = table_start<WIDE>(*fm, [&](uint32_t t) { return 3u - sc(U - 1 - t); }, Lw, ts);
            if(tk != 0) {
                f = ts.rvc; r = ts.fwd; fb = ts.rvc_broken; rb = ts.fwd_broken; t1 = tk;
            } else {
                f = init_interval<P>(sR, sc(U - 1));
                r = init_interval<P>(sF, 3u - sc(U - 1));
                n_rank += 2;
            }
        }
        for(uint32_t t = t1; t < Lw; ++t) {
            if(fb && rb) break;
            const uint32_t c = sc(U - 1 - t);
            if(!fb) { f = upd(sR, c, f); fb = f.lo > f.hi; }
            if(!rb) { r = upd(sF, 3u - c, r); rb = r.lo > r.hi; }
            if(fb && rb) break;
        }
    }
    LRSC_WALK_FN __forceinline__ void select_next(uint64_t slo, uint64_t shi, uint32_t U, uint32_t t, IvT<P>& f, IvT<P>& r)
    {
        const uint32_t back = U - 1 - t;
        const uint32_t b = back < 32 ? (uint32_t)(slo >> (2 * back)) & 3u : (uint32_t)(shi >> (2 * (back - 32))) & 3u;
        f = upd(sR, b, f);                           // no validity check here (.cpp:317-318)
        r = upd(sF, 3u - b, r);
    }
    LRSC_WALK_FN LRSC_WALK_NOINLINE uint64_t SelectFreqsOfrange(uint64_t LowerBound, uint64_t UpperBound, Leaf<P>* leaves, uint32_t n)
    {
        LRSC_WALK_TRACE(3, n, 0);
        int tempmaxfmfreqs = 0;
        const uint32_t U = (uint32_t)UpperBound, Lw = (uint32_t)LowerBound;
        for(uint32_t j = 0; j < n; ++j) {
            Leaf<P>& lf = leaves[j];
            IvT<P> f, r;
            select_first(lf.suf_lo, lf.suf_hi, U, Lw, f, r);
            lf.tflo = f.lo; lf.tfhi = f.hi; lf.trlo = r.lo; lf.trhi = r.hi;
            lf.tmpFreq = (int)(isize(f.lo, f.hi) + isize(r.lo, r.hi));
            if(lf.tmpFreq > tempmaxfmfreqs) tempmaxfmfreqs = lf.tmpFreq;
        }
        if(tempmaxfmfreqs - (int)freqsOfKmerSize[LowerBound] < 5) return LowerBound;

        for(uint64_t i = 1; i <= UpperBound - LowerBound; i++) {
            tempmaxfmfreqs = 0;
            for(uint32_t j = 0; j < n; ++j) {
                Leaf<P>& lf = leaves[j];
                IvT<P> f{lf.tflo, lf.tfhi}, r{lf.trlo, lf.trhi};
                select_next(lf.suf_lo, lf.suf_hi, U, (uint32_t)(UpperBound - LowerBound - i), f, r);
                lf.tflo = f.lo; lf.tfhi = f.hi; lf.trlo = r.lo; lf.trhi = r.hi;
                lf.tmpFreq = (int)(isize(f.lo, f.hi) + isize(r.lo, r.hi));
                if(lf.tmpFreq > tempmaxfmfreqs) tempmaxfmfreqs = lf.tmpFreq;
            }
            if(tempmaxfmfreqs - (int)freqsOfKmerSize[LowerBound + i] < 5) return LowerBound + i;
        }
        return UpperBound;
    }
    // the same for a frontier of one leaf, on values (the leaf's tf* scratch fields are write-only outside this function)
    LRSC_WALK_FN __forceinline__ uint64_t SelectFreqsOfrange1(uint64_t LowerBound, uint64_t UpperBound, uint64_t slo, uint64_t shi)
    {
        const uint32_t U = (uint32_t)UpperBound, Lw = (uint32_t)LowerBound;
        IvT<P> f, r;
        select_first(slo, shi, U, Lw, f, r);
        int freq = (int)(isize(f.lo, f.hi) + isize(r.lo, r.hi));
        int tempmaxfmfreqs = freq > 0 ? freq : 0;
        if(tempmaxfmfreqs - (int)freqsOfKmerSize[LowerBound] < 5) return LowerBound;
        for(uint64_t i = 1; i <= UpperBound - LowerBound; i++) {
            select_next(slo, shi, U, (uint32_t)(UpperBound - LowerBound - i), f, r);
            freq = (int)(isize(f.lo, f.hi) + isize(r.lo, r.hi));
            tempmaxfmfreqs = freq > 0 ? freq : 0;
            if(tempmaxfmfreqs - (int)freqsOfKmerSize[LowerBound + i] < 5) return LowerBound + i;
        }
        return UpperBound;
    }

    // isInsufficientFreqs (.cpp:334-352) over the children attempToExtend has just made: it counted those above the threshold
    LRSC_WALK_FN bool isInsufficientFreqs(uint64_t highfreqscount, uint32_t n)
    {
        if(highfreqscount == 0) return true;
        else if(highfreqscount <= 2 && n >= 5) return true;
        else if(highfreqscount <= 1 && n >= 3) return true;
        return false;
    }

    // ---- ismatchedbykmer (.cpp:787-821): any 5-mer hit of the extended path within the indel window --------
    LRSC_WALK_FN bool ismatchedbykmer(uint32_t code5, bool fvalid, bool rvalid)
    {
        const uint64_t startSeedIdx = (uint64_t)(((int)currentLength - (int)maxIndelSize) > 0 ? ((int)currentLength - (int)maxIndelSize) : 0);
        const uint64_t largeSeedIdx = currentLength + maxIndelSize;
        for(uint32_t j = head5[code5]; j != 0xFFFFu; j = next5[j]) {
            if(j >= startSeedIdx && j <= largeSeedIdx) {
                const uint32_t fl = flags5[j];
                if((fvalid && (fl & 1)) || (rvalid && (fl & 2))) return true;
            }
        }
        return false;
    }

    // ---- getFMIndexExtensions (.cpp:667-784): returns a bit mask of accepted bases, fills ext[] -------------
    struct Ext { IvT<P> f, r; int freq; };
    LRSC_WALK_FN __forceinline__ uint32_t getFMIndexExtensions(const Leaf<P>& lf, Ext ext[4], uint64_t& totalcount_out)
    {
        return getFMIndexExtensions_v(lf.flo, lf.fhi, lf.rlo, lf.rhi, lf.tailLetterCount, lf.suf_lo, ext, totalcount_out);
    }
    LRSC_WALK_FN __forceinline__ uint32_t getFMIndexExtensions_v(P lf_flo, P lf_fhi, P lf_rlo, P lf_rhi, uint32_t lf_tailLetterCount, uint64_t lf_suf_lo,
                                                               Ext ext[4], uint64_t& totalcount_out)
    {
        struct { P flo, fhi, rlo, rhi; uint32_t tailLetterCount; uint64_t suf_lo; } lf{lf_flo, lf_fhi, lf_rlo, lf_rhi, lf_tailLetterCount, lf_suf_lo};
        const uint64_t IntervalSizeCutoff = min_SA_threshold;
        uint64_t totalcount = 0;
        int maxfreqsofleave = 0;
        const bool fv = lf.flo <= lf.fhi, rv = lf.rlo <= lf.rhi;
        // all four bases of a strand from one pair of block loads (the reference issues eight updateIntervals, .cpp:685-700)
        IvT<P> fo[4], ro[4];
        if(fv) { update_interval_all<WIDE, true>(sF, IvT<P>{lf.flo, lf.fhi}, mtab, fo, n_blk); n_rank += 8; }
        if(rv) { update_interval_all<WIDE, true>(sR, IvT<P>{lf.rlo, lf.rhi}, mtab, ro, n_blk); n_rank += 8; }
#pragma unroll
        for(uint32_t b = 0; b < 4; ++b) {
            IvT<P> fp{lf.flo, lf.fhi}, rp{lf.rlo, lf.rhi};
            if(fv) fp = fo[b];
            if(rv) rp = ro[3u - b];
            ext[b].f = fp; ext[b].r = rp;
            ext[b].freq = (int)(isize(fp.lo, fp.hi) + isize(rp.lo, rp.hi));
            totalcount += (uint64_t)(int64_t)ext[b].freq;
            if(ext[b].freq > maxfreqsofleave) maxfreqsofleave = ext[b].freq;
        }
        totalcount_out = totalcount;
        uint32_t mask = 0;
        const bool isHomopolymer = lf.tailLetterCount >= 3;
        for(uint32_t b = 0; b < 4; ++b) {
            const uint64_t kmerFreq = (uint64_t)(int64_t)ext[b].freq;
            const double kmerRatioNotPass = 2;
            double kmerRatioCutoff = 0;
            const double kmerRatio = (double)kmerFreq / (double)maxfreqsofleave;
            const bool efv = ext[b].f.lo <= ext[b].f.hi, erv = ext[b].r.lo <= ext[b].r.hi;
            const uint32_t code5 = (uint32_t)(((lf.suf_lo << 2) | b) & 0x3FFu);
            const bool isFreqPass = kmerFreq >= IntervalSizeCutoff;
            const bool isLowCoverage = totalcount >= IntervalSizeCutoff + 2;
            const bool isRepeat = maxfreqsofleave > 100;
            const bool isHighlyRepeat = maxfreqsofleave > 150;
            const bool isLowlyRepeat = maxfreqsofleave > 50;
            // the 5-mer test (a walk over a chain in global memory) only enters the ladder for repeats: evaluated lazily, it has no
            // side effects (.cpp:716-733 computes it for every base)
            const bool isMatchedBy5mer = isLowlyRepeat && ismatchedbykmer(code5, efv, erv);
            if(isMatchedBy5mer && isHighlyRepeat) kmerRatioCutoff = 0.125;
            else if(isMatchedBy5mer && isLowlyRepeat) kmerRatioCutoff = 0.2;
            else if(isFreqPass) kmerRatioCutoff = 0.25;
            else if(isLowCoverage) kmerRatioCutoff = 0.6;
            else kmerRatioCutoff = kmerRatioNotPass;
            if(isHomopolymer && isRepeat) kmerRatioCutoff = kmerRatioCutoff > 0.3 ? kmerRatioCutoff : 0.3;
            else if(isHomopolymer) kmerRatioCutoff = kmerRatioCutoff > 0.6 ? kmerRatioCutoff : 0.6;
            if(kmerRatio >= kmerRatioCutoff) mask |= 1u << b;
        }
        return mask;
    }

    // capacities: the leaf buffer `leaf_small`, the children of a step, the result slots
    LRSC_WALK_FN __forceinline__ uint32_t small_cap() const { if constexpr(BIG) return this->cap; else return 32u; }
    LRSC_WALK_FN __forceinline__ uint32_t max_children() const { if constexpr(BIG) return this->cap_children; else return kMaxChildren; }
    LRSC_WALK_FN __forceinline__ uint32_t max_results() const { if constexpr(BIG) return this->cap_results; else return kMaxResults; }

    LRSC_WALK_FN void free_leaf_slots(const Leaf<P>& lf)
    {
        if constexpr(BIG) { bits_set(this->ring_bits, lf.ring); bits_set(this->path_bits, lf.path); }
        else {
            ring_free |= 1u << lf.ring;
            path_free |= 1u << lf.path;
        }
    }

    // ---- attempToExtend (.cpp:373-465) + updateLeaves (:468-488) -------------------------------------------
    LRSC_WALK_FN void attempToExtend()
    {
        double minimumErrorRate = 1;
        for(uint32_t i = 0; i < n_cur; i += 4) {                 // four loads in flight, same comparisons in the same order
            double e[4];
#pragma unroll
            for(uint32_t j = 0; j < 4; ++j) e[j] = cur[i + j < n_cur ? i + j : i].localErr;
#pragma unroll
            for(uint32_t j = 0; j < 4; ++j) if(i + j < n_cur && e[j] < minimumErrorRate) minimumErrorRate = e[j];
        }
        // trim leaves whose error rate relative to the best one is high
        uint32_t w = 0;
        for(uint32_t i = 0; i < n_cur; ++i) {
            const double errorRateDiff = cur[i].localErr - minimumErrorRate;
            if((errorRateDiff > 0.05 && currentLength > localK / 2) || (errorRateDiff > 0.1 && currentLength > 15)) {
                free_leaf_slots(cur[i]);
                continue;
            }
            if(w != i) leaf_move(&cur[w], &cur[i]);
            ++w;
        }
        if(w != n_cur) { LRSC_WALK_TRACE(8, n_cur - w, w); }
        n_cur = w;

        n_highfreq = 0;
        const int highfreqThreshold = PBcoverage > 60 ? (int)((uint64_t)(PBcoverage / 60) * 3) : 3;
        // (One leaf at a time on purpose.  Loading the next leaf's interval ends while this one is worked on, so that its rank
        //  blocks and the leaf itself come in one wait, was measured: 13 more VGPR spills and a bulk launch 24 ms LONGER than
        //  without it -- DESIGN 4b, "Leaf groups in the general step".)
        for(uint32_t i = 0; i < n_cur; ++i) {
            const Leaf<P> par = cur[i];                          // one burst of loads: the leaf in registers
            Ext ext[4];
            uint32_t mask = 0;
            int count = 0;
            while(count < 2) {
                if(count == 1 && !(par.localErr == minimumErrorRate && n_cur > 1)) break;
                if(count == 1) { LRSC_WALK_TRACE(2, i, n_cur); }
                uint64_t tc;
                const uint64_t tg = tick();
                mask = getFMIndexExtensions_v(par.flo, par.fhi, par.rlo, par.rhi, par.tailLetterCount, par.suf_lo, ext, tc);
                tock(3, tg);
                if(mask != 0) break;
                min_SA_threshold--;
                count++;
            }
            min_SA_threshold += (uint64_t)count;
            if(mask == 0) continue;
            // updateLeaves: children in base order; leafInfo(child) fields (LongReadCorrectByOverlap.h:172-203)
            for(uint32_t b = 0; b < 4; ++b) {
                if(!(mask & (1u << b))) continue;
                if(n_nxt >= max_children()) { LRSC_WALK_TRACE(4, n_nxt, i); error = LRSC_WALK_ERR_CHILDREN; return; }
                const Leaf<P> ch = make_child(par, i, b, ext[b]);
                if(ch.kmerFrequency > highfreqThreshold) n_highfreq++;      // for isInsufficientFreqs, which looks at exactly these values
                nxt[n_nxt++] = ch;
            }
        }
    }
    // updateLeaves' child of leaf i of cur[] by base b: createChild copies the node state (SAINode.cpp:166-189), leafInfo(child)
    // fields (LongReadCorrectByOverlap.h:172-203)
    LRSC_WALK_FN __forceinline__ Leaf<P> make_child(const Leaf<P>& par, uint32_t i, uint32_t b, const Ext& e) const
    {
        Leaf<P> ch = par;
        ch.flo = e.f.lo; ch.fhi = e.f.hi; ch.rlo = e.r.lo; ch.rhi = e.r.hi;
        ch.kmerFrequency = e.freq;
        ch.currOverlapLen++;
        ch.queryOverlapLen++;
        if(par.tailLetter == b) ch.tailLetterCount = par.tailLetterCount + 1;
        else { ch.tailLetter = b; ch.tailLetterCount = 1; }
        suf_push(ch, b);
        ch.parent = (uint16_t)i;
        ch.ext = (uint8_t)b;
        ch.alive = 1;
        return ch;
    }

    // ---- extendLeaves (.cpp:239-278) ------------------------------------------------------------------------
    LRSC_WALK_FN void extendLeaves()
    {
        n_nxt = 0;
        uint64_t t = tick();
        if(currentKmerSize > maxOverlap) refineSAInterval(cur, n_cur, maxOverlap);
        tock(1, t);
        t = tick();
        attempToExtend();
        tock(2, t);
        if(error) return;
        if(n_nxt == 0) {                                    // level 1: reduce the k-mer size
            LRSC_WALK_TRACE(5, n_cur, 0);
            const uint64_t LowerBound = (currentKmerSize - 2) > minOverlap ? (currentKmerSize - 2) : minOverlap;
            const uint64_t ts = tick();
            const uint64_t ReduceSize = SelectFreqsOfrange(LowerBound, currentKmerSize, cur, n_cur);
            tock(8, ts);
            refineSAInterval(cur, n_cur, ReduceSize);
            attempToExtend();
            if(error) return;
            if(n_nxt == 0) {                                // level 2: reduce the threshold
                LRSC_WALK_TRACE(6, n_cur, 0);
                min_SA_threshold--;
                attempToExtend();
                min_SA_threshold++;
                if(error) return;
            }
        }
        if(n_nxt != 0) {
            currentLength++;
            currentKmerSize++;
            if(isInsufficientFreqs(n_highfreq, n_nxt)) {    // frequencies are low: relax the k-mer size
                LRSC_WALK_TRACE(7, n_nxt, 0);
                const uint64_t LowerBound = (currentKmerSize - 2) > minOverlap ? (currentKmerSize - 2) : minOverlap;
                const uint64_t ts = tick();
                const uint64_t ReduceSize = SelectFreqsOfrange(LowerBound, currentKmerSize, nxt, n_nxt);
                tock(8, ts);
                refineSAInterval(nxt, n_nxt, ReduceSize);
            }
        }
    }

    // ---- isSupportedByNewSeed (.cpp:566-635) ------------------------------------------------------------------
    LRSC_WALK_FN LRSC_WALK_NOINLINE bool isSupportedByNewSeed(Leaf<P>& nd, uint64_t smallSeedIdx, uint64_t largeSeedIdx)
    {
        return seed_support_core(nd, smallSeedIdx, largeSeedIdx);
    }
    LRSC_WALK_FN __forceinline__ bool seed_support_core(Leaf<P>& nd, uint64_t smallSeedIdx, uint64_t largeSeedIdx)
    {
        const uint64_t seedIdxOffset = nd.lastOverlapLen < currentLength - seedSize ? (uint64_t)seedSize : currentLength - nd.lastOverlapLen;
        const uint64_t cand = nd.lastSeedIdx + seedIdxOffset;
        const uint64_t startSeedIdx = smallSeedIdx > cand ? smallSeedIdx : cand;
        bool isNewSeedFound = false;
        const bool fv = nd.flo <= nd.fhi, rv = nd.rlo <= nd.rhi;
        const uint32_t mask9 = seedSize >= 16 ? 0xFFFFFFFFu : ((1u << (2 * seedSize)) - 1u);
        const uint32_t code9 = (uint32_t)nd.suf_lo & mask9;
        const uint32_t hb = (code9 ^ (code9 >> 9)) & 255u;
        // fwd / rvc hit lists in post-sort order: entries of this k-mer chained in the bucket
        uint32_t jf = fv ? head9f[hb] : 0xFFFFu;
        uint32_t jr = rv ? head9r[hb] : 0xFFFFu;
        auto advance = [&](uint32_t j, const SortItem* it, const uint16_t* nx) -> uint32_t {
            while(j != 0xFFFFu && it[j].pad != code9) j = nx[j];
            return j;
        };
        jf = advance(jf, it9f, next9f);
        jr = advance(jr, it9r, next9r);
        int minIdxDiff = 10000;
        const uint64_t currSeedIdx = currentLength - seedSize;
        while(jf != 0xFFFFu || jr != 0xFFFFu) {
            const uint64_t vf = jf != 0xFFFFu ? it9f[jf].val : 0, vr = jr != 0xFFFFu ? it9r[jr].val : 0;
            if(fv && jf != 0xFFFFu && vf >= startSeedIdx && vf <= largeSeedIdx) {
                LRSC_WALK_TRACE(12, 0, 0);
                const int d = abs((int)vf - (int)currSeedIdx);
                if(d < minIdxDiff) { nd.lastSeedIdx = vf; nd.queryOverlapLen = vf + seedSize; minIdxDiff = d; }
                nd.lastOverlapLen = currentLength;
                nd.currOverlapLen = currentLength;
                isNewSeedFound = true;
            } else if(rv && jr != 0xFFFFu && vr >= startSeedIdx && vr <= largeSeedIdx) {
                LRSC_WALK_TRACE(12, 1, 0);
                const int d = abs((int)currSeedIdx - (int)vr);
                if(d < minIdxDiff) { nd.lastSeedIdx = vr; nd.queryOverlapLen = vr + seedSize; minIdxDiff = d; }
                nd.lastOverlapLen = currentLength;
                nd.currOverlapLen = currentLength;
                isNewSeedFound = true;
            }
            if(jf != 0xFFFFu) jf = advance(next9f[jf], it9f, next9f);
            if(jr != 0xFFFFu) jr = advance(next9r[jr], it9r, next9r);
        }
        if(isNewSeedFound) nd.totalSeeds++;
        return isNewSeedFound;
    }

    // seedSize-mer code of m_query at offset i (first character in the high bits)
    LRSC_WALK_FN __forceinline__ uint32_t kmer_code(uint32_t i) const
    {
        uint32_t c = 0;
        for(uint32_t t = 0; t < seedSize; ++t) c = (c << 2) | q[i + t];
        return c;
    }

    // ---- computeErrorRate (.cpp:638-664) ------------------------------------------------------------------
    LRSC_WALK_FN double computeErrorRate(Leaf<P>& nd, const double* parent_ring)
    {
        double matchedLen = (double)nd.totalSeeds + seedSize - 1;
        matchedLen += nd.numRedeemSeed;
        const double totalLen = (double)nd.currOverlapLen;
        const double unmatchedLen = totalLen - matchedLen;
        double currErrorRate = unmatchedLen / totalLen;
        nd.globalErr = currErrorRate;
        const uint32_t totalsize = nd.hist_size + 1;          // after the push_back
        nd.hist_size = totalsize;
        if(totalsize >= localK) {
            const double old = parent_ring[(totalsize - localK) % 100];
            currErrorRate = (currErrorRate * totalLen - old * (totalLen - localK)) / localK;
        }
        nd.localErr = currErrorRate;
        return currErrorRate;
    }

    // ---- PrunedBySeedSupport (.cpp:491-563) ------------------------------------------------------------------
    template <bool INLINE>
    LRSC_WALK_FN __forceinline__ void prune_leaf(Leaf<P>& leaf, const double* pring, uint64_t currSeedIdx, uint64_t smallSeedIdx, uint64_t largeSeedIdx)
    {
        bool isNewSeedFound = false;
        if(currentLength - leaf.lastOverlapLen > seedSize || currentLength - leaf.lastOverlapLen <= 1) {
            const uint64_t preSeedIdx = leaf.lastSeedIdx;
            isNewSeedFound = INLINE ? seed_support_core(leaf, smallSeedIdx, largeSeedIdx) : isSupportedByNewSeed(leaf, smallSeedIdx, largeSeedIdx);
            if(isNewSeedFound) {
                if(currSeedIdx + (uint64_t)(int64_t)leaf.lastSeedIdxOffset - preSeedIdx > seedSize)
                    leaf.numRedeemSeed += (seedSize - 1) * PacBioErrorRate;
                leaf.lastSeedIdxOffset = (int)leaf.lastSeedIdx - (int)currSeedIdx;
            } else {
                const uint64_t v = currSeedIdx + (uint64_t)(int64_t)leaf.lastSeedIdxOffset - leaf.lastSeedIdx;
                if(v % seedSize == 1) leaf.numOfErrors++;
                else if(v > (uint64_t)seedSize - 1) leaf.numRedeemSeed += 1 - PacBioErrorRate;
            }
        } else
            leaf.numRedeemSeed += 1 - PacBioErrorRate;
        const double currErrorRate = computeErrorRate(leaf, pring);
        if(currErrorRate > errorRate) leaf.alive = 0;
    }
    // Group sizes of the general step's per-leaf and per-child loops, by measurement ("Leaf groups in the general
    // step"): the kernel is compiled at its register limit, and a wider group spills what it keeps in flight.  Children of
    // PrunedBySeedSupport: 1 -> 598 ms, 2 -> 593 ms, 4 -> 649 ms per bulk launch (parent 630 ms).  Commit: 2 and 4 within the
    // spread of each other.  The isTerminated loop keeps one 8-byte suffix per leaf.
    static constexpr uint32_t kPruneGroup = 2;
    static constexpr uint32_t kCommitGroup = 2;
    static constexpr uint32_t kTermGroup = 4;
    LRSC_WALK_FN void PrunedBySeedSupport()
    {
        const uint64_t currSeedIdx = currentLength - seedSize;
        const uint64_t indelOffset = seedSize + maxIndelSize;
        const uint64_t smallSeedIdx = currSeedIdx <= indelOffset ? 0 : currSeedIdx - indelOffset;
        const uint64_t largeSeedIdx = (currSeedIdx + indelOffset) >= (Lq - seedSize) ? (Lq - seedSize) : currSeedIdx + indelOffset;
        alive_lo = 0; alive_hi = 0; has_child = 0;
        if constexpr(BIG) { bits_clear_all(this->alive_bits, n_nxt); bits_clear_all(this->child_bits, n_cur); }
        // prune_leaf for kPruneGroup children side by side.  Why the order inside a group cannot be observed: a child's evaluation
        // reads its own fields, the walk's tables (head9 / it9 / next9: fixed since begin_static) and one slot of its parent's ring
        // (rings are written by the commit only), and writes its own fields; the frontier's bit sets are set afterwards, per child
        // in child order.  So what differs from the loop of prune_leaf calls is only when the loads are issued: a group's fields
        // (the part of a leaf the evaluation touches, not the whole leaf), then its bucket heads and ring slots, then the chain
        // entries of all its cursors (two strands per child) step by step, each step one wait for the lane instead of one per
        // entry, strand and child.  An entry comes with its successor's index, so a skipped entry and a hit cost the same.
        // The arithmetic is prune_leaf's, seed_support_core's and computeErrorRate's, statement for statement.
        constexpr uint32_t G = kPruneGroup;
        constexpr uint32_t NIL = 0xFFFFu;
        const uint32_t mask9 = seedSize >= 16 ? 0xFFFFFFFFu : ((1u << (2 * seedSize)) - 1u);
        for(uint32_t c0 = 0; c0 < n_nxt; c0 += G) {
            const uint32_t g = n_nxt - c0 < G ? n_nxt - c0 : G;
            uint64_t lastSeedIdx[G], lastOverlapLen[G], totalSeeds[G], currOverlapLen[G], numOfErrors[G], queryOverlapLen[G];
            double numRedeemSeed[G];
            uint32_t hist_size[G], code9[G], ring[G], parent[G];
            int32_t lastSeedIdxOffset[G];
            bool fv[G], rv[G];
#pragma unroll
            for(uint32_t j = 0; j < G; ++j) {                    // a short group is padded with its first child (nothing of it is kept)
                const Leaf<P>& lf = nxt[c0 + (j < g ? j : 0)];
                lastSeedIdx[j] = lf.lastSeedIdx; lastOverlapLen[j] = lf.lastOverlapLen; totalSeeds[j] = lf.totalSeeds;
                currOverlapLen[j] = lf.currOverlapLen; numOfErrors[j] = lf.numOfErrors; queryOverlapLen[j] = lf.queryOverlapLen;
                numRedeemSeed[j] = lf.numRedeemSeed; hist_size[j] = lf.hist_size; lastSeedIdxOffset[j] = lf.lastSeedIdxOffset;
                code9[j] = (uint32_t)lf.suf_lo & mask9; ring[j] = lf.ring; parent[j] = lf.parent;
                fv[j] = lf.flo <= lf.fhi; rv[j] = lf.rlo <= lf.rhi;
            }
            // bucket heads and the ring slot computeErrorRate reads (slot 0, unused, while the history is shorter than localK).
            // createChild copied the parent's ring id into the child: cur[parent].ring == the child's ring until the commit
            bool need[G];
            uint64_t preSeedIdx[G], startSeedIdx[G];
            uint32_t jf[G], jr[G];
            double old[G];
#pragma unroll
            for(uint32_t j = 0; j < G; ++j) {
                const uint64_t d = currentLength - lastOverlapLen[j];
                need[j] = j < g && (d > seedSize || d <= 1);
                preSeedIdx[j] = lastSeedIdx[j];
                const uint64_t seedIdxOffset = lastOverlapLen[j] < currentLength - seedSize ? (uint64_t)seedSize : currentLength - lastOverlapLen[j];
                const uint64_t cand = lastSeedIdx[j] + seedIdxOffset;
                startSeedIdx[j] = smallSeedIdx > cand ? smallSeedIdx : cand;
                const uint32_t hb = (code9[j] ^ (code9[j] >> 9)) & 255u;
                jf[j] = head9f[hb]; jr[j] = head9r[hb];
                const uint32_t totalsize = hist_size[j] + 1;
                old[j] = rings[(uint64_t)ring[j] * 100 + (totalsize >= localK ? (totalsize - localK) % 100 : 0)];
            }
            // the hit lists in post-sort order (seed_support_core): per child and strand a cursor along the bucket's chain; mf / mr:
            // the cursor stands behind an entry of the child's k-mer that has not been consumed yet (its offset in vf / vr)
            bool mf[G], mr[G], found[G];
            uint32_t vf[G], vr[G];
            int minIdxDiff[G];
#pragma unroll
            for(uint32_t j = 0; j < G; ++j) {
                if(!(need[j] && fv[j])) jf[j] = NIL;
                if(!(need[j] && rv[j])) jr[j] = NIL;
                mf[j] = false; mr[j] = false; found[j] = false; vf[j] = 0; vr[j] = 0; minIdxDiff[j] = 10000;
            }
            while(true) {
                bool seek = false;
#pragma unroll
                for(uint32_t j = 0; j < G; ++j) seek = seek || (!mf[j] && jf[j] != NIL) || (!mr[j] && jr[j] != NIL);
                if(seek) {
                    // one chain step for every cursor that is looking for its next entry; a cursor at rest loads entry 0 for nothing
                    uint32_t pf[G], pr_[G], wf[G], wr[G], nf[G], nr[G];
#pragma unroll
                    for(uint32_t j = 0; j < G; ++j) {
                        const uint32_t a = (!mf[j] && jf[j] != NIL) ? jf[j] : 0u, b = (!mr[j] && jr[j] != NIL) ? jr[j] : 0u;
                        pf[j] = it9f[a].pad; wf[j] = it9f[a].val; nf[j] = next9f[a];
                        pr_[j] = it9r[b].pad; wr[j] = it9r[b].val; nr[j] = next9r[b];
                    }
#pragma unroll
                    for(uint32_t j = 0; j < G; ++j) {
                        if(!mf[j] && jf[j] != NIL) { if(pf[j] == code9[j]) { mf[j] = true; vf[j] = wf[j]; } jf[j] = nf[j]; }
                        if(!mr[j] && jr[j] != NIL) { if(pr_[j] == code9[j]) { mr[j] = true; vr[j] = wr[j]; } jr[j] = nr[j]; }
                    }
                    continue;
                }
                // every cursor has its next entry or is at its chain's end: one round of isSupportedByNewSeed's loop per child
                bool any = false;
#pragma unroll
                for(uint32_t j = 0; j < G; ++j) {
                    if(!(mf[j] || mr[j])) continue;
                    any = true;
                    const uint64_t f = vf[j], r = vr[j];
                    if(mf[j] && f >= startSeedIdx[j] && f <= largeSeedIdx) {
                        const int d = abs((int)f - (int)currSeedIdx);
                        if(d < minIdxDiff[j]) { lastSeedIdx[j] = f; queryOverlapLen[j] = f + seedSize; minIdxDiff[j] = d; }
                        lastOverlapLen[j] = currentLength;
                        currOverlapLen[j] = currentLength;
                        found[j] = true;
                    } else if(mr[j] && r >= startSeedIdx[j] && r <= largeSeedIdx) {
                        const int d = abs((int)currSeedIdx - (int)r);
                        if(d < minIdxDiff[j]) { lastSeedIdx[j] = r; queryOverlapLen[j] = r + seedSize; minIdxDiff[j] = d; }
                        lastOverlapLen[j] = currentLength;
                        currOverlapLen[j] = currentLength;
                        found[j] = true;
                    }
                    mf[j] = false; mr[j] = false;
                }
                if(!any) break;
            }
            // the rest of prune_leaf, computeErrorRate, the stores and the frontier's bit sets: per child, in child order
#pragma unroll
            for(uint32_t j = 0; j < G; ++j) {
                if(j >= g) continue;
                const uint32_t c = c0 + j;
                if(need[j]) {
                    if(found[j]) {
                        totalSeeds[j]++;
                        if(currSeedIdx + (uint64_t)(int64_t)lastSeedIdxOffset[j] - preSeedIdx[j] > seedSize)
                            numRedeemSeed[j] += (seedSize - 1) * PacBioErrorRate;
                        lastSeedIdxOffset[j] = (int)lastSeedIdx[j] - (int)currSeedIdx;
                    } else {
                        const uint64_t v = currSeedIdx + (uint64_t)(int64_t)lastSeedIdxOffset[j] - lastSeedIdx[j];
                        if(v % seedSize == 1) numOfErrors[j]++;
                        else if(v > (uint64_t)seedSize - 1) numRedeemSeed[j] += 1 - PacBioErrorRate;
                    }
                } else
                    numRedeemSeed[j] += 1 - PacBioErrorRate;
                double matchedLen = (double)totalSeeds[j] + seedSize - 1;
                matchedLen += numRedeemSeed[j];
                const double totalLen = (double)currOverlapLen[j];
                const double unmatchedLen = totalLen - matchedLen;
                double currErrorRate = unmatchedLen / totalLen;
                const double globalErr = currErrorRate;
                const uint32_t totalsize = hist_size[j] + 1;          // after the push_back
                if(totalsize >= localK) currErrorRate = (currErrorRate * totalLen - old[j] * (totalLen - localK)) / localK;
                const bool alive = !(currErrorRate > errorRate);
                Leaf<P>& lf = nxt[c];
                lf.lastSeedIdx = lastSeedIdx[j]; lf.lastOverlapLen = lastOverlapLen[j]; lf.totalSeeds = totalSeeds[j];
                lf.currOverlapLen = currOverlapLen[j]; lf.numOfErrors = numOfErrors[j]; lf.queryOverlapLen = queryOverlapLen[j];
                lf.numRedeemSeed = numRedeemSeed[j]; lf.localErr = currErrorRate; lf.globalErr = globalErr;
                lf.hist_size = totalsize; lf.lastSeedIdxOffset = lastSeedIdxOffset[j];
                if(!alive) lf.alive = 0;                             // createChild left it 1
                if constexpr(BIG) { if(alive) { bits_set(this->alive_bits, c); bits_set(this->child_bits, parent[j]); } }
                else if(alive) { if(c < 64) alive_lo |= 1ull << c; else alive_hi |= 1ull << (c - 64); has_child |= 1u << parent[j]; }
            }
        }
    }

    // profiling (WpArgs::gen_stats): the work of this step's PrunedBySeedSupport, counted before it runs -- the children that need
    // the seed-support search, and the chain entries their searches walk (every entry of the child's bucket, per valid strand)
    uint32_t ph_need, ph_chain;
    // ... and of its isTerminated loop, counted after the commit: the leaves that pass term_may_hit and the term rows they scan
    uint32_t ph_term, ph_rows;
    LRSC_WALK_FN void count_prune_work()
    {
        const uint32_t mask9 = seedSize >= 16 ? 0xFFFFFFFFu : ((1u << (2 * seedSize)) - 1u);
        ph_need = 0; ph_chain = 0;
        for(uint32_t c = 0; c < n_nxt; ++c) {
            const Leaf<P>& lf = nxt[c];
            const uint64_t d = currentLength - lf.lastOverlapLen;
            if(!(d > seedSize || d <= 1)) continue;
            ++ph_need;
            const uint32_t code9 = (uint32_t)lf.suf_lo & mask9;
            const uint32_t hb = (code9 ^ (code9 >> 9)) & 255u;
            if(lf.flo <= lf.fhi) for(uint32_t j = head9f[hb]; j != 0xFFFFu; j = next9f[j]) ++ph_chain;
            if(lf.rlo <= lf.rhi) for(uint32_t j = head9r[hb]; j != 0xFFFFu; j = next9r[j]) ++ph_chain;
        }
    }
    LRSC_WALK_FN void count_term_work()
    {
        ph_term = 0; ph_rows = 0;
        if(currentLength < minLength) return;
        for(uint32_t i = 0; i < n_cur; ++i) {
            if(!term_may_hit(cur[i].suf_lo)) continue;
            ++ph_term;
            const uint64_t i0 = (uint64_t)(cur[i].res_second > 0 ? cur[i].res_second : 0), end = (uint64_t)trg_len - (int)minOverlap;
            if(i0 <= end) ph_rows += (uint32_t)(end + 1 - i0);
        }
    }

    // ---- isTerminated for one leaf (.cpp:825-878); path given as (words, len) + optional extra char ------------
    LRSC_WALK_FN LRSC_WALK_NOINLINE void terminated_leaf(Leaf<P>& lf, const uint32_t* pw, uint32_t plen, int extra)
    {
        terminated_hit(lf, term_scan(lf), pw, plen, extra);
    }
    // ... from the scan's answer on (wp_deal_step.h's deal_term hands the owner a scan that another lane ran)
    LRSC_WALK_FN __forceinline__ void terminated_hit(Leaf<P>& lf, int hit, const uint32_t* pw, uint32_t plen, int extra)
    {
        if(hit < 0) return;
        if(lf.res_first == -1) {                         // the first hit of the scan takes a result slot
            if(n_results >= max_results()) { error = LRSC_WALK_ERR_RESULTS; return; }
            ++n_results;
            lf.res_first = (int)n_results;
        }
        lf.res_second = hit;
        LRSC_WALK_TRACE(11, lf.res_first, 0);
        term_store(lf, hit, pw, plen, extra);
    }
    // term_scan's filter: false = no target minOverlap-mer hashes like the last characters of the leaf's suffix
    LRSC_WALK_FN __forceinline__ bool term_may_hit(uint64_t suf_lo) const
    {
        if(currentKmerSize >= minOverlap) {
            const uint32_t L = minOverlap < 16 ? (uint32_t)minOverlap : 16u;
            const uint32_t code = (uint32_t)(suf_lo & (L >= 16 ? 0xFFFFFFFFull : ((1ull << (2 * L)) - 1ull)));
            const uint32_t h = (code * 0x9E3779B1u) >> 25;
            if((((h < 64 ? tmask0 : tmask1) >> (h & 63u)) & 1ull) == 0) return false;
        }
        return true;
    }
    // the scan: the last target offset whose minOverlap-mer interval contains the leaf's (either strand), -1 if none
    LRSC_WALK_FN __forceinline__ int term_scan(const Leaf<P>& lf) const
    {
        const bool fvalid = lf.flo <= lf.fhi, rvalid = lf.rlo <= lf.rhi;
        // A non-empty interval of a k-mer K lies inside the interval of a k-mer w with |w| <= |K| only if K ends with w (fwd strand:
        // reverse(w) is a prefix of reverse(K); rvc strand: revcomp(w) is a prefix of revcomp(K)).  So if no target minOverlap-mer
        // hashes like the leaf's last characters, the scan below cannot hit: skip its loads.
        if(!term_may_hit(lf.suf_lo)) return -1;
        const uint64_t i0 = (uint64_t)(lf.res_second > 0 ? lf.res_second : 0);
        int hit = -1;
        for(uint64_t i = i0; i <= (uint64_t)trg_len - (int)minOverlap; i++) {
            const P* t = term + i * 4;
            const bool isFwdTerminated = fvalid && lf.flo >= t[0] && lf.fhi <= t[1];
            const bool isRvcTerminated = rvalid && lf.rlo >= t[2] && lf.rhi <= t[3];
            if(isFwdTerminated || isRvcTerminated) hit = (int)i;
        }
        return hit;
    }
    // results.at(first - 1) = STresult: thread = getFullString() (+ target.substr(i + minOverlap) appended at the end)
    LRSC_WALK_FN __forceinline__ void term_store(const Leaf<P>& lf, int hit, const uint32_t* pw, uint32_t plen, int extra)
    {
        WalkResultRec& r = results[lf.res_first - 1];
        r.error_rate = lf.globalErr;
        r.match_i = (uint32_t)hit;
        uint32_t* dst = rpaths + (uint64_t)(lf.res_first - 1) * pathw;
        const uint32_t nw = (plen + 15) >> 4;
        burst_copy4(dst, pw, nw);
        uint32_t len = plen;
        if(extra >= 0) { path_set(dst, len, (uint32_t)extra); ++len; }
        r.path_len = len;
    }

    // ---- one walk = begin() + step() until it returns false + finish() ------------------------------------------
    // (split so that the persistent kernel can keep all lanes of a wavefront in the step loop: a lane whose walk
    //  ended sets up its next one while the others wait, instead of idling until the longest walk of the wave ends)
    LRSC_WALK_FN int run(uint32_t* out_len, uint32_t* out_words, uint32_t* out_match_i)
    {
        begin();
        while(step()) {}
        return finish(out_len, out_words, out_match_i);
    }

    bool ended;                        // the frontier overflowed maxLeaves: the loop ends after this isTerminated
    bool profile = false;              // per-step tick counters on (LRSC_CORRECT_PROFILE)
    // maxLeaves is a narrow launch's capacity below the walk's true -l: overflowing it (or the result slots) is not the walk's end
    // but LRSC_WALK_NEEDS_WIDE from finish()
    bool escalate = false;
    // test hook (LRSC_WP_BEGIN_SORT): every interval list takes the sort, repeated code or not
    bool sort_always = false;
    uint32_t rep9 = 0;                 // begin_static: bit 0 / 1 = it9f / it9r holds a repeated code (not looked for with sort_always)

    // The constructor's lengths of a walk across a gap of `dis` characters from a k-mer of initk characters (.cpp:55-58,78-79: double
    // expressions truncated to size_t)
    LRSC_WALK_FN __forceinline__ void set_lengths(int32_t dis, uint32_t initk)
    {
        if(dis > 100) maxIndelSize = (uint64_t)(dis * 0.2); else maxIndelSize = 20;
        maxLength = (uint64_t)((1.2 * (dis + 10)) + (double)(2 * (uint64_t)initk));
        minLength = (uint64_t)((0.8 * (dis - 20)) + (double)(2 * (uint64_t)initk));
    }

    // ---- the interval "trees" of the constructor (.cpp:127-152; PacBio/IntervalTree.cpp:18): per strand, the valid idmer entries of
    //      m_query sorted by interval start with std::sort, here as chains of equal-code entries through 256 hash buckets --------
    // build9: compact (emplace_back order), then chain; the step-for-step introsort runs only for a list in which some code occurs
    // twice among the valid entries.  Why any order is exact for the others:
    //  1. The consumer filters by code.  seed_support_core is the only reader of it9f / it9r: it walks one bucket's chain, skips
    //     every entry whose pad differs from the leaf's code and reads val of the rest, in chain order.  All it can see of the
    //     sort is the relative order of the entries that carry the same code.
    //  2. Equal key <=> equal code.  The key is the start of the idmer's suffix-array interval (reverse(kmer) in the rbwt,
    //     revcomp(kmer) in the bwt).  Equal k-mers have the same interval; different k-mers of one length have disjoint
    //     non-empty intervals, hence different starts.  So a list without a repeated code has no two equal keys and no two
    //     entries whose relative order can be observed; a list with one keeps the exact sort.  (The check compares pad, what the
    //     consumer compares: with seedSize > 16 pad holds the last 16 characters only, different k-mers can share it, and such a
    //     list takes the sort like any other repeat.)
    //  3. Entries with kNoKey (empty interval on this strand) are compacted away before the check: a repeat among them is never
    //     chained, and a code that is valid on one strand only counts on that strand only.
    LRSC_WALK_FN __forceinline__ uint32_t compact9(SortItem* it, uint32_t n_all) const
    {
        uint32_t n = 0;
        for(uint32_t i = 0; i < n_all; ++i)
            if(it[i].key != kNoKey) { if(n != i) it[n] = it[i]; ++n; }
        return n;
    }
    // chains over it[0, n) in array order, stopping at the first entry whose code is already in its bucket: true = a code repeats
    // (the chains are unfinished then: sort9 rebuilds them)
    LRSC_WALK_FN __forceinline__ bool chain9_unique(const SortItem* it, uint32_t n, uint16_t* head, uint16_t* next) const
    {
        for(uint32_t b = 0; b < 256; ++b) head[b] = 0xFFFFu;
        for(uint32_t j = 0; j < n; ++j) {
            const uint32_t code = it[j].pad;
            const uint32_t hb = (code ^ (code >> 9)) & 255u;
            uint32_t last = 0xFFFFu;
            for(uint32_t k = head[hb]; k != 0xFFFFu; k = next[k]) {
                if(it[k].pad == code) return true;
                last = k;
            }
            next[j] = 0xFFFFu;
            if(last == 0xFFFFu) head[hb] = (uint16_t)j; else next[last] = (uint16_t)j;
        }
        return false;
    }
    // introsort, then the chains appended in sorted order: they keep the post-sort order of equal keys
    LRSC_WALK_FN static __forceinline__ void sort9(SortItem* it, uint32_t n, uint16_t* head, uint16_t* next)
    {
        introsort(it, (int64_t)n);
        for(uint32_t b = 0; b < 256; ++b) head[b] = 0xFFFFu;
        uint16_t tail[256];
        for(uint32_t j = 0; j < n; ++j) {
            const uint32_t code = it[j].pad;
            const uint32_t hb = (code ^ (code >> 9)) & 255u;
            next[j] = 0xFFFFu;
            if(head[hb] == 0xFFFFu) head[hb] = (uint16_t)j; else next[tail[hb]] = (uint16_t)j;
            tail[hb] = (uint16_t)j;
        }
    }

    // The constructor's per-walk tables that stay fixed during the walk (.cpp:90-94,127-152 after the bulk look-ups of
    // prepare_offset): the interval "trees" as k-mer chains (build9 above), the 5-mer chains, the isTerminated filter.
    // defer: a list with a repeated code is left compacted and unsorted; the returned mask names it (bit 0 it9f, bit 1 it9r) and
    // the caller runs sort9() on it (wp_begin_kernel: the sorting lanes of a launch in wavefronts of their own).  0 otherwise.
    LRSC_WALK_FN LRSC_WALK_NOINLINE uint32_t begin_static(bool defer = false)
    {
        const uint32_t n9_all = Lq >= seedSize ? Lq - seedSize + 1 : 0;
        rep9 = 0;
        uint32_t todo = 0;
        for(uint32_t s = 0; s < 2; ++s) {
            SortItem* it = s ? it9r : it9f;
            uint16_t* head = s ? head9r : head9f;
            uint16_t* next = s ? next9r : next9f;
            const uint32_t n = compact9(it, n9_all);
            if(s) n9r = n; else n9f = n;
            bool sort = sort_always;
            if(!sort) { sort = chain9_unique(it, n, head, next); if(sort) rep9 |= 1u << s; }
            if(!sort) continue;
            if(defer) todo |= 1u << s; else sort9(it, n, head, next);
        }
        for(uint32_t c = 0; c < 1024; ++c) head5[c] = 0xFFFFu;
        const uint32_t n5 = Lq >= 5 ? Lq - 5 + 1 : 0;
        for(uint32_t i = n5; i-- > 0;) {                       // prepend while walking backwards: ascending chains
            if(flags5[i] == 0) continue;
            uint32_t code = 0;
            for(uint32_t t = 0; t < 5; ++t) code = (code << 2) | q[i + t];
            next5[i] = head5[code];
            head5[code] = (uint16_t)i;
        }

        // filter for isTerminated: a leaf can only be contained in the interval of a target k-mer it ends with
        {
            tmask0 = 0; tmask1 = 0;
            const uint32_t L = minOverlap < 16 ? (uint32_t)minOverlap : 16u;
            const uint32_t trg0 = initk + path_len;
            for(uint32_t i = 0; i < n_term; ++i) {
                uint32_t code = 0;
                const uint8_t* p = q + trg0 + i + (uint32_t)minOverlap - L;
                for(uint32_t t = 0; t < L; ++t) code = (code << 2) | p[t];
                const uint32_t h = (code * 0x9E3779B1u) >> 25;
                if(h < 64) tmask0 |= 1ull << h; else tmask1 |= 1ull << (h - 64);
            }
        }
        return todo;
    }

    // --- root (initialRootNode, .cpp:108-124; leafInfo ctor, .h:156-171).  root_iv: the root k-mer's bi-interval {fwd.lo,
    //     fwd.hi, rvc.lo, rvc.hi} when a preparation pass has already searched it, nullptr to search it here ---
    LRSC_WALK_FN LRSC_WALK_NOINLINE void begin_root(const P* root_iv)
    {
        ring_free = 0xFFFFFFFEu; path_free = 0xFFFFFFFEu;
        if constexpr(BIG)
            for(uint32_t w = 0; w < bits_words(this->cap); ++w) {
                const uint32_t n = this->cap - w * 64u;
                const uint64_t m = n >= 64 ? ~0ull : (1ull << n) - 1ull;
                this->ring_bits[w] = w ? m : m & ~1ull; this->path_bits[w] = w ? m : m & ~1ull;
            }
        Leaf<P>& root = cur[0];
        root.suf_lo = 0; root.suf_hi = 0;
        for(uint32_t t = 0; t < initk; ++t) suf_push(root, q[t]);
        if(root_iv) { root.flo = root_iv[0]; root.fhi = root_iv[1]; root.rlo = root_iv[2]; root.rhi = root_iv[3]; }
        else find_suffix(root, initk);
        root.lastOverlapLen = root.currOverlapLen = root.queryOverlapLen = initk;
        currentLength = currentKmerSize = initk;
        root.lastSeedIdx = (uint64_t)initk - seedSize;
        root.totalSeeds = (uint64_t)initk - seedSize + 1;
        root.numOfErrors = 0;
        root.numRedeemSeed = 0;
        root.localErr = 0; root.globalErr = 0; root.hist_size = 1;
        root.lastSeedIdxOffset = 0;
        root.res_first = -1; root.res_second = -1;
        root.kmerFrequency = (int)(isize(root.flo, root.fhi) + isize(root.rlo, root.rhi));
        root.tailLetter = q[initk - 1];
        root.tailLetterCount = 0;
        for(uint32_t t = initk; t-- > 0;) { if(q[t] == root.tailLetter) root.tailLetterCount++; else break; }
        root.ring = 0; root.path = 0; root.parent = 0; root.ext = 0; root.alive = 1;
        root.path_len = initk;
        rings[0] = 0.0;
        for(uint32_t t = 0; t < initk; ++t) path_set(paths, t, q[t]);
        n_cur = 1; n_nxt = 0; n_results = 0;
        ended = false;
    }

    LRSC_WALK_FN LRSC_WALK_NOINLINE void begin()
    {
        const uint64_t t_run0 = __builtin_readcyclecounter();
        begin_static();
        begin_root(nullptr);
        cyc_setup += __builtin_readcyclecounter() - t_run0;
    }

    // ---------------------------------------------------------------------------------------------------------
    // Single-leaf fast path.  While the frontier is ONE leaf (most steps: 1.36 leaves per step on average) the leaf lives in
    // registers (`L`) between steps, and a step touches memory only for what the algorithm itself reads: rank blocks, k-mer table
    // entries, the query's 9-mer chains, one error-history ring slot, one path word.  Same arithmetic in the same order as the
    // general step (extendLeaves / PrunedBySeedSupport / the commit in step_body); a step that is not of the simple kind -- no
    // accepted base, more than one -- is handed to the general code BEFORE it has had any effect.
    // ---------------------------------------------------------------------------------------------------------
    LRSC_WALK_FN __forceinline__ bool can_fast() const { return !ended && !error && n_cur == 1; }
    LRSC_WALK_FN __forceinline__ void enter_fast(Leaf<P>& L, uint32_t& pw)
    {
        L = cur[0];
        pw = (L.path_len & 15u) ? paths[(uint64_t)L.path * pathw + (L.path_len >> 4)] : 0u;
    }
    LRSC_WALK_FN __forceinline__ void leave_fast(const Leaf<P>& L) { cur[0] = L; }
    // 1: step done, the frontier is still the one leaf in L;  0: extendOverlap's loop is over (L written back, finish() decides);
    // 2: not a simple step -- nothing has happened, L written back: run the general step()
    LRSC_WALK_FN __forceinline__ int step_fast(Leaf<P>& L, uint32_t& pw)
    {
        if(!(currentLength <= maxLength)) { leave_fast(L); return 0; }
        // attempToExtend's trimming never fires for one leaf unless its local error rate is >= 1 (the minimum starts at 1): general code
        if(!(L.localErr < 1.0)) { leave_fast(L); return 2; }
        const uint32_t nr0 = n_rank, nb0 = n_blk;
        // --- extendLeaves (.cpp:239-278) ---
        uint64_t ck = currentKmerSize;
        P flo = L.flo, fhi = L.fhi, rlo = L.rlo, rhi = L.rhi;
        if(ck > maxOverlap) { find_suffix_v(L.suf_lo, L.suf_hi, (uint32_t)maxOverlap, flo, fhi, rlo, rhi); ck = maxOverlap; }
        Ext ext[4];
        uint64_t tc;
        const uint32_t mask = getFMIndexExtensions_v(flo, fhi, rlo, rhi, L.tailLetterCount, L.suf_lo, ext, tc);
        if(mask == 0 || (mask & (mask - 1u)) != 0) { n_rank = nr0; n_blk = nb0; leave_fast(L); return 2; }
        const uint32_t b = (uint32_t)__builtin_ctz(mask);
        // updateLeaves: the one child (createChild + leafInfo ctor)
        L.flo = ext[b].f.lo; L.fhi = ext[b].f.hi; L.rlo = ext[b].r.lo; L.rhi = ext[b].r.hi;
        L.kmerFrequency = ext[b].freq;
        L.currOverlapLen++;
        L.queryOverlapLen++;
        if(L.tailLetter == b) L.tailLetterCount = L.tailLetterCount + 1;
        else { L.tailLetter = b; L.tailLetterCount = 1; }
        suf_push(L, b);
        L.parent = 0; L.ext = (uint8_t)b; L.alive = 1;
        currentLength++;
        ck++;
        {   // isInsufficientFreqs for one leaf: no k-mer above the threshold
            const int highfreqThreshold = PBcoverage > 60 ? (int)((uint64_t)(PBcoverage / 60) * 3) : 3;
            if(!(L.kmerFrequency > highfreqThreshold)) {
                const uint64_t LowerBound = (ck - 2) > minOverlap ? (ck - 2) : minOverlap;
                const uint64_t ReduceSize = SelectFreqsOfrange1(LowerBound, ck, L.suf_lo, L.suf_hi);
                find_suffix_v(L.suf_lo, L.suf_hi, (uint32_t)ReduceSize, L.flo, L.fhi, L.rlo, L.rhi);
                ck = ReduceSize;
            }
        }
        currentKmerSize = ck;
        // --- PrunedBySeedSupport ---
        {
            const uint64_t currSeedIdx = currentLength - seedSize;
            const uint64_t indelOffset = seedSize + maxIndelSize;
            const uint64_t smallSeedIdx = currSeedIdx <= indelOffset ? 0 : currSeedIdx - indelOffset;
            const uint64_t largeSeedIdx = (currSeedIdx + indelOffset) >= (Lq - seedSize) ? (Lq - seedSize) : currSeedIdx + indelOffset;
            prune_leaf<true>(L, rings + (uint64_t)L.ring * 100, currSeedIdx, smallSeedIdx, largeSeedIdx);
        }
        ++steps; ++leaf_steps;
        if(!L.alive) { leave_fast(L); n_cur = 0; return 0; }         // the frontier is empty: "high error"
        // --- commit: the child takes over its parent's ring and path in place ---
        rings[(uint64_t)L.ring * 100 + (L.hist_size - 1) % 100] = L.globalErr;     // GlobalErrorRateRecord.push_back
        {
            const uint32_t sh = 2 * (L.path_len & 15u);
            if(sh == 0) pw = 0;
            pw = (pw & ~(3u << sh)) | (b << sh);
            paths[(uint64_t)L.path * pathw + (L.path_len >> 4)] = pw;
            L.path_len++;
        }
        // --- isTerminated ---
        if(currentLength >= minLength) {
            bool may_hit = true;
            if(currentKmerSize >= minOverlap) {
                const uint32_t Lm = minOverlap < 16 ? (uint32_t)minOverlap : 16u;
                const uint32_t code = (uint32_t)(L.suf_lo & (Lm >= 16 ? 0xFFFFFFFFull : ((1ull << (2 * Lm)) - 1ull)));
                const uint32_t h = (code * 0x9E3779B1u) >> 25;
                may_hit = (((h < 64 ? tmask0 : tmask1) >> (h & 63u)) & 1ull) != 0;
            }
            if(may_hit) {
                leave_fast(L);
                terminated_leaf(cur[0], paths + (uint64_t)L.path * pathw, L.path_len, -1);
                if(error) return 0;
                L.res_first = cur[0].res_first; L.res_second = cur[0].res_second;
            }
        }
        return 1;
    }

    // one iteration of extendOverlap's loop (.cpp:155-211); false when the loop is over (or on an internal error)
    LRSC_WALK_FN bool step()
    {
        if(ended || error || !(n_cur != 0 && n_cur <= maxLeaves && currentLength <= maxLength)) return false;
        leaf_steps += n_cur;
        if(n_cur > max_front) max_front = n_cur;
        if(profile) {                                    // two s_memtime round trips per step are not free: only when asked for
            const uint64_t t_step0 = __builtin_readcyclecounter();
            step_body();
            cyc_loop += __builtin_readcyclecounter() - t_step0;
        } else
            step_body();
        return true;
    }

    LRSC_WALK_FN void step_body()
    {
        {
            uint64_t t = tick();
            LRSC_WALK_TRACE(0, n_cur, 0);
            extendLeaves();
            tock(0, t);
            if(error) return;
            LRSC_WALK_TRACE(1, n_nxt, 0);
        }
        step_after_extend();
    }

    // the step from PrunedBySeedSupport on: what follows extendLeaves (or its dealt form, wp_deal.hip) in the walk's own lane
    LRSC_WALK_FN void step_after_extend()
    {
        const uint64_t t = tick();
        PrunedBySeedSupport();
        tock(4, t);
        if(step_commit()) step_terminated();
    }

    // the step from the survivor count to the end of the commit (alive_lo / alive_hi / has_child are PrunedBySeedSupport's, or
    // deal_prune's).  false: the step is over (the frontier overflowed, or an error)
    LRSC_WALK_FN bool step_commit()
    {
        {
            uint64_t t = tick();
            uint32_t survivors = (uint32_t)(__builtin_popcountll(alive_lo) + __builtin_popcountll(alive_hi));
            if constexpr(BIG) { survivors = 0; for(uint32_t w = 0; w < bits_words(n_nxt); ++w) survivors += (uint32_t)__builtin_popcountll(this->alive_bits[w]); }
            auto is_alive = [&](uint32_t c) -> bool {
                if constexpr(BIG) return bits_get(this->alive_bits, c);
                else return ((c < 64 ? alive_lo >> c : alive_hi >> (c - 64)) & 1ull) != 0;
            };
            ++steps;
            if(survivors > maxLeaves) {
                LRSC_WALK_TRACE(10, survivors, 0);
                // the frontier overflows: the loop ends after this isTerminated, no leaf state is needed any more
                if(currentLength >= minLength)
                    for(uint32_t c = 0; c < n_nxt; ++c) {
                        if(!is_alive(c)) continue;
                        const Leaf<P>& par = cur[nxt[c].parent];
                        terminated_leaf(nxt[c], paths + (uint64_t)par.path * pathw, par.path_len, (int)nxt[c].ext);
                        if(error) return false;
                    }
                n_cur = survivors;
                ended = true;
                return false;
            }
            // materialise the survivors: the first surviving child of a parent takes over its ring and path
            // in place (SAINode::extend), further ones get copies (createChild).  A child still carries its parent's
            // ring / path ids and path length (createChild copied them), so the parent need not be read again.
            // has_child (from PrunedBySeedSupport): bit i = leaf i of cur[] has a surviving child (n_cur <= 32)
            if constexpr(BIG) { for(uint32_t i = 0; i < n_cur; ++i) if(!bits_get(this->child_bits, i)) free_leaf_slots(cur[i]); }
            else for(uint32_t i = 0; i < n_cur; ++i) if(!((has_child >> i) & 1u)) free_leaf_slots(cur[i]);
            // The survivors a group at a time.  A survivor's materialisation needs seven of its fields (a child still carries its
            // parent's ring / path ids and path length: createChild copied them), one path word, and the whole leaf only where the
            // compaction moves it.  The fields of kCommitGroup consecutive children are loaded together, then -- in child order,
            // as before -- the slots are handed out and a further child's ring and path copied, then the group's path words are
            // loaded together, and the pushes, path appends and the compaction follow in child order.  Why the loads may go ahead
            // of the stores of earlier children of the group:
            //  * fields: the compaction writes nxt[w] with w below the child it moves, never a later child's leaf;
            //  * path words: every survivor appends to a path slot of its own (the parent's for its first survivor, a fresh one
            //    for each further survivor), so no word is another survivor's;
            //  * a further child's copies read the parent's ring and path, to which the parent's in-place child -- an earlier
            //    child, possibly of the same group -- appends.  Whether that append comes before or after the copy, the copy's
            //    only slot and only two path bits that could differ are the ones the further child overwrites with its own push
            //    and its own character (see the note on the ring below; the path append changes two bits of one word).
            constexpr uint32_t G = kCommitGroup;
            uint32_t seen = 0, w = 0;
            if constexpr(BIG) bits_clear_all(this->seen_bits, n_cur);
            for(uint32_t c0 = 0; c0 < n_nxt; c0 += G) {
                bool live[G];
                uint32_t parent[G], ring[G], path[G], hist_size[G], plen[G], ext[G];
                double globalErr[G];
                bool anylive = false;
#pragma unroll
                for(uint32_t j = 0; j < G; ++j) { live[j] = c0 + j < n_nxt && is_alive(c0 + j); anylive = anylive || live[j]; }
                if(!anylive) continue;
#pragma unroll
                for(uint32_t j = 0; j < G; ++j) {                // a dead or missing child's slot reads child c0 for nothing
                    const Leaf<P>& lf = nxt[live[j] ? c0 + j : c0];
                    parent[j] = lf.parent; ring[j] = lf.ring; path[j] = lf.path; hist_size[j] = lf.hist_size; plen[j] = lf.path_len;
                    ext[j] = lf.ext; globalErr[j] = lf.globalErr;
                }
#pragma unroll
                for(uint32_t j = 0; j < G; ++j) {
                    if(!live[j]) continue;
                    bool further;
                    if constexpr(BIG) further = bits_get(this->seen_bits, parent[j]); else further = ((seen >> parent[j]) & 1u) != 0;
                    if(further) {
                        LRSC_WALK_TRACE(9, parent[j], 0);
                        // a further child of this parent: copies of the ring and of the path as they are BEFORE this step's appends
                        // (the in-place child of the parent has only written slots the copies do not read: see below)
                        const uint32_t pr = ring[j], pp = path[j];
                        if constexpr(BIG) {                                                  // survivors <= cap slots: never empty here
                            ring[j] = bits_take_lowest(this->ring_bits, this->cap);
                            path[j] = bits_take_lowest(this->path_bits, this->cap);
                        } else {
                            ring[j] = (uint32_t)__builtin_ctz(ring_free); ring_free &= ring_free - 1u;     // survivors <= 32 slots: never empty here
                            path[j] = (uint32_t)__builtin_ctz(path_free); path_free &= path_free - 1u;
                        }
                        // The ring: only the slots the lineage has pushed so far.  The parent has made hist_size - 1 pushes (its
                        // hist_size is this child's minus the push of this step), into slots 0, 1, ... in turn, wrapping at 100.
                        // computeErrorRate is the only reader of a slot: it reads (totalsize - localK) % 100 once totalsize >=
                        // localK = 100, the slot written 100 pushes earlier on the same lineage.  So a slot at or beyond the
                        // number of pushes is never read before it has been written, and need not be copied.  The count is
                        // rounded up to whole bursts (a row is 10 of them): what that copies beyond the live slots is the
                        // child's own slot -- as the parent's in-place child may or may not have written it yet -- which the
                        // push below overwrites, and slots of the never-read kind.
                        const uint32_t nlive = hist_size[j] - 1 < 100 ? hist_size[j] - 1 : 100;
                        const uint32_t nburst = (nlive * 8 + kCopyChunk16 * 16 - 1) / (kCopyChunk16 * 16);
                        burst_copy16(rings + (uint64_t)ring[j] * 100, rings + (uint64_t)pr * 100, nburst);
                        burst_copy4(paths + (uint64_t)path[j] * pathw, paths + (uint64_t)pp * pathw, (plen[j] + 16) >> 4);
                    }
                    if constexpr(BIG) bits_set(this->seen_bits, parent[j]); else seen |= 1u << parent[j];
                }
                uint32_t word[G];
#pragma unroll
                for(uint32_t j = 0; j < G; ++j) word[j] = paths[(uint64_t)path[j] * pathw + (plen[j] >> 4)];
#pragma unroll
                for(uint32_t j = 0; j < G; ++j) {
                    if(!live[j]) continue;
                    rings[(uint64_t)ring[j] * 100 + (hist_size[j] - 1) % 100] = globalErr[j];     // GlobalErrorRateRecord.push_back
                    const uint32_t sh = 2 * (plen[j] & 15u);                                     // path_set
                    paths[(uint64_t)path[j] * pathw + (plen[j] >> 4)] = (word[j] & ~(3u << sh)) | (ext[j] << sh);
                    if(w != c0 + j) leaf_move(&nxt[w], &nxt[c0 + j]);  // compaction
                    nxt[w].ring = (uint16_t)ring[j]; nxt[w].path = (uint16_t)path[j]; nxt[w].path_len = plen[j] + 1;
                    ++w;
                }
            }
            // m_leaves = newLeaves: the two leaf buffers trade places when the old `cur` region (32 or kMaxChildren slots) can take
            // the next step's children (4 per survivor); otherwise the survivors are copied down as before
            if(4u * w <= (cur == leaf_small ? small_cap() : max_children())) { Leaf<P>* t2 = cur; cur = nxt; nxt = t2; }
            else for(uint32_t i = 0; i < w; ++i) leaf_move(&cur[i], &nxt[i]);
            n_cur = w;
            tock(5, t);
        }
        return true;
    }

    // isTerminated over the new frontier, after a commit that went through
    LRSC_WALK_FN void step_terminated()
    {
        {
            const uint64_t t = tick();
            // isTerminated over the new frontier.  term_scan starts with a filter on the leaf's last characters that rules most
            // leaves out; it is a function of suf_lo and of the walk's constants alone, and terminated_leaf writes nothing but its
            // own leaf's result index, the result slots and `error`.  So the suffixes of kTermGroup leaves are loaded together and
            // a leaf the filter rules out is passed over without its own round trip; the others go through terminated_leaf in
            // leaf order, with the same stop at the first error.
            if(currentLength >= minLength)
                for(uint32_t i0 = 0; i0 < n_cur; i0 += kTermGroup) {
                    uint64_t slo[kTermGroup];
#pragma unroll
                    for(uint32_t j = 0; j < kTermGroup; ++j) slo[j] = cur[i0 + j < n_cur ? i0 + j : i0].suf_lo;
#pragma unroll
                    for(uint32_t j = 0; j < kTermGroup; ++j) {
                        const uint32_t i = i0 + j;
                        if(i >= n_cur || !term_may_hit(slo[j])) continue;
                        terminated_leaf(cur[i], paths + (uint64_t)cur[i].path * pathw, cur[i].path_len, -1);
                        if(error) return;
                    }
                }
            tock(6, t);
        }
    }

    LRSC_WALK_FN LRSC_WALK_NOINLINE int finish(uint32_t* out_len, uint32_t* out_words, uint32_t* out_match_i)
    {
        // a walk that outgrew the narrow capacity of an escalating launch goes to the wide launch (the same walk from its start)
        if(escalate && (ended || error == LRSC_WALK_ERR_RESULTS)) return LRSC_WALK_NEEDS_WIDE;
        if(error) return error;
        // --- findTheBestPath (.cpp:214-236) ---
        if(n_results > 0) {
            double minErrorRate = 1;
            int best = -1;
            for(uint32_t i = 0; i < n_results; ++i)
                if(results[i].error_rate < minErrorRate) { minErrorRate = results[i].error_rate; best = (int)i; }
            if(best < 0) return -4;
            *out_len = results[best].path_len;
            *out_match_i = results[best].match_i;
            const uint32_t* src = rpaths + (uint64_t)best * pathw;
            const uint32_t nw = (results[best].path_len + 15) >> 4;
            burst_copy4(out_words, src, nw);
            return 1;
        }
        if(n_cur == 0) return -1;                    // high error
        else if(currentLength > maxLength) return -2;   // exceed search depth
        else if(n_cur > maxLeaves) return -3;        // too much repeats
        return -4;
    }
};

// A walk of lrsc_extend_walks (walk_extend_kernel, walk_extend_wide_kernel): the index, walk ww's query, parameters and lengths, and
// the tables walk_prepare_kernel left in its workspace ws.  The leaf, ring, path and result regions are the kernel's to bind.
template <bool WIDE, bool BIG>
__device__ __forceinline__ void walk_bind_work(Walk<WIDE, BIG>& W, const FmIndexDev& fm, const uint32_t* mtab, const ExtendArgs& a,
                                               const WalkWork& ww, uint8_t* ws)
{
    using P = typename Lay<WIDE>::pos_t;
    W.sF = strand_consts<P>(fm.strand[LRSC_RBWT]);
    W.sR = strand_consts<P>(fm.strand[LRSC_BWT]);
    W.fm = &fm;
    W.mtab = mtab;
    W.q = a.codes + ww.codes_off;
    W.Lq = ww.lq; W.initk = ww.initk; W.path_len = ww.path_len; W.trg_len = ww.trg_len; W.dis = ww.dis;
    W.seedSize = a.seed_size; W.minOverlap = a.min_overlap; W.maxOverlap = ww.max_overlap; W.maxLeaves = a.max_leaves;
    W.min_SA_threshold = ww.min_sa;
    W.PBcoverage = a.pb_coverage; W.PacBioErrorRate = a.pacbio_error_rate; W.errorRate = 0.25; W.localK = 100;
    W.freqsOfKmerSize = a.freqs_of_kmer_size;
    W.set_lengths(ww.dis, ww.initk);
    W.it9f = reinterpret_cast<SortItem*>(ws + ww.o_item9f);
    W.it9r = reinterpret_cast<SortItem*>(ws + ww.o_item9r);
    W.next9f = reinterpret_cast<uint16_t*>(ws + ww.o_next9f);
    W.next9r = reinterpret_cast<uint16_t*>(ws + ww.o_next9r);
    W.head9f = reinterpret_cast<uint16_t*>(ws + ww.o_head9);
    W.head9r = W.head9f + 256;
    W.head5 = reinterpret_cast<uint16_t*>(ws + ww.o_head5);
    W.next5 = reinterpret_cast<uint16_t*>(ws + ww.o_next5);
    W.flags5 = ws + ww.o_flags5;
    W.term = reinterpret_cast<const P*>(ws + ww.o_term);
    W.n_term = ww.trg_len >= a.min_overlap ? ww.trg_len - a.min_overlap + 1 : 0;
}


} // namespace lrsc
