// saipb_device.h -- the hash-guided seed-pair merge as device code: what one object of the reference's
// SAIPBSelfCorrectTree does (PacBio/SAIPBSelfCTree.h:140-287): addHashBySingleSeed (.cpp:704-787, insertKmerToHash :891-914),
// mergeTwoSeedsUsingHash (:91-256), attempToExtendUsingHash (:977-1111), isExtensionValid (:1131-1175), getFMIndexRightExtensions
// (:1213-1253), isTerminated (:1258-1294) and the banded global alignment that picks among several results (stdaln, restated in
// host/GlobalAlign.h).  New code written from the behaviour; host/SAIPBSelfCTree.cpp is the independent second implementation.
//
// ONE SOURCE, TWO BUILDS.  saipb_run_job() is the whole job.  It is written for `nl` cooperating lanes: the kernel (saipb.hip) calls it
// with the 64 lanes of a wavefront, tests/host_saipb compiles the very same function for the host and calls it with one lane.  The
// three lane primitives at the top (barrier, any, exclusive count) are the only places that differ.  In the product the qualifier
// macro is __device__ only; nothing there can reach a host build.
//
// Mapping (a first, sound one -- DESIGN.md section 4c):
//   collect   one lane per LF-walk (<= 30 rows per strand per seed), the seeds of a job as ordered phases; a rolling 2-bit k-mer, one
//             record per character, into the job's own open-addressing table in global memory (64-bit CAS on the key, 32-bit atomic
//             adds on the position buckets);
//   tree      leaf i on lane i for the index work (refine = findInterval of the (k-1)-suffix, then the four extensions of both
//             strands from two block loads each); the hash validation of the candidates, which mutates the table in leaf order then
//             base order, and the termination test run on lane 0 over what the lanes left in the job's workspace;
//   results   result r on lane r: materialise its string from the (parent, base) path store, align it to the raw read.
//
// How the bit-exactness hazards of this algorithm are kept:
//   1 bucket count of a key: an entry stores the bucket count of the phase (seed) that created it; phases are separated by barriers,
//     inside a phase every insert agrees on it and the counts are sums, so no order is needed there;
//   2 positions: computed in 64-bit unsigned arithmetic as the reference's size_t, reinterpreted as signed, divided by 35 with C's
//     truncation, clamped into the bucket range on insert; the read side (saipb_sum_of_freq) returns 0 outside the table;
//   3 isExtensionValid: serial on one lane in leaf order then base order, so the running maximum is simply the stored value; the
//     retry with min_SA_threshold - 1 sees what the first attempt left; doubles as written, -ffp-contract=off;
//   4 invalid intervals: refine is findInterval with its per-strand early exit (table_start + walk_step, the helpers of
//     lrsc_find_kmers); an extension replaces a strand's interval only when that strand was valid; bcount for the validation uses raw
//     sizes (signed, summed, reinterpreted as unsigned);
//   5 repeat guard: the reverse-complement size is added raw under the forward interval's validity, in wrapping unsigned arithmetic;
//     30 rows per strand;
//   6 frontier: terminated leaves stay; isTerminated runs from min_length on; max_used_leaves before the swap; the length advances
//     only when a child exists; among several results the first maximal match count wins (strict >).
#pragma once
#include "rank_device.h"
#include "saipb.h"

#ifndef LRSC_SAIPB_FN
#define LRSC_SAIPB_FN __device__ __forceinline__
#endif

namespace lrsc {

// ---- lane primitives: the only code that differs between the wavefront build and the one-lane host build --------------------------
LRSC_SAIPB_FN void saipb_barrier()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();             // launched as one wavefront per block: a wave barrier that also orders the job's global memory
#endif
}
LRSC_SAIPB_FN bool saipb_any(bool f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(f) != 0ull;
#else
    return f;
#endif
}
// lanes before this one with f set; total = lanes with f set
LRSC_SAIPB_FN uint32_t saipb_excl_count(bool f, uint32_t lane, uint32_t& total)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long m = __ballot(f);
    total = (uint32_t)__popcll(m);
    return (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
#else
    (void)lane;
    total = f ? 1u : 0u;
    return 0;
#endif
}
LRSC_SAIPB_FN uint64_t saipb_cas64(uint64_t* p, uint64_t expect, uint64_t val)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expect, (unsigned long long)val);
#else
    const uint64_t old = *p;
    if(old == expect) *p = val;
    return old;
#endif
}
// Table words that atomics write are read back with relaxed atomic loads, never through a cache line that an earlier plain load left
LRSC_SAIPB_FN uint64_t saipb_ld64(const uint64_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
LRSC_SAIPB_FN uint32_t saipb_ld32(const uint32_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
LRSC_SAIPB_FN void saipb_add32(uint32_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, 1u);
#else
    *p += 1;
#endif
}

// ---- k-mers as 2-bit words -----------------------------------------------------------------------------------------------------
// key = 1 followed by the k codes (a leading 1 keeps the empty slot value 0 free)
LRSC_SAIPB_FN uint64_t saipb_key(uint64_t kmer, uint32_t k) { return (1ull << (2 * k)) | kmer; }
LRSC_SAIPB_FN uint64_t saipb_revcomp(uint64_t kmer, uint32_t k)
{
    uint64_t o = 0;
    for(uint32_t t = 0; t < k; ++t) { o = (o << 2) | (3u - (kmer & 3u)); kmer >>= 2; }
    return o;
}
LRSC_SAIPB_FN uint32_t saipb_slot0(uint64_t key, uint32_t mask)
{
    key ^= key >> 33; key *= 0xff51afd7ed558ccdull; key ^= key >> 33; key *= 0xc4ceb9fe1a85ec53ull; key ^= key >> 33;
    return (uint32_t)key & mask;
}

template <bool WIDE>
struct SaipbCtx {
    using P = typename Lay<WIDE>::pos_t;
    StrandC<P> sF, sR;                 // RBWT (forward intervals), BWT (reverse-complement intervals)
    const FmIndexDev* fm;
    const uint32_t* mtab;
    const uint8_t* codes;
};

// findBiInterval with findInterval's early exit per strand (BWTAlgorithms.cpp:28): what lrsc_find_kmers computes
template <bool WIDE, class Get>
LRSC_SAIPB_FN void saipb_find(const SaipbCtx<WIDE>& c, Get get, uint32_t k, uint64_t& flo, uint64_t& fhi, uint64_t& rlo, uint64_t& rhi)
{
    using P = typename Lay<WIDE>::pos_t;
    WalkState<P> st = walk_init<P>();
    table_start<WIDE>(*c.fm, get, k, st);
    for(uint32_t s = st.size; s < k; ++s) {
        if(st.fwd_broken && st.rvc_broken) break;
        st = walk_step<WIDE>(c.sF, c.sR, get(s), k, st, c.mtab);
    }
    flo = st.fwd.lo; fhi = st.fwd.hi; rlo = st.rvc.lo; rhi = st.rvc.hi;
}

// addHashBySingleSeed up to its repeat guard (:704-726)
template <bool WIDE>
LRSC_SAIPB_FN SaipbSeedInfo saipb_seed_info(const SaipbCtx<WIDE>& c, const SaipbSeed& sd)
{
    SaipbSeedInfo si;
    const uint8_t* w = c.codes + sd.off + (sd.len - sd.large_kmer);
    saipb_find<WIDE>(c, [&](uint32_t t) -> uint32_t { return w[t]; }, sd.large_kmer, si.flo, si.fhi, si.rlo, si.rhi);
    uint64_t f = 0;
    if(si.flo <= si.fhi) {
        f += si.fhi - si.flo + 1;
        f += (uint64_t)((int64_t)si.rhi - (int64_t)si.rlo + 1);      // sic (:720): raw size, guarded by the forward interval
    }
    si.freq = f;
    return si;
}

// one LF step on a strand: the character of the row, and the row it maps to; false on a '$' row
template <bool WIDE>
LRSC_SAIPB_FN bool saipb_lf(const StrandC<typename Lay<WIDE>::pos_t>& s, const uint32_t* mtab, uint64_t& row, uint32_t& code)
{
    using L = Lay<WIDE>;
    using P = typename L::pos_t;
    const P idx = (P)row;
    const P b = idx / L::kSyms;
    const uint32_t off = (uint32_t)(idx - b * L::kSyms);
    typename L::Regs r;
    L::load(s.blocks, b, r);
    code = L::symbol(r, off);
    const bool flagged = L::flagged(r);
    if(code == 0 && flagged && dollars_in_c(s, (uint64_t)idx, (uint64_t)idx + 1) != 0) return false;
    uint64_t cnt = L::count(r, code, mtab + off * L::kRow);
    if(code == 0 && off != 0 && flagged) cnt -= dollars_in_c(s, (uint64_t)b * L::kSyms, (uint64_t)b * L::kSyms + off);
    row = (uint64_t)(pred_of(s, code) + (P)cnt);
    return true;
}

struct SaipbHash {
    uint64_t* keys;
    SaipbMeta* meta;
    double* maxavg;
    uint32_t* pool;
    uint32_t mask, pool_cap;
};
LRSC_SAIPB_FN int64_t saipb_lookup(const SaipbHash& h, uint64_t key)
{
    uint32_t s = saipb_slot0(key, h.mask);
    for(uint32_t n = 0; n <= h.mask; ++n, s = (s + 1) & h.mask) {
        const uint64_t k = saipb_ld64(&h.keys[s]);
        if(k == key) return (int64_t)s;
        if(k == 0) return -1;
    }
    return -1;
}
// KmerFeatures::getSumOfFreq: the bucket of the position and its two neighbours, 0 outside the table
LRSC_SAIPB_FN uint64_t saipb_sum_of_freq(const SaipbHash& h, int64_t slot, int64_t pos)
{
    if(slot < 0) return 0;
    const SaipbMeta m = h.meta[slot];
    const int64_t index = pos / (int64_t)kSaipbBucket;
    if(index < 0 || index >= (int64_t)m.nb) return 0;
    const uint32_t* f = h.pool + m.off;
    uint64_t s = saipb_ld32(f + index);
    if(index > 0) s += saipb_ld32(f + index - 1);
    if(index < (int64_t)m.nb - 1) s += saipb_ld32(f + index + 1);
    return s;
}

// ---- the banded global alignment (host/GlobalAlign.h restated without the back-pointer matrix) ----------------------------------
// Every layer of every cell carries the match and column counts of the path its back pointer would lead along (t = matches << 16 |
// columns), so the corner holds what the trace-back would count: a real score's predecessor is always a real score, the blanked
// band edges (kInf) are never on the path.  a: the raw read (columns), b: the candidate (rows); codes 0..3, no N.
LRSC_SAIPB_FN void saipb_diag(SaipbCell& c, const SaipbCell& p, int s, bool same)
{
    int from;
    if(p.m >= p.i) from = p.m >= p.d ? 0 : 2; else from = p.i > p.d ? 1 : 2;
    c.m = (from == 0 ? p.m : from == 1 ? p.i : p.d) + s;
    c.tm = (from == 0 ? p.tm : from == 1 ? p.ti : p.td) + 1u + (same ? 0x10000u : 0u);
}
LRSC_SAIPB_FN void saipb_above(SaipbCell& c, const SaipbCell& p, int e)
{
    const bool opens = p.m - 1 > p.i;
    c.i = opens ? p.m - 1 - e : p.i - e;
    c.ti = (opens ? p.tm : p.ti) + 1u;
}
LRSC_SAIPB_FN void saipb_left(SaipbCell& c, const SaipbCell& p, int e)
{
    const bool opens = p.m - 1 > p.d;
    c.d = opens ? p.m - 1 - e : p.d - e;
    c.td = (opens ? p.tm : p.td) + 1u;
}
LRSC_SAIPB_FN void saipb_blank(SaipbCell& c) { c.m = c.i = c.d = -1073741823; c.tm = c.ti = c.td = 0; }

LRSC_SAIPB_FN void saipb_global_align(const uint8_t* a, int n1, const uint8_t* b, int n2, SaipbCell* r0, SaipbCell* r1,
                                                           int& matches, int& score, int& columns)
{
    matches = score = columns = 0;
    if(n1 == 0 || n2 == 0) return;
    const int ext = 1, endExt = 0, band = 50;
    int w1 = n1 > n2 ? n1 - n2 + band : band, w2 = n1 > n2 ? band : n2 - n1 + band;
    if(w1 > n1) w1 = n1;
    if(w2 > n2) w2 = n2;
    for(int i = 0; i <= n1; ++i) { r0[i].m = r0[i].i = r0[i].d = 0; r0[i].tm = r0[i].ti = r0[i].td = 0; r1[i] = r0[i]; }
    SaipbCell* cur = r0;
    SaipbCell* prev = r1;
    // x[i] = a[i - 1], y[j] = b[j - 1]
#define SAIPB_SUB(j, i) (b[(j) - 1] == a[(i) - 1] ? 1 : -8)
#define SAIPB_SAME(j, i) (b[(j) - 1] == a[(i) - 1])
#define SAIPB_FLIP() { SaipbCell* t_ = cur; cur = prev; prev = t_; }
    saipb_blank(cur[0]); cur[0].m = 0;
    for(int i = 1; i < w1; ++i) { saipb_blank(cur[i]); saipb_left(cur[i], cur[i - 1], endExt); }
    SAIPB_FLIP();
    int j = 1;
    const int anchored = w2 < n2 ? w2 : n2 - 1;
    // rows whose band starts at column 0; `last` = the candidate's last row (free end gaps)
    for(int pass = 0; pass < 2; ++pass) {
        const bool last = pass == 1;
        if(last && !(j == n2 && w2 != n2 - 1)) break;
        for(; last ? j == n2 : j <= anchored; ++j) {
            saipb_blank(cur[0]);
            saipb_above(cur[0], prev[0], endExt);
            const int stop = (j + w1 <= n1 + 1) ? (j + w1 - 1) : n1;
            int i = 1;
            for(; i != stop; ++i) {
                saipb_diag(cur[i], prev[i - 1], SAIPB_SUB(j, i), SAIPB_SAME(j, i));
                saipb_above(cur[i], prev[i], ext);
                saipb_left(cur[i], cur[i - 1], last ? endExt : ext);
            }
            saipb_diag(cur[i], prev[i - 1], SAIPB_SUB(j, i), SAIPB_SAME(j, i));
            saipb_left(cur[i], cur[i - 1], last ? endExt : ext);
            if(j + w1 - 1 > n1) saipb_above(cur[i], prev[i], endExt); else cur[i].i = -1073741823;
            SAIPB_FLIP();
        }
    }
    for(; j <= n2 - w2 + 1; ++j) {                                              // both band edges inside the row
        saipb_blank(cur[j - w2]);
        const int stop = j + w1 - 1;
        int i = j - w2 + 1;
        for(; i != stop; ++i) {
            saipb_diag(cur[i], prev[i - 1], SAIPB_SUB(j, i), SAIPB_SAME(j, i));
            saipb_above(cur[i], prev[i], ext);
            saipb_left(cur[i], cur[i - 1], ext);
        }
        saipb_diag(cur[i], prev[i - 1], SAIPB_SUB(j, i), SAIPB_SAME(j, i));
        saipb_left(cur[i], cur[i - 1], ext);
        cur[i].i = -1073741823;
        SAIPB_FLIP();
    }
    for(; j <= n2; ++j) {                                                       // the band ends at the last column
        const bool last = j == n2;
        saipb_blank(cur[j - w2]);
        int i = j - w2 + 1;
        for(; i < n1; ++i) {
            saipb_diag(cur[i], prev[i - 1], SAIPB_SUB(j, i), SAIPB_SAME(j, i));
            saipb_above(cur[i], prev[i], ext);
            saipb_left(cur[i], cur[i - 1], last ? endExt : ext);
        }
        saipb_diag(cur[i], prev[n1 - 1], SAIPB_SUB(j, i), SAIPB_SAME(j, i));
        saipb_above(cur[i], prev[i], endExt);
        saipb_left(cur[i], cur[i - 1], last ? endExt : ext);
        SAIPB_FLIP();
    }
#undef SAIPB_SUB
#undef SAIPB_SAME
#undef SAIPB_FLIP
    const SaipbCell& corner = prev[n1];
    int best = corner.m;
    uint32_t t = corner.tm;
    if(corner.i > best) { best = corner.i; t = corner.ti; }
    if(corner.d > best) { best = corner.d; t = corner.td; }
    score = best;
    matches = (int)(t >> 16);
    columns = (int)(t & 0xFFFFu);
}

// ---- one job ---------------------------------------------------------------------------------------------------------------
// info: the job's seeds' SaipbSeedInfo (index seed_first + s); ws: the chunk's workspace; out: the chunk's output (ASCII).
template <bool WIDE>
LRSC_SAIPB_FN void saipb_run_job(const SaipbCtx<WIDE>& c, const SaipbJob& job, const SaipbSeed* seeds, const SaipbSeedInfo* info, uint8_t* ws,
                                 char* out, SaipbOut& result, uint32_t lane, uint32_t nl)
{
    using P = typename Lay<WIDE>::pos_t;
    const SaipbLayout lay = saipb_layout(job);
    uint8_t* base = ws + job.ws_off;
    SaipbHash h;
    h.keys = reinterpret_cast<uint64_t*>(base + lay.keys);
    h.meta = reinterpret_cast<SaipbMeta*>(base + lay.meta);
    h.maxavg = reinterpret_cast<double*>(base + lay.maxavg);
    h.pool = reinterpret_cast<uint32_t*>(base + lay.pool);
    h.mask = job.hash_slots - 1;
    h.pool_cap = job.pool_words;
    uint32_t* nodes = reinterpret_cast<uint32_t*>(base + lay.nodes);
    SaipbLeaf* cur = reinterpret_cast<SaipbLeaf*>(base + lay.leaves);
    SaipbLeaf* nxt = cur + kSaipbFrontier;
    SaipbCand* cands = reinterpret_cast<SaipbCand*>(base + lay.cands);
    SaipbRes* res = reinterpret_cast<SaipbRes*>(base + lay.res);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(base + lay.ctl);       // [0] children, [1] results, [2] status, [3] matches' winner
    const uint32_t k = job.hash_kmer;
    const uint64_t kmask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1ull);
    const uint64_t stem_mask = (1ull << (2 * (k - 1))) - 1ull;

    for(uint32_t i = lane; i < job.hash_slots; i += nl) h.keys[i] = 0;
    if(lane == 0) { ctl[0] = 0; ctl[1] = 0; ctl[2] = LRSC_SAIPB_OK; ctl[3] = 0; }
    saipb_barrier();

    // ---- collect: the seeds as ordered phases (hazard 1) -----------------------------------------------------------------------
    uint32_t pool_used = 0, entries = 0, status = LRSC_SAIPB_OK;       // uniform over the lanes
    for(uint32_t s = 0; s < job.n_seeds; ++s) {
        const SaipbSeed sd = seeds[job.seed_first + s];
        const SaipbSeedInfo si = info[job.seed_first + s];
        if(sd.skip_repeat && si.freq > 128) continue;
        const uint32_t nf = si.flo <= si.fhi ? (uint32_t)((si.fhi - si.flo + 1 < kSaipbMaxRows) ? si.fhi - si.flo + 1 : kSaipbMaxRows) : 0u;
        const uint32_t nr = si.rlo <= si.rhi ? (uint32_t)((si.rhi - si.rlo + 1 < kSaipbMaxRows) ? si.rhi - si.rlo + 1 : kSaipbMaxRows) : 0u;
        const uint32_t nb = sd.max_length / kSaipbBucket + 1;
        uint64_t tail = 0;                                          // the seed's last k bases
        for(uint32_t t = 0; t < k; ++t) tail = (tail << 2) | c.codes[sd.off + sd.len - k + t];
        for(uint32_t w0 = 0; w0 < nf + nr; w0 += nl) {
            const uint32_t w = w0 + lane;
            bool active = w < nf + nr;
            const bool fwd = w < nf;                                // RBWT: the read onwards; BWT: the other strand's read backwards
            uint64_t row = fwd ? si.flo + w : si.rlo + (w - nf);
            uint64_t kmer = fwd ? tail : saipb_revcomp(tail, k);
            uint64_t len = sd.len;                                  // currentLength of the record about to be inserted
            while(saipb_any(active)) {
                int64_t slot = -1;
                bool isnew = false;
                if(active) {
                    const uint64_t key = saipb_key(kmer, k);
                    uint32_t sl = saipb_slot0(key, h.mask);
                    for(uint32_t n = 0; n <= h.mask; ++n, sl = (sl + 1) & h.mask) {
                        uint64_t old = saipb_ld64(&h.keys[sl]);
                        if(old == 0) { old = saipb_cas64(&h.keys[sl], 0, key); if(old == 0) { isnew = true; slot = sl; break; } }
                        if(old == key) { slot = sl; break; }
                    }
                }
                uint32_t total;
                const uint32_t before = saipb_excl_count(isnew, lane, total);
                if(isnew) {
                    const uint64_t off = (uint64_t)pool_used + (uint64_t)before * nb;
                    if(off + nb <= h.pool_cap) {
                        for(uint32_t t = 0; t < nb; ++t) h.pool[off + t] = 0;
                        h.meta[slot].off = (uint32_t)off; h.meta[slot].nb = nb;
                    } else { h.meta[slot].off = 0; h.meta[slot].nb = 0; }
                    h.maxavg[slot] = 0.0;
                }
                if((uint64_t)pool_used + (uint64_t)total * nb > h.pool_cap) status = LRSC_SAIPB_INTERNAL;     // the planner's bound makes this unreachable
                else pool_used += total * nb;
                entries += total;
                saipb_barrier();
                if(active && slot < 0) status = LRSC_SAIPB_INTERNAL;
                if(active && slot >= 0 && h.meta[slot].nb != 0) {
                    // insertKmerToHash's position (:891-914), size_t arithmetic as written (hazard 2)
                    const uint64_t upos = sd.expected_length < 0 ? len - (uint64_t)sd.len : (uint64_t)(int64_t)sd.expected_length - len + (uint64_t)k;
                    const SaipbMeta m = h.meta[slot];
                    int64_t index = (int64_t)upos / (int64_t)kSaipbBucket;
                    if(index < 0) index = 0; else if(index > (int64_t)m.nb - 1) index = (int64_t)m.nb - 1;
                    saipb_add32(&h.pool[m.off + index]);
                }
                if(active) {
                    uint32_t code = 0;
                    if(len + 1 > sd.max_length) active = false;
                    else if(!saipb_lf<WIDE>(fwd ? c.sF : c.sR, c.mtab, row, code)) active = false;
                    else {
                        kmer = fwd ? (((kmer << 2) | code) & kmask) : (((uint64_t)code << (2 * (k - 1))) | (kmer >> 2));
                        ++len;
                    }
                }
            }
        }
        saipb_barrier();
    }
    status = saipb_any(status != LRSC_SAIPB_OK) ? LRSC_SAIPB_INTERNAL : LRSC_SAIPB_OK;

    // ---- the tree --------------------------------------------------------------------------------------------------------------
    uint64_t tflo, tfhi, trlo, trhi;                                // initializeTerminalIntervals (:75-88)
    {
        const uint8_t* d = c.codes + job.dest_off;
        saipb_find<WIDE>(c, [&](uint32_t t) -> uint32_t { return d[t]; }, k, tflo, tfhi, trlo, trhi);
    }
    if(lane == 0) {
        SaipbLeaf root;
        root.stem = 0;
        for(uint32_t t = 0; t + 1 < k; ++t) root.stem = (root.stem << 2) | c.codes[job.src_off + job.src_len - (k - 1) + t];
        root.flo = root.rlo = 1; root.fhi = root.rhi = 0; root.count = 0; root.node = 0; root.pad = 0;
        cur[0] = root;
        nodes[0] = 0;
    }
    saipb_barrier();
    uint32_t n = 1, steps = 0, max_used = 0, n_nodes = 1, n_res = 0;      // n_nodes, n_res: lane 0's
    int32_t cur_len = (int32_t)job.src_len;
    const int32_t seed_len = (int32_t)job.src_len;
    while(status == LRSC_SAIPB_OK && n > 0 && n <= job.max_leaves && (uint64_t)cur_len <= (uint64_t)job.max_length) {
        ++steps;
        // refineSAInterval + getFMIndexRightExtensions, leaf i on lane i (hazard 4)
        for(uint32_t i = lane; i < n; i += nl) {
            SaipbLeaf lf = cur[i];
            const uint64_t stem = lf.stem;
            saipb_find<WIDE>(c, [&](uint32_t t) -> uint32_t { return (uint32_t)(stem >> (2 * (k - 2 - t))) & 3u; }, k - 1, lf.flo, lf.fhi, lf.rlo, lf.rhi);
            cur[i] = lf;
            const bool vf = lf.flo <= lf.fhi, vr = lf.rlo <= lf.rhi;
            IvT<P> of[4], orv[4];
            uint32_t nblk = 0;
            if(vf) { IvT<P> iv; iv.lo = (P)lf.flo; iv.hi = (P)lf.fhi; update_interval_all<WIDE, true>(c.sF, iv, c.mtab, of, nblk); }
            if(vr) { IvT<P> iv; iv.lo = (P)lf.rlo; iv.hi = (P)lf.rhi; update_interval_all<WIDE, true>(c.sR, iv, c.mtab, orv, nblk); }
            for(uint32_t b = 0; b < 4; ++b) {
                SaipbCand cd;
                cd.flo = vf ? (uint64_t)of[b].lo : lf.flo; cd.fhi = vf ? (uint64_t)of[b].hi : lf.fhi;
                cd.rlo = vr ? (uint64_t)orv[3 - b].lo : lf.rlo; cd.rhi = vr ? (uint64_t)orv[3 - b].hi : lf.rhi;
                uint64_t bcount = 0;
                if(cd.flo <= cd.fhi) bcount += cd.fhi - cd.flo + 1;
                if(cd.rlo <= cd.rhi) bcount += cd.rhi - cd.rlo + 1;
                cd.ok = bcount >= 2 ? 1u : 0u;
                cd.pad = 0;
                cands[i * 4 + b] = cd;
            }
        }
        saipb_barrier();
        // attempToExtendUsingHash, its retry, and isTerminated: serial, leaf order then base order (hazards 3 and 6)
        if(lane == 0) {
            uint32_t nn = 0, st = LRSC_SAIPB_OK;
            for(uint32_t attempt = 0; attempt < 2 && nn == 0; ++attempt) {
                const uint64_t thr = (uint64_t)job.min_sa - attempt;            // size_t arithmetic: 0 - 1 wraps, as m_min_SA_threshold-- does
                for(uint32_t i = 0; i < n; ++i) {
                    const SaipbLeaf lf = cur[i];
                    const double currAvgFreq = (double)lf.count / (cur_len + 1000000);
                    for(uint32_t b = 0; b < 4; ++b) {
                        const SaipbCand cd = cands[i * 4 + b];
                        if(!cd.ok) continue;
                        const uint64_t bcount = (uint64_t)(((int64_t)cd.fhi - (int64_t)cd.flo + 1) + ((int64_t)cd.rhi - (int64_t)cd.rlo + 1));   // raw sizes (:1022,:1061)
                        const uint64_t kmer = (lf.stem << 2) | b;
                        const int64_t s1 = saipb_lookup(h, saipb_key(kmer, k));
                        if(s1 >= 0 && n > 8 && currAvgFreq < h.maxavg[s1]) continue;             // bubble removal once the frontier is wide
                        if(s1 >= 0 && currAvgFreq > h.maxavg[s1]) h.maxavg[s1] = currAvgFreq;
                        const int64_t s2 = saipb_lookup(h, saipb_key(saipb_revcomp(kmer, k), k));
                        const int64_t here = (int64_t)(cur_len - seed_len);
                        const uint64_t kf = saipb_sum_of_freq(h, s1, here) + saipb_sum_of_freq(h, s2, here);
                        if(!(kf >= thr || (bcount >= 7 && kf >= 1))) continue;
                        if(nn >= kSaipbFrontier || n_nodes >= job.node_cap) { st = LRSC_SAIPB_PATH_LIMIT; continue; }
                        SaipbLeaf ch;
                        ch.stem = kmer & stem_mask;
                        ch.flo = cd.flo; ch.fhi = cd.fhi; ch.rlo = cd.rlo; ch.rhi = cd.rhi;
                        ch.count = lf.count + kf;
                        ch.node = n_nodes; ch.pad = 0;
                        nodes[n_nodes++] = (lf.node << 2) | b;
                        nxt[nn++] = ch;
                    }
                }
            }
            const int32_t new_len = cur_len + (nn ? 1 : 0);
            if((uint64_t)new_len >= (uint64_t)job.min_length)
                for(uint32_t i = 0; i < nn; ++i) {
                    const SaipbLeaf& lf = nxt[i];
                    const bool f = lf.flo <= lf.fhi && lf.flo >= tflo && lf.fhi <= tfhi;
                    const bool r = lf.rlo <= lf.rhi && lf.rlo >= trlo && lf.rhi <= trhi;
                    if(!(f || r)) continue;
                    if(n_res >= kSaipbMaxResults) { st = LRSC_SAIPB_RESULT_LIMIT; continue; }
                    res[n_res].count = lf.count; res[n_res].node = lf.node; res[n_res].len = (uint32_t)new_len;
                    ++n_res;
                }
            ctl[0] = nn; ctl[1] = n_res; ctl[2] = st;
        }
        saipb_barrier();
        const uint32_t nn = ctl[0];
        status = ctl[2];
        if(n > max_used) max_used = n;
        if(nn) ++cur_len;
        SaipbLeaf* t = cur; cur = nxt; nxt = t;
        n = nn;
        saipb_barrier();                                            // ctl is rewritten in the next step
    }
    n_res = ctl[1];

    // ---- result choice -----------------------------------------------------------------------------------------------------------
    result.steps = steps; result.max_used_leaves = max_used; result.n_results = n_res; result.hash_entries = entries;
    result.out_len = 0; result.pad = 0; result.status = status; result.code = 0;
    if(status != LRSC_SAIPB_OK) return;                                  // never an approximated number: no code, no sequence
    if(n_res == 0) {
        const int32_t half = (int32_t)(job.expected_length - (uint32_t)seed_len) / 2 + seed_len;
        int32_t code = -5;
        if(n == 0 && cur_len >= half) code = -1;
        else if((uint64_t)cur_len > (uint64_t)job.max_length) code = -2;
        else if(n > job.max_leaves) code = -3;
        else if(n == 0 && cur_len < half) code = -4;
        result.code = code;
        return;
    }
    result.code = 1;
    const uint32_t tail_len = job.dest_len > k ? job.dest_len - k : 0;
    uint8_t* strs = base + lay.str;
    SaipbCell* rows = reinterpret_cast<SaipbCell*>(base + lay.rows);
    int32_t* match = reinterpret_cast<int32_t*>(cands);             // the candidates' space is free once the tree has ended
    for(uint32_t r = lane; r < n_res; r += nl) {
        // the result's string: src, then the path from the root, then dest beyond its first k bases
        uint8_t* sp = strs + (uint64_t)r * job.str_cap;
        const SaipbRes rr = res[r];
        for(uint32_t t = 0; t < job.src_len; ++t) sp[t] = c.codes[job.src_off + t];
        uint32_t node = rr.node;
        for(uint32_t t = rr.len; t > job.src_len; --t) { const uint32_t v = nodes[node]; sp[t - 1] = (uint8_t)(v & 3u); node = v >> 2; }
        for(uint32_t t = 0; t < tail_len; ++t) sp[rr.len + t] = c.codes[job.dest_off + k + t];
        int m = 0, sc = 0, col = 0;
        if(n_res > 1)
            saipb_global_align(c.codes + job.raw_off, (int)job.raw_len, sp, (int)(rr.len + tail_len),
                               rows + (uint64_t)r * 2 * (job.raw_len + 1), rows + (uint64_t)r * 2 * (job.raw_len + 1) + (job.raw_len + 1), m, sc, col);
        match[r] = m;
    }
    saipb_barrier();
    uint32_t win = 0;
    bool have = false;
    if(n_res > 1) {
        double maxMatchPercent = -100;
        for(uint32_t r = 0; r < n_res; ++r) {
            const double matchPercent = (double)match[r] / job.raw_len;
            if(maxMatchPercent < matchPercent) { maxMatchPercent = matchPercent; win = r; have = true; }
        }
    } else {
        // one result: the length / coverage rule against the initial minLengthDiff = 100000, maxKmerCoverage = 0
        const int32_t total = (int32_t)(res[0].len + tail_len);
        int32_t diff = total - (int32_t)job.expected_length; if(diff < 0) diff = -diff;
        int32_t dd = diff - 100000; if(dd < 0) dd = -dd;
        const double avgCov = (double)res[0].count / (total + 1000000);
        have = (diff < 100000 && dd > 3) || (dd <= 3 && 0.0 < avgCov);
    }
    if(have) {
        const uint32_t total = res[win].len + tail_len;
        const uint8_t* sp = strs + (uint64_t)win * job.str_cap;
        for(uint32_t t = lane; t < total; t += nl) out[job.out_off + t] = "ACGT"[sp[t] & 3u];
        result.out_len = total;
    }
}

} // namespace lrsc
