// wp_wave.hip -- wp_extend_wave_kernel: the one-walk-per-wavefront extension launches (lane_stride 64) with the walk's frontier spread
// over the wavefront.
//
// wp_extend_kernel at stride 64 runs a walk on lane 0 while 63 lanes wait.  Here the single-leaf fast step (Walk::step_fast) still runs
// on lane 0, but the general step runs leaf i of the frontier on lane i and child c of the next frontier on lane c & 63 (two rounds
// above 64 children): refine, getFMIndexExtensions with its per-leaf min_SA_threshold retry, SelectFreqsOfrange's searches,
// PrunedBySeedSupport, isTerminated's scan, and the ring / path copies of a copied child (by the whole wavefront).  What crosses leaves
// -- the error-rate minimum, the trim, the order of the children, the frequency maxima, the slot hand-out, the result slots -- goes
// through ballots, shuffles and prefix counts, so that every decision, every value and every rank-query counter is the one of the
// serial step (walk_device.h: the per-leaf pieces are the same member functions).
//
// The walk's scalars (currentLength, n_cur, ring_free, ...) sit in every lane's Walk object with the same value: every lane runs the
// same cross-leaf code on them.  After a fast-step segment (lane 0 only) the ones it changed are broadcast from lane 0.  Leaves live
// in the wavefront's workspace (wp_lane_layout) as in the serial kernel; a phase that reads what another lane wrote starts after
// wave_sync().  Rank queries are counted per lane and summed over the wavefront (flush_counters).
#define LRSC_WALK_FN __device__ __forceinline__
#define LRSC_WALK_NOINLINE
#include <hip/hip_runtime.h>

#include "walk_device.h"
#include "wp.h"
#include "wp_walk.h"

namespace lrsc {

#ifndef LRSC_WP_EXTEND_OCC
#define LRSC_WP_EXTEND_OCC 2          // wavefronts per SIMD, as wp_extend_kernel (capi_core.cpp sizes the launches for that)
#endif

namespace {

// ---- wavefront helpers of this kernel (the shared ones are in wp_walk.h; call them with the whole wavefront active) -------------
__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
    for(int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
    return first_u32(v);
}
// the k-th lowest set bit of m (k = 0: the lowest): the slot that k rounds of `ctz, clear` leave at the front
__device__ __forceinline__ uint32_t kth_bit(uint32_t m, uint32_t k)
{
    for(uint32_t j = 0; j < k; ++j) m &= m - 1u;
    return m ? (uint32_t)__builtin_ctz(m) : 0u;          // (survivors <= maxLeaves <= 32 slots: never empty)
}

// ---- SelectFreqsOfrange (.cpp:281-331): leaf j on lane j & 63, a wavefront maximum per k-mer size -------------------------
template <bool WIDE>
__device__ __forceinline__ uint64_t wave_select(Walk<WIDE>& W, uint64_t LowerBound, uint64_t UpperBound, const Leaf<typename Lay<WIDE>::pos_t>* leaves,
                                                uint32_t n, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint32_t U = (uint32_t)UpperBound, Lw = (uint32_t)LowerBound;
    const bool h0 = lane < n, h1 = lane + 64 < n;
    uint64_t s0lo = 0, s0hi = 0, s1lo = 0, s1hi = 0;
    if(h0) { s0lo = leaves[lane].suf_lo; s0hi = leaves[lane].suf_hi; }
    if(h1) { s1lo = leaves[lane + 64].suf_lo; s1hi = leaves[lane + 64].suf_hi; }
    IvT<P> f0{}, r0{}, f1{}, r1{};
    int mx = 0;                                          // tempmaxfmfreqs starts at 0
    if(h0) { W.select_first(s0lo, s0hi, U, Lw, f0, r0); const int fr = (int)(isize(f0.lo, f0.hi) + isize(r0.lo, r0.hi)); mx = fr > mx ? fr : mx; }
    if(h1) { W.select_first(s1lo, s1hi, U, Lw, f1, r1); const int fr = (int)(isize(f1.lo, f1.hi) + isize(r1.lo, r1.hi)); mx = fr > mx ? fr : mx; }
    mx = wave_max(mx);
    if(mx - (int)W.freqsOfKmerSize[LowerBound] < 5) return LowerBound;
    for(uint64_t i = 1; i <= UpperBound - LowerBound; i++) {
        const uint32_t t = (uint32_t)(UpperBound - LowerBound - i);
        mx = 0;
        if(h0) { W.select_next(s0lo, s0hi, U, t, f0, r0); const int fr = (int)(isize(f0.lo, f0.hi) + isize(r0.lo, r0.hi)); mx = fr > mx ? fr : mx; }
        if(h1) { W.select_next(s1lo, s1hi, U, t, f1, r1); const int fr = (int)(isize(f1.lo, f1.hi) + isize(r1.lo, r1.hi)); mx = fr > mx ? fr : mx; }
        mx = wave_max(mx);
        if(mx - (int)W.freqsOfKmerSize[LowerBound + i] < 5) return LowerBound + i;
    }
    return UpperBound;
}

// ---- attempToExtend (.cpp:373-465) + updateLeaves (:468-488): leaf i on lane i (n_cur <= maxLeaves <= 32) ----------------
template <bool WIDE>
__device__ __forceinline__ void wave_attempt(Walk<WIDE>& W, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint32_t n = W.n_cur;
    const bool have = lane < n;
    Leaf<P> par = {};
    if(have) par = W.cur[lane];
    // minimumErrorRate starts at 1 and takes every smaller localErr
    const double minimumErrorRate = wave_min(have && par.localErr < 1.0 ? par.localErr : 1.0);
    // trim leaves whose error rate relative to the best one is high; the survivors keep their order
    bool keep = false;
    if(have) {
        const double errorRateDiff = par.localErr - minimumErrorRate;
        keep = !((errorRateDiff > 0.05 && W.currentLength > W.localK / 2) || (errorRateDiff > 0.1 && W.currentLength > 15));
    }
    W.ring_free |= wave_or(have && !keep ? 1u << par.ring : 0u);
    W.path_free |= wave_or(have && !keep ? 1u << par.path : 0u);
    const uint64_t below = lanes_below(lane);
    const uint64_t km = __ballot(keep);
    const uint32_t pos = popc64(km & below);
    const uint32_t n_kept = popc64(km);
    if(keep && pos != lane) W.cur[pos] = par;             // every lane has read its leaf: the compaction overwrites nothing unread
    W.n_cur = n_kept;

    // the extensions of each kept leaf; the threshold retry acts on this lane's copy of min_SA_threshold
    const uint32_t nr0 = W.n_rank, nb0 = W.n_blk;
    typename Walk<WIDE>::Ext ext[4];
    uint32_t mask = 0;
    if(keep) {
        int count = 0;
        while(count < 2) {
            if(count == 1 && !(par.localErr == minimumErrorRate && n_kept > 1)) break;
            uint64_t tc;
            mask = W.getFMIndexExtensions_v(par.flo, par.fhi, par.rlo, par.rhi, par.tailLetterCount, par.suf_lo, ext, tc);
            if(mask != 0) break;
            W.min_SA_threshold--;
            count++;
        }
        W.min_SA_threshold += (uint64_t)count;
    }
    // children in (parent, base) order: exclusive prefix of the accepted bases
    uint32_t off = 0, total = 0;
#pragma unroll
    for(uint32_t b = 0; b < 4; ++b) {
        const uint64_t m = __ballot(((mask >> b) & 1u) != 0);
        off += popc64(m & below);
        total += popc64(m);
    }
    // the serial loop stops at the child that would overflow nxt[]: a leaf after that one never ran its extensions
    if(off > kMaxChildren) { W.n_rank = nr0; W.n_blk = nb0; }
    if(total > kMaxChildren) { W.error = LRSC_WALK_ERR_CHILDREN; return; }
    const int highfreqThreshold = W.PBcoverage > 60 ? (int)((uint64_t)(W.PBcoverage / 60) * 3) : 3;
    uint32_t hf = 0, k = off;
#pragma unroll
    for(uint32_t b = 0; b < 4; ++b) {
        if(!((mask >> b) & 1u)) continue;
        const Leaf<P> ch = W.make_child(par, pos, b, ext[b]);
        if(ch.kmerFrequency > highfreqThreshold) ++hf;
        W.nxt[k++] = ch;
    }
    W.n_highfreq = wave_sum(hf);
    W.n_nxt = total;
    wave_sync();
}

// ---- extendLeaves (.cpp:239-278) ------------------------------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ void wave_extend(Walk<WIDE>& W, uint32_t lane)
{
    W.n_nxt = 0;
    uint64_t t = W.tick();
    if(W.currentKmerSize > W.maxOverlap) { wave_refine(W, W.cur, W.n_cur, W.maxOverlap, lane); wave_sync(); }
    W.tock(1, t);
    t = W.tick();
    wave_attempt(W, lane);
    W.tock(2, t);
    if(W.error) return;
    if(W.n_nxt == 0) {                                    // level 1: reduce the k-mer size
        const uint64_t LowerBound = (W.currentKmerSize - 2) > W.minOverlap ? (W.currentKmerSize - 2) : W.minOverlap;
        const uint64_t ReduceSize = wave_select(W, LowerBound, W.currentKmerSize, W.cur, W.n_cur, lane);
        wave_refine(W, W.cur, W.n_cur, ReduceSize, lane);
        wave_sync();
        wave_attempt(W, lane);
        if(W.error) return;
        if(W.n_nxt == 0) {                                // level 2: reduce the threshold
            W.min_SA_threshold--;
            wave_attempt(W, lane);
            W.min_SA_threshold++;
            if(W.error) return;
        }
    }
    if(W.n_nxt != 0) {
        W.currentLength++;
        W.currentKmerSize++;
        if(W.isInsufficientFreqs(W.n_highfreq, W.n_nxt)) {   // frequencies are low: relax the k-mer size
            const uint64_t LowerBound = (W.currentKmerSize - 2) > W.minOverlap ? (W.currentKmerSize - 2) : W.minOverlap;
            const uint64_t ReduceSize = wave_select(W, LowerBound, W.currentKmerSize, W.nxt, W.n_nxt, lane);
            wave_refine(W, W.nxt, W.n_nxt, ReduceSize, lane);
        }
    }
}

// ---- PrunedBySeedSupport (.cpp:491-563): child c on lane c & 63; the children stay in registers for the commit -------------
template <bool WIDE>
__device__ __forceinline__ void wave_prune(Walk<WIDE>& W, uint32_t lane, Leaf<typename Lay<WIDE>::pos_t>& c0, Leaf<typename Lay<WIDE>::pos_t>& c1)
{
    const uint64_t currSeedIdx = W.currentLength - W.seedSize;
    const uint64_t indelOffset = W.seedSize + W.maxIndelSize;
    const uint64_t smallSeedIdx = currSeedIdx <= indelOffset ? 0 : currSeedIdx - indelOffset;
    const uint64_t largeSeedIdx = (currSeedIdx + indelOffset) >= (W.Lq - W.seedSize) ? (W.Lq - W.seedSize) : currSeedIdx + indelOffset;
    const uint32_t n = W.n_nxt;
    bool a0 = false, a1 = false;
    uint32_t hc = 0;
    // a child still carries its parent's ring id: the parent's error history, which no commit has touched yet
    if(lane < n) {
        c0 = W.nxt[lane];
        W.template prune_leaf<true>(c0, W.rings + (uint64_t)c0.ring * 100, currSeedIdx, smallSeedIdx, largeSeedIdx);
        W.nxt[lane] = c0;
        a0 = c0.alive != 0;
        if(a0) hc |= 1u << c0.parent;
    }
    if(lane + 64 < n) {
        c1 = W.nxt[lane + 64];
        W.template prune_leaf<true>(c1, W.rings + (uint64_t)c1.ring * 100, currSeedIdx, smallSeedIdx, largeSeedIdx);
        W.nxt[lane + 64] = c1;
        a1 = c1.alive != 0;
        if(a1) hc |= 1u << c1.parent;
    }
    W.alive_lo = __ballot(a0);
    W.alive_hi = __ballot(a1);
    W.has_child = wave_or(hc);
}

// ---- the commit of step_body (walk_device.h) and isTerminated (.cpp:825-878) ------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ void wave_commit(Walk<WIDE>& W, uint32_t lane, Leaf<typename Lay<WIDE>::pos_t>& c0, Leaf<typename Lay<WIDE>::pos_t>& c1)
{
    using P = typename Lay<WIDE>::pos_t;
    uint64_t t = W.tick();
    const uint64_t am0 = W.alive_lo, am1 = W.alive_hi;
    const uint32_t survivors = popc64(am0) + popc64(am1);
    ++W.steps;
    if(survivors > W.maxLeaves) {
        // the frontier overflows: the loop ends after this isTerminated (children in order, on lane 0 as in the serial step)
        wave_sync();
        if(lane == 0 && W.currentLength >= W.minLength)
            for(uint32_t c = 0; c < W.n_nxt; ++c) {
                if((((c < 64 ? am0 >> c : am1 >> (c - 64)) & 1ull)) == 0) continue;
                const Leaf<P>& par = W.cur[W.nxt[c].parent];
                W.terminated_leaf(W.nxt[c], W.paths + (uint64_t)par.path * W.pathw, par.path_len, (int)W.nxt[c].ext);
                if(W.error) break;
            }
        W.n_results = first_u32(W.n_results);
        W.error = (int)first_u32((uint32_t)W.error);
        W.n_cur = survivors;
        W.ended = true;
        return;
    }
    const uint64_t below = lanes_below(lane);
    // 1. the parents without a surviving child give their slots back
    uint32_t fr = 0, fp = 0;
    if(lane < W.n_cur && !((W.has_child >> lane) & 1u)) { fr = 1u << W.cur[lane].ring; fp = 1u << W.cur[lane].path; }
    W.ring_free |= wave_or(fr);
    W.path_free |= wave_or(fp);
    // 2. the first surviving child of a parent takes over its slots; a further one is a child whose previous surviving child (the
    //    children are in parent order) has the same parent
    const bool a0 = ((am0 >> lane) & 1ull) != 0, a1 = ((am1 >> lane) & 1ull) != 0;
    const uint32_t p0 = c0.parent, p1 = c1.parent;
    const uint64_t m0 = am0 & below, m1 = am1 & below;
    const uint32_t prev0 = (uint32_t)__shfl((int)p0, m0 ? 63 - __builtin_clzll(m0) : (int)lane, 64);
    const uint32_t prev1 = (uint32_t)__shfl((int)p1, m1 ? 63 - __builtin_clzll(m1) : (int)lane, 64);
    const uint32_t last0 = am0 ? lane_u32(p0, 63u - (uint32_t)__builtin_clzll(am0)) : 0xFFFFFFFFu;
    const bool fur0 = a0 && m0 != 0 && prev0 == p0;
    const bool fur1 = a1 && (m1 != 0 ? prev1 == p1 : last0 == p1);
    // 3. the k-th further child in child order takes the k-th lowest free slot
    const uint64_t f0 = __ballot(fur0), f1 = __ballot(fur1);
    const uint32_t n_further = popc64(f0) + popc64(f1);
    uint32_t r0 = c0.ring, q0 = c0.path, r1 = c1.ring, q1 = c1.path;
    if(fur0) { const uint32_t k = popc64(f0 & below); r0 = kth_bit(W.ring_free, k); q0 = kth_bit(W.path_free, k); }
    if(fur1) { const uint32_t k = popc64(f0) + popc64(f1 & below); r1 = kth_bit(W.ring_free, k); q1 = kth_bit(W.path_free, k); }
    for(uint32_t j = 0; j < n_further; ++j) { W.ring_free &= W.ring_free - 1u; W.path_free &= W.path_free - 1u; }
    // 4. copies for the further children (all but the own ring entry: it is written with the copy), then the in-place children's
    //    GlobalErrorRateRecord.push_back and path character
    wave_copy_slots(W, f0, c0, r0, q0, lane);
    wave_copy_slots(W, f1, c1, r1, q1, lane);
    if(a0 && !fur0) {
        W.rings[(uint64_t)c0.ring * 100 + (c0.hist_size - 1) % 100] = c0.globalErr;
        path_set(W.paths + (uint64_t)c0.path * W.pathw, c0.path_len, c0.ext);
    }
    if(a1 && !fur1) {
        W.rings[(uint64_t)c1.ring * 100 + (c1.hist_size - 1) % 100] = c1.globalErr;
        path_set(W.paths + (uint64_t)c1.path * W.pathw, c1.path_len, c1.ext);
    }
    c0.ring = (uint16_t)r0; c0.path = (uint16_t)q0; c0.path_len++;
    c1.ring = (uint16_t)r1; c1.path = (uint16_t)q1; c1.path_len++;
    W.tock(5, t);
    t = W.tick();
    // isTerminated over the new frontier in leaf order: the scans side by side, result slots by a prefix count of the leaves that
    // need a new one
    int hit0 = -1, hit1 = -1;
    uint64_t h0 = 0, h1 = 0;
    if(W.currentLength >= W.minLength) {
        if(a0) hit0 = W.term_scan(c0);
        if(a1) hit1 = W.term_scan(c1);
        const bool need0 = hit0 >= 0 && c0.res_first == -1, need1 = hit1 >= 0 && c1.res_first == -1;
        const uint64_t n0 = __ballot(need0), n1 = __ballot(need1);
        bool bad = false;
        if(need0) { const uint32_t k = W.n_results + popc64(n0 & below); if(k >= kMaxResults) bad = true; else c0.res_first = (int)k + 1; }
        if(need1) { const uint32_t k = W.n_results + popc64(n0) + popc64(n1 & below); if(k >= kMaxResults) bad = true; else c1.res_first = (int)k + 1; }
        if(hit0 >= 0) c0.res_second = hit0;
        if(hit1 >= 0) c1.res_second = hit1;
        if(__ballot(bad)) W.error = LRSC_WALK_ERR_RESULTS;
        W.n_results += popc64(n0) + popc64(n1);
        h0 = __ballot(hit0 >= 0);
        h1 = __ballot(hit1 >= 0);
    }
    // 5. m_leaves = newLeaves (compaction in child order), into the buffer the serial swap rule leaves as `cur`
    const bool swap = 4u * survivors <= (W.cur == W.leaf_small ? 32u : kMaxChildren);
    Leaf<P>* dest = swap ? W.nxt : W.cur;
    if(a0) dest[popc64(m0)] = c0;
    if(a1) dest[popc64(am0) + popc64(m1)] = c1;
    if(swap) { Leaf<P>* t2 = W.cur; W.cur = W.nxt; W.nxt = t2; }
    W.n_cur = survivors;
    wave_sync();
    if(!W.error && (h0 | h1)) {
        wave_store_results(W, h0, c0, hit0, lane);
        wave_store_results(W, h1, c1, hit1, lane);
        wave_sync();
    }
    W.tock(6, t);
}

// ---- one iteration of extendOverlap's loop (Walk::step) ---------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ bool wave_step(Walk<WIDE>& W, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    if(W.ended || W.error || !(W.n_cur != 0 && W.n_cur <= W.maxLeaves && W.currentLength <= W.maxLength)) return false;
    W.leaf_steps += W.n_cur;
    if(W.n_cur > W.max_front) W.max_front = W.n_cur;
    wave_sync();
    uint64_t t = W.tick();
    wave_extend(W, lane);
    W.tock(0, t);
    if(W.error) return true;
    t = W.tick();
    Leaf<P> c0 = {}, c1 = {};
    wave_prune(W, lane, c0, c1);
    W.tock(4, t);
    wave_commit(W, lane, c0, c1);
    return true;
}

} // namespace

// ---------------------------------------------------------------------------------------
// one walk per wavefront over a queue of walks (the same queue, workspace and results as wp_extend_kernel at stride 64)
// ---------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(64, LRSC_WP_EXTEND_OCC) void wp_extend_wave_kernel(FmIndexDev fm, WpArgs a)
{
    using P = typename Lay<WIDE>::pos_t;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTabSize<WIDE>::value];
    init_mask_table<WIDE>(mtab);
    const uint32_t lane = threadIdx.x;
    const uint32_t wave = blockIdx.x;
    Walk<WIDE> W;
    wp_walk_consts(W, fm, a, mtab);
    const WpLaneLayout LL = wp_lane_layout(a.lbytes, a.lane_pathw);
    uint8_t* lws = a.lane_ws + (uint64_t)(wave < a.n_lanes ? wave : 0u) * a.lane_ws_bytes;
    Leaf<P>* const leaf_base = reinterpret_cast<Leaf<P>*>(lws + LL.leaves);
    W.rings = reinterpret_cast<double*>(lws + LL.rings);
    W.results = reinterpret_cast<WalkResultRec*>(lws + LL.results);
    W.paths = reinterpret_cast<uint32_t*>(lws + LL.paths);
    W.pathw = a.lane_pathw;
    W.rpaths = W.paths + (uint64_t)32 * a.lane_pathw;

    Leaf<P> L;                                            // lane 0: the single-leaf fast path's leaf in registers
    uint32_t pw = 0;
    // profiling (a.prof): wall ticks of the wavefront in the step's regions (Walk::tock slots 0-6, 7 = fast steps), 8 = refill,
    // 9 = finish, 10 = whole loop; lane 0 reports them
    uint64_t pr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t_refill = 0, t_finish = 0, n_fast = 0;
    const bool prof = a.prof != nullptr;
    if(prof) W.prof = pr;
    const uint64_t t_loop0 = prof ? __builtin_readcyclecounter() : 0;
    if(wave < a.n_lanes)
    while(true) {
        const uint64_t tr0 = prof ? __builtin_readcyclecounter() : 0;
        uint32_t i = 0;
        if(lane == 0) i = atomicAdd(a.queue, 1u);
        i = first_u32(i);
        if(i >= a.n_list) break;
        if(a.reqs && a.reqs[i].kind != kWpReqFm) continue;
        const uint32_t si = a.list ? a.list[i] : (uint32_t)a.slot_base + i;
        if(a.slots[si].flags & kWpGeomBad) continue;
        W.cur = leaf_base; W.nxt = leaf_base + 32; W.leaf_small = leaf_base;
        wp_walk_bind(W, a, a.slots[si]);                  // every lane: the same values into the same words
        const uint64_t steps0 = W.steps;
        if(prof) t_refill += __builtin_readcyclecounter() - tr0;
        while(true) {
            int r = 2;
            if(W.can_fast()) r = wave_fast_steps(W, L, pw, lane, prof, pr[7], n_fast);
            if(r == 2) r = wave_step(W, lane) ? 1 : 0;
            if(r == 0) break;
        }
        const uint64_t tf0 = prof ? __builtin_readcyclecounter() : 0;
        wave_sync();
        if(lane == 0) wp_walk_finish(W, a, si, steps0);
        if(prof) t_finish += __builtin_readcyclecounter() - tf0;
    }
    if(prof && wave < a.n_lanes && lane == 0) {
        for(int j = 0; j < 8; ++j) atomicAdd(&a.prof[j], (unsigned long long)pr[j]);
        atomicAdd(&a.prof[8], (unsigned long long)t_refill);
        atomicAdd(&a.prof[9], (unsigned long long)t_finish);
        atomicAdd(&a.prof[10], (unsigned long long)(__builtin_readcyclecounter() - t_loop0));
        atomicAdd(&a.prof[11], (unsigned long long)W.steps);
        atomicAdd(&a.prof[12], (unsigned long long)n_fast);
    }
    flush_counters(a.ctr, W.n_rank, W.n_blk);
}

hipError_t launch_wp_extend_wave(const FmIndexDev& fm, const WpArgs& a, hipStream_t stream)
{
    if(a.n_list == 0 || a.n_lanes == 0) return hipSuccess;
    // n_lanes = walks in flight = wavefronts (lane_stride 64)
    if(fm.wide) hipLaunchKernelGGL(wp_extend_wave_kernel<true>, dim3(a.n_lanes), dim3(64), 0, stream, fm, a);
    else        hipLaunchKernelGGL(wp_extend_wave_kernel<false>, dim3(a.n_lanes), dim3(64), 0, stream, fm, a);
    return hipGetLastError();
}

hipError_t wp_extend_wave_static_lds(bool wide, uint32_t* bytes)
{
    hipFuncAttributes fa{};
    const void* f = wide ? reinterpret_cast<const void*>(wp_extend_wave_kernel<true>) : reinterpret_cast<const void*>(wp_extend_wave_kernel<false>);
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if(e == hipSuccess) *bytes = (uint32_t)fa.sharedSizeBytes;
    return e;
}

} // namespace lrsc
