// wp_wide.hip -- wp_extend_wide_kernel: the walks of -l above 32 (Walk<WIDE, true>), one walk per wavefront with the frontier spread over
// the lanes.
//
// With -l L > 32 every walk first runs in the narrow launches with a cap of 32 leaves.  A walk whose frontier outgrows that cap (or
// its 160 result slots) ends there with LRSC_WALK_NEEDS_WIDE and runs again here from its start with room for L leaves, 4 L
// children and 5 L result slots.  The step generalises wp_wave.hip's: leaf j of the frontier on lane j & 63 and child c on lane
// c & 63, in ceil(n / 64) rounds.  What crosses leaves -- the error-rate minimum, the trim, the order of the children, the frequency
// maxima, the ring / path / result slot hand-out -- carries from round to round in the serial order through ballots and prefix
// counts, so that every decision and value is the one of the serial step (walk_device.h: the per-leaf pieces are the same member
// functions).  The single-leaf fast step stays on lane 0.
//
// Leaves, rings, paths and results live in the wavefront's workspace (wp_wide_layout); the slot bitsets (ring / path free, children
// alive, parents with a surviving child) in LDS.  The walk's scalars sit in every lane's Walk object with the same value; after a
// fast-step segment the ones it changed are broadcast from lane 0.  A phase that reads what another lane wrote starts after wave_sync().
#define LRSC_WALK_FN __device__ __forceinline__
#define LRSC_WALK_NOINLINE
#include <hip/hip_runtime.h>

#include "walk_device.h"
#include "wp.h"
#include "wp_walk.h"

namespace lrsc {

#ifndef LRSC_WP_WIDE_OCC
#define LRSC_WP_WIDE_OCC 2            // wavefronts per SIMD, as the other extension kernels
#endif

namespace {

constexpr uint32_t kBitsLeaf = kWideMaxLeaves / 64, kBitsChild = 4 * kWideMaxLeaves / 64;

// ---- bitsets of this kernel (the wavefront helpers are in wp_walk.h) -----------------------------------------------------------
// the k-th lowest set bit of the bitset (k = 0: the lowest), n bits; wave-uniform words
__device__ __forceinline__ uint32_t bits_kth(const uint64_t* b, uint32_t n, uint32_t k)
{
    for(uint32_t w = 0; w < bits_words(n); ++w) {
        uint64_t m = b[w];
        const uint32_t pc = popc64(m);
        if(k < pc) {
            for(uint32_t j = 0; j < k; ++j) m &= m - 1ull;
            return w * 64u + (uint32_t)__builtin_ctzll(m);
        }
        k -= pc;
    }
    return 0;                                            // (survivors <= cap slots: never reached)
}
// clear the lowest `k` set bits (by lane 0; the caller syncs)
__device__ __forceinline__ void bits_take(uint64_t* b, uint32_t n, uint32_t k)
{
    for(uint32_t w = 0; w < bits_words(n) && k; ++w) {
        uint64_t m = b[w];
        while(m && k) { m &= m - 1ull; --k; }
        b[w] = m;
    }
}

template <bool WIDE> using WWalk = Walk<WIDE, true>;
template <bool WIDE> using WLeaf = Leaf<typename Lay<WIDE>::pos_t>;

// ---- SelectFreqsOfrange (.cpp:281-331): leaf j on lane j & 63 (its intervals in the leaf's tf* fields), a wavefront maximum per size
template <bool WIDE>
__device__ __forceinline__ uint64_t wide_select(WWalk<WIDE>& W, uint64_t LowerBound, uint64_t UpperBound, WLeaf<WIDE>* leaves, uint32_t n, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint32_t U = (uint32_t)UpperBound, Lw = (uint32_t)LowerBound;
    int mx = 0;                                          // tempmaxfmfreqs starts at 0
    for(uint32_t j = lane; j < n; j += 64) {
        WLeaf<WIDE>& lf = leaves[j];
        IvT<P> f, r;
        W.select_first(lf.suf_lo, lf.suf_hi, U, Lw, f, r);
        lf.tflo = f.lo; lf.tfhi = f.hi; lf.trlo = r.lo; lf.trhi = r.hi;
        const int fr = (int)(isize(f.lo, f.hi) + isize(r.lo, r.hi));
        mx = fr > mx ? fr : mx;
    }
    mx = wave_max(mx);
    if(mx - (int)W.freqsOfKmerSize[LowerBound] < 5) return LowerBound;
    for(uint64_t i = 1; i <= UpperBound - LowerBound; i++) {
        const uint32_t t = (uint32_t)(UpperBound - LowerBound - i);
        mx = 0;
        for(uint32_t j = lane; j < n; j += 64) {
            WLeaf<WIDE>& lf = leaves[j];
            IvT<P> f{lf.tflo, lf.tfhi}, r{lf.trlo, lf.trhi};
            W.select_next(lf.suf_lo, lf.suf_hi, U, t, f, r);
            lf.tflo = f.lo; lf.tfhi = f.hi; lf.trlo = r.lo; lf.trhi = r.hi;
            const int fr = (int)(isize(f.lo, f.hi) + isize(r.lo, r.hi));
            mx = fr > mx ? fr : mx;
        }
        mx = wave_max(mx);
        if(mx - (int)W.freqsOfKmerSize[LowerBound + i] < 5) return LowerBound + i;
    }
    return UpperBound;
}

// ---- attempToExtend (.cpp:373-465) + updateLeaves (:468-488) ------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ void wide_attempt(WWalk<WIDE>& W, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint64_t below = lanes_below(lane);
    const uint32_t n = W.n_cur;
    // minimumErrorRate starts at 1 and takes every smaller localErr
    double mn = 1.0;
    for(uint32_t j = lane; j < n; j += 64) { const double e = W.cur[j].localErr; mn = e < mn ? e : mn; }
    const double minimumErrorRate = wave_min(mn);
    // trim leaves whose error rate relative to the best one is high; the survivors keep their order (a round writes below what
    // later rounds read), the trimmed give their slots back
    uint32_t n_kept = 0;
    for(uint32_t r0 = 0; r0 < n; r0 += 64) {
        const uint32_t j = r0 + lane;
        const bool have = j < n;
        Leaf<P> par = {};
        bool keep = false;
        if(have) {
            par = W.cur[j];
            const double errorRateDiff = par.localErr - minimumErrorRate;
            keep = !((errorRateDiff > 0.05 && W.currentLength > W.localK / 2) || (errorRateDiff > 0.1 && W.currentLength > 15));
            if(!keep) {
                atomicOr((unsigned long long*)&W.ring_bits[par.ring >> 6], 1ull << (par.ring & 63u));
                atomicOr((unsigned long long*)&W.path_bits[par.path >> 6], 1ull << (par.path & 63u));
            }
        }
        const uint64_t km = __ballot(keep);
        const uint32_t pos = n_kept + popc64(km & below);
        if(keep && pos != j) W.cur[pos] = par;
        n_kept += popc64(km);
    }
    W.n_cur = n_kept;
    wave_sync();

    // the extensions of each kept leaf, children in (parent, base) order; the threshold retry acts on this lane's copy of
    // min_SA_threshold.  n_kept <= cap: the children always fit (4 cap)
    const int highfreqThreshold = W.PBcoverage > 60 ? (int)((uint64_t)(W.PBcoverage / 60) * 3) : 3;
    uint32_t n_ch = 0, hf = 0;
    for(uint32_t r0 = 0; r0 < n_kept; r0 += 64) {
        const uint32_t j = r0 + lane;
        const bool have = j < n_kept;
        Leaf<P> par = {};
        typename WWalk<WIDE>::Ext ext[4];
        uint32_t mask = 0;
        if(have) {
            par = W.cur[j];
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
        uint32_t off = n_ch, total = 0;
#pragma unroll
        for(uint32_t b = 0; b < 4; ++b) {
            const uint64_t m = __ballot(((mask >> b) & 1u) != 0);
            off += popc64(m & below);
            total += popc64(m);
        }
#pragma unroll
        for(uint32_t b = 0; b < 4; ++b) {
            if(!((mask >> b) & 1u)) continue;
            const Leaf<P> ch = W.make_child(par, j, b, ext[b]);
            if(ch.kmerFrequency > highfreqThreshold) ++hf;
            W.nxt[off++] = ch;
        }
        n_ch += total;
    }
    W.n_highfreq = wave_sum(hf);
    W.n_nxt = n_ch;
    wave_sync();
}

// ---- extendLeaves (.cpp:239-278) ------------------------------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ void wide_extend(WWalk<WIDE>& W, uint32_t lane)
{
    W.n_nxt = 0;
    if(W.currentKmerSize > W.maxOverlap) { wave_refine(W, W.cur, W.n_cur, W.maxOverlap, lane); wave_sync(); }
    wide_attempt(W, lane);
    if(W.n_nxt == 0) {                                    // level 1: reduce the k-mer size
        const uint64_t LowerBound = (W.currentKmerSize - 2) > W.minOverlap ? (W.currentKmerSize - 2) : W.minOverlap;
        const uint64_t ReduceSize = wide_select(W, LowerBound, W.currentKmerSize, W.cur, W.n_cur, lane);
        wave_refine(W, W.cur, W.n_cur, ReduceSize, lane);
        wave_sync();
        wide_attempt(W, lane);
        if(W.n_nxt == 0) {                                // level 2: reduce the threshold
            W.min_SA_threshold--;
            wide_attempt(W, lane);
            W.min_SA_threshold++;
        }
    }
    if(W.n_nxt != 0) {
        W.currentLength++;
        W.currentKmerSize++;
        if(W.isInsufficientFreqs(W.n_highfreq, W.n_nxt)) {   // frequencies are low: relax the k-mer size
            const uint64_t LowerBound = (W.currentKmerSize - 2) > W.minOverlap ? (W.currentKmerSize - 2) : W.minOverlap;
            const uint64_t ReduceSize = wide_select(W, LowerBound, W.currentKmerSize, W.nxt, W.n_nxt, lane);
            wave_refine(W, W.nxt, W.n_nxt, ReduceSize, lane);
        }
    }
    wave_sync();
}

// ---- PrunedBySeedSupport (.cpp:491-563): child c on lane c & 63; alive bits per round, parents with a surviving child ----------
template <bool WIDE>
__device__ __forceinline__ void wide_prune(WWalk<WIDE>& W, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint64_t currSeedIdx = W.currentLength - W.seedSize;
    const uint64_t indelOffset = W.seedSize + W.maxIndelSize;
    const uint64_t smallSeedIdx = currSeedIdx <= indelOffset ? 0 : currSeedIdx - indelOffset;
    const uint64_t largeSeedIdx = (currSeedIdx + indelOffset) >= (W.Lq - W.seedSize) ? (W.Lq - W.seedSize) : currSeedIdx + indelOffset;
    const uint32_t n = W.n_nxt;
    if(lane < bits_words(W.n_cur)) W.child_bits[lane] = 0;
    wave_sync();
    // a child still carries its parent's ring id: the parent's error history, which no commit has touched yet
    for(uint32_t r0 = 0; r0 < n; r0 += 64) {
        const uint32_t c = r0 + lane;
        bool a = false;
        if(c < n) {
            Leaf<P> ch = W.nxt[c];
            W.template prune_leaf<true>(ch, W.rings + (uint64_t)ch.ring * 100, currSeedIdx, smallSeedIdx, largeSeedIdx);
            W.nxt[c] = ch;
            a = ch.alive != 0;
            if(a) atomicOr((unsigned long long*)&W.child_bits[ch.parent >> 6], 1ull << (ch.parent & 63u));
        }
        const uint64_t m = __ballot(a);
        if(lane == 0) W.alive_bits[r0 >> 6] = m;
    }
    wave_sync();
}

// ---- the commit of step_body (walk_device.h) and isTerminated (.cpp:825-878) ------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ void wide_commit(WWalk<WIDE>& W, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint64_t below = lanes_below(lane);
    const uint32_t n = W.n_nxt, nw = bits_words(n);
    uint32_t survivors = 0;
    for(uint32_t w = 0; w < nw; ++w) survivors += popc64(W.alive_bits[w]);
    ++W.steps;
    if(survivors > W.maxLeaves) {
        // the frontier overflows: the loop ends after this isTerminated (children in order, on lane 0 as in the serial step)
        if(lane == 0 && W.currentLength >= W.minLength)
            for(uint32_t c = 0; c < n; ++c) {
                if(!bits_get(W.alive_bits, c)) continue;
                const Leaf<P>& par = W.cur[W.nxt[c].parent];
                W.terminated_leaf(W.nxt[c], W.paths + (uint64_t)par.path * W.pathw, par.path_len, (int)W.nxt[c].ext);
                if(W.error) break;
            }
        W.n_results = first_u32(W.n_results);
        W.error = (int)first_u32((uint32_t)W.error);
        W.n_cur = survivors;
        W.ended = true;
        wave_sync();
        return;
    }
    // 1. the parents without a surviving child give their slots back
    for(uint32_t j = lane; j < W.n_cur; j += 64)
        if(!bits_get(W.child_bits, j)) {
            const Leaf<P>& par = W.cur[j];
            atomicOr((unsigned long long*)&W.ring_bits[par.ring >> 6], 1ull << (par.ring & 63u));
            atomicOr((unsigned long long*)&W.path_bits[par.path >> 6], 1ull << (par.path & 63u));
        }
    wave_sync();
    // 2.-4. round by round in child order: a further child (its previous surviving child has the same parent) takes the k-th lowest
    //       free slot for the k-th further child of the step and copies its parent's ring and path; the first child of a parent
    //       appends to them in place.  5. m_leaves = newLeaves: compaction in child order into the buffer the serial swap rule
    //       leaves as `cur` (a round writes below what later rounds read)
    const bool swap = 4u * survivors <= (W.cur == W.leaf_small ? W.small_cap() : W.max_children());
    Leaf<P>* dest = swap ? W.nxt : W.cur;
    uint32_t last_parent = 0xFFFFFFFFu, n_further = 0, n_alive = 0;
    for(uint32_t r0 = 0; r0 < n; r0 += 64) {
        const uint32_t c = r0 + lane;
        const uint64_t am = W.alive_bits[r0 >> 6];
        const bool a = ((am >> lane) & 1ull) != 0;
        Leaf<P> ch = {};
        if(a) ch = W.nxt[c];
        const uint32_t p = ch.parent;
        const uint64_t m = am & below;
        const uint32_t prev = (uint32_t)__shfl((int)p, m ? 63 - __builtin_clzll(m) : (int)lane, 64);
        const bool fur = a && (m != 0 ? prev == p : last_parent == p);
        if(am) last_parent = lane_u32(p, 63u - (uint32_t)__builtin_clzll(am));
        const uint64_t fm = __ballot(fur);
        uint32_t rr = ch.ring, pp = ch.path;
        if(fur) {
            const uint32_t k = n_further + popc64(fm & below);
            rr = bits_kth(W.ring_bits, W.cap, k);
            pp = bits_kth(W.path_bits, W.cap, k);
        }
        n_further += popc64(fm);
        wave_copy_slots(W, fm, ch, rr, pp, lane);
        if(a && !fur) {
            W.rings[(uint64_t)ch.ring * 100 + (ch.hist_size - 1) % 100] = ch.globalErr;
            path_set(W.paths + (uint64_t)ch.path * W.pathw, ch.path_len, ch.ext);
        }
        ch.ring = (uint16_t)rr; ch.path = (uint16_t)pp; ch.path_len++;
        if(a) dest[n_alive + popc64(m)] = ch;
        n_alive += popc64(am);
    }
    // the slots handed out are the n_further lowest free ones
    wave_sync();
    if(lane == 0) { bits_take(W.ring_bits, W.cap, n_further); bits_take(W.path_bits, W.cap, n_further); }
    if(swap) { Leaf<P>* t2 = W.cur; W.cur = W.nxt; W.nxt = t2; }
    W.n_cur = survivors;
    wave_sync();
    // isTerminated over the new frontier in leaf order: the scans side by side, result slots by a prefix count of the leaves that
    // need a new one
    if(W.currentLength >= W.minLength) {
        for(uint32_t r0 = 0; r0 < survivors; r0 += 64) {
            const uint32_t j = r0 + lane;
            const bool have = j < survivors;
            Leaf<P> lf = {};
            int hit = -1;
            if(have) { lf = W.cur[j]; hit = W.term_scan(lf); }
            const bool need = hit >= 0 && lf.res_first == -1;
            const uint64_t nm = __ballot(need);
            bool bad = false;
            if(need) { const uint32_t k = W.n_results + popc64(nm & below); if(k >= W.max_results()) bad = true; else lf.res_first = (int)k + 1; }
            if(hit >= 0) { lf.res_second = hit; W.cur[j] = lf; }
            if(__ballot(bad)) W.error = LRSC_WALK_ERR_RESULTS;
            W.n_results += popc64(nm);
            if(W.error) break;
            const uint64_t hm = __ballot(hit >= 0);
            if(hm) { wave_store_results(W, hm, lf, hit, lane); }
        }
        wave_sync();
    }
}

// ---- one iteration of extendOverlap's loop (Walk::step) ---------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ bool wide_step(WWalk<WIDE>& W, uint32_t lane)
{
    if(W.ended || W.error || !(W.n_cur != 0 && W.n_cur <= W.maxLeaves && W.currentLength <= W.maxLength)) return false;
    W.leaf_steps += W.n_cur;
    if(W.n_cur > W.max_front) W.max_front = W.n_cur;
    wave_sync();
    wide_extend(W, lane);
    wide_prune(W, lane);
    wide_commit(W, lane);
    return true;
}

// the extendOverlap loop of a bound walk (begin_root done by every lane): the single-leaf fast steps on lane 0, the general step by
// the wavefront
template <bool WIDE>
__device__ __forceinline__ void wide_run(WWalk<WIDE>& W, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    Leaf<P> L;
    uint32_t pw = 0;
    uint64_t no_ticks = 0, no_steps = 0;                  // (no profile counters)
    while(true) {
        int r = 2;
        if(W.can_fast()) r = wave_fast_steps(W, L, pw, lane, false, no_ticks, no_steps);
        if(r == 2) r = wide_step(W, lane) ? 1 : 0;
        if(r == 0) break;
    }
    wave_sync();
}

// the Walk<WIDE, true> of one wavefront: constants, the capacity L, its workspace regions and LDS bitsets
template <bool WIDE>
__device__ __forceinline__ void wide_bind_ws(WWalk<WIDE>& W, uint8_t* lws, uint32_t cap, uint32_t lbytes, uint32_t pathw, uint64_t* bits)
{
    using P = typename Lay<WIDE>::pos_t;
    const WpWideLayout LL = wp_wide_layout(lbytes, pathw, cap);
    W.cap = cap; W.cap_children = 4 * cap; W.cap_results = wide_results(cap);
    W.ring_bits = bits; W.path_bits = bits + kBitsLeaf; W.child_bits = bits + 2 * kBitsLeaf; W.seen_bits = bits + 3 * kBitsLeaf;
    W.alive_bits = bits + 4 * kBitsLeaf;
    W.leaf_small = reinterpret_cast<Leaf<P>*>(lws + LL.leaves);
    W.cur = W.leaf_small; W.nxt = W.leaf_small + cap;
    W.rings = reinterpret_cast<double*>(lws + LL.rings);
    W.results = reinterpret_cast<WalkResultRec*>(lws + LL.results);
    W.paths = reinterpret_cast<uint32_t*>(lws + LL.paths);
    W.pathw = pathw;
    W.rpaths = W.paths + (uint64_t)cap * pathw;
}

} // namespace

// ---------------------------------------------------------------------------------------
// walk-parallel flow: the escalated walks of a round, one per wavefront over a queue (a.list = their slots)
// ---------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(64, LRSC_WP_WIDE_OCC) void wp_extend_wide_kernel(FmIndexDev fm, WpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTabSize<WIDE>::value];
    __shared__ uint64_t bits[4 * kBitsLeaf + kBitsChild];
    init_mask_table<WIDE>(mtab);
    const uint32_t lane = threadIdx.x;
    const uint32_t wave = blockIdx.x;
    WWalk<WIDE> W;
    wp_walk_consts(W, fm, a, mtab);
    wide_bind_ws<WIDE>(W, a.lane_ws + (uint64_t)(wave < a.n_lanes ? wave : 0u) * a.lane_ws_bytes, a.max_leaves, a.lbytes, a.lane_pathw, bits);
    if(wave < a.n_lanes)
    while(true) {
        uint32_t i = 0;
        if(lane == 0) i = atomicAdd(a.queue, 1u);
        i = first_u32(i);
        if(i >= a.n_list) break;
        const uint32_t si = a.list[i];
        W.cur = W.leaf_small; W.nxt = W.leaf_small + W.cap;
        wp_walk_bind(W, a, a.slots[si], true);            // every lane: the same values into the same words
        const uint64_t steps0 = W.steps;
        wide_run(W, lane);
        if(lane == 0) wp_walk_finish(W, a, si, steps0);
    }
    flush_counters(a.ctr, W.n_rank, W.n_blk);
}

// ---------------------------------------------------------------------------------------
// lrsc_extend_walks with -l above 32: walk w of the batch on wavefront w (grid-stride), prepared by walk_prepare_kernel
// ---------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(64, LRSC_WP_WIDE_OCC) void walk_extend_wide_kernel(FmIndexDev fm, ExtendArgs a)
{
    using P = typename Lay<WIDE>::pos_t;
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTabSize<WIDE>::value];
    __shared__ uint64_t bits[4 * kBitsLeaf + kBitsChild];
    init_mask_table<WIDE>(mtab);
    const uint32_t lane = threadIdx.x;
    uint32_t n_rank = 0, n_blk = 0;
    for(uint32_t slot = blockIdx.x; slot < a.n_walks; slot += gridDim.x) {
        const uint32_t w = a.order ? a.order[slot] : slot;
        const WalkWork ww = a.work[w];
        uint8_t* ws = a.workspace + ww.ws_off;
        WWalk<WIDE> W;
        walk_bind_work(W, fm, mtab, a, ww, ws);
        wide_bind_ws<WIDE>(W, ws + ww.o_leaves, a.max_leaves, (uint32_t)sizeof(Leaf<P>), ww.pathw, bits);
        W.n_rank = 0; W.n_blk = 0; W.steps = 0; W.leaf_steps = 0; W.max_front = 1; W.error = 0; W.cyc_setup = 0; W.cyc_loop = 0;
        W.prof = nullptr; W.profile = false;
        // the per-walk tables (an in-place sort) and the root interval by lane 0, then the root by every lane
        P riv[4] = {0, 0, 0, 0};
        if(lane == 0) {
            W.begin_static();
            Leaf<P> root;
            root.suf_lo = 0; root.suf_hi = 0;
            for(uint32_t t = 0; t < W.initk; ++t) suf_push(root, W.q[t]);
            W.find_suffix(root, W.initk);
            riv[0] = root.flo; riv[1] = root.fhi; riv[2] = root.rlo; riv[3] = root.rhi;
        }
        W.n9f = first_u32(W.n9f); W.n9r = first_u32(W.n9r); W.tmask0 = first_u64(W.tmask0); W.tmask1 = first_u64(W.tmask1);
        for(int t = 0; t < 4; ++t) riv[t] = (P)first_u64((uint64_t)riv[t]);
        wave_sync();
        W.begin_root(riv);
        wide_run(W, lane);
        if(lane == 0) {
            WalkOut& o = a.out[w];
            uint32_t len = 0, mi = 0;
            const int code = W.finish(&len, reinterpret_cast<uint32_t*>(a.out_paths + ww.out_off), &mi);
            o.code = code; o.path_len = len; o.match_i = mi; o.steps = (uint32_t)W.steps;
        }
        n_rank += W.n_rank; n_blk += W.n_blk;
        wave_sync();
    }
    flush_counters(a.ctr, n_rank, n_blk);
}

// the slots of this round's list whose narrow walk ended with LRSC_WALK_NEEDS_WIDE -> out[0 .. *n_out)
__global__ __launch_bounds__(256) void wp_wide_collect_kernel(WpArgs a, uint32_t* out, uint32_t* n_out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if(i >= a.n_list) return;
    if(a.reqs && a.reqs[i].kind != kWpReqFm) return;
    const uint32_t si = a.list ? a.list[i] : (uint32_t)a.slot_base + i;
    const WpSlot& s = a.slots[si];
    if(!(s.flags & kWpGeomBad) && (s.flags & kWpFmValid) && s.code == LRSC_WALK_NEEDS_WIDE) out[atomicAdd(n_out, 1u)] = si;
}

hipError_t launch_wp_wide_collect(const WpArgs& a, uint32_t* out, uint32_t* n_out, hipStream_t stream)
{
    if(a.n_list == 0) return hipSuccess;
    hipLaunchKernelGGL(wp_wide_collect_kernel, dim3((a.n_list + 255) / 256), dim3(256), 0, stream, a, out, n_out);
    return hipGetLastError();
}

hipError_t launch_wp_extend_wide(const FmIndexDev& fm, const WpArgs& a, hipStream_t stream)
{
    if(a.n_list == 0 || a.n_lanes == 0) return hipSuccess;
    if(a.max_leaves < 1 || a.max_leaves > kWideMaxLeaves) return hipErrorInvalidValue;
    // n_lanes = walks in flight = wavefronts
    if(fm.wide) hipLaunchKernelGGL(wp_extend_wide_kernel<true>, dim3(a.n_lanes), dim3(64), 0, stream, fm, a);
    else        hipLaunchKernelGGL(wp_extend_wide_kernel<false>, dim3(a.n_lanes), dim3(64), 0, stream, fm, a);
    return hipGetLastError();
}

hipError_t launch_walk_extend_wide(const FmIndexDev& fm, const ExtendArgs& a, uint32_t n_waves, hipStream_t stream)
{
    if(a.n_walks == 0) return hipSuccess;
    if(a.max_leaves < 1 || a.max_leaves > kWideMaxLeaves) return hipErrorInvalidValue;
    const uint32_t nb = a.n_walks < n_waves ? a.n_walks : n_waves;
    if(fm.wide) hipLaunchKernelGGL(walk_extend_wide_kernel<true>, dim3(nb), dim3(64), 0, stream, fm, a);
    else        hipLaunchKernelGGL(walk_extend_wide_kernel<false>, dim3(nb), dim3(64), 0, stream, fm, a);
    return hipGetLastError();
}

} // namespace lrsc
