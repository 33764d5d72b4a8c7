// wp_walk.h -- device glue between the walk-parallel flow's slots (wp.h) and the walk (walk_device.h), shared by the extension
// kernels of wp.hip, wp_wave.hip and wp_wide.hip, and the wavefront pieces of the two one-walk-per-wavefront kernels (wp_wave.hip,
// wp_wide.hip).  Include after walk_device.h and wp.h.
#pragma once

namespace lrsc {

// ---- wavefront helpers (call them with the whole wavefront active) ----------------------------------------------------------
__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ uint32_t popc64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
__device__ __forceinline__ uint32_t first_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t first_u64(uint64_t v) { return (uint64_t)first_u32((uint32_t)v) | ((uint64_t)first_u32((uint32_t)(v >> 32)) << 32); }
__device__ __forceinline__ double first_f64(double v) { return __longlong_as_double((long long)first_u64((uint64_t)__double_as_longlong(v))); }
// the value of lane l (l wave-uniform)
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ double lane_f64(double v, uint32_t l)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return __longlong_as_double((long long)((uint64_t)lane_u32((uint32_t)b, l) | ((uint64_t)lane_u32((uint32_t)(b >> 32), l) << 32)));
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for(int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return first_u32(v);
}
__device__ __forceinline__ int wave_max(int v)
{
    for(int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return (int)first_u32((uint32_t)v);
}
// minimum of values that are not NaN (exact in any order)
__device__ __forceinline__ double wave_min(double v)
{
    for(int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return first_f64(v);
}
// what a lane stored before is visible to every lane of the wavefront after it
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// a.gen_stats: one general step of a lane-per-walk wavefront.  Called by the lanes that went into the step together; `took` = the
// lane's Walk::step() ran its body.  Sums and maxima over those lanes a bit plane at a time (ballots only: nothing crosses a lane
// that is not here), added by the first of them.
__device__ __forceinline__ void wp_gen_count(unsigned long long* g, bool took, uint32_t n_cur, uint32_t n_nxt)
{
    const uint64_t m = __ballot(took);
    if(m == 0) return;
    uint32_t sum[2], mx[2];
    for(int k = 0; k < 2; ++k) {
        const uint32_t v = k ? n_nxt : n_cur;
        bool cand = took;
        sum[k] = 0; mx[k] = 0;
        for(int b = 15; b >= 0; --b) {
            const bool bit = took && ((v >> b) & 1u);
            sum[k] += (uint32_t)__builtin_popcountll(__ballot(bit)) << b;
            if(__ballot(cand && bit)) { mx[k] |= 1u << b; cand = cand && bit; }
        }
    }
    if(threadIdx.x == (uint32_t)__builtin_ctzll(m)) {
        atomicAdd(&g[0], 1ull);
        atomicAdd(&g[1], (unsigned long long)__builtin_popcountll(m));
        atomicAdd(&g[2], (unsigned long long)sum[0]); atomicAdd(&g[3], (unsigned long long)mx[0]);
        atomicAdd(&g[4], (unsigned long long)sum[1]); atomicAdd(&g[5], (unsigned long long)mx[1]);
        // what the serial step pays for, in leaf passes: every lane taking part waits for the widest one
        atomicAdd(&g[6], (unsigned long long)mx[0] * (unsigned long long)__builtin_popcountll(m));
        atomicAdd(&g[7], (unsigned long long)mx[1] * (unsigned long long)__builtin_popcountll(m));
        // ... and what the same leaves are in passes of 64 lanes
        atomicAdd(&g[8], (unsigned long long)((sum[0] + 63u) / 64u));
        atomicAdd(&g[9], (unsigned long long)((sum[1] + 63u) / 64u));
    }
}

// the same for the work of the step's PrunedBySeedSupport and isTerminated phases (Walk::count_prune_work / count_term_work):
// g[3 k + 0] sum, g[3 k + 1] sum of the per-step maximum, g[3 k + 2] sum of (maximum x lanes taking part), for k = 0 children that
// need the seed-support search, 1 chain entries they walk, 2 leaves that pass term_may_hit, 3 term rows they scan
__device__ __forceinline__ void wp_gen_count_phases(unsigned long long* g, bool took, uint32_t need, uint32_t chain, uint32_t term, uint32_t rows)
{
    const uint64_t m = __ballot(took);
    if(m == 0) return;
    const uint32_t v[4] = {need, chain, term, rows};
    uint32_t sum[4], mx[4];
    for(int k = 0; k < 4; ++k) {
        bool cand = took;
        sum[k] = 0; mx[k] = 0;
        for(int b = 23; b >= 0; --b) {
            const bool bit = took && ((v[k] >> b) & 1u);
            sum[k] += (uint32_t)__builtin_popcountll(__ballot(bit)) << b;
            if(__ballot(cand && bit)) { mx[k] |= 1u << b; cand = cand && bit; }
        }
    }
    if(threadIdx.x == (uint32_t)__builtin_ctzll(m))
        for(int k = 0; k < 4; ++k) {
            atomicAdd(&g[3 * k], (unsigned long long)sum[k]);
            atomicAdd(&g[3 * k + 1], (unsigned long long)mx[k]);
            atomicAdd(&g[3 * k + 2], (unsigned long long)mx[k] * (unsigned long long)__builtin_popcountll(m));
        }
}

// ---- a walk's slot: setup and finish ----------------------------------------------------------------------------------------
// the walk's fixed inputs: the query and the tables wp_prepare_kernel / wp_begin_kernel built in the slot's prepared workspace
template <bool WIDE, bool BIG>
__device__ __forceinline__ void wp_bind_static(Walk<WIDE, BIG>& W, const WpArgs& a, const WpSlot& s)
{
    using P = typename Lay<WIDE>::pos_t;
    const WpPrepLayout L = wp_prep_layout(s.lq, s.trg_len, a.seed_size, a.min_overlap, a.psz);
    uint8_t* ws = s.prep;
    W.q = s.q;
    W.Lq = s.lq; W.initk = s.k; W.path_len = s.gap; W.trg_len = s.trg_len; W.dis = (int32_t)s.gap;
    W.it9f = reinterpret_cast<SortItem*>(ws + L.item9f);
    W.it9r = reinterpret_cast<SortItem*>(ws + L.item9r);
    W.next9f = reinterpret_cast<uint16_t*>(ws + L.next9f);
    W.next9r = reinterpret_cast<uint16_t*>(ws + L.next9r);
    W.head9f = reinterpret_cast<uint16_t*>(ws + L.head9);
    W.head9r = W.head9f + 256;
    W.head5 = reinterpret_cast<uint16_t*>(ws + L.head5);
    W.next5 = reinterpret_cast<uint16_t*>(ws + L.next5);
    W.flags5 = ws + L.flags5;
    W.term = reinterpret_cast<const P*>(ws + L.term);
    W.n_term = s.trg_len >= a.min_overlap ? s.trg_len - a.min_overlap + 1 : 0;
}

// constants of an extension kernel's Walk object that do not depend on the walk.  Only the narrow walk escalates (a.escalate): the
// wide one is where escalated walks go.
template <bool WIDE, bool BIG>
__device__ __forceinline__ void wp_walk_consts(Walk<WIDE, BIG>& W, const FmIndexDev& fm, const WpArgs& a, const uint32_t* mtab)
{
    using P = typename Lay<WIDE>::pos_t;
    W.sF = strand_consts<P>(fm.strand[LRSC_RBWT]);
    W.sR = strand_consts<P>(fm.strand[LRSC_BWT]);
    W.fm = &fm; W.mtab = mtab;
    W.seedSize = a.seed_size; W.minOverlap = a.min_overlap; W.maxLeaves = a.max_leaves;
    if constexpr(!BIG) W.escalate = a.escalate != 0;
    W.PBcoverage = a.pb_coverage; W.PacBioErrorRate = a.pacbio_error_rate; W.errorRate = 0.25; W.localK = 100;
    W.freqsOfKmerSize = a.freqs_of_kmer_size;
    W.n_rank = 0; W.n_blk = 0; W.steps = 0; W.leaf_steps = 0; W.error = 0; W.cyc_setup = 0; W.cyc_loop = 0; W.prof = nullptr; W.profile = false;
}

// the walk of slot s, from its root, into the leaf buffers the kernel has bound (W.cur, W.nxt, W.leaf_small): the prepared state
// and its header, the parameters and lengths of the walk.  sync: the lanes of a wavefront write the root together, after a
// wave_sync() (wp_wide.hip)
template <bool WIDE, bool BIG>
__device__ __forceinline__ void wp_walk_bind(Walk<WIDE, BIG>& W, const WpArgs& a, const WpSlot& s, bool sync = false)
{
    using P = typename Lay<WIDE>::pos_t;
    wp_bind_static(W, a, s);
    const WpStatic* H = reinterpret_cast<const WpStatic*>(s.prep);
    W.n9f = H->n9f; W.n9r = H->n9r; W.tmask0 = H->tmask0; W.tmask1 = H->tmask1;
    W.maxOverlap = (uint32_t)s.k + 2;
    W.min_SA_threshold = a.pb_coverage > 60 ? (uint64_t)((a.pb_coverage / 60) * 3) : 3;
    W.set_lengths((int32_t)s.gap, s.k);
    W.error = 0;
    W.leaf_steps = 0; W.max_front = 1;
    const P riv[4] = {(P)H->root[0], (P)H->root[1], (P)H->root[2], (P)H->root[3]};
    if(sync) wave_sync();
    W.begin_root(riv);
}

// extendOverlap is over: findTheBestPath / the failure code and the walk's counters into slot si, and a failed walk with next == 0
// to the DP stage of the round.  steps0: W.steps when the walk began
template <bool WIDE, bool BIG>
__device__ __forceinline__ void wp_walk_finish(Walk<WIDE, BIG>& W, const WpArgs& a, uint32_t si, uint64_t steps0)
{
    WpSlot& s = a.slots[si];
    uint32_t plen = 0, mi = 0;
    const int code = W.finish(&plen, s.path, &mi);
    s.code = code; s.path_len = plen; s.match_i = mi; s.steps = (uint32_t)(W.steps - steps0); s.leaf_steps = W.leaf_steps;
    s.max_front = (uint8_t)(W.max_front < 255u ? W.max_front : 255u);
    s.flags |= (uint8_t)kWpFmValid;
    if(code <= 0 && code > LRSC_WALK_ERR_CHILDREN && a.auto_dp && s.next == 0) {
        const uint32_t j = atomicAdd(a.n_dp_items, 1u);
        if(j < a.dp_items_cap) {
            WpDpItem d; d.q = (uint64_t)s.dpq; d.slot = si; d.lq = s.dp_lq; d.k = s.dp_k; d.total_freq = s.dp_total_freq;
            a.dp_items[j] = d;
        }
    }
}

// ---- per-leaf pieces of the one-walk-per-wavefront step (Walk<WIDE> in wp_wave.hip, Walk<WIDE, true> in wp_wide.hip) ----------
// refineSAInterval (.cpp:355-369): leaf j on lane j & 63
template <class WalkT>
__device__ __forceinline__ void wave_refine(WalkT& W, Leaf<typename WalkT::P>* leaves, uint32_t n, uint64_t newKmerSize, uint32_t lane)
{
    for(uint32_t j = lane; j < n; j += 64) W.find_suffix(leaves[j], (uint32_t)newKmerSize);
    W.currentKmerSize = newKmerSize;
}

// a further child's copies of its parent's ring and path, by the whole wavefront, with this step's own entries already in place
// (the serial commit copies everything but the own ring entry, then writes that entry and sets the new path character)
template <class WalkT>
__device__ __forceinline__ void wave_copy_slots(WalkT& W, uint64_t further, const Leaf<typename WalkT::P>& ch, uint32_t new_ring, uint32_t new_path,
                                                uint32_t lane)
{
    while(further) {
        const uint32_t l = (uint32_t)__builtin_ctzll(further);
        further &= further - 1ull;
        const uint32_t sr = lane_u32(ch.ring, l), dr = lane_u32(new_ring, l), sp = lane_u32(ch.path, l), dp = lane_u32(new_path, l);
        const uint32_t own = (lane_u32(ch.hist_size, l) - 1u) % 100u, plen = lane_u32(ch.path_len, l), ex = lane_u32(ch.ext, l);
        const double ge = lane_f64(ch.globalErr, l);
        const double* src = W.rings + (uint64_t)sr * 100;
        double* dst = W.rings + (uint64_t)dr * 100;
        for(uint32_t k = lane; k < 100; k += 64) dst[k] = k == own ? ge : src[k];
        const uint32_t* ps = W.paths + (uint64_t)sp * W.pathw;
        uint32_t* pd = W.paths + (uint64_t)dp * W.pathw;
        const uint32_t nw = (plen + 16) >> 4, wi = plen >> 4, sh = 2 * (plen & 15u);
        for(uint32_t k = lane; k < nw; k += 64) {
            uint32_t v = ps[k];
            if(k == wi) v = (v & ~(3u << sh)) | (ex << sh);
            pd[k] = v;
        }
    }
}

// results.at(first - 1) of every leaf of `hits` (lanes in leaf order: a later leaf with the same result slot overwrites, as in the
// serial loop): the record by lane 0, the path by the whole wavefront
template <class WalkT>
__device__ __forceinline__ void wave_store_results(WalkT& W, uint64_t hits, const Leaf<typename WalkT::P>& lf, int hit, uint32_t lane)
{
    while(hits) {
        const uint32_t l = (uint32_t)__builtin_ctzll(hits);
        hits &= hits - 1ull;
        const uint32_t slot = lane_u32((uint32_t)lf.res_first, l) - 1u, path = lane_u32(lf.path, l), plen = lane_u32(lf.path_len, l);
        const uint32_t mi = lane_u32((uint32_t)hit, l);
        const double ge = lane_f64(lf.globalErr, l);
        if(lane == 0) { WalkResultRec& r = W.results[slot]; r.error_rate = ge; r.match_i = mi; r.path_len = plen; }
        const uint32_t* src = W.paths + (uint64_t)path * W.pathw;
        uint32_t* dst = W.rpaths + (uint64_t)slot * W.pathw;
        const uint32_t nw = (plen + 15) >> 4;
        for(uint32_t k = lane; k < nw; k += 64) dst[k] = src[k];
    }
}

// single-leaf fast steps (Walk::step_fast) on lane 0 until the frontier leaves that regime, then what a fast step changes broadcast
// from lane 0 (rank-query counters stay per lane).  Returns step_fast's last answer: 0 = the walk is over, 2 = the general step is
// next.  prof: the segment's wall ticks are added to `ticks` and its steps to `n_fast`
template <class WalkT>
__device__ __forceinline__ int wave_fast_steps(WalkT& W, Leaf<typename WalkT::P>& L, uint32_t& pw, uint32_t lane, bool prof, uint64_t& ticks,
                                               uint64_t& n_fast)
{
    int r = 2;
    wave_sync();
    const uint64_t tq = prof ? __builtin_readcyclecounter() : 0;
    if(lane == 0) {
        W.enter_fast(L, pw);
        do { r = W.step_fast(L, pw); if(prof && r == 1) ++n_fast; } while(r == 1);
    }
    if(prof) ticks += __builtin_readcyclecounter() - tq;
    r = (int)first_u32((uint32_t)r);
    W.currentLength = first_u64(W.currentLength); W.currentKmerSize = first_u64(W.currentKmerSize);
    W.steps = first_u64(W.steps); W.leaf_steps = first_u32(W.leaf_steps);
    W.n_cur = first_u32(W.n_cur); W.n_results = first_u32(W.n_results); W.error = (int)first_u32((uint32_t)W.error);
    return r;
}

} // namespace lrsc
