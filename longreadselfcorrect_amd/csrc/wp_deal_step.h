// wp_deal_step.h -- the general step of a lane-per-walk wavefront with extendLeaves' per-leaf work dealt across the 64 lanes
// (wp_deal.hip's kernel; tests/host_walk_deal runs the same source on the CPU).  Include after walk_device.h.
//
// Every function here is entered by all 64 lanes of the wavefront.  What a lane learns of another lane goes through the
// wavefront type X and nothing else:
//   X::shfl(v, l)     lane l's v (l is the reader's own)          X::lane(v, l)   the same with l wavefront-uniform
//   X::shfl_up(v, o)  lane (own - o)'s v, the own v below lane o   X::ballot(b)    bit l = lane l's b
//   X::sync()         what a lane stored before is visible to every lane after it
// Between two such calls a lane's code reads and writes only its own registers and, in memory, what no other lane touches
// before the next X::sync().  So the code is a sequence of phases of (lane, wavefront state), and running the lanes one after
// the other from one X call to the next -- which is what the host's X does -- is an exact model of the wavefront.
//
// The tasks rely on the per-kernel constants being wavefront-uniform: a task runs getFMIndexExtensions_v, find_suffix and
// make_child on the EXECUTING lane's Walk object, so sF / sR / fm / mtab, PBcoverage, PacBioErrorRate, freqsOfKmerSize, minOverlap
// and whatever else wp_walk_consts sets must be the same on all lanes.  What differs from walk to walk and a task reads
// (min_SA_threshold, currentLength, maxIndelSize, the 5-mer chains) steps aside for the owner's in deal_attempt; a constant that
// becomes per-walk has to join that list.
#pragma once

#ifndef LRSC_DEAL_TRACE
#define LRSC_DEAL_TRACE(kind, a, b, c)         // test hook (tests/host_walk_deal): which shapes of the dealt passes were run
#endif

namespace lrsc {

template <class X> LRSC_WALK_FN uint64_t deal_shfl_u64(uint64_t v, uint32_t l)
{
    return (uint64_t)X::shfl((uint32_t)v, l) | ((uint64_t)X::shfl((uint32_t)(v >> 32), l) << 32);
}
template <class X, class T> LRSC_WALK_FN T* deal_shfl_ptr(T* p, uint32_t l) { return reinterpret_cast<T*>(deal_shfl_u64<X>(reinterpret_cast<uint64_t>(p), l)); }
template <class X> LRSC_WALK_FN uint32_t deal_incl_sum(uint32_t v, uint32_t lane)
{
    for(uint32_t o = 1; o < 64; o <<= 1) { const uint32_t w = X::shfl_up(v, o); if(lane >= o) v += w; }
    return v;
}

// The tasks of a dealt phase: lane o owns cnt[o] of them, task t belongs to the lane whose [excl, incl) holds t.
struct Deal {
    uint32_t incl, excl, total;
};
template <class X> LRSC_WALK_FN Deal deal_make(uint32_t cnt, uint32_t lane)
{
    Deal d;
    d.incl = deal_incl_sum<X>(cnt, lane);
    d.excl = d.incl - cnt;
    d.total = X::lane(d.incl, 63);
    return d;
}
// owner of task t < total: the number of lanes whose inclusive count is <= t (the counts do not decrease from lane to lane)
template <class X> LRSC_WALK_FN uint32_t deal_owner(const Deal& d, uint32_t t)
{
    uint32_t lo = 0;
    for(uint32_t s = 32; s > 0; s >>= 1) {
        const uint32_t v = X::shfl(d.incl, lo + s - 1);
        if(v <= t) lo += s;
    }
    return lo;
}

// ---- refineSAInterval (.cpp:355-369) of the owners with `on`: leaves[0, n) to suffix length l --------------------------------
template <class X, bool WIDE>
LRSC_WALK_FN void deal_refine(Walk<WIDE>& W, bool on, Leaf<typename Lay<WIDE>::pos_t>* leaves, uint32_t n, uint64_t l, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    const Deal d = deal_make<X>(on ? n : 0u, lane);
    if(lane == 0) { LRSC_DEAL_TRACE(3, d.total, 0, 0); }
    for(uint32_t base = 0; base < d.total; base += 64) {
        const uint32_t t = base + lane;
        const bool have = t < d.total;
        const uint32_t o = deal_owner<X>(d, have ? t : d.total - 1);
        const uint32_t i = (have ? t : d.total - 1) - X::shfl(d.excl, o);
        Leaf<P>* const arr = deal_shfl_ptr<X>(leaves, o);
        const uint32_t ol = X::shfl((uint32_t)l, o);
        if(have) W.find_suffix(arr[i], ol);
    }
    if(on) W.currentKmerSize = l;
    X::sync();
}

// ---- attempToExtend (.cpp:373-465) + updateLeaves (:468-488) of the owners with `on` --------------------------------------------
template <class X, bool WIDE>
LRSC_WALK_FN void deal_attempt(Walk<WIDE>& W, bool on, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    // in the owner, as attempToExtend has it: the minimum error rate, then the trim (the survivors keep their order)
    double minimumErrorRate = 1;
    if(on) {
        for(uint32_t i = 0; i < W.n_cur; i += 4) {
            double e[4];
#pragma unroll
            for(uint32_t j = 0; j < 4; ++j) e[j] = W.cur[i + j < W.n_cur ? i + j : i].localErr;
#pragma unroll
            for(uint32_t j = 0; j < 4; ++j) if(i + j < W.n_cur && e[j] < minimumErrorRate) minimumErrorRate = e[j];
        }
        uint32_t w = 0;
        for(uint32_t i = 0; i < W.n_cur; ++i) {
            const double errorRateDiff = W.cur[i].localErr - minimumErrorRate;
            if((errorRateDiff > 0.05 && W.currentLength > W.localK / 2) || (errorRateDiff > 0.1 && W.currentLength > 15)) {
                W.free_leaf_slots(W.cur[i]);
                continue;
            }
            if(w != i) leaf_move(&W.cur[w], &W.cur[i]);
            ++w;
        }
        W.n_cur = w;
        W.n_highfreq = 0;
    }
    X::sync();
    const int highfreqThreshold = W.PBcoverage > 60 ? (int)((uint64_t)(W.PBcoverage / 60) * 3) : 3;   // wavefront-uniform (see the top)
    // the children an owner's nxt[] takes: the buffer that is not leaf_small holds kMaxChildren, leaf_small 32 (Walk::step_body's
    // swap rule leaves room for four children per leaf; the bound is checked all the same before a child is stored)
    const uint32_t my_cap = W.nxt == W.leaf_small ? W.small_cap() : W.max_children();
    bool overflow = false;
    const Deal d = deal_make<X>(on ? W.n_cur : 0u, lane);
    if(lane == 0) { LRSC_DEAL_TRACE(0, d.total, 0, 0); }
    for(uint32_t base = 0; base < d.total; base += 64) {
        const uint32_t t = base + lane;
        const bool have = t < d.total;
        const uint32_t tt = have ? t : d.total - 1;
        const uint32_t o = deal_owner<X>(d, tt);
        const uint32_t o_excl = X::shfl(d.excl, o);
        const uint32_t i = tt - o_excl;
        // the owner's walk, as far as this task reads it
        Leaf<P>* const o_cur = deal_shfl_ptr<X>(W.cur, o);
        Leaf<P>* const o_nxt = deal_shfl_ptr<X>(W.nxt, o);
        const uint32_t o_n = X::shfl(W.n_cur, o), o_cap = X::shfl(my_cap, o);
        const uint32_t o_count = X::shfl(W.n_nxt, o);                        // children the owner has from earlier passes
        const double o_min = __builtin_bit_cast(double, deal_shfl_u64<X>(__builtin_bit_cast(uint64_t, minimumErrorRate), o));
        const uint64_t o_sa = deal_shfl_u64<X>(W.min_SA_threshold, o), o_len = deal_shfl_u64<X>(W.currentLength, o),
                       o_indel = deal_shfl_u64<X>(W.maxIndelSize, o);
        uint16_t* const o_head5 = deal_shfl_ptr<X>(W.head5, o);
        uint16_t* const o_next5 = deal_shfl_ptr<X>(W.next5, o);
        const uint8_t* const o_flags5 = deal_shfl_ptr<X>(W.flags5, o);
        // this lane's own walk steps aside for the task's getFMIndexExtensions
        const uint64_t s_sa = W.min_SA_threshold, s_len = W.currentLength, s_indel = W.maxIndelSize;
        uint16_t* const s_head5 = W.head5;
        uint16_t* const s_next5 = W.next5;
        const uint8_t* const s_flags5 = W.flags5;
        W.min_SA_threshold = o_sa; W.currentLength = o_len; W.maxIndelSize = o_indel;
        W.head5 = o_head5; W.next5 = o_next5; W.flags5 = o_flags5;
        Leaf<P> par = {};
        typename Walk<WIDE>::Ext ext[4];
        uint32_t mask = 0;
        if(have) {
            LRSC_DEAL_TRACE(1, base, o_excl, o_count);
            par = o_cur[i];
            int count = 0;
            while(count < 2) {
                if(count == 1 && !(par.localErr == o_min && o_n > 1)) break;
                uint64_t tc;
                mask = W.getFMIndexExtensions_v(par.flo, par.fhi, par.rlo, par.rhi, par.tailLetterCount, par.suf_lo, ext, tc);
                if(mask != 0) break;
                W.min_SA_threshold--;
                count++;
            }
        }
        W.min_SA_threshold = s_sa; W.currentLength = s_len; W.maxIndelSize = s_indel;
        W.head5 = s_head5; W.next5 = s_next5; W.flags5 = s_flags5;
        // accepted bases in the low half, those above isInsufficientFreqs' threshold in the high half: one prefix sum for both
        uint32_t v = 0;
#pragma unroll
        for(uint32_t b = 0; b < 4; ++b)
            if((mask >> b) & 1u) v += 1u + (ext[b].freq > highfreqThreshold ? 0x10000u : 0u);
        const uint32_t v_incl = deal_incl_sum<X>(v, lane), v_excl = v_incl - v;
        // the owner's first task of this pass: the prefix restarts there
        const uint32_t first = o_excl > base ? o_excl - base : 0u;
        const uint32_t off = o_count + ((v_excl - X::shfl(v_excl, first)) & 0xFFFFu);
        if(have) {
            uint32_t k = off;
#pragma unroll
            for(uint32_t b = 0; b < 4; ++b) {
                if(!((mask >> b) & 1u)) continue;
                if(k >= o_cap) { overflow = true; break; }
                o_nxt[k++] = W.make_child(par, i, b, ext[b]);
            }
        }
        // the owners take their tasks' totals of this pass
        const uint32_t s0 = d.excl > base ? d.excl : base, s1 = d.incl < base + 64 ? d.incl : base + 64;
        const bool mine = on && s0 < s1;
        const uint32_t sum = X::shfl(v_incl, mine ? s1 - 1 - base : 0u) - X::shfl(v_excl, mine ? s0 - base : 0u);
        const uint64_t ovf = X::ballot(overflow);
        if(mine) {
            LRSC_DEAL_TRACE(2, base, d.excl, sum);
            W.n_nxt += sum & 0xFFFFu; W.n_highfreq += sum >> 16;
        }
        // A child that found no room: its owner's walk ends with LRSC_WALK_ERR_CHILDREN, the code the serial loop gives it.  Only
        // the code is the serial loop's: that loop stops at the child and counts no rank query behind it, while here n_nxt and
        // n_highfreq have taken the pass's full sums and the tasks behind the child have run and are counted.  Walk::step()
        // cannot get here (at most maxLeaves = 32 leaves of four children, and nxt[] then holds kMaxChildren = 128); the check
        // is what keeps a store inside the buffer if that ever changes.
        uint64_t m = ovf;
        while(m) {
            const uint32_t l = (uint32_t)__builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t bad_owner = X::lane(o, l);
            if(lane == bad_owner) W.error = LRSC_WALK_ERR_CHILDREN;
        }
        overflow = false;
    }
    X::sync();
}

// ---- one iteration of extendOverlap's loop (Walk::step) for the lanes with `act`; every lane of the wavefront comes here ----------
// returns Walk::step()'s answer for an `act` lane (false otherwise)
template <class X, bool WIDE>
LRSC_WALK_FN bool deal_step(Walk<WIDE>& W, bool act, uint32_t lane)
{
    if(act && (W.ended || W.error || !(W.n_cur != 0 && W.n_cur <= W.maxLeaves && W.currentLength <= W.maxLength))) act = false;
    const bool took = act;
    if(act) {
        W.leaf_steps += W.n_cur;
        if(W.n_cur > W.max_front) W.max_front = W.n_cur;
        W.n_nxt = 0;
    }
    X::sync();                                            // the owners' frontiers are in memory for every lane
    // --- extendLeaves (.cpp:239-278) ---
    const uint64_t t_ext = W.tick();
    uint64_t t = t_ext;
    deal_refine<X>(W, act && W.currentKmerSize > W.maxOverlap, W.cur, W.n_cur, W.maxOverlap, lane);
    if(took) W.tock(1, t);
    t = W.tick();
    deal_attempt<X>(W, act, lane);
    if(took) W.tock(2, t);
    if(W.error) act = false;
    const bool lvl1 = act && W.n_nxt == 0;                // level 1: reduce the k-mer size
    if(X::ballot(lvl1)) {
        uint64_t ReduceSize = 0;
        if(lvl1) {
            const uint64_t LowerBound = (W.currentKmerSize - 2) > W.minOverlap ? (W.currentKmerSize - 2) : W.minOverlap;
            const uint64_t ts = W.tick();
            ReduceSize = W.SelectFreqsOfrange(LowerBound, W.currentKmerSize, W.cur, W.n_cur);
            W.tock(8, ts);
        }
        X::sync();
        deal_refine<X>(W, lvl1, W.cur, W.n_cur, ReduceSize, lane);
        deal_attempt<X>(W, lvl1, lane);
        if(W.error) act = false;
        const bool lvl2 = lvl1 && act && W.n_nxt == 0;    // level 2: reduce the threshold
        if(X::ballot(lvl2)) {
            if(lvl2) W.min_SA_threshold--;
            deal_attempt<X>(W, lvl2, lane);
            if(lvl2) W.min_SA_threshold++;
            if(W.error) act = false;
        }
    }
    bool relax = false;
    uint64_t RelaxSize = 0;
    if(act && W.n_nxt != 0) {
        W.currentLength++;
        W.currentKmerSize++;
        if(W.isInsufficientFreqs(W.n_highfreq, W.n_nxt)) {   // frequencies are low: relax the k-mer size
            const uint64_t LowerBound = (W.currentKmerSize - 2) > W.minOverlap ? (W.currentKmerSize - 2) : W.minOverlap;
            const uint64_t ts = W.tick();
            RelaxSize = W.SelectFreqsOfrange(LowerBound, W.currentKmerSize, W.nxt, W.n_nxt);
            W.tock(8, ts);
            relax = true;
        }
    }
    if(X::ballot(relax)) {
        X::sync();
        deal_refine<X>(W, relax, W.nxt, W.n_nxt, RelaxSize, lane);
    }
    if(took) W.tock(0, t_ext);
    // --- PrunedBySeedSupport, the commit and isTerminated, in the walk's own lane ---
    if(act) W.step_after_extend();
    return took;
}

} // namespace lrsc
