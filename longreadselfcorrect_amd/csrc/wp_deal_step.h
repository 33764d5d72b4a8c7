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
// becomes per-walk has to join that list.  deal_prune's tasks run prune_leaf on the executing lane's Walk object in the same way:
// seedSize, PacBioErrorRate, errorRate and localK are wavefront-uniform, and what steps aside for the owner's is currentLength and
// the 9-mer tables (head9f/r, it9f/r, next9f/r); nxt, rings, maxIndelSize and Lq are read across lanes into the task's own
// values.  deal_term's tasks run term_scan: minOverlap is uniform, and currentKmerSize, tmask0/1, term and trg_len step aside;
// cur is read across lanes.
#pragma once
#include "wp_deal_level.h"

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

// the tasks of the pass at `base` that belong to this lane as an owner: [s0, s1) of the deal, none where s0 >= s1
struct DealSpan {
    uint32_t s0, s1;
};
LRSC_WALK_FN DealSpan deal_span(const Deal& d, uint32_t base)
{
    DealSpan s;
    s.s0 = d.excl > base ? d.excl : base;
    s.s1 = d.incl < base + 64 ? d.incl : base + 64;
    return s;
}
// bit k = bit (s0 - base + k) of a ballot over the pass's task lanes, for the s1 - s0 tasks of the span
LRSC_WALK_FN uint64_t deal_span_bits(uint64_t ballot, const DealSpan& s, uint32_t base)
{
    const uint32_t n = s.s1 - s.s0;
    return (ballot >> (s.s0 - base)) & (n >= 64 ? ~0ull : (1ull << n) - 1ull);
}

// ---- PrunedBySeedSupport (.cpp:491-563) of the owners with `on`: a task is prune_leaf<true> of one child of nxt[0, n_nxt) ----------
// The order of the children cannot be observed (the comment in Walk::PrunedBySeedSupport): a child's evaluation reads its own
// fields, the walk's tables, fixed since begin_static, and one slot of its parent's ring, which only the commit writes; it writes
// its own fields.  The owner receives the frontier's bit sets: alive_lo / alive_hi from a ballot of the pass's tasks, shifted to
// the owner's child indices and accumulated over the passes its children fall into; has_child from an OR over the owner's tasks of
// the pass (a scan that restarts at the owner's first task).  Both are ORs of one bit per surviving child, so the order in which
// they are set is the serial loop's as far as anything can tell.
template <class X, bool WIDE>
LRSC_WALK_FN void deal_prune(Walk<WIDE>& W, bool on, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    if(on) { W.alive_lo = 0; W.alive_hi = 0; W.has_child = 0; }
    const Deal d = deal_make<X>(on ? W.n_nxt : 0u, lane);
    if(lane == 0) { LRSC_DEAL_TRACE(4, d.total, 0, 0); }
    for(uint32_t base = 0; base < d.total; base += 64) {
        const uint32_t t = base + lane;
        const bool have = t < d.total;
        const uint32_t tt = have ? t : d.total - 1;
        const uint32_t o = deal_owner<X>(d, tt);
        const uint32_t o_excl = X::shfl(d.excl, o);
        const uint32_t c = tt - o_excl;
        // the owner's walk, as far as prune_leaf, seed_support_core and computeErrorRate read it
        Leaf<P>* const o_nxt = deal_shfl_ptr<X>(W.nxt, o);
        double* const o_rings = deal_shfl_ptr<X>(W.rings, o);
        uint16_t* const o_head9f = deal_shfl_ptr<X>(W.head9f, o);
        uint16_t* const o_head9r = deal_shfl_ptr<X>(W.head9r, o);
        SortItem* const o_it9f = deal_shfl_ptr<X>(W.it9f, o);
        SortItem* const o_it9r = deal_shfl_ptr<X>(W.it9r, o);
        uint16_t* const o_next9f = deal_shfl_ptr<X>(W.next9f, o);
        uint16_t* const o_next9r = deal_shfl_ptr<X>(W.next9r, o);
        const uint64_t o_len = deal_shfl_u64<X>(W.currentLength, o), o_indel = deal_shfl_u64<X>(W.maxIndelSize, o);
        const uint32_t o_Lq = X::shfl(W.Lq, o);
        // this lane's own walk steps aside for the task
        const uint64_t s_len = W.currentLength;
        uint16_t* const s_head9f = W.head9f;
        uint16_t* const s_head9r = W.head9r;
        SortItem* const s_it9f = W.it9f;
        SortItem* const s_it9r = W.it9r;
        uint16_t* const s_next9f = W.next9f;
        uint16_t* const s_next9r = W.next9r;
        W.currentLength = o_len;
        W.head9f = o_head9f; W.head9r = o_head9r; W.it9f = o_it9f; W.it9r = o_it9r; W.next9f = o_next9f; W.next9r = o_next9r;
        bool alive = false;
        uint32_t pbit = 0;
        if(have) {
            // PrunedBySeedSupport's window of the owner's step
            const uint64_t currSeedIdx = o_len - W.seedSize;
            const uint64_t indelOffset = W.seedSize + o_indel;
            const uint64_t smallSeedIdx = currSeedIdx <= indelOffset ? 0 : currSeedIdx - indelOffset;
            const uint64_t largeSeedIdx = (currSeedIdx + indelOffset) >= (o_Lq - W.seedSize) ? (o_Lq - W.seedSize) : currSeedIdx + indelOffset;
            Leaf<P>& ch = o_nxt[c];
            LRSC_DEAL_TRACE(5, base, o_excl, (o_len - ch.lastOverlapLen > W.seedSize || o_len - ch.lastOverlapLen <= 1) ? 1 : 0);
            // a child still carries its parent's ring id: the parent's error history, which no commit has touched yet
            W.template prune_leaf<true>(ch, o_rings + (uint64_t)ch.ring * 100, currSeedIdx, smallSeedIdx, largeSeedIdx);
            alive = ch.alive != 0;
            if(alive) pbit = 1u << ch.parent;
            LRSC_DEAL_TRACE(6, c, alive, ch.parent);
        }
        W.currentLength = s_len;
        W.head9f = s_head9f; W.head9r = s_head9r; W.it9f = s_it9f; W.it9r = s_it9r; W.next9f = s_next9f; W.next9r = s_next9r;
        // the owners take their children's bits of this pass
        const uint64_t am = X::ballot(alive);
        const uint32_t first = o_excl > base ? o_excl - base : 0u;      // the lane of the first task of this task's owner in this pass
        uint32_t hc = pbit;
        for(uint32_t s = 1; s < 64; s <<= 1) { const uint32_t w = X::shfl_up(hc, s); if(lane >= first + s) hc |= w; }
        const DealSpan sp = deal_span(d, base);
        const bool mine = on && sp.s0 < sp.s1;
        const uint32_t got = X::shfl(hc, mine ? sp.s1 - 1 - base : 0u);
        if(mine) {
            const uint64_t seg = deal_span_bits(am, sp, base);
            const uint32_t c0 = sp.s0 - d.excl;                          // the owner's first child of this pass
            LRSC_DEAL_TRACE(7, base, d.excl, (seg != 0 ? 1 : 0) | ((W.alive_lo | W.alive_hi) != 0 ? 2 : 0));
            if(c0 < 64) { W.alive_lo |= seg << c0; if(c0) W.alive_hi |= seg >> (64 - c0); }
            else W.alive_hi |= seg << (c0 - 64);
            W.has_child |= got;
        }
    }
    X::sync();                                            // the children's fields are in memory for their owners' commits
}

// ---- isTerminated (.cpp:825-878) over the new frontier of the owners with `on`: a task is term_scan of one leaf of cur[0, n_cur) ----
// term_scan is a function of the leaf and of the walk's constants and issues no rank query.  The owner then takes its hits of the
// pass in leaf order and does with each what terminated_leaf does from the scan's answer on (the result slot, LRSC_WALK_ERR_RESULTS,
// res_second, term_store), and stops at the first error as the serial loop does: a later hit of the same owner, in this pass or a
// later one, is dropped.  The scan that ran for a leaf behind the error cannot be observed: it stores nothing and counts nothing.
template <class X, bool WIDE>
LRSC_WALK_FN void deal_term(Walk<WIDE>& W, bool on, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    X::sync();                                            // the owners' new frontiers are in memory for every lane
    const Deal d = deal_make<X>(on ? W.n_cur : 0u, lane);
    if(lane == 0) { LRSC_DEAL_TRACE(8, d.total, 0, 0); }
    for(uint32_t base = 0; base < d.total; base += 64) {
        const uint32_t t = base + lane;
        const bool have = t < d.total;
        const uint32_t tt = have ? t : d.total - 1;
        const uint32_t o = deal_owner<X>(d, tt);
        const uint32_t i = tt - X::shfl(d.excl, o);
        // the owner's walk, as far as term_may_hit and term_scan read it
        Leaf<P>* const o_cur = deal_shfl_ptr<X>(W.cur, o);
        const P* const o_term = deal_shfl_ptr<X>(W.term, o);
        const uint64_t o_kmer = deal_shfl_u64<X>(W.currentKmerSize, o), o_tm0 = deal_shfl_u64<X>(W.tmask0, o), o_tm1 = deal_shfl_u64<X>(W.tmask1, o);
        const uint32_t o_trg = X::shfl(W.trg_len, o);
        // this lane's own walk steps aside for the task
        const P* const s_term = W.term;
        const uint64_t s_kmer = W.currentKmerSize, s_tm0 = W.tmask0, s_tm1 = W.tmask1;
        const uint32_t s_trg = W.trg_len;
        W.term = o_term; W.currentKmerSize = o_kmer; W.tmask0 = o_tm0; W.tmask1 = o_tm1; W.trg_len = o_trg;
        int hit = -1;
        if(have) {
            LRSC_DEAL_TRACE(9, base, W.term_may_hit(o_cur[i].suf_lo), 0);
            hit = W.term_scan(o_cur[i]);
        }
        W.term = s_term; W.currentKmerSize = s_kmer; W.tmask0 = s_tm0; W.tmask1 = s_tm1; W.trg_len = s_trg;
        // the owners take their leaves' hits of this pass, lowest leaf first
        const uint64_t hm = X::ballot(hit >= 0);
        const DealSpan sp = deal_span(d, base);
        uint64_t todo = on && sp.s0 < sp.s1 && !W.error ? deal_span_bits(hm, sp, base) : 0ull;
        while(X::ballot(todo != 0)) {
            const uint32_t l = todo ? sp.s0 - base + (uint32_t)__builtin_ctzll(todo) : 0u;
            const int h = (int)X::shfl((uint32_t)hit, l);
            if(todo) {
                todo &= todo - 1ull;
                Leaf<P>& lf = W.cur[base + l - d.excl];
                LRSC_DEAL_TRACE(10, lf.res_first == -1, todo != 0 || d.incl > base + 64, 0);
                W.terminated_hit(lf, h, W.paths + (uint64_t)lf.path * W.pathw, lf.path_len, -1);
                if(W.error) { LRSC_DEAL_TRACE(11, todo != 0 || d.incl > base + 64, 0, 0); todo = 0; }
            }
        }
    }
}

// ---- one iteration of extendOverlap's loop (Walk::step) for the lanes with `act`; every lane of the wavefront comes here ----------
// level (wp_deal_level.h, wavefront-uniform): what follows extendLeaves is dealt too -- from kDealLevelPrune PrunedBySeedSupport,
// from kDealLevelTerm isTerminated's scans; below that it runs in the walk's own lane, as Walk::step_after_extend() has it.
// MAXLVL: the highest level this instantiation can run (a lower one carries neither the dealt phases' code nor their registers).
// returns Walk::step()'s answer for an `act` lane (false otherwise)
template <class X, bool WIDE, uint32_t MAXLVL = kDealLevelTerm>
LRSC_WALK_FN bool deal_step(Walk<WIDE>& W, bool act, uint32_t lane, uint32_t level = kDealLevelDefault)
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
    if constexpr(MAXLVL < kDealLevelPrune) {
        // --- PrunedBySeedSupport, the commit and isTerminated, in the walk's own lane ---
        // (Walk::step_after_extend(), with the phases' work counted between its pieces in a profiling launch)
        if(W.prof) { W.ph_need = 0; W.ph_chain = 0; W.ph_term = 0; W.ph_rows = 0; }
        if(act) {
            if(W.prof) W.count_prune_work();
            t = W.tick();
            W.PrunedBySeedSupport();
            W.tock(4, t);
            if(W.step_commit()) {
                if(W.prof) W.count_term_work();
                W.step_terminated();
            }
        }
        return took;
    }
    // profiling launches: what the two phases below have to do, for the general-step counters (wp_gen_count_phases)
    if(W.prof) {
        W.ph_need = 0; W.ph_chain = 0; W.ph_term = 0; W.ph_rows = 0;
        if(act) W.count_prune_work();
    }
    // --- PrunedBySeedSupport: dealt, or in the walk's own lane ---
    t = W.tick();
    if(level >= kDealLevelPrune) deal_prune<X>(W, act, lane);
    else if(act) W.PrunedBySeedSupport();
    if(act) W.tock(4, t);
    // --- the commit, in the walk's own lane (with the overflow branch and its terminated_leaf calls) ---
    const bool committed = act && W.step_commit();
    if(W.prof && committed) W.count_term_work();
    // --- isTerminated over the new frontier: the scans dealt, or all of it in the walk's own lane ---
    if(level >= kDealLevelTerm) {
        const bool scan = committed && W.currentLength >= W.minLength;
        if(X::ballot(scan)) {
            t = W.tick();
            deal_term<X>(W, scan, lane);
            if(scan) W.tock(6, t);
        }
    } else if(committed) W.step_terminated();
    return took;
}

} // namespace lrsc
