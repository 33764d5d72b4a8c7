// wp_deal.hip -- wp_extend_deal_kernel: the lane-per-walk extension launches (lane_stride 1) with extendLeaves' per-leaf work dealt
// across the wavefront.
//
// wp_extend_kernel runs Walk::step() in the walk's own lane: the lanes of a wavefront that take a general step together wait for
// the one with the widest frontier (7.6 leaves, where the 42 lanes taking part hold 2.3 on average: profiles/walk_deal_premise.txt).
// Here the loop is the same -- persistent lanes over the queue, one walk per lane, step_fast in the lane, the quorum decided per
// wavefront -- but the general step is entered by all 64 lanes, and the per-leaf pieces of extendLeaves are tasks (owner lane,
// leaf index) in owner-major order, 64 per pass, whichever lane they fall on.  The step itself is wp_deal_step.h, which
// tests/host_walk_deal also runs on the CPU, lane by lane between two cross-lane operations:
//   deal_refine    refineSAInterval: find_suffix of one leaf
//   deal_attempt   attempToExtend: getFMIndexExtensions with the per-leaf min_SA_threshold retry, and make_child; a child's place in
//                  the owner's nxt[] is the owner's count so far plus a segmented exclusive prefix of the accepted bases, which is
//                  (parent, base) order
// What a task needs of its owner's walk comes by cross-lane reads: the leaf buffers, min_SA_threshold, the minimum error rate, the
// kept count, and what ismatchedbykmer reads (currentLength, maxIndelSize, the 5-mer chains).  Everything else of the step stays
// in the owner lane, in step_body's order: the error-rate minimum and the trim, SelectFreqsOfrange, the retry levels and
// isInsufficientFreqs (an owner that needs a further refine or attempt takes part in another dealt round; the others sit it out),
// and Walk::step_after_extend() -- PrunedBySeedSupport, the commit, isTerminated.  Rank queries are counted in the lane that ran
// them and summed over the launch (flush_counters), so the totals are those of the serial step.  No LDS beyond the mask table.
#define LRSC_WALK_FN __device__ __forceinline__
#define LRSC_WALK_NOINLINE
#include <hip/hip_runtime.h>

#include "walk_device.h"
#include "wp.h"
#include "wp_walk.h"
#include "wp_deal_step.h"

namespace lrsc {

#ifndef LRSC_WP_EXTEND_OCC
#define LRSC_WP_EXTEND_OCC 2          // wavefronts per SIMD, as wp_extend_kernel (capi_core.cpp sizes the launches for that)
#endif

namespace {

// the wavefront of wp_deal_step.h on the device (call these with the whole wavefront active)
struct DevLanes {
    static __device__ __forceinline__ uint32_t shfl(uint32_t v, uint32_t l) { return (uint32_t)__shfl((int)v, (int)l, 64); }
    static __device__ __forceinline__ uint32_t shfl_up(uint32_t v, uint32_t o) { return (uint32_t)__shfl_up((int)v, o, 64); }
    static __device__ __forceinline__ uint32_t lane(uint32_t v, uint32_t l) { return lane_u32(v, l); }
    static __device__ __forceinline__ uint64_t ballot(bool b) { return __ballot(b); }
    static __device__ __forceinline__ void sync() { wave_sync(); }
};

} // namespace

// ---------------------------------------------------------------------------------------
// persistent lanes over a queue of walks: wp_extend_kernel's loop, with the general step entered by the whole wavefront.  A lane
// whose queue has run dry stays as a worker until every lane of its wavefront is done.
// PROF: the LRSC_CORRECT_PROFILE instantiation.  The tick slots are an array the Walk object points to, which lives in scratch
// memory whether or not a launch asks for ticks (72 B of the private segment); the launches that do not ask run without it.
// ---------------------------------------------------------------------------------------
// MAXLVL: the highest LRSC_WP_DEAL level the body can run.  Two kernels share the body: wp_extend_deal_kernel is level 1, compiled
// without deal_prune and deal_term, so that it pays neither for their registers nor for their spills; wp_extend_deal_phases_kernel
// runs levels 2 and 3 (a.deal_level, wavefront-uniform).  As one kernel with the level read at run time the body had 152 / 163
// spilled VGPRs against 85 / 97 and ran level 1 one per cent slower; as two bodies in one kernel its private segment was 592 /
// 736 B, past the bound tests/test_deal_kernel_build.py holds it to ("The prune and isTerminated dealt").
template <bool WIDE, bool PROF, uint32_t MAXLVL>
__device__ __forceinline__ void wp_extend_deal_body(const FmIndexDev& fm, const WpArgs& a, const uint32_t* mtab)
{
    using P = typename Lay<WIDE>::pos_t;
    const uint32_t lane = threadIdx.x;
    const uint32_t lane_id = blockIdx.x * 64 + lane;
    bool done = lane_id >= a.n_lanes;
    Walk<WIDE> W;
    wp_walk_consts(W, fm, a, mtab);
    const WpLaneLayout LL = wp_lane_layout(a.lbytes, a.lane_pathw);
    uint8_t* lws = a.lane_ws + (uint64_t)(done ? 0u : lane_id) * a.lane_ws_bytes;
    Leaf<P>* const leaf_base = reinterpret_cast<Leaf<P>*>(lws + LL.leaves);
    W.rings = reinterpret_cast<double*>(lws + LL.rings);
    W.results = reinterpret_cast<WalkResultRec*>(lws + LL.results);
    W.paths = reinterpret_cast<uint32_t*>(lws + LL.paths);
    W.pathw = a.lane_pathw;
    W.rpaths = W.paths + (uint64_t)32 * a.lane_pathw;
    // a lane without a walk takes no part as an owner, but its Walk object is read as one's: harmless values
    W.cur = leaf_base; W.nxt = leaf_base + 32; W.leaf_small = leaf_base;
    W.n_cur = 0; W.n_nxt = 0; W.n_highfreq = 0; W.ended = false;
    W.currentLength = 0; W.currentKmerSize = 0; W.maxOverlap = 0; W.maxLength = 0; W.maxIndelSize = 0; W.min_SA_threshold = 0;
    W.head5 = nullptr; W.next5 = nullptr; W.flags5 = nullptr;

    bool in_walk = false;
    uint32_t si = 0;
    uint64_t steps0 = 0;
    Leaf<P> L;                                            // single-leaf fast path (walk_device.h): the one leaf of the frontier in registers
    uint32_t pw = 0;
    bool fast = false;
    uint32_t gen_wait = 0;
    bool want_gen = false;
    // profiling (a.prof): as wp_extend_kernel; the ticks of a dealt phase go to the lanes whose walks take the step
    uint64_t pr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t_refill = 0, t_finish = 0, n_fast = 0;
    const bool prof = PROF && a.prof != nullptr;
    if constexpr(PROF) { if(prof) W.prof = pr; }
    const uint64_t t_loop0 = prof ? __builtin_readcyclecounter() : 0;
    while(true) {
        int r = 3;                                        // 3: no walk in this lane in this iteration
        if(!done) {
            if(!in_walk) {
                const uint64_t tr0 = prof ? __builtin_readcyclecounter() : 0;
                const uint32_t i = atomicAdd(a.queue, 1u);
                if(i >= a.n_list) done = true;
                else if(!(a.reqs && a.reqs[i].kind != kWpReqFm)) {
                    si = a.list ? a.list[i] : (uint32_t)a.slot_base + i;
                    const WpSlot& s = a.slots[si];
                    if(!(s.flags & kWpGeomBad)) {
                        W.cur = leaf_base; W.nxt = leaf_base + 32; W.leaf_small = leaf_base;
                        steps0 = W.steps;
                        wp_walk_bind(W, a, s);
                        in_walk = true;
                        fast = false; want_gen = false; gen_wait = 0;
                    }
                }
                if(prof) t_refill += __builtin_readcyclecounter() - tr0;
            }
            if(in_walk) {
                if(!fast && !want_gen && W.can_fast()) { W.enter_fast(L, pw); fast = true; }
                r = 2;
                if(fast) {
                    const uint64_t tq = prof ? __builtin_readcyclecounter() : 0;
                    r = W.step_fast(L, pw);
                    if(r != 1) fast = false;
                    if(prof) { pr[7] += __builtin_readcyclecounter() - tq; if(r == 1) ++n_fast; }
                }
            }
        }
        // the quorum of wp_extend_kernel, decided once for the wavefront
        const uint64_t need = __ballot(r == 2);
        if(need) {
            const uint32_t n_need = popc64(need);
            const uint32_t n_busy = n_need + popc64(__ballot(r == 1));
            const bool waited = __ballot(r == 2 && gen_wait >= a.general_max_wait) != 0;
            if(n_need * 100u < n_busy * a.general_quorum_pct && !waited) {
                if(r == 2) { ++gen_wait; want_gen = true; r = 1; }
            } else {
                const bool act = r == 2;
                if(act) { gen_wait = 0; want_gen = false; }
                const uint32_t n_cur0 = W.n_cur;
                const bool took = deal_step<DevLanes, WIDE, MAXLVL>(W, act, lane, a.deal_level);
                if(act) r = took ? 1 : 0;
                if constexpr(PROF) {
                    if(a.gen_stats) {
                        wp_gen_count(a.gen_stats, took, n_cur0, W.n_nxt);
                        if(prof) wp_gen_count_phases(a.gen_stats + 10, took, W.ph_need, W.ph_chain, W.ph_term, W.ph_rows);
                    }
                }
            }
        }
        if(r == 0) {
            in_walk = false;
            const uint64_t tf0 = prof ? __builtin_readcyclecounter() : 0;
            wp_walk_finish(W, a, si, steps0);
            W.n_cur = 0; W.n_nxt = 0;
            if(prof) t_finish += __builtin_readcyclecounter() - tf0;
        }
        if(__ballot(!done) == 0) break;
    }
    if(prof && lane_id < a.n_lanes) {
        for(int j = 0; j < 8; ++j) atomicAdd(&a.prof[j], (unsigned long long)pr[j]);
        atomicAdd(&a.prof[8], (unsigned long long)t_refill);
        atomicAdd(&a.prof[9], (unsigned long long)t_finish);
        atomicAdd(&a.prof[10], (unsigned long long)(__builtin_readcyclecounter() - t_loop0));
        atomicAdd(&a.prof[11], (unsigned long long)W.steps);
        atomicAdd(&a.prof[12], (unsigned long long)n_fast);
        atomicAdd(&a.prof[13], (unsigned long long)pr[8]);
    }
    flush_counters(a.ctr, W.n_rank, W.n_blk);
}

template <bool WIDE, bool PROF>
__global__ __launch_bounds__(64, LRSC_WP_EXTEND_OCC) void wp_extend_deal_kernel(FmIndexDev fm, WpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTabSize<WIDE>::value];
    init_mask_table<WIDE>(mtab);
    wp_extend_deal_body<WIDE, PROF, kDealLevelExtend>(fm, a, mtab);
}
template <bool WIDE, bool PROF>
__global__ __launch_bounds__(64, LRSC_WP_EXTEND_OCC) void wp_extend_deal_phases_kernel(FmIndexDev fm, WpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTabSize<WIDE>::value];
    init_mask_table<WIDE>(mtab);
    wp_extend_deal_body<WIDE, PROF, kDealLevelTerm>(fm, a, mtab);
}

hipError_t launch_wp_extend_deal(const FmIndexDev& fm, const WpArgs& a, hipStream_t stream)
{
    if(a.n_list == 0 || a.n_lanes == 0) return hipSuccess;
    if(a.lane_stride > 1) return hipErrorInvalidValue;                 // one walk per lane only
    const unsigned nb = (unsigned)(((uint64_t)a.n_lanes + 63) / 64);
    const bool prof = a.prof != nullptr || a.gen_stats != nullptr;
    if(a.deal_level >= kDealLevelPrune) {
        if(fm.wide) {
            if(prof) hipLaunchKernelGGL((wp_extend_deal_phases_kernel<true, true>), dim3(nb), dim3(64), 0, stream, fm, a);
            else     hipLaunchKernelGGL((wp_extend_deal_phases_kernel<true, false>), dim3(nb), dim3(64), 0, stream, fm, a);
        } else {
            if(prof) hipLaunchKernelGGL((wp_extend_deal_phases_kernel<false, true>), dim3(nb), dim3(64), 0, stream, fm, a);
            else     hipLaunchKernelGGL((wp_extend_deal_phases_kernel<false, false>), dim3(nb), dim3(64), 0, stream, fm, a);
        }
    } else if(fm.wide) {
        if(prof) hipLaunchKernelGGL((wp_extend_deal_kernel<true, true>), dim3(nb), dim3(64), 0, stream, fm, a);
        else     hipLaunchKernelGGL((wp_extend_deal_kernel<true, false>), dim3(nb), dim3(64), 0, stream, fm, a);
    } else {
        if(prof) hipLaunchKernelGGL((wp_extend_deal_kernel<false, true>), dim3(nb), dim3(64), 0, stream, fm, a);
        else     hipLaunchKernelGGL((wp_extend_deal_kernel<false, false>), dim3(nb), dim3(64), 0, stream, fm, a);
    }
    return hipGetLastError();
}

} // namespace lrsc
