// walk_host_deal_phases.hip -- TEST INFRASTRUCTURE ONLY (never linked into or loaded by the product).
//
// The dealt general step of wp_extend_deal_kernel (longreadselfcorrect_amd/csrc/wp_deal_step.h, the very source the kernel compiles)
// on the CPU at a level the job names (wp_deal_level.h: 2 = PrunedBySeedSupport dealt too, 3 = isTerminated's scans too), 64 walks
// per emulated wavefront, against Walk::step() of the same walks.  The wavefront, the loop and the comparison are those of
// tests/host_walk_deal/walk_host_deal.hip, which runs the step without a level (the default); what is new here is the level and
// the shapes of deal_prune and deal_term, counted through the trace kinds 4 and up of LRSC_DEAL_TRACE.
//
// The model.  wp_deal_step.h reaches another lane only through its wavefront type X (shfl, shfl_up, lane, ballot, sync), and
// between two X calls a lane touches nothing another lane touches.  Here every lane is a fibre on one thread, and an X call
// publishes the lane's value and hands over to the next lane; the call returns when all 64 lanes have published.  So the lanes
// run one after the other from one cross-lane operation to the next -- a host loop over the 64 lanes per phase -- and a call that
// the lanes do not make together (another operation, or not at all) is caught (`lockstep`).
//
// The loop around the step is wp_extend_deal_kernel's: persistent lanes over a queue of walks, refill and finish in the lane,
// step_fast while the frontier is one leaf, the quorum per wavefront.  Each lane carries a twin of its walk with buffers of its
// own that takes the same steps through Walk::step_fast() and Walk::step().  After every general step the twin's leaves, rings,
// paths, results and scalars are compared with the dealt walk's, and the wavefront's rank-query and block-load totals with the
// twins' (a task is counted in the lane that ran it, so only the totals are the serial step's).
//
// A stand-alone program: walk_host_deal_phases JOB RESULT.  tests/test_host_walk_deal_phases.py writes the job (index units, walks), reads the
// result (what each walk came to, the shapes reached) and holds it against the oracle; the Makefile also builds it with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ucontext.h>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/common_interface_defs.h>
#define HWD_ASAN 1
#endif
#endif

// ---- the shapes reached ----------------------------------------------------------------------------------------------------------
struct DealShapes {
    // the serial reference: Walk::step() of the twins, through walk_device.h's LRSC_WALK_TRACE
    uint64_t steps, max_leaves, max_children, steps_over_64_children, threshold_retries, level1, level2, relax_refines, trims,
        trimmed_leaves, further_children, overflow_branches, children_overflows, shared_slot_steps;
    // the wavefront, counted on the twins: general steps of the wavefront; those whose twins hold more than 64 leaves after all
    // of the step's trims (a lower bound of the first attempt's tasks); lanes that never had a walk; walks begun after the
    // wavefront's first general step
    uint64_t wave_steps, wave_steps_over_64_leaves, max_wave_leaves, lanes_without_walk, refills_mid_launch;
    // the dealt code, through wp_deal_step.h's LRSC_DEAL_TRACE
    uint64_t attempts, attempts_over_64_tasks, max_attempt_tasks, later_pass_tasks, straddling_tasks, carried_count_tasks,
        later_pass_owner_sums, later_pass_highfreq_sums, refines_over_64_tasks;
    uint64_t compared_steps, mismatches;
    // deal_prune, through LRSC_DEAL_TRACE 4..7 and (inside a task) LRSC_WALK_TRACE 12: rounds; rounds of more than 64 tasks; tasks of
    // a second or later pass; owners that take bits in a pass their children did not begin in, with surviving children on both
    // sides of the boundary; children with / without the seed-support search; searches that hit on the fwd / rvc strand; a pruned
    // child next to a surviving child of the same parent; pruned children in all
    uint64_t prunes, prunes_over_64_tasks, prune_later_pass_tasks, prune_straddling_owners, prune_straddle_alive_both, prune_need_tasks,
        prune_noneed_tasks, prune_fwd_hits, prune_rvc_hits, prune_dead_beside_alive, prune_dead_tasks;
    // on the twins: steps that leave a parent without a surviving child
    uint64_t childless_parent_steps;
    // deal_term, through LRSC_DEAL_TRACE 8..11: rounds; tasks of a second or later pass; tasks the filter rules out / lets through;
    // hits that take a new result slot / find res_first set; LRSC_WALK_ERR_RESULTS, and those with later leaves of the owner pending
    uint64_t terms, term_later_pass_tasks, term_filtered_tasks, term_scanned_tasks, term_hits_new_slot, term_hits_old_slot,
        term_result_errors, term_result_errors_pending;
};
static DealShapes g_sh;
static bool g_serial = false;                 // inside a twin's Walk::step()
static uint64_t g_step_trimmed = 0;           // leaves the twin's step has trimmed
static uint64_t g_step_slots[4];              // result slots the twin's step has stored into
static bool g_prune_task = false;             // inside a task of deal_prune (a fibre runs a task without handing over)
static uint64_t g_prev_child[3] = {~0ull, 0, 0};   // the prune task before this one: child index, alive, parent

static inline void walk_trace(int kind, uint64_t a, uint64_t b)
{
    (void)b;
    if(kind == 12) { if(g_prune_task) { if(a) g_sh.prune_rvc_hits++; else g_sh.prune_fwd_hits++; } return; }
    if(!g_serial) return;
    switch(kind) {
    case 0: g_sh.steps++; if(a > g_sh.max_leaves) g_sh.max_leaves = a; g_step_slots[0] = g_step_slots[1] = g_step_slots[2] = g_step_slots[3] = 0; break;
    case 1: if(a > g_sh.max_children) g_sh.max_children = a; if(a > 64) g_sh.steps_over_64_children++; break;
    case 2: g_sh.threshold_retries++; break;
    case 4: g_sh.children_overflows++; break;
    case 5: g_sh.level1++; break;
    case 6: g_sh.level2++; break;
    case 7: g_sh.relax_refines++; break;
    case 8: g_sh.trims++; g_sh.trimmed_leaves += a; g_step_trimmed += a; break;
    case 9: g_sh.further_children++; break;
    case 10: g_sh.overflow_branches++; break;
    case 11:
        if(a < 256) {
            if((g_step_slots[a >> 6] >> (a & 63)) & 1ull) g_sh.shared_slot_steps++;
            g_step_slots[a >> 6] |= 1ull << (a & 63);
        }
        break;
    default: break;
    }
}
static inline void deal_trace(int kind, uint64_t a, uint64_t b, uint64_t c)
{
    switch(kind) {
    case 0: g_sh.attempts++; if(a > 64) g_sh.attempts_over_64_tasks++; if(a > g_sh.max_attempt_tasks) g_sh.max_attempt_tasks = a; break;
    case 1:                                   // a task of the pass at `a`, its owner's first task at b, the owner's count so far c
        if(a >= 64) g_sh.later_pass_tasks++;
        if(b < a) { g_sh.straddling_tasks++; if(c != 0) g_sh.carried_count_tasks++; }
        break;
    case 2:                                   // an owner takes its sums of the pass at `a`; its first task at b; the sums c
        if(a >= 64) g_sh.later_pass_owner_sums++;
        if(b < a && (c >> 16) != 0) g_sh.later_pass_highfreq_sums++;
        break;
    case 3: if(a > 64) g_sh.refines_over_64_tasks++; break;
    case 4: g_sh.prunes++; if(a > 64) g_sh.prunes_over_64_tasks++; break;
    case 5:                                   // a prune task of the pass at `a` begins; c = the child needs the seed-support search
        if(a >= 64) g_sh.prune_later_pass_tasks++;
        if(c) g_sh.prune_need_tasks++; else g_sh.prune_noneed_tasks++;
        g_prune_task = true;
        break;
    case 6:                                   // ... and ends: child a of its owner, alive b, parent c
        g_prune_task = false;
        if(!b) g_sh.prune_dead_tasks++;
        if(a != 0 && g_prev_child[0] + 1 == a && g_prev_child[2] == c && g_prev_child[1] != b) g_sh.prune_dead_beside_alive++;
        g_prev_child[0] = a; g_prev_child[1] = b; g_prev_child[2] = c;
        break;
    case 7:                                   // an owner takes its bits of the pass at `a`; its first task at b; c: bit 0 = survivors in this pass, bit 1 = before
        if(b < a) { g_sh.prune_straddling_owners++; if(c == 3) g_sh.prune_straddle_alive_both++; }
        break;
    case 8: g_sh.terms++; break;
    case 9:                                   // a term task of the pass at `a`; b = the filter lets the leaf through
        if(a >= 64) g_sh.term_later_pass_tasks++;
        if(b) g_sh.term_scanned_tasks++; else g_sh.term_filtered_tasks++;
        break;
    case 10: if(a) g_sh.term_hits_new_slot++; else g_sh.term_hits_old_slot++; break;
    case 11: g_sh.term_result_errors++; if(a) g_sh.term_result_errors_pending++; break;
    default: break;
    }
}
#if defined(__HIP_DEVICE_COMPILE__)
#define LRSC_WALK_TRACE(kind, a, b)
#define LRSC_DEAL_TRACE(kind, a, b, c)
#else
#define LRSC_WALK_TRACE(kind, a, b) walk_trace((kind), (uint64_t)(a), (uint64_t)(b))
#define LRSC_DEAL_TRACE(kind, a, b, c) deal_trace((kind), (uint64_t)(a), (uint64_t)(b), (uint64_t)(c))
#endif

#include "../host_walk/walk_host.hip"
#include "../../longreadselfcorrect_amd/csrc/wp_deal_step.h"

// ---- the wavefront: 64 fibres, a cross-lane operation is where a lane hands over to the next ------------------------------------
namespace {

constexpr size_t kStack = 1u << 20;
struct Wave {
    ucontext_t ctx[64], main_ctx;
    uint8_t* stack[64];
    uint64_t slot[2][64];
    uint32_t kind[2][64];
    uint32_t opn[64];
    uint32_t cur;
    const void* main_bottom;
    size_t main_size;
    bool lockstep_broken;
};
Wave* g_wave = nullptr;

void fibre_switch(ucontext_t* from, ucontext_t* to, const void* to_bottom, size_t to_size, bool from_ends)
{
#ifdef HWD_ASAN
    void* fake = nullptr;
    __sanitizer_start_switch_fiber(from_ends ? nullptr : &fake, to_bottom, to_size);
    swapcontext(from, to);
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#else
    (void)to_bottom; (void)to_size; (void)from_ends;
    swapcontext(from, to);
#endif
}

// publish v as this lane's value of its next cross-lane operation (of kind k); back when every lane has published theirs
const uint64_t* exchange(uint64_t v, uint32_t k)
{
    Wave& w = *g_wave;
    const uint32_t l = w.cur, par = w.opn[l]++ & 1u;
    w.slot[par][l] = v;
    w.kind[par][l] = k;
    const uint32_t n = (l + 1) & 63u;
    w.cur = n;
    fibre_switch(&w.ctx[l], &w.ctx[n], w.stack[n], kStack, false);
    for(uint32_t j = 0; j < 64; ++j) if(w.kind[par][j] != k) w.lockstep_broken = true;
    return w.slot[par];
}

struct HostLanes {
    static uint32_t shfl(uint32_t v, uint32_t l) { return (uint32_t)exchange(v, 1)[l & 63u]; }
    static uint32_t shfl_up(uint32_t v, uint32_t o) { const uint32_t me = g_wave->cur; const uint64_t* s = exchange(v, 2); return me >= o ? (uint32_t)s[me - o] : v; }
    static uint32_t lane(uint32_t v, uint32_t l) { return (uint32_t)exchange(v, 3)[l & 63u]; }
    static uint64_t ballot(bool b)
    {
        const uint64_t* s = exchange(b ? 1u : 0u, 4);
        uint64_t m = 0;
        for(uint32_t j = 0; j < 64; ++j) m |= (s[j] & 1ull) << j;
        return m;
    }
    static void sync() { exchange(0, 5); }
};

// ---- a walk with buffers of its own ------------------------------------------------------------------------------------------------
struct WalkDesc { uint64_t codes_off, initk, path_len, trg_len; int64_t dis; uint64_t max_overlap, min_sa, pad; };

template <bool WIDE>
struct Box {
    using P = typename Lay<WIDE>::pos_t;
    std::vector<SortItem> it9f, it9r;
    std::vector<P> term;
    std::vector<uint16_t> next9f, next9r, head9, head5, next5;
    std::vector<uint8_t> flags5;
    std::vector<Leaf<P>> leaves;
    std::vector<double> rings;
    std::vector<WalkResultRec> results;
    std::vector<uint32_t> paths, outw;
    double freqs[101];
    Walk<WIDE> W;
    uint32_t pathw = 1;

    // the per-launch constants (wp_walk_consts) and the harmless values of a lane without a walk
    void init(HostIndex* ix, const HwParams& p)
    {
        for(int i = 0; i <= 100; ++i) freqs[i] = 0;
        for(int i = p.min_kmer_len; i <= 100; i++) freqs[i] = pow(1 - p.error_rate, i) * (size_t)p.pb_coverage;
        head9.assign(512, 0); head5.assign(1024, 0);
        leaves.assign(32 + kMaxChildren, Leaf<P>{});
        rings.assign(32 * 100, 0.0);
        results.assign(kMaxResults, WalkResultRec{});
        std::memset(static_cast<void*>(&W), 0, sizeof(W));
        const FmIndexDev& fm = ix->dev;
        W.sF = strand_consts<P>(fm.strand[LRSC_RBWT]);
        W.sR = strand_consts<P>(fm.strand[LRSC_BWT]);
        W.fm = &fm; W.mtab = ix->mtab.data();
        W.seedSize = (uint32_t)p.idmer_len; W.minOverlap = (uint32_t)p.min_kmer_len; W.maxLeaves = (uint32_t)p.max_leaves;
        W.PBcoverage = (uint64_t)p.pb_coverage; W.PacBioErrorRate = p.error_rate; W.errorRate = 0.25; W.localK = 100;
        W.freqsOfKmerSize = freqs;
        W.cur = leaves.data(); W.nxt = W.cur + 32; W.leaf_small = W.cur;
        W.rings = rings.data(); W.results = results.data();
        W.max_front = 1;
    }
    // wp_walk_bind + the tables wp_begin builds, as tests/host_walk's run_walk has them
    void bind(HostIndex* ix, const HwParams& p, const uint8_t* codes, const WalkDesc& d)
    {
        const uint32_t initk = (uint32_t)d.initk, path_len = (uint32_t)d.path_len, trg_len = (uint32_t)d.trg_len;
        const int32_t dis = (int32_t)d.dis;
        const uint32_t lq = initk + path_len + trg_len;
        const uint32_t seed = (uint32_t)p.idmer_len, mino = (uint32_t)p.min_kmer_len;
        const double maxLength = (1.2 * (dis + 10)) + (double)(2 * (uint64_t)initk);
        pathw = (uint32_t)(((uint64_t)maxLength + 4 + 15) / 16 + 1);
        const uint32_t n9 = lq - seed + 1, n5 = lq - 5 + 1, nT = trg_len - mino + 1;
        it9f.assign(n9, SortItem{}); it9r.assign(n9, SortItem{});
        term.assign((size_t)nT * 4, P{});
        next9f.assign(n9, 0); next9r.assign(n9, 0); next5.assign(n5, 0);
        head9.assign(512, 0); head5.assign(1024, 0);
        flags5.assign(n5, 0);
        leaves.assign(32 + kMaxChildren, Leaf<P>{});
        rings.assign(32 * 100, 0.0);
        results.assign(kMaxResults, WalkResultRec{});
        paths.assign((size_t)(32 + kMaxResults) * pathw, 0u);
        outw.assign(pathw, 0u);
        const FmIndexDev& fm = ix->dev;
        uint32_t cr = 0, cb = 0;
        for(uint32_t i = 0; i < lq; ++i)
            prepare_offset<WIDE>(fm, W.sF, W.sR, ix->mtab.data(), codes, i, lq, initk + path_len, seed, mino, it9f.data(), it9r.data(),
                                 flags5.data(), term.data(), cr, cb);
        W.q = codes;
        W.Lq = lq; W.initk = initk; W.path_len = path_len; W.trg_len = trg_len; W.dis = dis;
        W.maxOverlap = (uint32_t)d.max_overlap;
        W.min_SA_threshold = d.min_sa;
        W.set_lengths(dis, initk);
        W.it9f = it9f.data(); W.it9r = it9r.data();
        W.next9f = next9f.data(); W.next9r = next9r.data();
        W.head9f = head9.data(); W.head9r = head9.data() + 256;
        W.head5 = head5.data(); W.next5 = next5.data(); W.flags5 = flags5.data();
        W.term = term.data();
        W.n_term = trg_len >= mino ? trg_len - mino + 1 : 0;
        W.cur = leaves.data(); W.nxt = W.cur + 32; W.leaf_small = W.cur;
        W.rings = rings.data();
        W.paths = paths.data(); W.pathw = pathw; W.rpaths = W.paths + (uint64_t)32 * pathw;
        W.results = results.data();
        W.steps = 0; W.leaf_steps = 0; W.max_front = 1; W.error = 0; W.ended = false;    // n_rank / n_blk run on over the lane's walks
        W.begin_static();
        W.begin_root(nullptr);
    }
};

struct WalkOutRec { int64_t code; uint64_t steps, out_len, pad; };

template <bool WIDE>
struct Run {
    HostIndex* ix;
    HwParams p;
    const uint8_t* codes;
    const WalkDesc* descs;
    uint32_t n_walks, n_lanes, quorum_pct, max_wait, level;
    uint32_t queue = 0;
    bool stepped = false;
    Box<WIDE> dealt[64], twin[64];
    uint64_t lane_leaves[64];
    std::vector<WalkOutRec> out;
    std::vector<std::vector<uint8_t>> merged;
    char msg[512];
};

template <bool WIDE>
void fail(Run<WIDE>& R, uint32_t lane, uint32_t walk, const char* what)
{
    if(g_sh.mismatches++ == 0)
        std::snprintf(R.msg, sizeof(R.msg), "lane %u, walk %u, wavefront step %llu: %s differs", lane, walk, (unsigned long long)g_sh.wave_steps, what);
}

template <bool WIDE>
void compare(Run<WIDE>& R, uint32_t lane, uint32_t walk, bool took, bool stook)
{
    Box<WIDE>& A = R.dealt[lane];
    Box<WIDE>& B = R.twin[lane];
    const Walk<WIDE>& W = A.W;
    const Walk<WIDE>& S = B.W;
    g_sh.compared_steps++;
    if(took != stook) { fail(R, lane, walk, "step()'s answer"); return; }
#define HWD_CMP(f) if(W.f != S.f) fail(R, lane, walk, #f)
    HWD_CMP(n_cur); HWD_CMP(n_nxt); HWD_CMP(currentLength); HWD_CMP(currentKmerSize); HWD_CMP(min_SA_threshold); HWD_CMP(maxIndelSize);
    HWD_CMP(ended); HWD_CMP(error); HWD_CMP(steps); HWD_CMP(leaf_steps); HWD_CMP(max_front); HWD_CMP(n_results);
    HWD_CMP(ring_free); HWD_CMP(path_free); HWD_CMP(n_highfreq); HWD_CMP(alive_lo); HWD_CMP(alive_hi); HWD_CMP(has_child);
#undef HWD_CMP
    if(W.cur - A.leaves.data() != S.cur - B.leaves.data()) fail(R, lane, walk, "cur");
    if(W.nxt - A.leaves.data() != S.nxt - B.leaves.data()) fail(R, lane, walk, "nxt");
    if(W.head5 != A.head5.data() || W.next5 != A.next5.data() || W.flags5 != A.flags5.data()) fail(R, lane, walk, "the 5-mer chains (not put back)");
    if(std::memcmp(A.leaves.data(), B.leaves.data(), A.leaves.size() * sizeof(A.leaves[0])) != 0) fail(R, lane, walk, "leaves");
    if(std::memcmp(A.rings.data(), B.rings.data(), A.rings.size() * sizeof(double)) != 0) fail(R, lane, walk, "rings");
    if(std::memcmp(A.paths.data(), B.paths.data(), A.paths.size() * sizeof(uint32_t)) != 0) fail(R, lane, walk, "paths");
    if(std::memcmp(A.results.data(), B.results.data(), A.results.size() * sizeof(WalkResultRec)) != 0) fail(R, lane, walk, "results");
}

// wp_extend_deal_kernel's loop for one lane, with the twin alongside
template <bool WIDE>
void lane_body(Run<WIDE>& R, uint32_t lane)
{
    using P = typename Lay<WIDE>::pos_t;
    using X = HostLanes;
    bool done = lane >= R.n_lanes;
    Walk<WIDE>& W = R.dealt[lane].W;
    Walk<WIDE>& S = R.twin[lane].W;
    bool in_walk = false, had_walk = false;
    uint32_t wi = 0;
    Leaf<P> L{}, LS{};
    uint32_t pw = 0, pwS = 0;
    bool fast = false;
    uint32_t gen_wait = 0;
    bool want_gen = false;
    while(true) {
        int r = 3;
        if(!done) {
            if(!in_walk) {
                const uint32_t i = R.queue++;
                if(i >= R.n_walks) done = true;
                else {
                    wi = i;
                    R.dealt[lane].bind(R.ix, R.p, R.codes + R.descs[i].codes_off, R.descs[i]);
                    R.twin[lane].bind(R.ix, R.p, R.codes + R.descs[i].codes_off, R.descs[i]);
                    in_walk = true; had_walk = true;
                    fast = false; want_gen = false; gen_wait = 0;
                    if(R.stepped) g_sh.refills_mid_launch++;
                }
            }
            if(in_walk) {
                if(!fast && !want_gen && W.can_fast()) { W.enter_fast(L, pw); S.enter_fast(LS, pwS); fast = true; }
                r = 2;
                if(fast) {
                    r = W.step_fast(L, pw);
                    if(S.step_fast(LS, pwS) != r) fail(R, lane, wi, "step_fast()'s answer");
                    if(r != 1) fast = false;
                }
            }
        }
        const uint64_t need = X::ballot(r == 2);
        if(need) {
            const uint32_t n_need = (uint32_t)__builtin_popcountll(need);
            const uint32_t n_busy = n_need + (uint32_t)__builtin_popcountll(X::ballot(r == 1));
            const bool waited = X::ballot(r == 2 && gen_wait >= R.max_wait) != 0;
            if(n_need * 100u < n_busy * R.quorum_pct && !waited) {
                if(r == 2) { ++gen_wait; want_gen = true; r = 1; }
            } else {
                const bool act = r == 2;
                if(act) { gen_wait = 0; want_gen = false; }
                const uint64_t leaves0 = act ? S.n_cur : 0;
                const bool took = lrsc::deal_step<X>(W, act, lane, R.level);
                R.lane_leaves[lane] = 0;
                if(act) {
                    g_serial = true; g_step_trimmed = 0;
                    const bool stook = S.step();
                    g_serial = false;
                    if(stook) R.lane_leaves[lane] = leaves0 - g_step_trimmed;
                    // a parent without a surviving child (the frontier after the trims against has_child)
                    if(stook && !S.error && (uint64_t)__builtin_popcount(S.has_child) < leaves0 - g_step_trimmed) g_sh.childless_parent_steps++;
                    compare(R, lane, wi, took, stook);
                    r = took ? 1 : 0;
                }
                X::sync();                                // (the harness's own) every lane has compared
                if(lane == 0) {
                    R.stepped = true;
                    uint64_t nr = 0, nb = 0, sr = 0, sb = 0, lv = 0;
                    for(uint32_t j = 0; j < 64; ++j) {
                        nr += R.dealt[j].W.n_rank; nb += R.dealt[j].W.n_blk; sr += R.twin[j].W.n_rank; sb += R.twin[j].W.n_blk;
                        lv += R.lane_leaves[j];
                    }
                    if(nr != sr) fail(R, lane, wi, "the wavefront's rank queries");
                    if(nb != sb) fail(R, lane, wi, "the wavefront's block loads");
                    g_sh.wave_steps++;
                    if(lv > 64) g_sh.wave_steps_over_64_leaves++;
                    if(lv > g_sh.max_wave_leaves) g_sh.max_wave_leaves = lv;
                }
            }
        }
        if(r == 0) {
            in_walk = false;
            uint32_t len = 0, mi = 0, lenS = 0, miS = 0;
            const int code = W.finish(&len, R.dealt[lane].outw.data(), &mi);
            const int codeS = S.finish(&lenS, R.twin[lane].outw.data(), &miS);
            if(code != codeS || len != lenS || mi != miS || W.steps != S.steps) fail(R, lane, wi, "finish()");
            else if(code > 0 && std::memcmp(R.dealt[lane].outw.data(), R.twin[lane].outw.data(), ((len + 15) >> 4) * 4) != 0) fail(R, lane, wi, "the chosen path");
            WalkOutRec& o = R.out[wi];
            o.code = code; o.steps = W.steps; o.out_len = 0; o.pad = 0;
            if(code > 0) {
                const uint32_t mino = W.minOverlap, trg_len = W.trg_len;
                const uint32_t tail_from = mi + mino;
                const uint32_t tail = trg_len > mino && tail_from <= trg_len ? trg_len - tail_from : 0;
                std::vector<uint8_t>& m = R.merged[wi];
                m.resize(len + tail);
                for(uint32_t i = 0; i < len; ++i) m[i] = (uint8_t)path_get(R.dealt[lane].outw.data(), i);
                const uint8_t* trg = W.q + W.initk + W.path_len;
                for(uint32_t i = 0; i < tail; ++i) m[len + i] = trg[tail_from + i];
                o.out_len = len + tail;
            }
            W.n_cur = 0; W.n_nxt = 0;
        }
        if(X::ballot(!done) == 0) break;
    }
    if(!had_walk) g_sh.lanes_without_walk++;
}

template <bool WIDE> Run<WIDE>* g_run = nullptr;

template <bool WIDE>
void fibre_main(int lane)
{
    Wave& w = *g_wave;
#ifdef HWD_ASAN
    const void* ob = nullptr; size_t os = 0;
    __sanitizer_finish_switch_fiber(nullptr, &ob, &os);
    if(lane == 0) { w.main_bottom = ob; w.main_size = os; }
#endif
    lane_body<WIDE>(*g_run<WIDE>, (uint32_t)lane);
    // the lanes leave the loop together (its last ballot): each hands over to the next, the last one to main
    if(lane < 63) { w.cur = (uint32_t)lane + 1; fibre_switch(&w.ctx[lane], &w.ctx[lane + 1], w.stack[lane + 1], kStack, true); }
    else fibre_switch(&w.ctx[lane], &w.main_ctx, w.main_bottom, w.main_size, true);
}

template <bool WIDE>
int run_wave(HostIndex* ix, const HwParams& p, const uint8_t* codes, const WalkDesc* descs, uint32_t n_walks, uint32_t n_lanes, uint32_t quorum,
             uint32_t wait, uint32_t level, std::vector<WalkOutRec>& out, std::vector<std::vector<uint8_t>>& merged, char* msg, size_t msg_len)
{
    Run<WIDE>* R = new Run<WIDE>();
    R->ix = ix; R->p = p; R->codes = codes; R->descs = descs; R->n_walks = n_walks; R->n_lanes = n_lanes; R->quorum_pct = quorum; R->max_wait = wait; R->level = level;
    R->out.assign(n_walks, WalkOutRec{});
    R->merged.assign(n_walks, std::vector<uint8_t>());
    R->msg[0] = 0;
    for(int l = 0; l < 64; ++l) { R->dealt[l].init(ix, p); R->twin[l].init(ix, p); R->lane_leaves[l] = 0; }
    Wave* w = new Wave();
    std::memset(static_cast<void*>(w), 0, sizeof(*w));
    g_wave = w;
    g_run<WIDE> = R;
    for(int l = 0; l < 64; ++l) {
        w->stack[l] = new uint8_t[kStack];
        getcontext(&w->ctx[l]);
        w->ctx[l].uc_stack.ss_sp = w->stack[l];
        w->ctx[l].uc_stack.ss_size = kStack;
        w->ctx[l].uc_link = nullptr;
        makecontext(&w->ctx[l], (void (*)())fibre_main<WIDE>, 1, l);
    }
    w->cur = 0;
    fibre_switch(&w->main_ctx, &w->ctx[0], w->stack[0], kStack, false);
    const bool broken = w->lockstep_broken;
    for(int l = 0; l < 64; ++l) delete[] w->stack[l];
    delete w;
    g_wave = nullptr;
    out = R->out; merged = R->merged;
    std::snprintf(msg, msg_len, "%s", R->msg);
    delete R;
    g_run<WIDE> = nullptr;
    if(broken) { std::snprintf(msg, msg_len, "lockstep: the lanes did not make the same cross-lane calls"); return 2; }
    return g_sh.mismatches ? 1 : 0;
}

bool read_all(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

} // namespace

// JOB: 24 uint64 {magic, wide, n_tables, k[5], n_symbols, n_bwt, n_rbwt, idmer_len, min_kmer_len, max_leaves, pb_coverage, error_rate (a double's
// bits), quorum_pct, max_wait, n_lanes, n_walks, n_codes, 0, 0, 0}, the bwt and rbwt units, n_walks WalkDesc, the codes.  The first 0 of the header is the level here (2 or 3).
// RESULT: uint64 {return value, n_walks, words of DealShapes}, DealShapes, n_walks WalkOutRec, the merged codes back to back, then the first
// mismatch as text.
int main(int argc, char** argv)
{
    if(argc != 3) { std::fprintf(stderr, "usage: %s JOB RESULT\n", argv[0]); return 64; }
    FILE* f = std::fopen(argv[1], "rb");
    if(!f) { std::perror(argv[1]); return 65; }
    uint64_t h[24];
    if(!read_all(f, h, sizeof(h)) || h[0] != 0x4C41454444574800ull) { std::fprintf(stderr, "bad job header\n"); return 65; }
    const bool wide = h[1] != 0;
    int ks[5];
    const int n_tables = (int)(h[2] < 5 ? h[2] : 5);
    for(int i = 0; i < 5; ++i) ks[i] = (int)h[3 + i];
    const uint64_t n_sym = h[8], n0 = h[9], n1 = h[10];
    HwParams p;
    p.idmer_len = (int32_t)h[11]; p.min_kmer_len = (int32_t)h[12]; p.max_leaves = (int32_t)h[13]; p.pb_coverage = (int32_t)h[14];
    std::memcpy(&p.error_rate, &h[15], 8);
    const uint32_t quorum = (uint32_t)h[16], wait = (uint32_t)h[17], n_lanes = (uint32_t)h[18], n_walks = (uint32_t)h[19];
    const uint64_t n_codes = h[20];
    const uint32_t level = (uint32_t)h[21];
    if(level < lrsc::kDealLevelPrune || level > lrsc::kDealLevelTerm) { std::fprintf(stderr, "bad level\n"); return 65; }
    if(n_lanes == 0 || n_lanes > 64 || p.max_leaves < 1 || p.max_leaves > 32) { std::fprintf(stderr, "bad job\n"); return 65; }
    std::vector<uint8_t> u0(n0), u1(n1), codes(n_codes);
    std::vector<WalkDesc> descs(n_walks);
    if(!read_all(f, u0.data(), n0) || !read_all(f, u1.data(), n1) || !read_all(f, descs.data(), n_walks * sizeof(WalkDesc)) ||
       !read_all(f, codes.data(), n_codes)) { std::fprintf(stderr, "short job\n"); return 65; }
    std::fclose(f);
    for(const WalkDesc& d : descs)
        if(d.codes_off + d.initk + d.path_len + d.trg_len > n_codes || d.trg_len < (uint64_t)p.min_kmer_len ||
           d.initk + d.path_len + d.trg_len < (uint64_t)p.idmer_len) { std::fprintf(stderr, "bad walk\n"); return 65; }
    HostIndex* ix = static_cast<HostIndex*>(hw_index_create(u0.data(), n0, u1.data(), n1, n_sym, wide ? 1 : 0, ks, n_tables));
    if(!ix) { std::fprintf(stderr, "index\n"); return 66; }
    std::memset(&g_sh, 0, sizeof(g_sh));
    std::vector<WalkOutRec> out;
    std::vector<std::vector<uint8_t>> merged;
    char msg[512];
    const int rc = wide ? run_wave<true>(ix, p, codes.data(), descs.data(), n_walks, n_lanes, quorum, wait, level, out, merged, msg, sizeof(msg))
                        : run_wave<false>(ix, p, codes.data(), descs.data(), n_walks, n_lanes, quorum, wait, level, out, merged, msg, sizeof(msg));
    hw_index_free(ix);
    FILE* g = std::fopen(argv[2], "wb");
    if(!g) { std::perror(argv[2]); return 65; }
    const uint64_t head[3] = {(uint64_t)rc, n_walks, sizeof(DealShapes) / 8};
    std::fwrite(head, 8, 3, g);
    std::fwrite(&g_sh, sizeof(g_sh), 1, g);
    if(n_walks) std::fwrite(out.data(), sizeof(WalkOutRec), n_walks, g);
    for(const auto& m : merged) if(!m.empty()) std::fwrite(m.data(), 1, m.size(), g);
    std::fwrite(msg, 1, std::strlen(msg), g);
    std::fclose(g);
    if(rc) std::fprintf(stderr, "walk_host_deal_phases: %s (%llu mismatches)\n", msg, (unsigned long long)g_sh.mismatches);
    return rc;
}
