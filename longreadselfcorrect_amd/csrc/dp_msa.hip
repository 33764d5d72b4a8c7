// dp_msa.hip -- MultipleAlignment::addOverlap / _addSequence / calculateBaseConsensus
// (Thirdparty/multiple_alignment.cpp:208-393,517-594, as driven by LongReadOverlap::buildMultipleAlignment,
// PacBio/LongReadOverlap.cpp:17-55) on the device: one workgroup per correctByMSAlignment call, of one wavefront for the many
// narrow pile-ups and of several for the few of thousands of columns, where one wavefront leaves the device empty and makes 64
// columns per trip.  One body, msa_pileup<GLOBAL, NW>, for all of them: its passes stride by the NT = 64 x NW threads of the
// workgroup, and its state is in LDS or (GLOBAL) in a workspace slot, where dp_msa_layout.h says.
//
// The reference keeps every row's padded string; the consensus only needs, per column, how many rows show
// A / C / G / T / '-', plus the padded base row.  So the state here is
//   T[]            the base row's padded_sequence (codes 0-3, kGap),
//   cnt[col]       five 12-bit counters per global column,
//   lead[e],size[e] leading_columns and padded length of every other row (what insertGapBeforeColumn looks at),
// and the operations are the reference's, step for step, including its quirks: incoming rows are aligned against
// the base row only; an insertion opens a new column unless the base row already has a gap column *at the
// current template position*; leading_columns of the base row is read once per incoming row (:306), so an
// insertion in front of base 0 moves the template cursor past a base without consuming a cigar op.
// Rows are added in retrieval order (source-seed strings, then target-seed strings).
//
// One incoming row is added in a few wavefront-wide passes instead of one dependent step per column (a.row_batch,
// the default).  What makes that possible: in the coordinates the base row has when the row starts, every cigar
// op's effect is known from prefix counts over the cigar alone --
//   * an M/D op consumes the next base of the base row; the b-th base sits at bpos[b];
//   * a run of r I ops in front of base b first fills the G = bpos[b] - bpos[b-1] - 1 gap columns already there
//     (op i < G lands in column bpos[b-1] + 1 + i), the others each open a new column in front of bpos[b];
//   * gap columns of the base row the cigar walks over without an I show '-' in the new row;
// and insertGapBeforeColumn's effect on every other row (leading_columns += 1 when the column is at or before its
// start, one more padded symbol when strictly inside) only depends on where the new column is in those OLD
// coordinates, because all earlier insertions of the same row lie at or before it.  So: one pass over the cigar
// (prefix counts by ballot), the row's symbols scattered into a per-column byte array, one shift of T / cnt / that
// array by "insertions at or before me", the new columns written, the row's symbols counted in.  Rows that meet the
// reference's corner cases -- leading insertions in front of base 0 (the cursor quirk above), insertions behind the
// last base, more than msa_max_ins() new columns -- take the step-by-step walk (msa_row_walk), which stays in the kernel and
// which one wavefront runs.
//
// What differs between one wavefront and several is behind three helpers, whose NW == 1 arms touch neither LDS nor a barrier:
//   WgXchg<NW>      a pass's running prefix across the wavefronts: each ballots its 64 entries and posts its counts; one wavefront
//                   gets its own counts back (nothing in front of it);
//   one_to_all<NW>  a value one thread has (the position found, the last op's column, the next ticket, the walk's outcome) to all:
//                   LDS words and a barrier, or readlane; as one_posts / all_fetch around a barrier that is there anyway;
//   msa_row_walk    the step walk in wavefront 0 while the others wait; in a workgroup of one wavefront that is everyone.
// Per (GLOBAL, NW), as constants of the body: the new columns a row may open on the passes (msa_max_ins), where the small arrays
// are (LDS, but the workspace slot for GLOBAL and one wavefront: that launch has no LDS), and how many chunks the right shift
// moves per barrier pair (1, or kShiftChunks with several wavefronts).
#include <hip/hip_runtime.h>

#include "dp_dev.h"
#include "dp_msa_layout.h"

namespace lrsc {

namespace {
constexpr uint32_t kGap = 4;
// per-column counters of A C G T '-' : five 12-bit fields of one 64-bit word (at most 4095 rows)
using Cnt = unsigned long long;
constexpr uint32_t kCntBits = 12;
constexpr uint32_t kUnset = 0xFEu;
__device__ __forceinline__ uint32_t cnt_get(Cnt v, uint32_t sym) { return (uint32_t)(v >> (kCntBits * sym)) & ((1u << kCntBits) - 1u); }

__device__ __forceinline__ uint32_t mbcnt(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// the exchange words (kXchgWords of them, NW > 1 only): two buffers of kXchgBuf, then the single values of one_to_all
constexpr uint32_t kXchgBuf = 32;
constexpr uint32_t kMbNext = 64, kMbTi = 65, kMbLastY = 66, kMbWalk = 67;   // kMbWalk .. + 3: lead_b, size_b, nout, overflow
constexpr uint32_t kShiftChunks = 4;                                // columns per thread and barrier pair in the right shift, NW > 1

// Where a pass carries a running prefix, every wavefront ballots its own 64 entries, posts its counts, and after one barrier every
// thread adds up the wavefronts in front of its own; the carry is the sum of all of them, so it stays the same in every thread of
// the workgroup, and so do the early exits.  One wavefront: the posted words are just handed back.
template <uint32_t NW>
struct WgXchg {
    uint32_t* w;
    uint32_t wv, lane, par;
    struct Posted {                        // the buffer of all wavefronts' words, or (one wavefront) its own three
        const uint32_t* buf; uint32_t x, y, z;
        __device__ __forceinline__ uint32_t own(uint32_t k) const { return k == 0 ? x : k == 1 ? y : z; }
    };
    // every wavefront posts up to three words (the same in all its lanes); what all of them can be read from afterwards
    __device__ __forceinline__ Posted all(uint32_t x, uint32_t y = 0, uint32_t z = 0)
    {
        if constexpr(NW == 1) return Posted{nullptr, x, y, z};
        else {
            uint32_t* buf = w + par * kXchgBuf;
            if(lane == 0) { buf[wv * 4] = x; buf[wv * 4 + 1] = y; buf[wv * 4 + 2] = z; }
            __syncthreads();
            par ^= 1u;
            return Posted{buf, 0u, 0u, 0u};
        }
    }
    // word k: the sum over the wavefronts in front of this one, and over all
    __device__ __forceinline__ void prefix(const Posted& p, uint32_t k, uint32_t& before, uint32_t& total) const
    {
        before = 0; total = 0;
        if constexpr(NW == 1) total = p.own(k);
        else {
#pragma unroll
            for(uint32_t x = 0; x < NW; ++x) { const uint32_t c = p.buf[x * 4 + k]; before += x < wv ? c : 0u; total += c; }
        }
    }
    // word k where it is a position (0: the wavefront has none): the last one in front of this wavefront, and of all; `carry` if none
    __device__ __forceinline__ void latest(const Posted& p, uint32_t k, uint32_t carry, uint32_t& before, uint32_t& last) const
    {
        before = carry; last = carry;
        if constexpr(NW == 1) { if(p.own(k)) last = p.own(k); }
        else {
#pragma unroll
            for(uint32_t x = 0; x < NW; ++x) {
                const uint32_t c = p.buf[x * 4 + k];
                if(c) { last = c; if(x < wv) before = c; }
            }
        }
    }
};

// One thread's values to every thread of the workgroup, in two halves so that a barrier the caller has anyway can stand between
// them: one_posts, a workgroup barrier, all_fetch.  Several wavefronts: through LDS words.  One wavefront: one_posts reads them from
// the lane that has them, all_fetch does nothing.  `mine` must hold in exactly one thread (in none, the source lane is undefined),
// every thread must get to both halves, and the same words must not be posted again before a barrier behind the fetch.
template <uint32_t NW, typename... V>
__device__ __forceinline__ void one_posts(uint32_t* words, bool mine, V&... v)
{
    if constexpr(NW == 1) {
        const int src = __builtin_ctzll(__ballot(mine));
        ((v = (uint32_t)__builtin_amdgcn_readlane((int)v, src)), ...);
    } else {
        uint32_t n = 0;
        if(mine) ((words[n++] = v), ...);
    }
}
template <uint32_t NW, typename... V>
__device__ __forceinline__ void all_fetch(const uint32_t* words, V&... v)
{
    if constexpr(NW > 1) {
        uint32_t n = 0;
        ((v = words[n++]), ...);
    }
}
// ... and both with a barrier of their own
template <uint32_t NW, typename... V>
__device__ __forceinline__ void one_to_all(uint32_t* words, bool mine, V&... v)
{
    one_posts<NW>(words, mine, v...);
    if constexpr(NW > 1) __syncthreads();
    all_fetch<NW>(words, v...);
}

// The step walk runs in one wavefront: its lanes' stores before, its own loads behind -- a workgroup fence and a wavefront barrier.
// In a workgroup of 64 threads that is what __syncthreads() gives.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The step-by-step cigar walk of one row, one dependent step per column, run by ONE wavefront: the whole workgroup, or wavefront 0 of
// several while the others wait at the barrier behind it.  To keep a step at register speed the next 64 bytes of the base row, of
// the cigar and of the incoming string sit one per lane in a register and are picked with v_readlane; the output symbols are
// collected the same way and counted into their columns 64 at a time.  Returns false when the pile-up's column capacity is exceeded.
__device__ __forceinline__ bool msa_row_walk(uint32_t lane, uint32_t W, Cnt* cnt, uint8_t* T, const uint8_t* ops, const uint8_t* S, uint32_t* lead,
                                             uint32_t* size, uint32_t n_el, uint32_t n_ops, uint32_t s2_len, uint32_t m1s, uint32_t ti, uint32_t tl,
                                             uint32_t& lead_b_io, uint32_t& size_b_io, uint32_t& nout_r, uint32_t& n_ins_io, uint64_t& t_ins_io)
{
    uint32_t lead_b = lead_b_io, size_b = size_b_io, n_ins = n_ins_io;      // copies: these stay in registers
    uint64_t t_ins = t_ins_io;
    const uint32_t op_last = n_ops - 1, il = ti + tl;
    uint32_t inc = m1s, cig = 0, nout = 0;
    uint32_t tb = 0xFFFFFF00u, ob = 0xFFFFFF00u, sb = 0xFFFFFF00u, Tw = 0, Ow = 0, Sw = 0, acc = 0;
    bool ok = true;
    auto getT = [&](uint32_t i) -> uint32_t {
        if(i - tb >= 64u) { tb = i; const uint32_t j = i + lane; Tw = j < size_b ? (uint32_t)T[j] : 0xFFu; }   // past the end: the string's NUL, not a gap
        return (uint32_t)__builtin_amdgcn_readlane((int)Tw, (int)(i - tb));
    };
    auto getO = [&](uint32_t i) -> uint32_t {
        if(i - ob >= 64u) { ob = i; const uint32_t j = i + lane; Ow = j < n_ops ? (uint32_t)ops[op_last - j] : 0u; }
        return (uint32_t)__builtin_amdgcn_readlane((int)Ow, (int)(i - ob));
    };
    auto getS = [&](uint32_t i) -> uint32_t {
        if(i - sb >= 64u) { sb = i; const uint32_t j = i + lane; Sw = j < s2_len ? (uint32_t)S[j] : 0u; }
        return (uint32_t)__builtin_amdgcn_readlane((int)Sw, (int)(i - sb));
    };
    auto flush = [&](uint32_t first, uint32_t n) {                  // outputs first .. first + n land in columns il + first ..
        const uint32_t col = il + first + lane;
        if(lane < n && col < W) cnt[col] += 1ull << (kCntBits * acc);
    };
    while(cig < n_ops) {
        ti = (uint32_t)__builtin_amdgcn_readfirstlane((int)ti);
        cig = (uint32_t)__builtin_amdgcn_readfirstlane((int)cig);
        inc = (uint32_t)__builtin_amdgcn_readfirstlane((int)inc);
        const uint32_t tsym = getT(ti);
        const uint32_t op = getO(cig);
        uint32_t sym;
        if(tsym == kGap) {
            if(op == 'I') { sym = getS(inc); ++inc; ++cig; }
            else sym = kGap;
        } else if(op == 'M') { sym = getS(inc); ++inc; ++cig; }
        else if(op == 'D') { sym = kGap; ++cig; }
        else {
            // insertGapBeforeColumn(template_index + template_leading) on every row (:1205-1211, :165-180)
            const uint64_t t_i0 = __builtin_readcyclecounter();
            ++n_ins;
            wave_sync();                                             // the flushes so far, before the columns move
            const uint32_t c = ti + tl;
            uint32_t ngap = 0;
            for(uint32_t e0 = 0; e0 < n_el; e0 += 64) {
                const uint32_t e = e0 + lane;
                bool inside = false;
                if(e < n_el) {
                    const uint32_t le = lead[e], se = size[e];
                    if(c <= le) lead[e] = le + 1;
                    else if(c - le < se) { size[e] = se + 1; inside = true; }
                }
                ngap += (uint32_t)__builtin_popcountll(__ballot(inside));
            }
            const uint32_t end_b = lead_b + size_b;                  // tracked columns: [0, end_b)
            bool base_inside = false;
            if(c <= lead_b) lead_b += 1;
            else if(c - lead_b < size_b) {
                base_inside = true;
                const uint32_t ip = c - lead_b;
                if(size_b + 1 > W) { ok = false; break; }
                for(uint32_t hi = size_b; hi > ip;) {                // T.insert(ip, '-')
                    const uint32_t n = hi - ip < 64 ? hi - ip : 64;
                    const uint32_t i = hi - 1 - lane;
                    uint8_t v = 0;
                    if(lane < n) v = T[i];
                    wave_sync();
                    if(lane < n) T[i + 1] = v;
                    wave_sync();
                    hi -= n;
                }
                if(lane == 0) T[ip] = (uint8_t)kGap;
                size_b += 1;
                tb = 0xFFFFFF00u;                                    // the register window of T is stale
            }
            if(c < end_b) {                                          // columns at / after c move right
                if(end_b + 1 > W) { ok = false; break; }
                for(uint32_t hi = end_b; hi > c;) {
                    const uint32_t n = hi - c < 64 ? hi - c : 64;
                    const uint32_t i = hi - 1 - lane;
                    Cnt v = 0;
                    if(lane < n) v = cnt[i];
                    wave_sync();
                    if(lane < n) cnt[i + 1] = v;
                    wave_sync();
                    hi -= n;
                }
            }
            if(c < W && lane == 0) cnt[c] = (Cnt)(ngap + (base_inside ? 1u : 0u)) << (kCntBits * kGap);
            wave_sync();
            t_ins += __builtin_readcyclecounter() - t_i0;
            sym = getS(inc); ++inc; ++cig;
        }
        if(nout >= W) { ok = false; break; }
        acc = lane == (nout & 63u) ? sym : acc;
        ++nout;
        if((nout & 63u) == 0) flush(nout - 64, 64);
        ++ti;
    }
    if(ok && (nout & 63u) != 0) flush(nout & ~63u, nout & 63u);
    lead_b_io = lead_b; size_b_io = size_b; nout_r = nout; n_ins_io = n_ins; t_ins_io = t_ins;
    return ok;
}

// One pile-up per workgroup of NT = 64 x NW threads; every pass strides by NT.
template <bool GLOBAL, uint32_t NW>
__device__ __forceinline__ void msa_pileup(const DpPipeArgs& a, uint8_t* smem_lds)
{
    constexpr uint32_t NT = 64u * NW, KI = msa_max_ins(GLOBAL, NW), SC = NW == 1 ? 1u : kShiftChunks;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = NW == 1 ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // MsaLayout's two groups of arrays: the small ones are in LDS unless one wavefront works in the global workspace, the per-column
    // ones in LDS or in the workgroup's workspace slot (a.lds_bytes each)
    uint8_t* slot = GLOBAL ? a.msa_ws + (uint64_t)blockIdx.x * a.lds_bytes : nullptr;
    uint8_t* small = (!GLOBAL || NW > 1) ? smem_lds : slot;
    uint8_t* cols = GLOBAL ? slot : smem_lds;
    uint32_t* xw = reinterpret_cast<uint32_t*>(small + msa_layout(0, 0, 0, 0, 0, NW, GLOBAL).xchg);
    WgXchg<NW> xc{xw, wv, lane, 0u};
    const uint32_t n_work = a.req_list ? a.n_list : a.n_reqs;
    for(uint32_t wi = blockIdx.x; wi < n_work;) {
        const uint32_t rq = a.req_list ? a.req_list[wi] : wi;
        // the next request: round-robin, or (work_ctr) whichever is next when this workgroup is done -- the lists come biggest first
        uint32_t ticket = 0;
        if(a.work_ctr) {
            if(tid == 0) ticket = gridDim.x + atomicAdd(a.work_ctr, 1u);
            one_posts<NW>(xw + kMbNext, tid == 0, ticket);                 // fetched behind the barrier in front of the base row, into
                                                                           // this variable: fetched into one that also held the atomic's
                                                                           // result, the compiler takes the request for divergent
        }
        const DpRequest R = a.reqs[rq];
        const uint64_t t_req0 = __builtin_readcyclecounter();
        uint64_t t_stage = 0, t_ins = 0;
        uint32_t n_ins = 0, n_walk = 0;
        const uint32_t W = R.w_cols, E = R.n_str + 2;
        const MsaLayout L = msa_layout(W, R.lq, R.str_cap, R.ops_cap, R.n_str, NW, GLOBAL);
        uint32_t* insx = reinterpret_cast<uint32_t*>(small + L.insx);
        uint16_t* insg = reinterpret_cast<uint16_t*>(small + L.insg);
        uint8_t* inss = small + L.inss;
        uint32_t* lead = reinterpret_cast<uint32_t*>(small + L.lead);
        uint32_t* size = reinterpret_cast<uint32_t*>(small + L.size);
        Cnt* cnt = reinterpret_cast<Cnt*>(cols + L.cnt);
        uint32_t* bpos = reinterpret_cast<uint32_t*>(cols + L.bpos);
        uint8_t* T = cols + L.T;
        uint8_t* Rw = cols + L.Rw;
        uint8_t* Sbase = cols + L.S;
        uint8_t* ops = cols + L.ops;
        __syncthreads();
        uint32_t wi_next = wi + gridDim.x;
        if(a.work_ctr) { all_fetch<NW>(xw + kMbNext, ticket); wi_next = ticket; }
        const uint8_t* q = a.codes + R.q_off;
        for(uint32_t c = tid; c < W; c += NT) {
            Cnt z = 0;
            if(c < R.lq) { T[c] = q[c]; z = 1ull << (kCntBits * q[c]); }
            cnt[c] = z;
        }
        __syncthreads();
        uint32_t lead_b = 0, size_b = R.lq, n_el = 0, n_rows = 1;
        bool overflow = false;

        DpAlignOut A_next{};
        DpJob J_next{};
        if(R.n_str) { A_next = a.align[R.job_first]; J_next = a.jobs[R.job_first]; }
        for(uint32_t s = 0; s < R.n_str && !overflow; ++s) {
            const DpAlignOut A = A_next;
            const DpJob J = J_next;
            if(s + 1 < R.n_str) { A_next = a.align[R.job_first + s + 1]; J_next = a.jobs[R.job_first + s + 1]; }   // in flight during this row
            if(!A.accept) continue;
            ++n_rows;
            const uint64_t t_s0 = __builtin_readcyclecounter();
            __syncthreads();
            // staged four bytes per thread; the string from the aligned address at or below its start
            const uint32_t so = (uint32_t)(J.s2_off & 3u);
            const uint8_t* S = Sbase + so;
            {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(a.strings + (J.s2_off - so));
                uint32_t* dst = reinterpret_cast<uint32_t*>(Sbase);
                for(uint32_t i = tid, n = (so + J.s2_len + 3) >> 2; i < n; i += NT) dst[i] = src[i];
                const uint32_t* osrc = reinterpret_cast<const uint32_t*>(a.ops + J.ops_off);
                uint32_t* odst = reinterpret_cast<uint32_t*>(ops);
                for(uint32_t i = tid, n = (A.n_ops + 3) >> 2; i < n; i += NT) odst[i] = osrc[i];
            }
            __syncthreads();
            const uint32_t op_last = A.n_ops - 1;                         // forward op j = ops[op_last - j]
            t_stage += __builtin_readcyclecounter() - t_s0;

            // getPaddedPositionOfBase(match[0].start): index in T of the match0_start-th non-gap symbol
            uint32_t ti = 0;
            {
                uint32_t seen = 0;
                const uint32_t want = (uint32_t)A.m0s;
                for(uint32_t base = 0; base < size_b; base += NT) {
                    const uint32_t i = base + tid;
                    const bool ng = i < size_b && T[i] != kGap;
                    const uint64_t m = __ballot(ng);
                    uint32_t before, nn;
                    xc.prefix(xc.all((uint32_t)__builtin_popcountll(m)), 0, before, nn);
                    if(seen + nn > want) {
                        ti = i;
                        one_to_all<NW>(xw + kMbTi, ng && seen + before + mbcnt(m) == want, ti);
                        break;
                    }
                    seen += nn;
                }
            }
            const uint32_t tl = lead_b;                         // template_leading, read once (:306)
            const uint32_t il = ti + tl;                        // incoming_leading
            bool batched = false;
            if(a.row_batch && A.n_ops > 0 && !(ti == 0 && ops[op_last] == 'I')) {
                const uint32_t ti0 = ti, m1s = (uint32_t)A.m1s;
                // bases from ti0 on, and the row's default symbol per position: '-' over a gap column, unset over a base
                uint32_t nbr = 0;
                for(uint32_t base = ti0; base < size_b; base += NT) {
                    const uint32_t i = base + tid;
                    const bool in = i < size_b;
                    const bool ng = in && T[i] != kGap;
                    const uint64_t m = __ballot(ng);
                    uint32_t before, nn;
                    xc.prefix(xc.all((uint32_t)__builtin_popcountll(m)), 0, before, nn);
                    if(ng) { const uint32_t b = nbr + before + mbcnt(m); if(b < R.lq + 1) bpos[b] = i; }
                    if(in) Rw[i] = ng ? (uint8_t)kUnset : (uint8_t)kGap;
                    nbr += nn;
                }
                bool bad = nbr > R.lq + 1;
                if(tid == 0 && !bad) bpos[nbr] = size_b;
                __syncthreads();
                uint32_t md_tot = 0, mi_tot = 0, st_tot = 0, run_carry = 0, last_y = 0;
                for(uint32_t cb = 0; cb < A.n_ops && !bad; cb += NT) {
                    const uint32_t j = cb + tid, wb = cb + wv * 64u;
                    const bool valid = j < A.n_ops;
                    const uint32_t op = valid ? (uint32_t)ops[op_last - j] : 0u;
                    const bool isM = op == 'M', isD = op == 'D', isI = op == 'I';
                    const uint64_t mMD = __ballot(isM || isD), mMI = __ballot(isM || isI);
                    // per wavefront: its M/D and M/I counts and the position behind its last M/D op (0: it has none)
                    const auto px = xc.all((uint32_t)__builtin_popcountll(mMD), (uint32_t)__builtin_popcountll(mMI),
                                           mMD ? wb + 64u - (uint32_t)__builtin_clzll(mMD) : 0u);
                    uint32_t md_before, md_all, mi_before, mi_all, carry_before, carry_all;
                    xc.prefix(px, 0, md_before, md_all);
                    xc.prefix(px, 1, mi_before, mi_all);
                    xc.latest(px, 2, run_carry, carry_before, carry_all);
                    const uint32_t brel = md_tot + md_before + mbcnt(mMD);
                    const uint32_t inc = m1s + mi_tot + mi_before + mbcnt(mMI);
                    const uint64_t lower = mMD & ((1ull << lane) - 1ull);
                    const uint32_t run_start = lower ? wb + 64u - (uint32_t)__builtin_clzll(lower) : carry_before;
                    const uint32_t i_rank = j - run_start;
                    bool lane_bad = valid && !(isM || isD || isI);
                    uint32_t y = 0, G = 0;
                    bool st = false, fill = false;
                    if((isM || isD) && brel >= nbr) lane_bad = true;
                    if(isI && brel >= nbr) lane_bad = true;                // behind the last base: the walk's job
                    if(!lane_bad && valid) {
                        const uint32_t pb = bpos[brel];
                        if(isI) {
                            if(brel > 0) { const uint32_t pp = bpos[brel - 1]; G = pb - pp - 1; y = pp + 1 + i_rank; }
                            fill = i_rank < G; st = !fill;
                            if(st) y = pb - 1;                              // last position consumed if the cigar ends here
                        } else y = pb;
                    }
                    const uint64_t mS = __ballot(st);
                    const auto ps = xc.all((uint32_t)__builtin_popcountll(mS), __ballot(lane_bad) ? 1u : 0u);
                    uint32_t st_before, st_all, bad_before, bad_all;
                    xc.prefix(ps, 0, st_before, st_all);
                    xc.prefix(ps, 1, bad_before, bad_all);
                    const uint32_t k = st_tot + st_before + mbcnt(mS);
                    // more than KI new columns: some op of this chunk has k >= KI exactly when the total passes it
                    if(bad_all || st_tot + st_all > KI) { bad = true; break; }
                    const uint32_t sym = (isM || isI) ? (inc < J.s2_len ? (uint32_t)S[inc] : 0u) : kGap;
                    if(isM || isD || fill) Rw[y] = (uint8_t)sym;
                    if(st) { insx[k] = y + 1; inss[k] = (uint8_t)sym; }
                    // the last op's y, fetched behind the loop's barrier.  Several wavefronts: stored by the thread that has it, in
                    // whichever chunk -- not one_posts under "the last chunk", which carries a register round the loop
                    if constexpr(NW > 1) { if(j == op_last) xw[kMbLastY] = y; }
                    else if(cb + NT >= A.n_ops) { last_y = y; one_posts<NW>(xw + kMbLastY, j == op_last, last_y); }
                    md_tot += md_all; mi_tot += mi_all; st_tot += st_all;
                    run_carry = carry_all;
                }
                __syncthreads();
                if(!bad) {
                    batched = true;
                    all_fetch<NW>(xw + kMbLastY, last_y);
                    const uint32_t nin = st_tot;
                    if(nin) {
                        const uint64_t t_i0 = __builtin_readcyclecounter();
                        n_ins += nin;
                        if(size_b + nin > W || lead_b + size_b + nin > W) { overflow = true; break; }
                        // rows showing a gap in each new column (strictly inside, old coordinates) ...
                        for(uint32_t k = tid; k < nin; k += NT) {
                            const uint32_t xg = insx[k] + tl;
                            uint32_t g = 0;
                            for(uint32_t e = 0; e < n_el; ++e) { const uint32_t le = lead[e], se = size[e]; g += (le < xg && xg - le < se) ? 1u : 0u; }
                            insg[k] = (uint16_t)g;
                        }
                        __syncthreads();
                        // ... then every row takes all of them at once
                        for(uint32_t e = tid; e < n_el; e += NT) {
                            const uint32_t le = lead[e], se = size[e];
                            uint32_t before = 0, inside = 0;
                            for(uint32_t k = 0; k < nin; ++k) {
                                const uint32_t xg = insx[k] + tl;
                                before += xg <= le ? 1u : 0u;
                                inside += (le < xg && xg - le < se) ? 1u : 0u;
                            }
                            lead[e] = le + before; size[e] = se + inside;
                        }
                        // T, cnt and the row's symbols move right by the number of new columns at or before them: from the top
                        // down, SC chunks of NT columns read, a barrier, and written -- a block's targets are its own columns and
                        // columns above it, which earlier blocks have read
                        const uint32_t x0 = insx[0];
                        for(uint32_t hi = size_b; hi > x0;) {
                            const uint32_t n = hi - x0 < NT * SC ? hi - x0 : NT * SC;
                            Cnt v[SC]; uint32_t t[SC], r[SC], sh[SC];
#pragma unroll
                            for(uint32_t c = 0; c < SC; ++c) {
                                const uint32_t idx = tid + c * NT;
                                v[c] = 0; t[c] = 0; r[c] = 0; sh[c] = 0;
                                if(idx < n) {
                                    const uint32_t yy = hi - 1 - idx;
                                    v[c] = cnt[yy + tl]; t[c] = T[yy]; r[c] = Rw[yy];
                                    uint32_t lo = 0, hi2 = nin;                  // upper_bound(insx, yy)
                                    while(lo < hi2) { const uint32_t mid = (lo + hi2) >> 1; if(insx[mid] <= yy) lo = mid + 1; else hi2 = mid; }
                                    sh[c] = lo;
                                }
                            }
                            __syncthreads();
#pragma unroll
                            for(uint32_t c = 0; c < SC; ++c) {
                                const uint32_t idx = tid + c * NT;
                                if(idx < n && sh[c]) { const uint32_t yy = hi - 1 - idx; cnt[yy + sh[c] + tl] = v[c]; T[yy + sh[c]] = (uint8_t)t[c]; Rw[yy + sh[c]] = (uint8_t)r[c]; }
                            }
                            __syncthreads();
                            hi -= n;
                        }
                        for(uint32_t k = tid; k < nin; k += NT) {
                            const uint32_t np = insx[k] + k;
                            T[np] = (uint8_t)kGap; Rw[np] = inss[k];
                            cnt[np + tl] = (Cnt)((uint32_t)insg[k] + 1u) << (kCntBits * kGap);
                        }
                        size_b += nin;
                        __syncthreads();
                        t_ins += __builtin_readcyclecounter() - t_i0;
                    }
                    const uint32_t nout = last_y + 1 - ti0 + nin;
                    if(nout > W) { overflow = true; break; }
                    for(uint32_t z = tid; z < nout; z += NT) {
                        const uint32_t sym = Rw[ti0 + z];
                        if(sym <= kGap && ti0 + z + tl < W) cnt[ti0 + z + tl] += 1ull << (kCntBits * sym);
                    }
                    __syncthreads();
                    if(n_el >= E) { overflow = true; break; }
                    if(tid == 0) { lead[n_el] = il; size[n_el] = nout; }
                    ++n_el;
                    __syncthreads();
                }
            }
            if(batched) continue;
            ++n_walk;
            // the step walk, in wavefront 0; its outcome to the others, which wait for it
            uint32_t nout = 0, over = 0;
            if(wv == 0)
                over = msa_row_walk(lane, W, cnt, T, ops, S, lead, size, n_el, A.n_ops, J.s2_len, (uint32_t)A.m1s, ti, tl, lead_b, size_b, nout,
                                    n_ins, t_ins) ? 0u : 1u;
            one_to_all<NW>(xw + kMbWalk, tid == 0, lead_b, size_b, nout, over);
            if(over) { overflow = true; break; }
            if(n_el >= E) { overflow = true; break; }
            if(tid == 0) { lead[n_el] = il; size[n_el] = nout; }
            ++n_el;
            __syncthreads();
        }

        // calculateBaseConsensus(min_call_coverage, -1) over the base row's columns
        uint32_t cons_len = 0;
        uint8_t* cons = a.cons + R.cons_off;
        if(!overflow) {
            for(uint32_t base = 0; base < size_b; base += NT) {
                const uint32_t i = base + tid;
                uint32_t sym = kGap;
                if(i < size_b && lead_b + i < W) {
                    const Cnt v = cnt[lead_b + i];
                    int max_count = -1; uint32_t max_symbol = 0;
#pragma unroll
                    for(uint32_t x = 0; x < 5; ++x)                         // "ACGT" then '-' ('N' never counted)
                        if((int)cnt_get(v, x) > max_count) { max_count = (int)cnt_get(v, x); max_symbol = x; }
                    const uint32_t base_symbol = T[i];
                    const int base_count = (int)cnt_get(v, base_symbol);
                    sym = (max_count >= base_count && base_count < R.min_call_coverage) ? max_symbol : base_symbol;
                }
                const bool keep = i < size_b && sym != kGap;
                const uint64_t m = __ballot(keep);
                uint32_t before, nn;
                xc.prefix(xc.all((uint32_t)__builtin_popcountll(m)), 0, before, nn);
                if(keep) {
                    const uint32_t pos = cons_len + before + mbcnt(m);
                    if(pos < R.cons_cap) cons[pos] = (uint8_t)sym;
                }
                cons_len += nn;
            }
            if(cons_len > R.cons_cap) { overflow = true; cons_len = 0xFFFFFFFFu; }
        }
        if(tid == 0) {
            DpMsaOut o;
            o.n_rows = n_rows; o.cons_len = overflow ? 0 : cons_len; o.error = !overflow ? 0u : cons_len == 0xFFFFFFFFu ? 2u : 1u; o.pad = n_walk;
            o.kc_total = (uint32_t)((__builtin_readcyclecounter() - t_req0) >> 10); o.kc_stage = (uint32_t)(t_stage >> 10);
            o.kc_insert = (uint32_t)(t_ins >> 10); o.n_insert = n_ins;
            a.msa[rq] = o;
        }
        wi = wi_next;
    }
}
} // namespace

uint32_t dp_msa_small_bytes(uint32_t n_str) { return msa_layout(0, 0, 0, 0, n_str, 2, true).small_total; }

uint32_t dp_msa_lds_bytes(uint32_t w_cols, uint32_t lq, uint32_t str_cap, uint32_t ops_cap, uint32_t n_str, uint32_t nw)
{
    return msa_layout(w_cols, lq, str_cap, ops_cap, n_str, nw, false).total;
}

// GLOBAL = false: state in LDS (dynamic, a.lds_bytes); true: the per-column state in a global workspace slot per workgroup, for the
// few pile-ups too wide for 160 KB.  NW: wavefronts per workgroup (1 for the many narrow pile-ups).
template <bool GLOBAL, uint32_t NW>
__global__ __launch_bounds__(64 * NW) void dp_msa_kernel(DpPipeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_lds[];
    msa_pileup<GLOBAL, NW>(a, smem_lds);
}

uint32_t dp_msa_waves(const DpPipeArgs& a, bool global, uint32_t lds_per_cu)
{
    int cus = 256, dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    uint32_t per_cu = global ? 8u : (a.lds_bytes ? lds_per_cu / a.lds_bytes : 16u);
    if(global && a.msa_nw > 1 && a.lds_small) per_cu = per_cu < lds_per_cu / a.lds_small ? per_cu : lds_per_cu / a.lds_small;   // its small arrays are LDS
    per_cu = per_cu < 1 ? 1 : per_cu > 32 ? 32 : per_cu;
    if(a.msa_nw > 1 && per_cu > 28u / a.msa_nw) per_cu = 28u / a.msa_nw;
    uint32_t n_waves = (uint32_t)cus * per_cu;
    const uint32_t n_work = a.req_list ? a.n_list : a.n_reqs;
    return n_waves > n_work ? n_work : n_waves;
}

namespace {
template <bool GLOBAL, uint32_t NW>
hipError_t launch_msa_as(const DpPipeArgs& a, uint32_t grid, uint32_t lds, hipStream_t stream)
{
    if(lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dp_msa_kernel<GLOBAL, NW>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if(e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((dp_msa_kernel<GLOBAL, NW>), dim3(grid), dim3(64 * NW), lds, stream, a);
    return hipGetLastError();
}

template <bool GLOBAL>
hipError_t launch_msa_nw(const DpPipeArgs& a, uint32_t grid, uint32_t lds, hipStream_t stream)
{
    switch(a.msa_nw) {
    case 1: return launch_msa_as<GLOBAL, 1>(a, grid, lds, stream);
    case 2: return launch_msa_as<GLOBAL, 2>(a, grid, lds, stream);
    case 4: return launch_msa_as<GLOBAL, 4>(a, grid, lds, stream);
    case 8: return launch_msa_as<GLOBAL, 8>(a, grid, lds, stream);
    default: return hipErrorInvalidValue;
    }
}
} // namespace

hipError_t launch_dp_msa(const DpPipeArgs& a, uint32_t lds_per_cu, hipStream_t stream)
{
    const uint32_t n_work = a.req_list ? a.n_list : a.n_reqs;
    if(n_work == 0) return hipSuccess;
    // global-workspace variant: a.lds_bytes = bytes per workgroup slot; several wavefronts keep the small arrays in LDS
    if(a.msa_ws) return launch_msa_nw<true>(a, dp_msa_waves(a, true, lds_per_cu), a.msa_nw > 1 ? a.lds_small : 0u, stream);
    if(a.lds_bytes > kLdsPerCu) return hipErrorInvalidValue;
    return launch_msa_nw<false>(a, dp_msa_waves(a, false, lds_per_cu), a.lds_bytes, stream);
}

} // namespace lrsc
