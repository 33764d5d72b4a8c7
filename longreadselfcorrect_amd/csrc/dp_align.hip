// dp_align.hip -- Overlapper::extendMatch (Thirdparty/overlapper.cpp:421-701) on the device: banded
// semi-global DP (band 201 around the seed diagonal, scores +1 / -1 / -8 at the call site,
// LongReadOverlap.cpp:635-643) plus the homopolymer-aware traceback, one WAVEFRONT per alignment.
//
// Fill: columns (s1 = the query) are processed in order; the <= 255 cells of a band column live four per
// lane in registers.  The in-column dependency cell[j] = max(A[j], cell[j-1] + gap) is a prefix maximum of
// A[j] - gap*j, so a column costs one wave scan instead of a serial chain.  The reference's quirks are kept:
// the first computed row of a column ignores "up", the last computed row ignores "left" (:476,:506-512),
// never-written cells read as 0.  Cells are stored with gap*(band row) already subtracted, and the columns run
// in turns of four, each turn in the code of its class (outside the matrix / interior / cut by a matrix edge):
// straight-line code under wave-uniform branches only (dp_column).
// Traceback: which neighbour the traceback takes at a cell (:604-661) depends only on that cell: its score against the three
// neighbour scores as _getBandedCellScore sees them, the two homopolymer tests and the mismatch test.  The last three are functions of
// the two sequences alone, so the fill stores only the two score comparisons the decision can need -- 2 bits per cell, one 64-byte line
// per column -- and the traceback, which visits a few hundred of a matrix's tens of thousands of cells, finishes the decision at the
// cells it walks: trace words 16 columns per fetch, sequence characters in windows across the lanes.
#include <hip/hip_runtime.h>

#include "dp_dev.h"

namespace lrsc {

namespace {
constexpr int kNeg = -(1 << 29);
constexpr int kIntMin = -2147483647 - 1;
constexpr uint32_t kS2Pad = 264;

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// DPP moves (GFX9 encodings): row_shr:n = 0x110 + n, row_bcast:15 = 0x142, row_bcast:31 = 0x143, wave_shl:1 = 0x130,
// wave_shr:1 = 0x138.  Lanes without a source (and rows masked out) receive `old`.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp(int old, int x) { return __builtin_amdgcn_update_dpp(old, x, CTRL, ROW_MASK, 0xF, false); }

// inclusive prefix max over the wave (lane order): Kogge-Stone inside each row of 16, then two row broadcasts; a lane without a
// source takes the maximum with the identity, which lets each step be one v_max_i32 with a DPP operand
__device__ __forceinline__ int wave_prefix_max(int x)
{
    x = imax(x, dpp<0x111>(kIntMin, x));
    x = imax(x, dpp<0x112>(kIntMin, x));
    x = imax(x, dpp<0x114>(kIntMin, x));
    x = imax(x, dpp<0x118>(kIntMin, x));
    x = imax(x, dpp<0x142, 0xA>(kIntMin, x));
    x = imax(x, dpp<0x143, 0xC>(kIntMin, x));
    return x;
}
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) { return (uint64_t)uni((uint32_t)(x >> 32)) << 32 | uni((uint32_t)x); }
__device__ __forceinline__ int lane_below(int old, int x) { return dpp<0x138>(old, x); }     // value of lane - 1
__device__ __forceinline__ int lane_above(int old, int x) { return dpp<0x130>(old, x); }     // value of lane + 1

// The traceback's choice at a cell (overlapper.cpp:604-661) as the reference's decision tree: 0 = M, 1 = M over a mismatch, 2 = I, 3 = D.
constexpr uint32_t dp_dir_tree(bool eq_diag, bool eq_up, bool eq_left, bool h1, bool h2, bool mismatch)
{
    uint32_t dir = 0;
    if(h2) dir = eq_up ? 2u : eq_left ? 3u : 0u;
    else if(h1) dir = eq_left ? 3u : eq_up ? 2u : 0u;
    else dir = eq_diag ? 0u : eq_left ? 3u : 2u;
    if(dir == 0u && mismatch) dir = 1u;
    return dir;
}
// What the fill stores of it (dp_column): B = eq_left, and A = the one of eq_up / eq_diag the tree can ask for at this cell: eq_up where a
// homopolymer test holds, eq_diag where neither does.  The traceback has h1, h2 and mismatch from the sequences and finishes the choice.
constexpr uint32_t dp_dir_finish(bool A, bool B, bool h1, bool h2, bool mismatch)
{
    uint32_t dir = 0;
    if(h2) dir = A ? 2u : B ? 3u : 0u;
    else if(h1) dir = B ? 3u : A ? 2u : 0u;
    else dir = A ? 0u : B ? 3u : 2u;
    if(dir == 0u && mismatch) dir = 1u;
    return dir;
}
constexpr bool dp_dir_finish_matches_tree()
{
    for(uint32_t m = 0; m < 64; ++m) {
        const bool d = m & 1, u = m & 2, l = m & 4, h1 = m & 8, h2 = m & 16, x = m & 32;
        if(dp_dir_tree(d, u, l, h1, h2, x) != dp_dir_finish((h1 | h2) ? u : d, l, h1, h2, x)) return false;
    }
    return true;
}
static_assert(dp_dir_finish_matches_tree(), "the traceback's decision from the two stored comparisons differs from the reference's tree");
// The traceback's step, dp_dir_finish without the mismatch (which only turns M into M over a mismatch), as a table of 16 two-bit
// entries indexed by A | B << 1 | h1 << 2 | h2 << 3: bit 0 = ti steps back, bit 1 = tj steps back, so 3 = M, 2 = I, 1 = D.  One shift on
// the traceback's serial chain.
constexpr uint32_t dp_step_table()
{
    uint32_t tab = 0;
    for(uint32_t m = 0; m < 16; ++m) {
        const uint32_t dir = dp_dir_finish(m & 1, m & 2, m & 4, m & 8, false);
        tab |= (dir == 0u ? 3u : dir == 2u ? 2u : 1u) << (2 * m);
    }
    return tab;
}
constexpr uint32_t kDpStepTable = dp_step_table();

// What a lane knows about its four band rows r0 .. r0 + 3 for the whole launch.
struct DpLane {
    int r0;
    int zero[4];                  // a never-written cell in the form the fill keeps (see dp_column): score 0 in the band, kNeg above it
    bool top1, top3;              // row r0 + 1 / r0 + 3 is row bw, the first above the band (bw is odd)
};
struct DpScores { int ms, mx, g, g2; };

// Columns K .. of a turn of four.  Cells are kept BIASED: H[t] = score - gap * r for band row r = r0 + t.  A cell's diagonal neighbour
// has the same r in the previous column and its left neighbour r + 1, so diag = Hp[t] + match/mismatch and left = Hp[t + 1] + 2 gap in
// biased form, the in-column chain cell[j] = max(A[j], cell[j - 1] + gap) is a plain prefix maximum, and "came from above" is
// Hc[t] == Hc[t - 1].  Row bw, just above the band, is kept at kNeg in every column: row bw - 1 then never takes "left" and never equals
// it, which is the reference's r + 1 < bw test; rows beyond hold values nothing reads.  Row 0 compares "up" with kIntMin.
// EDGE = false: an interior column (band rows 0 .. bw - 1 all inside the matrix, row L2 not among them): every band row is computed, the
// first is row 0 and the last row bw - 1.  EDGE = true: rows [rlo, rhi) are computed (wave-uniform; empty = a skipped column); rlast is
// the last of them unless it is also the first, else -1: the row that ignores "left" (overlapper.cpp:476,:506-512; the first computed
// row never takes "up" because the rows below it are masked out of the scan).
// c1 / h1: this column's s1 character and its homopolymer test (wave-uniform); e[K .. K + 4]: s2 characters of rows r0 .. r0 + 4;
// h2[K + t]: e[K + t] == e[K + t + 1].  Returns the lane's four 2-bit traceback codes, A | B << 1 of dp_dir_finish.
// The codes of rows outside [rlo, rhi) (and of rows >= bw) are whatever the comparisons give: the traceback reads a code only at a cell
// (ti, tj) with 1 <= tj <= L2 and band row 0 <= tj - jb < bw (it stops with `bad` outside the band), and [rlo, rhi) is exactly the band
// rows r of the column with 1 <= jb + r <= L2.  For the same reason the zero line of a column whose band lies outside the matrix (the
// first class of a turn) is never read: no row of such a column has 1 <= j <= L2.  That matters now: a code of 0 is no neutral "M"
// any more, it reads as "I" where neither homopolymer test holds.
template <bool EDGE, int K>
__device__ __forceinline__ uint32_t dp_column(const DpLane& C, const DpScores& sc, const int (&Hp)[4], int (&Hc)[4], uint32_t c1, bool h1,
                                              const uint32_t (&e)[8], const bool (&h2)[7], int rlo, int rhi, int rlast)
{
    const int hp4 = lane_above(0, Hp[0]);
    int diag[4], leftg[4], B[4];
    bool inr[4], mis[4];
#pragma unroll
    for(int t = 0; t < 4; ++t) {
        const int r = C.r0 + t;
        mis[t] = c1 != e[K + t];
        diag[t] = Hp[t] + (mis[t] ? sc.mx : sc.ms);
        leftg[t] = (t < 3 ? Hp[t + 1] : hp4) + sc.g2;
        if(EDGE) {
            inr[t] = (r >= rlo) & (r < rhi);
            const int A = imax(diag[t], r == rlast ? kNeg : leftg[t]);
            B[t] = inr[t] ? A : kNeg;
        } else {
            B[t] = imax(diag[t], leftg[t]);
        }
    }
    const int p0 = B[0], p1 = imax(p0, B[1]), p2 = imax(p1, B[2]), p3 = imax(p2, B[3]);
    const int incl = wave_prefix_max(p3);
    const int excl = lane_below(kNeg, incl);
    const int P[4] = {imax(p0, excl), imax(p1, excl), imax(p2, excl), imax(p3, excl)};
#pragma unroll
    for(int t = 0; t < 4; ++t) Hc[t] = EDGE ? (inr[t] ? P[t] : C.zero[t]) : P[t];
    if(!EDGE) { Hc[1] = C.top1 ? kNeg : Hc[1]; Hc[3] = C.top3 ? kNeg : Hc[3]; }
    const int below = lane_below(kIntMin, Hc[3]);               // band row r0 - 1 of this column
    uint32_t flags = 0;
#pragma unroll
    for(int t = 0; t < 4; ++t) {
        const int up = t > 0 ? Hc[t - 1] : below;
        const bool eq_a = Hc[t] == ((h1 | h2[K + t]) ? up : diag[t]);
        const bool eq_left = Hc[t] == leftg[t];
        flags |= (eq_a ? 1u << (2 * t) : 0u) | (eq_left ? 2u << (2 * t) : 0u);
    }
    return flags;
}

// Column K of a turn whose band is cut by the first or the last matrix row, or holds the matrix's last row (whose best cell the
// traceback may start from): the computed rows follow from the column's first matrix row jb.
struct DpEdge { int jb0, num_rows, bw, L2, i; };
template <int K>
__device__ __forceinline__ void dp_edge_column(const DpLane& C, const DpScores& sc, const DpEdge& E, const int (&Hp)[4], int (&Hc)[4],
                                               const uint32_t (&c)[5], const bool (&h1)[4], const uint32_t (&e)[8], const bool (&h2)[7],
                                               uint8_t* tr, int& best_row_val, int& best_row_i)
{
    const int jb = E.jb0 + K;
    const int rlo = jb < 1 ? 1 - jb : 0;
    const int rhi = E.num_rows - jb < E.bw ? E.num_rows - jb : E.bw;
    const int rlast = rhi - 1 != rlo ? rhi - 1 : -1;
    tr[K * kDpTraceStride] = (uint8_t)dp_column<true, K>(C, sc, Hp, Hc, c[K], h1[K], e, h2, rlo, rhi, rlast);
    const int rl = E.L2 - jb;                                   // band row of the matrix's last row
    if(rl >= 0 && rl < E.bw) {                                  // (wave-uniform: its best cell is tracked in scalar registers)
        const int ln = rl >> 2, ts = rl & 3;
        const int h = ts == 0 ? __builtin_amdgcn_readlane(Hc[0], ln) : ts == 1 ? __builtin_amdgcn_readlane(Hc[1], ln)
                    : ts == 2 ? __builtin_amdgcn_readlane(Hc[2], ln) : __builtin_amdgcn_readlane(Hc[3], ln);
        const int v = h + sc.g * rl;
        if(v > best_row_val) { best_row_val = v; best_row_i = E.i + K; }
    }
}
// The next ticket of a wavefront that has had its first (its block index): tickets from the grid size on come from the launch's head
// word, one relaxed device-scope add by one lane.  An alignment takes hundreds of microseconds, so one word per launch is far from
// its limit, and nothing is ordered by the add: every alignment reads only what earlier launches wrote.
__device__ __forceinline__ uint32_t dp_next_ticket(uint32_t* head)
{
    uint32_t t = 0;
    if(threadIdx.x == 0) t = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return gridDim.x + uni(t);
}
__device__ __forceinline__ void dp_copy(int (&dst)[4], const int (&src)[4])
{
#pragma unroll
    for(int t = 0; t < 4; ++t) dst[t] = src[t];
}
} // namespace

// amdgpu_waves_per_eu(8): the kernel is sized for eight wavefronts per SIMD, i.e. 64 VGPRs, and says so: left to itself the register
// allocator took 66 in the global variant.  tests/test_align_kernel_build.py holds that the limit costs no scratch and no spills.
template <bool GLOBAL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void dp_align_kernel(DpAlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    // the two sequences are staged in LDS, or -- for the few alignments beyond it -- in this wavefront's slice of a global workspace
    uint8_t* smem = GLOBAL ? a.seq_ws + (uint64_t)blockIdx.x * a.seq_ws_stride : lds;
    uint8_t* S1 = smem;                                        // s1 codes, S1[L1] = 4 (the string's NUL)
    const uint32_t tid = threadIdx.x;
    uint8_t* trace = a.trace + (uint64_t)blockIdx.x * a.trace_stride;
    const int half = (int)a.band_width / 2;
    const int bw = 2 * half + 1;
    const DpScores sc = {a.match_score, a.mismatch_penalty, a.gap_penalty, 2 * a.gap_penalty};
    const int g = sc.g;
    const int r0 = 4 * (int)tid;
    DpLane C;
    C.r0 = r0; C.top1 = r0 + 1 == bw; C.top3 = r0 + 3 == bw;
#pragma unroll
    for(int t = 0; t < 4; ++t) {
        const int r = r0 + t;
        C.zero[t] = r < bw ? -g * r : kNeg;
    }

    // The launch's alignments are a.list: the jobs of its staging-size class (dp_order.h).  A wavefront's first ticket is its block index, so that the
    // launch does not open with every wavefront at the head word; each further one is drawn when the alignment before it is done,
    // so a wavefront that met long alignments, or shares its CU with another kernel, takes fewer.
    for(uint32_t ticket = blockIdx.x; ticket < a.n_list; ticket = dp_next_ticket(a.head)) {
        const uint32_t job = uni(a.list[ticket]);
        // (the lane number is made opaque here and before the traceback: addresses derived from it are then formed where they are used and
        //  do not stay in registers through the fill)
        uint32_t lane = tid;
        asm volatile("" : "+v"(lane));
        DpJob J = a.jobs[job];                                     // the same for every lane: keep it in scalar registers
        J.s1_off = uni64(J.s1_off); J.s2_off = uni64(J.s2_off); J.ops_off = uni64(J.ops_off);
        J.s1_len = uni(J.s1_len); J.s2_len = uni(J.s2_len); J.start1 = (int32_t)uni((uint32_t)J.start1); J.start2 = (int32_t)uni((uint32_t)J.start2);
        J.mode = uni(J.mode); J.req = uni(J.req);
        DpAlignOut o;
        o.m0s = 0; o.m0e = -1; o.m1s = 0; o.m1e = -1; o.score = -1; o.edit_distance = -1; o.total_columns = -1; o.n_ops = 0;
        o.accept = 0; o.skipped = 1; o.t_fill = 0; o.t_trace = 0; o.t_trips = 0; o.wave = blockIdx.x;
        const uint64_t t_job0 = __builtin_readcyclecounter();
        if(J.s1_len == 0 || J.s2_len == 0) {
            if(lane == 0) a.out[job] = o;
            continue;
        }
        const int L1 = (int)J.s1_len, L2 = (int)J.s2_len;
        // s2 codes at S2[0 .. L2), sentinel 4 in the kS2Pad bytes before and the 16 after: the twelve aligned bytes that hold a lane's
        // characters s2[j - 1 .. j + 6] of four columns can then be read for any band position
        uint8_t* S2buf = smem + (((uint32_t)L1 + 2 + 3) & ~3u);
        uint8_t* S2 = S2buf + kS2Pad;
        __syncthreads();
        if(GLOBAL) __threadfence_block();
        for(uint32_t i = lane; i < kS2Pad; i += 64) S2buf[i] = 4;
        for(int i = (int)lane; i <= L1; i += 64) S1[i] = i < L1 ? a.codes[J.s1_off + i] : (uint8_t)4;
        for(int j = (int)lane; j < L2 + 16; j += 64) S2[j] = j < L2 ? a.strings[J.s2_off + j] : (uint8_t)4;
        __syncthreads();
        if(GLOBAL) __threadfence_block();
        if(J.mode != 0 && L2 >= L1) {                              // identical sequence from the forward / backward extension
            const int shift = J.mode == 1 ? 0 : L2 - L1;
            bool diff = false;
            for(int i = (int)lane; i < L1; i += 64) diff = diff || S1[i] != S2[shift + i];
            if(__ballot(diff) == 0) {
                if(lane == 0) a.out[job] = o;
                continue;
            }
        }
        o.skipped = 0;

        const int origin = (J.start2 - J.start1 + 1) - (half + 1);
        const int num_rows = L2 + 1;
        int best_row_val = kIntMin, best_row_i = 0;
        int H[4], T[4];
#pragma unroll
        for(int t = 0; t < 4; ++t) H[t] = C.zero[t];
        const uint32_t* S1w = reinterpret_cast<const uint32_t*>(S1);
        const uint32_t s2_shift = (uint32_t)origin & 3u;            // byte offset of a lane's first character in its aligned window: the
                                                                    // window starts at origin + i - 1 + 4 lane + kS2Pad with i = 1 (mod 4)
        const int s2_last = (int)kS2Pad + ((L2 + 4) & ~3);          // last window start whose twelve bytes are staged

        // four columns per turn: i = 1 (mod 4), so their s1 characters are one aligned dword (plus one byte for the last h1) and a
        // lane's s2 characters one 8-byte window that moves by a byte per column
        for(int i = 1; i <= L1; i += 4) {
            const int n = L1 - i + 1 < 4 ? L1 - i + 1 : 4;
            const int jb0 = origin + i;                             // first matrix row of the band in the first of the columns
            uint8_t* tr = trace + (uint64_t)i * kDpTraceStride + lane;
            if(n == 4 && (jb0 + 3 + bw <= 1 || jb0 >= num_rows)) {  // the band lies outside the matrix in all four: cells read as 0
                                                                    // (codes the traceback never reads, see dp_column)
#pragma unroll
                for(int k = 0; k < 4; ++k) tr[k * kDpTraceStride] = 0;
#pragma unroll
                for(int t = 0; t < 4; ++t) H[t] = C.zero[t];
                continue;
            }
            uint32_t c[5];
            bool h1[4];
            {
                const uint32_t w0 = uni(S1w[(i - 1) >> 2]);
                const int nxt = (i + 3) >> 2 < L1 >> 2 ? (i + 3) >> 2 : L1 >> 2;      // only a full turn looks at its byte
                const uint32_t w1 = uni(S1w[nxt]);
#pragma unroll
                for(int k = 0; k < 4; ++k) c[k] = (w0 >> (8 * k)) & 0xFFu;
                c[4] = w1 & 0xFFu;
#pragma unroll
                for(int k = 0; k < 4; ++k) h1[k] = c[k] == c[k + 1];
            }
            uint32_t e[8];
            bool h2[7];
            {
                // lanes whose window is clamped have no row inside the matrix in any of the four columns
                int b = jb0 + r0 - 1 + (int)kS2Pad;
                b = (b < 0 ? 0 : b) & ~3;
                b = b > s2_last ? s2_last : b;
                const uint32_t* p32 = reinterpret_cast<const uint32_t*>(S2buf + b);
                const uint32_t d0 = p32[0], d1 = p32[1], d2 = p32[2];
                const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, s2_shift), hi = __builtin_amdgcn_alignbyte(d2, d1, s2_shift);
#pragma unroll
                for(int m = 0; m < 4; ++m) { e[m] = (lo >> (8 * m)) & 0xFFu; e[4 + m] = (hi >> (8 * m)) & 0xFFu; }
#pragma unroll
                for(int m = 0; m < 7; ++m) h2[m] = e[m] == e[m + 1];
            }
            if(n == 4 && jb0 >= 1 && jb0 + 3 + bw <= L2) {
                tr[0 * kDpTraceStride] = (uint8_t)dp_column<false, 0>(C, sc, H, T, c[0], h1[0], e, h2, 0, 0, 0);
                tr[1 * kDpTraceStride] = (uint8_t)dp_column<false, 1>(C, sc, T, H, c[1], h1[1], e, h2, 0, 0, 0);
                tr[2 * kDpTraceStride] = (uint8_t)dp_column<false, 2>(C, sc, H, T, c[2], h1[2], e, h2, 0, 0, 0);
                tr[3 * kDpTraceStride] = (uint8_t)dp_column<false, 3>(C, sc, T, H, c[3], h1[3], e, h2, 0, 0, 0);
                continue;
            }
            // the band is cut by the first or the last matrix row, or the last row of the matrix (whose best cell the traceback may
            // start from) is inside it
            const DpEdge E = {jb0, num_rows, bw, L2, i};
            dp_edge_column<0>(C, sc, E, H, T, c, h1, e, h2, tr, best_row_val, best_row_i);
            if(n == 1) dp_copy(H, T);
            else {
                dp_edge_column<1>(C, sc, E, T, H, c, h1, e, h2, tr, best_row_val, best_row_i);
                if(n > 2) {
                    dp_edge_column<2>(C, sc, E, H, T, c, h1, e, h2, tr, best_row_val, best_row_i);
                    if(n == 3) dp_copy(H, T);
                    else dp_edge_column<3>(C, sc, E, T, H, c, h1, e, h2, tr, best_row_val, best_row_i);
                }
            }
        }

        // best of the last column (rows ascending, first maximum wins) and of the last row (columns ascending)
        int best_col_val = kIntMin, best_col_j = 0;
        {
            const int jbase = origin + L1;
#pragma unroll
            for(int t = 0; t < 4; ++t) {
                const int r = r0 + t, j = jbase + r;
                const int v = H[t] + g * r;
                if(r < bw && j >= 1 && j <= L2 && v > best_col_val) { best_col_val = v; best_col_j = j; }
            }
        }
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1) {
            const int ov = __shfl_xor(best_col_val, d), oj = __shfl_xor(best_col_j, d);
            if(ov > best_col_val || (ov == best_col_val && ov != kIntMin && oj < best_col_j)) { best_col_val = ov; best_col_j = oj; }
        }
        int ti, tj;
        if(best_col_val > best_row_val) { ti = L1; tj = best_col_j; o.score = best_col_val; }
        else { ti = best_row_i; tj = L2; o.score = best_row_val; }
        ti = __builtin_amdgcn_readfirstlane(ti);
        tj = __builtin_amdgcn_readfirstlane(tj);
        o.m0e = ti - 1; o.m1e = tj - 1;
        o.edit_distance = 0;

        // ---- traceback ----------------------------------------------------------------------------------------
        const uint64_t t_job1 = __builtin_readcyclecounter();
        asm volatile("" : "+v"(lane));
        __threadfence();
        uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        int wb = -1;                                                // first column of the 16-column window held in w0..w3
        uint32_t wcur = 0, key = ~0u;                               // the one of w0..w3 that holds band rows 16 d ..: key = wb | d
        // the sequence tests of a cell come from two windows across the lanes (the fill's indexing: h1 = c[k] == c[k + 1]
        // with c[k] = S1[i - 1]; h2 = e == e' and mismatch = c[k] != e with e = S2[j - 1], e' = S2[j]; S1[L1] = 4, S2[j >= L2] = 4):
        uint32_t v1 = 0;                                            // lane l, column i = wb + (l >> 2): S1[i - 1] << 4 | h1 << 2; loaded with w0..w3
        uint32_t v2 = 0;                                            // lane l, row j = s2_base + l + 1: S2[j - 1] << 4 | h2 << 3
        int s2_base = 0x40000000;
        uint32_t acc = 0, n_ops = 0, trips = 0;
        uint8_t* ops = a.ops + J.ops_off;
        bool bad = false;
        // One trip takes a whole run of M steps and the I or D step behind it.  A diagonal step keeps the band row r, so the cells an M
        // run would visit from (ti, tj) lie in the window's columns wb + c, c = col, col - 1, ..., at row tj - (col - c), and the lane
        // (c << 2 | r >> 6) that holds the code of (wb + c, r) finishes the decision of that cell: all 16 at once, each as if the walk
        // stood there.  The walk does stand there exactly as long as every cell before it said M, so the steps are the serial walk's.
        while(ti > 0 && tj > 0) {
            const int r = tj - origin - ti;
            if((uint32_t)r >= (uint32_t)bw) { bad = true; break; }
            const uint32_t k = (uint32_t)(ti & ~15) | (((uint32_t)r >> 4) & 3u);
            if(k != key) {                                          // every few steps: another 16 columns, or another 16 rows of the band
                key = k;
                if((ti & ~15) != wb) {
                    wb = ti & ~15;
                    const uint32_t* src = reinterpret_cast<const uint32_t*>(trace + (uint64_t)(wb + (int)(lane >> 2)) * kDpTraceStride + (lane & 3u) * 16u);
                    w0 = __hip_atomic_load(src + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    w1 = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    w2 = __hip_atomic_load(src + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    w3 = __hip_atomic_load(src + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    int x = wb + (int)(lane >> 2);                  // a column is taken at 1 <= i <= L1; the others stay inside S1[0 .. L1]
                    x = x < 1 ? 1 : x > L1 ? L1 : x;
                    const uint32_t c_prev = S1[x - 1], c_here = S1[x];
                    v1 = c_prev << 4 | (c_prev == c_here ? 4u : 0u);
                }
                const uint32_t d = k & 3u;
                wcur = d == 0 ? w0 : d == 1 ? w1 : d == 2 ? w2 : w3;
            }
            if((uint32_t)(tj - 1 - s2_base) > 63u) {                // every 64 rows
                s2_base = tj - 64;                                  // S2[tj - 64 .. tj] lies in [-63, L2]: staged (pad before, 4 from S2[L2] on)
                const uint8_t* p = S2 + (s2_base + (int)lane);
                const uint32_t e_prev = p[0], e_here = p[1];
                v2 = e_prev << 4 | (e_prev == e_here ? 8u : 0u);
            }
            ++trips;
            const uint32_t col = (uint32_t)(ti - wb), t0 = (uint32_t)(tj - 1 - s2_base);
            // the lane's cell: column wb + (lane >> 2), whose row tj - (col - (lane >> 2)) lane t0 - (col - (lane >> 2)) of v2 holds (a lane
            // index that wraps belongs to a cell beyond `lim` below).  Bits 2, 3 of x: h1, h2; above them the two characters' difference.
            const uint32_t ab = (wcur >> (2 * ((uint32_t)r & 15u))) & 3u;
            const uint32_t x = v1 ^ (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane & ~3u) + 4u * (t0 - col)), (int)v2);
            const uint32_t step = (kDpStepTable >> (2 * (ab | (x & 12u)))) & 3u;                      // 3 = M, 2 = I, 1 = D
            // the cells' answers in walk order from bit 63 down, one per four bits: the lanes of band rows 64 (r >> 6) ..
            const uint32_t up = 63u - (col << 2 | (uint32_t)r >> 6);
            const uint64_t mine = 0x1111111111111111ull << ((uint32_t)r >> 6);
            const uint64_t stop = (__builtin_amdgcn_ballot_w64(step != 3u) & mine) << up;
            const uint64_t mism = (__builtin_amdgcn_ballot_w64(x > 15u) & mine) << up;
            const uint64_t ins = __builtin_amdgcn_ballot_w64(step == 2u) << up;
            // M cells before the first other one; at most 15 because of the guard bit: 16 M cells count as 15
            const uint32_t run = (uint32_t)__builtin_clzll(stop | 1u) >> 2;
            // No step the serial walk would not take: ti > 0 and tj > 0 before each, the column in the window, the row in the v2 window,
            // not past the next flush of `ops`, and not beyond the 15 cells `run` can tell of (the 16th waits for the next trip).
            // (The minima are kept apart pair by pair so that they stay scalar: a three-way minimum exists on the vector side only.)
            uint32_t lim = (uint32_t)(ti < tj ? ti : tj), lim_w = col < t0 ? col + 1 : t0 + 1;
            asm volatile("" : "+s"(lim), "+s"(lim_w));
            lim = lim < lim_w ? lim : lim_w;
            asm volatile("" : "+s"(lim));
            lim = lim < 64u - (n_ops & 63u) ? lim : 64u - (n_ops & 63u);
            asm volatile("" : "+s"(lim));
            lim = lim < 15u ? lim : 15u;
            const uint32_t n = run < lim ? run : lim;               // M steps of this trip
            const uint32_t other = run < lim ? 1u : 0u;             // and the I or D step behind them, where it is inside the limits too
            const uint32_t is_i = other & (uint32_t)((ins << (4 * run)) >> 63);
            o.edit_distance += (int)other + __builtin_popcountll((mism >> 4) >> (60 - 4 * n));        // M over a mismatch counts
            ti -= (int)(n + (other ^ is_i));
            tj -= (int)(n + is_i);
            const uint32_t at = lane - (n_ops & 63u), tot = n + other;
            const uint32_t last = other ? (is_i ? (uint32_t)'I' : (uint32_t)'D') : (uint32_t)'M';
            acc = at < tot ? (at == tot - 1 ? last : (uint32_t)'M') : acc;
            n_ops += tot;
            if((n_ops & 63u) == 0) ops[n_ops - 64 + lane] = (uint8_t)acc;
        }
        o.total_columns = (int)n_ops;
        if((n_ops & 63u) != 0 && lane < (n_ops & 63u)) ops[(n_ops & ~63u) + lane] = (uint8_t)acc;
        o.m0s = ti; o.m1s = tj;
        o.n_ops = bad ? 0xFFFFFFFFu : n_ops;
        o.t_fill = (uint32_t)(t_job1 - t_job0); o.t_trace = (uint32_t)(__builtin_readcyclecounter() - t_job1); o.t_trips = trips;
        if(a.reqs && !bad) {
            const DpRequest& R = a.reqs[J.req];
            const bool bPassedOverlap = (uint64_t)(int64_t)o.total_columns >= (uint64_t)R.min_overlap;
            const double pid = (double)(o.total_columns - o.edit_distance) * 100.0f / o.total_columns;      // getPercentIdentity
            o.accept = (bPassedOverlap && pid / 100 >= R.min_identity) ? 1u : 0u;
        }
        if(lane == 0) a.out[job] = o;
    }
}

hipError_t launch_dp_align(const DpAlignArgs& a, uint32_t n_waves, hipStream_t stream)
{
    if(a.n_list == 0) return hipSuccess;
    if(a.band_width < 2 || (a.band_width / 2) * 2 + 1 > kDpMaxBand) return hipErrorInvalidValue;
    if(!a.list || !a.head || a.n_list > a.n_jobs || n_waves == 0) return hipErrorInvalidValue;
    const size_t lds = a.stage_max;
    if(n_waves > a.n_list) n_waves = a.n_list;
    if(a.seq_ws) {
        if(a.seq_ws_stride < lds) return hipErrorInvalidValue;
        hipLaunchKernelGGL(dp_align_kernel<true>, dim3(n_waves), dim3(64), 0, stream, a);
    } else {
        if(lds > kDpAlignLdsCap) return hipErrorInvalidValue;
        hipLaunchKernelGGL(dp_align_kernel<false>, dim3(n_waves), dim3(64), lds, stream, a);
    }
    return hipGetLastError();
}

} // namespace lrsc
