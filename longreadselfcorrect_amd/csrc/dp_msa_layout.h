// dp_msa_layout.h -- where the pile-up kernel (dp_msa.hip) keeps the arrays of one multiple alignment, in bytes.  Plain C++: the
// kernel carves its pointers from it, the host sizes the launches' LDS and workspace from it (dp_msa_lds_bytes,
// dp_msa_small_bytes), and tests/host_msa_layout prints it.
#pragma once
#include <stdint.h>

namespace lrsc {

constexpr uint32_t kMaxIns = 256;         // new columns one row may open on the batched path
// ... and in the global-workspace variant with several wavefronts, whose LDS holds little else: a row of a 16 k-column pile-up
// opens several hundred, and the step walk there is a shift of all columns behind every one of them, each trip a round trip to memory
constexpr uint32_t kMaxInsGlobal = 4096;
constexpr uint32_t msa_max_ins(bool global, uint32_t nw) { return global && nw > 1 ? kMaxInsGlobal : kMaxIns; }
// A workgroup of several wavefronts: the words its wavefronts exchange their ballot counts in -- two buffers of 8 wavefronts x 4
// words, used in turn, so one barrier per exchange is enough -- and the single values one thread hands to all
constexpr uint32_t kXchgWords = 96;

// Two groups of arrays.  The small ones: the exchange words (nw > 1), the new columns of the current row (insx: position in old
// coordinates, insg: rows showing a gap there, inss: the row's own symbol; msa_max_ins() entries each) and lead / size of the
// n_str + 2 rows.  The per-column ones: cnt, bpos, T, Rw and the staged string and cigar.
//   LDS variants:         one region in LDS, the small arrays first; `total` is its size.  With several wavefronts lead / size come
//                         last instead, so that the per-column arrays start at an offset that does not depend on n_str.
//   global, nw > 1:       the small arrays in LDS (`small_total` bytes), the per-column ones from the start of the workspace slot
//                         (`total` bytes of it).
//   global, nw == 1:      one region again, in the workspace slot.
// This function is what guarantees the alignment: cnt 8 bytes, every uint32_t array 4, insg 2, S and ops 4 (staged by dwords).
struct MsaLayout {
    uint32_t xchg, insx, insg, inss, lead, size, small_total;
    uint32_t cnt, bpos, T, Rw, S, ops, total;
};

constexpr MsaLayout msa_layout(uint32_t w_cols, uint32_t lq, uint32_t str_cap, uint32_t ops_cap, uint32_t n_str, uint32_t nw, bool global)
{
    const uint32_t W = w_cols, E = n_str + 2, KI = msa_max_ins(global, nw);
    MsaLayout L{};
    uint32_t o = 0;
    auto take = [&o](uint32_t bytes, uint32_t align) { o = (o + align - 1) & ~(align - 1); const uint32_t at = o; o += bytes; return at; };
    L.xchg = take(nw > 1 ? kXchgWords * 4 : 0, 4);
    L.insx = take(KI * 4, 4);
    L.insg = take(KI * 2, 2);
    L.inss = take(KI, 1);
    const bool tail = !global && nw > 1;   // lead / size behind everything else
    if(!tail) { L.lead = take(E * 4, 4); L.size = take(E * 4, 4); }
    L.small_total = o;
    if(global && nw > 1) o = 0;            // the per-column arrays are in another memory
    L.cnt = take(W * 8, 8);
    L.bpos = take((lq + 2) * 4, 4);         // padded position of the base row's bases from match[0].start on
    L.T = take((W + 3) & ~3u, 1);
    L.Rw = take((W + 3) & ~3u, 1);          // the current row's symbol per base-row position
    L.S = take((str_cap + 7) & ~3u, 4);     // staged from the aligned address at or below the string's start
    L.ops = take((ops_cap + 3) & ~3u, 4);   // the cigar as the alignment kernel wrote it: last op first
    if(tail) { L.lead = take(E * 4, 4); L.size = take(E * 4, 4); }
    L.total = o;
    return L;
}

} // namespace lrsc
