// merge_driver.cpp -- the device merge's per-lane functions (csrc/fm_merge.h) compiled for the CPU and run in the kernels' order.
//
//   merge_driver <wide_a: 0|1> <wide_b: 0|1> <small: 0|1> < input
//
// input:  for A, then for B: u64 N, u64 n_units, the RL units of the strand's BWT.
// The two images come from build_strand_image (fm_layout.cpp), Block64 where wide, as lrsc_index_upload would hold them.  Then,
// as fm_merge.hip does: merge_walk_step for every read of B until its '$' (rank[]), merge_tile_search for every tile edge,
// per tile the B positions, decode_block for the blocks of either span and merge_fill16 for every lane, and
// merge_origin_slot for every '$' row of B; with the kernels' tile (small = 0) or one of 384 positions, two Block32 or three
// Block64 (small = 1).  What the kernels leave unwritten in LDS is 0xA5 here.
// output: u64 N_A + N_B, the merged codes ($ACGT = 0..4); u64 N_B, rank[] as u64; u64 n_A + n_B, the origin bytes.
static const char kDriver[] = "merge_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_merge.h"

using namespace lrsc;

template <class T>
static void dump(const std::vector<T>& v)
{
    const uint64_t n = v.size();
    std::fwrite(&n, 8, 1, stdout);
    std::fwrite(v.data(), sizeof(T), v.size(), stdout);
}

template <class BA, class BB, uint32_t kLanes>
static void merge(const StrandImage& ia, const StrandImage& ib, bool wide_a, bool wide_b)
{
    constexpr uint32_t kTile = kLanes * 16;
    using SA = MergeStage<BA, kTile>;
    using SB = MergeStage<BB, kTile>;
    const FmStrand fa = strand_of(ia, wide_a), fb = strand_of(ib, wide_b);
    const StrandView<BA> A = strand_view<BA>(fa);
    const StrandView<BB> B = strand_view<BB>(fb);
    const std::vector<uint32_t> mtab_a = mask_table<BA>(), mtab_b = mask_table<BB>();
    const uint64_t N = A.N + B.N, n_a = A.n_dollars, n_b = B.n_dollars;
    if(n_b == 0) die("B holds no read");

    // 1. the walk
    const uint64_t unset = ~0ull;
    std::vector<uint64_t> rank(B.N, unset);
    for(uint64_t read = 0; read < n_b; ++read) {
        MergeWalk<BA, BB> w = merge_walk_start<BA, BB>(read, n_a);
        uint64_t step = 0;
        for(; step < B.N; ++step) {
            if(w.i >= B.N || w.r > A.N) die("a walk left its index");
            if(rank[w.i] != unset) die("a row of B visited twice");
            rank[w.i] = w.r;
            const BB bb = B.blocks[block_of<BB>(w.i)];
            const BA ba = A.blocks[block_of<BA>(w.r)];
            if(!merge_walk_step(A, B, ba, bb, mtab_a.data(), mtab_b.data(), w)) break;
        }
        if(step == B.N) die("a walk met no '$'");
    }
    for(uint64_t r : rank) if(r == unset) die("a row of B never visited");

    // 2. the tile edges
    const uint64_t n_tiles = (N + kTile - 1) / kTile;
    std::vector<uint64_t> tile_row(n_tiles + 1);
    for(uint64_t t = 0; t <= n_tiles; ++t) tile_row[t] = merge_tile_search(rank.data(), B.N, t * kTile < N ? t * kTile : N);

    // 3. the tiles
    std::vector<uint8_t> out((N + 15) / 16 * 16, 0xEE);
    std::vector<Sym16> sym_a(SA::kRows), sym_b(SB::kRows);
    std::vector<uint16_t> pos_b(kTile);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        std::memset(sym_a.data(), 0xA5, sym_a.size() * sizeof(Sym16));
        std::memset(sym_b.data(), 0xA5, sym_b.size() * sizeof(Sym16));
        std::memset(pos_b.data(), 0xA5, pos_b.size() * sizeof(uint16_t));
        const uint64_t p0 = t * kTile, p1 = p0 + kTile < N ? p0 + kTile : N;
        const uint64_t j0 = tile_row[t], j1 = tile_row[t + 1];
        if(j0 > p0 || j1 < j0 || j1 - j0 > p1 - p0) die("tile edges out of order");
        const uint32_t n_bt = (uint32_t)(j1 - j0);
        const MergeSpan span_a = merge_span<BA>(p0 - j0, p1 - j1);
        const MergeSpan span_b = merge_span<BB>(j0, j1);
        if(span_a.n_blocks > SA::kBlocks || span_b.n_blocks > SB::kBlocks) die("a span beyond its stage");
        for(uint32_t k = 0; k < n_bt; ++k) pos_b[k] = (uint16_t)(j0 + k + rank[j0 + k] - p0);
        for(uint32_t u = 0; u < span_a.n_blocks; ++u) decode_block<BA>(A, span_a.first_block + u, &sym_a[u * SA::kChunks]);
        for(uint32_t u = 0; u < span_b.n_blocks; ++u) decode_block<BB>(B, span_b.first_block + u, &sym_b[u * SB::kChunks]);
        const uint32_t n_valid = (uint32_t)(p1 - p0);
        for(uint32_t lane = 0; lane < kLanes; ++lane) {
            const uint32_t q = lane * 16;
            if(q >= n_valid) continue;
            const Sym16 v = merge_fill16(pos_b.data(), n_bt, sym_a.data(), span_a.skip, sym_b.data(), span_b.skip, q, n_valid);
            std::memcpy(&out[p0 + q], &v, 16);
        }
    }
    for(uint64_t p = N; p < out.size(); ++p) if(out[p] != 0) die("codes beyond the end are not 0");
    out.resize(N);

    // 4. the origin of the '$' rows
    std::vector<uint8_t> origin(n_a + n_b, 0);
    for(uint64_t k = 0; k < n_b; ++k) {
        const uint64_t slot = merge_origin_slot(A.dollars, n_a, rank[B.dollars[k]], k);
        if(slot >= origin.size() || origin[slot]) die("origin slot");
        origin[slot] = 1;
    }
    dump(out);
    dump(rank);
    dump(origin);
}

template <class BA, class BB>
static void merge_tiled(const StrandImage& ia, const StrandImage& ib, bool wide_a, bool wide_b, bool small)
{
    static_assert(kMergeTile == kMergeLanes * 16, "the kernels' tile");
    if(small) merge<BA, BB, 24>(ia, ib, wide_a, wide_b);
    else merge<BA, BB, kMergeLanes>(ia, ib, wide_a, wide_b);
}

int main(int argc, char** argv)
{
    if(argc != 4) { std::fprintf(stderr, "usage: merge_driver <wide_a> <wide_b> <small> < input\n"); return 2; }
    const bool wide_a = std::atoi(argv[1]) != 0, wide_b = std::atoi(argv[2]) != 0, small = std::atoi(argv[3]) != 0;
    StrandImage ia, ib;
    read_image(wide_a, ia);
    read_image(wide_b, ib);
    if(wide_a) { if(wide_b) merge_tiled<Block64, Block64>(ia, ib, true, true, small); else merge_tiled<Block64, Block32>(ia, ib, true, false, small); }
    else { if(wide_b) merge_tiled<Block32, Block64>(ia, ib, false, true, small); else merge_tiled<Block32, Block32>(ia, ib, false, false, small); }
    return 0;
}
