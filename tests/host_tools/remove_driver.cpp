// remove_driver.cpp -- the device read removal's per-lane functions (csrc/fm_remove.h) compiled for the CPU and run in the kernels' order.
//
//   remove_driver <wide: 0|1> <small: 0|1> <defect: 0|1> < input
//
// input:  u64 N, u64 n_units, the RL units of the strand's BWT; u64 n_drop, the dropped reads as u32, ascending; u64 N', u64
//         n_units', the RL units of the BWT that is expected of the kept reads.
// The image comes from build_strand_image (fm_layout.cpp), Block64 where wide, as lrsc_index_upload would hold it.  Then, as
// fm_remove.hip does: remove_mark_read for every dropped read, the kept rows of every tile lane by lane and their exclusive scan,
// and per tile decode_block for its blocks, remove_keep16 / remove_scatter16 for every lane at the prefix sum of the lanes
// before it and remove_store_chunk for every chunk; with the kernels' tile (small = 0) or one of 384 rows, two Block32 or three
// Block64 (small = 1).  What the kernels leave unwritten in LDS is 0xA5 here.  The compacted codes are then packed with
// fm_pack.h's functions in fm_pack.hip's order and held against build_strand_image of the expected units, byte for byte.
// defect = 1: the '$' list of the image is emptied first, so that no walk meets its '$' row; the run must end in the FORMAT
// path (exit status 3, "FORMAT" on stdout) with every mark inside the bitmap.
// output: u64 N', the compacted codes ($ACGT = 0..4).
static const char kDriver[] = "remove_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_remove.h"

using namespace lrsc;

static void format_path(const char* why)
{
    std::fprintf(stderr, "remove_driver: %s\n", why);
    std::fputs("FORMAT", stdout);
    std::exit(3);
}

// fm_pack.hip's steps on the CPU (tests/host_tools/pack_driver.cpp)
template <class Block>
static void pack_host(const std::vector<uint8_t>& codes, StrandImage& out)
{
    const uint64_t N = codes.size();
    const uint64_t n_blocks = N / Block::kSyms + 1;
    std::vector<Sym16> syms(n_blocks * (Block::kSyms / 16));
    std::memset(syms.data(), 0xA5, syms.size() * sizeof(Sym16));
    std::memcpy(syms.data(), codes.data(), N);
    auto n_valid = [&](uint64_t b) { const uint64_t left = N - b * Block::kSyms; return (uint32_t)(left < Block::kSyms ? left : Block::kSyms); };
    std::vector<uint64_t> cnt[5];
    for(auto& v : cnt) v.assign(n_blocks + 1, 0);
    for(uint64_t b = 0; b < n_blocks; ++b) {
        uint32_t c[5];
        block_hist<Block>(&syms[b * (Block::kSyms / 16)], n_valid(b), c);
        for(int k = 0; k < 5; ++k) cnt[k][b] = c[k];
    }
    for(auto& v : cnt) {
        uint64_t run = 0;
        for(uint64_t& x : v) { const uint64_t h = x; x = run; run += h; }
    }
    out.n_blocks = n_blocks;
    out.n_symbols = N;
    out.blocks.resize(n_blocks * sizeof(Block));
    for(uint64_t b = 0; b < n_blocks; ++b) {
        const uint64_t before[4] = {cnt[0][b], cnt[1][b], cnt[2][b], cnt[3][b]};
        const Block blk = pack_block<Block>(&syms[b * (Block::kSyms / 16)], n_valid(b), before);
        std::memcpy(&out.blocks[b * sizeof(Block)], &blk, sizeof(Block));
    }
    out.dollars.clear();
    for(uint64_t i = 0; i < N; ++i) if(codes[i] == 0) out.dollars.push_back(i);
    out.dollar_dir.resize((n_blocks >> kDollarDirShift) + 2);
    for(uint64_t g = 0; g < out.dollar_dir.size(); ++g) out.dollar_dir[g] = dollar_dir_entry(cnt[4].data(), n_blocks, g);
    out.pred[0] = 0;
    out.pred[1] = cnt[4][n_blocks];
    for(int c = 2; c < 5; ++c) out.pred[c] = out.pred[c - 1] + cnt[c - 2][n_blocks];
}

template <class Block, uint32_t kLanes>
static void remove(StrandImage& im, bool wide, bool defect, const std::vector<uint32_t>& ids, const StrandImage& want)
{
    constexpr uint32_t kTile = kLanes * 16;
    static_assert(kTile % Block::kSyms == 0 && kTile % 32 == 0, "a tile is whole rank blocks and bitmap words");
    if(defect) for(uint64_t& d : im.dollars) d = ~0ull;           // no row is a '$' row any more
    const FmStrand fs = strand_of(im, wide);
    const StrandView<Block> S = strand_view<Block>(fs);
    const std::vector<uint32_t> mtab = mask_table<Block>();
    const uint64_t N = S.N;

    // 1. the walks
    std::vector<uint32_t> bitmap(remove_bitmap_words(N, kTile), 0u);
    uint64_t rows = 0;
    bool broken = false;
    for(uint32_t read : ids) {
        if(read >= S.n_dollars) die("a dropped read beyond the index");
        const uint32_t st = remove_mark_read<Block>(S, mtab.data(), read, [&](uint64_t row) {
            if(row >= N || (row >> 5) >= bitmap.size()) die("a mark outside the bitmap");
            if(!defect && ((bitmap[row >> 5] >> (row & 31)) & 1u)) die("a row visited twice");
            bitmap[row >> 5] |= 1u << (row & 31);
        }, rows);
        broken = broken || st != kWalkOk;
    }
    if(broken) format_path("a walk did not end at a '$' row");
    if(defect) die("the defective index was walked to an end");

    // 2. kept rows per tile, a lane of 64 at a time, and their exclusive scan
    const uint64_t n_tiles = (N + kTile - 1) / kTile;
    constexpr uint32_t kWords = kTile / 32, kPerLane = (kWords + 63) / 64;
    std::vector<uint64_t> tile_off(n_tiles + 1, 0);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        uint32_t marked = 0;
        for(uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t w = lane * kPerLane;
            if(w < kWords) marked += remove_words_marked(bitmap.data(), t * kWords + w, kPerLane < kWords - w ? kPerLane : kWords - w);
        }
        tile_off[t] = (N - t * kTile < kTile ? N - t * kTile : kTile) - marked;
    }
    uint64_t total = 0;
    for(uint64_t& x : tile_off) { const uint64_t h = x; x = total; total += h; }
    if(total > N || N - total != rows) format_path("the marked rows are not the rows the walks visited");
    if(total == 0) die("nothing is kept");

    // 3. the tiles
    const uint64_t cap = (total + 15) / 16 * 16;
    std::vector<Sym16> out_rows(cap / 16);
    uint8_t* out = reinterpret_cast<uint8_t*>(out_rows.data());
    std::memset(out, 0xEE, cap);
    std::memset(out + cap - 16, 0, 16);
    std::vector<Sym16> sym(kTile / 16), stage(RemoveStage<kTile>::kRows);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        std::memset(sym.data(), 0xA5, sym.size() * sizeof(Sym16));
        std::memset(stage.data(), 0xA5, stage.size() * sizeof(Sym16));
        const uint64_t p0 = t * kTile;
        const uint32_t n_valid = (uint32_t)(N - p0 < kTile ? N - p0 : kTile);
        const uint64_t off = tile_off[t];
        const uint32_t n_kept = (uint32_t)(tile_off[t + 1] - off);
        if(n_kept > n_valid) die("a tile keeps more rows than it has");
        if(n_kept == 0) continue;
        const uint32_t n_blk = (n_valid + Block::kSyms - 1) / Block::kSyms;
        for(uint32_t u = 0; u < n_blk; ++u) decode_block<Block>(S, p0 / Block::kSyms + u, &sym[u * (Block::kSyms / 16)]);
        const uint32_t shift = (uint32_t)(off & 15u);
        uint32_t before = 0;
        for(uint32_t lane = 0; lane < kLanes; ++lane) {
            const uint32_t keep = remove_keep16(bitmap.data(), p0, lane, n_valid);
            const uint32_t cnt = (uint32_t)__builtin_popcount(keep);
            if(shift + before + cnt > stage.size() * 16) die("the stage overflows");
            if(keep) remove_scatter16(sym.data(), lane, keep, reinterpret_cast<uint8_t*>(stage.data()) + shift + before);
            before += cnt;
        }
        if(before != n_kept) die("the lanes' kept rows are not the tile's");
        if(off - shift + ((shift + n_kept + 15) / 16) * 16 > cap + 15) die("a tile's chunks leave the output");
        for(uint32_t c = 0; 16 * c < shift + n_kept; ++c) {
            if(16 * c >= shift && 16 * c + 16 <= shift + n_kept && off - shift + 16 * c + 16 > cap) die("a 16-byte store leaves the output");
            remove_store_chunk(stage.data(), shift, n_kept, c, out + (off - shift));
        }
    }
    for(uint64_t p = total; p < cap; ++p) if(out[p] != 0) die("codes beyond the end are not 0");
    const std::vector<uint8_t> codes(out, out + total);
    for(uint8_t c : codes) if(c > 4) die("a position of the output was never written");

    // 4. the packer, against the host builder on the expected units
    StrandImage packed;
    pack_host<Block>(codes, packed);
    if(packed.n_blocks != want.n_blocks || packed.n_symbols != want.n_symbols || packed.blocks.size() != want.blocks.size() ||
       std::memcmp(packed.blocks.data(), want.blocks.data(), want.blocks.size()) != 0 || packed.dollars != want.dollars ||
       packed.dollar_dir != want.dollar_dir || std::memcmp(packed.pred, want.pred, sizeof(want.pred)) != 0)
        die("the packed image is not build_strand_image's of the kept reads");
    std::fwrite(&total, 8, 1, stdout);
    std::fwrite(codes.data(), 1, codes.size(), stdout);
}

int main(int argc, char** argv)
{
    if(argc != 4) { std::fprintf(stderr, "usage: remove_driver <wide> <small> <defect> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0, small = std::atoi(argv[2]) != 0, defect = std::atoi(argv[3]) != 0;
    StrandImage im, want;
    read_image(wide, im);
    uint64_t n_drop = 0;
    read_exact(&n_drop, 8);
    std::vector<uint32_t> ids(n_drop);
    read_exact(ids.data(), ids.size() * 4);
    read_image(wide, want);
    if(wide) { if(small) remove<Block64, 24>(im, true, defect, ids, want); else remove<Block64, kRemoveLanes>(im, true, defect, ids, want); }
    else { if(small) remove<Block32, 24>(im, false, defect, ids, want); else remove<Block32, kRemoveLanes>(im, false, defect, ids, want); }
    return 0;
}
