// unrle_driver.cpp -- the device RL decoder's per-lane functions (csrc/fm_unrle.h, fm_pack.h) compiled for the CPU, beside
// the host builder.
//
//   unrle_driver pack <wide: 0|1> <small: 0|1> <N> < units      (one byte per RL unit)
//
// runs the decoder's phases in the order of fm_unrle.hip (sums per unit tile, exclusive scans and the first invalid unit, the
// host's checks, then per symbol tile: seek, expand chunk by chunk, block_hist, scan, pack_block, '$' list and directory) and
// build_strand_image (fm_layout.cpp) on the same units.  When both accept the units it writes both images to stdout, the
// decoder's first, in pack_driver's format: u64 n_blocks, the blocks, u64 n_dollars, the list, u64 n_dir, the directory,
// pred[5].  When either refuses them it writes three lines of text instead (the decoder's message, the host builder's, the
// index of the first corrupt unit or -1) and returns 3.  <small> = 1 shrinks the tiles: a unit tile of one lane (16 units), a
// chunk of two lanes, a symbol tile of two rank blocks.
//
//   unrle_driver seek <n_tiles> < positions                    (u64 each)
//
// runs the seek alone on a made-up stream of n_tiles unit tiles of the kernels' size, tile t made of units of symbol t % 5
// and run 1 + t % 31, and writes per position: u64 unit index, u64 offset inside the unit, u64 A,C,G,T,'$' before the position.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../longreadselfcorrect_amd/csrc/fm_layout.h"
#include "../../longreadselfcorrect_amd/csrc/fm_unrle.h"

using namespace lrsc;

namespace {

struct Shape {
    uint32_t unit_lanes, chunk_lanes, blocks;
};

// fm_unrle.hip's load_units16
Sym16 load_units16(const std::vector<uint8_t>& units, uint64_t first, uint32_t& n)
{
    Sym16 v{{0u, 0u, 0u, 0u}};
    n = first >= units.size() ? 0u : (uint32_t)(units.size() - first < 16 ? units.size() - first : 16);
    for(uint32_t i = 0; i < n; ++i) v.w[i >> 2] |= (uint32_t)units[first + i] << (8 * (i & 3));
    return v;
}

// one chunk in "LDS": the units of its lanes and the lanes' scanned run sums
struct Chunk {
    std::vector<Sym16> units;
    std::vector<uint32_t> n, starts;
    void load(const std::vector<uint8_t>& all, uint64_t first, uint32_t lanes)
    {
        units.resize(lanes);
        n.resize(lanes);
        starts.assign(lanes + 1, 0);
        for(uint32_t l = 0; l < lanes; ++l) {
            units[l] = load_units16(all, first + 16ull * l, n[l]);
            starts[l + 1] = starts[l] + units16_total(units[l], n[l]);
        }
    }
    const uint8_t* bytes() const { return reinterpret_cast<const uint8_t*>(units.data()); }
    uint32_t total() const { return starts.back(); }
};

const char* kShort = "BWT runs do not add up to the symbol count in the header";

template <class Block>
int decode(const std::vector<uint8_t>& units, uint64_t N, const Shape& sh, StrandImage& out, uint64_t& first_bad, std::string& err)
{
    using Tile = PackTile<Block>;
    using CountT = decltype(Block::cnt[0] + 0);
    first_bad = ~0ull;
    if(units.empty()) { err = kShort; return 1; }
    const uint64_t unit_tile = 16ull * sh.unit_lanes;
    const uint64_t n_tiles = (units.size() + unit_tile - 1) / unit_tile, n1 = n_tiles + 1;
    // 1. unrle_tile_kernel
    std::vector<uint64_t> scan(6 * n1, 0);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        uint64_t total = 0;
        for(uint32_t l = 0; l < sh.unit_lanes; ++l) {
            uint32_t n;
            const Sym16 v = load_units16(units, t * unit_tile + 16ull * l, n);
            const UnitSums s = units16_sums(v, n);
            for(int k = 0; k < 5; ++k) { scan[k * n1 + t] += s.c[k]; total += s.c[k]; }
            if(s.bad != kUnrleNone && first_bad == ~0ull) first_bad = t * unit_tile + 16ull * l + s.bad;
        }
        scan[5 * n1 + t] = total;
    }
    // 2. the scans and the host's checks
    for(int k = 0; k < 6; ++k) {
        uint64_t run = 0;
        for(uint64_t t = 0; t < n1; ++t) { const uint64_t h = scan[k * n1 + t]; scan[k * n1 + t] = run; run += h; }
    }
    const uint64_t n_dollars = scan[4 * n1 + n_tiles];
    if(first_bad != ~0ull) { err = "corrupt RL unit in BWT"; return 1; }
    if(scan[5 * n1 + n_tiles] > N) { err = "BWT runs exceed the symbol count in the header"; return 1; }
    if(scan[5 * n1 + n_tiles] < N) { err = kShort; return 1; }

    const uint64_t n_blocks = N / Block::kSyms + 1;
    const uint64_t n_dir = (n_blocks >> kDollarDirShift) + 2;
    out.n_blocks = n_blocks;
    out.n_symbols = N;
    out.blocks.assign(n_blocks * sizeof(Block), 0xEE);
    out.dollars.assign(n_dollars, ~0ull);
    out.dollar_dir.assign(n_dir, 0xEEEEEEEEu);
    // 3. unrle_pack_kernel, one "workgroup" per symbol tile
    const uint32_t tile_syms = sh.blocks * Block::kSyms;
    const uint64_t* pos = &scan[5 * n1];
    Chunk ch;
    std::vector<Sym16> rows(sh.blocks * Tile::kRow);
    for(uint64_t first = 0; first < n_blocks; first += sh.blocks) {
        std::memset(rows.data(), 0xA5, rows.size() * sizeof(Sym16));     // what a lane does not write is arbitrary
        const uint64_t p = first * Block::kSyms;
        const uint32_t n_syms = (uint32_t)(N - p < tile_syms ? N - p : tile_syms);
        const uint32_t n_q = (n_syms + 15) / 16;
        uint64_t seed[5];
        if(n_syms == 0) {
            for(int k = 0; k < 5; ++k) seed[k] = scan[k * n1 + n_tiles];
        } else {
            const uint64_t t = unrle_seek_tile(pos, n_tiles, p);
            uint64_t cb = t * unit_tile, cpos = pos[t];
            uint32_t q_done = 0;
            for(bool seek = true;; seek = false) {
                ch.load(units, cb, sh.chunk_lanes);
                if(seek) {
                    for(int k = 0; k < 5; ++k) seed[k] = scan[k * n1 + t];
                    for(uint32_t l = 0; l < sh.chunk_lanes; ++l) {
                        uint32_t c[5];
                        units16_before(ch.units[l], ch.n[l], ch.starts[l], (uint32_t)(p - cpos), c);
                        for(int k = 0; k < 5; ++k) seed[k] += c[k];
                    }
                }
                const uint64_t cover = cpos + ch.total() - p;
                const uint32_t q_end = cover >= n_syms ? n_q : (uint32_t)(cover >> 4);
                for(uint32_t q = q_done; q < q_end; ++q) {
                    const uint32_t x = (uint32_t)(p + 16ull * q - cpos);
                    const uint32_t left = n_syms - 16 * q;
                    rows[(q / Tile::kChunks) * Tile::kRow + q % Tile::kChunks] =
                        expand_sym16(ch.bytes(), ch.starts.data(), sh.chunk_lanes, x, left < 16 ? left : 16);
                }
                q_done = q_end;
                if(q_done == n_q) break;
                const uint32_t l = unrle_find_lane(ch.starts.data(), sh.chunk_lanes, (uint32_t)(p + 16ull * q_done - cpos));
                if(l == 0) { err = "the chunks do not advance"; return 2; }
                cb += 16ull * l;
                cpos += ch.starts[l];
            }
        }
        uint64_t run[5];
        for(int k = 0; k < 5; ++k) run[k] = seed[k];
        for(uint32_t i = 0; i < sh.blocks && first + i < n_blocks; ++i) {
            const uint64_t b = first + i;
            const Sym16* row = &rows[i * Tile::kRow];
            const uint64_t left = N - b * Block::kSyms;
            const uint32_t n_valid = (uint32_t)(left < Block::kSyms ? left : Block::kSyms);
            const uint64_t none[4] = {0, 0, 0, 0};
            uint32_t h[5];
            block_hist<Block>(row, n_valid, h);
            Block blk = pack_block<Block>(row, n_valid, none);
            for(int k = 0; k < 4; ++k) blk.cnt[k] += (CountT)run[k];
            std::memcpy(&out.blocks[b * sizeof(Block)], &blk, sizeof(Block));
            uint64_t d = run[4];
            if((b & ((1u << kDollarDirShift) - 1)) == 0) out.dollar_dir.at(b >> kDollarDirShift) = (uint32_t)d;
            for(uint32_t wi = 0; wi < Block::kWords; ++wi)
                for(uint32_t m = sym_bits32(row, wi, n_valid).dollar; m; m &= m - 1, ++d)
                    out.dollars.at(d) = b * Block::kSyms + 32 * wi + (uint32_t)__builtin_ctz(m);
            if(b == n_blocks - 1)
                for(uint64_t g = (b >> kDollarDirShift) + 1; g < n_dir; ++g) out.dollar_dir.at(g) = (uint32_t)n_dollars;
            for(int k = 0; k < 5; ++k) run[k] += h[k];
        }
    }
    out.pred[0] = 0;
    out.pred[1] = n_dollars;
    for(int c = 2; c < 5; ++c) out.pred[c] = out.pred[c - 1] + scan[(c - 2) * n1 + n_tiles];
    return 0;
}

void dump(const StrandImage& im)
{
    const uint64_t n[3] = {im.n_blocks, im.dollars.size(), im.dollar_dir.size()};
    std::fwrite(&n[0], 8, 1, stdout);
    std::fwrite(im.blocks.data(), 1, im.blocks.size(), stdout);
    std::fwrite(&n[1], 8, 1, stdout);
    if(!im.dollars.empty()) std::fwrite(im.dollars.data(), 8, im.dollars.size(), stdout);
    std::fwrite(&n[2], 8, 1, stdout);
    std::fwrite(im.dollar_dir.data(), 4, im.dollar_dir.size(), stdout);
    std::fwrite(im.pred, 8, 5, stdout);
}

std::vector<uint8_t> read_stdin()
{
    std::vector<uint8_t> in;
    uint8_t buf[4096];
    for(size_t got; (got = std::fread(buf, 1, sizeof buf, stdin)) > 0;) in.insert(in.end(), buf, buf + got);
    return in;
}

int pack_main(bool wide, bool small, uint64_t N)
{
    const std::vector<uint8_t> units = read_stdin();
    const Shape sh = small ? Shape{1, 2, 2} : Shape{kUnrleLanes, kUnrleLanes, kUnrleBlocks};
    StrandImage packed, built;
    std::string err_d, err_h;
    uint64_t first_bad = ~0ull;
    const int st_d = wide ? decode<Block64>(units, N, sh, packed, first_bad, err_d) : decode<Block32>(units, N, sh, packed, first_bad, err_d);
    if(st_d == 2) { std::fprintf(stderr, "%s\n", err_d.c_str()); return 2; }
    const int st_h = build_strand_image(units.data(), units.size(), N, wide, built, err_h);
    if(st_d != 0 || st_h != 0) {
        std::printf("%s\n%s\n%lld\n", err_d.c_str(), err_h.c_str(), (long long)first_bad);
        return 3;
    }
    dump(packed);
    dump(built);
    return 0;
}

int seek_main(uint64_t n_tiles)
{
    const std::vector<uint8_t> in = read_stdin();
    const uint64_t n1 = n_tiles + 1;
    std::vector<uint64_t> scan(6 * n1, 0);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        const uint64_t syms = (uint64_t)kUnrleTile * (1 + t % 31);
        for(int k = 0; k < 6; ++k) scan[k * n1 + t + 1] = scan[k * n1 + t];
        scan[unit_slot((uint32_t)(t % 5)) * n1 + t + 1] += syms;
        scan[5 * n1 + t + 1] += syms;
    }
    std::vector<uint8_t> tile(kUnrleTile);
    Chunk ch;
    for(size_t i = 0; i + 8 <= in.size(); i += 8) {
        uint64_t p;
        std::memcpy(&p, &in[i], 8);
        if(p >= scan[5 * n1 + n_tiles]) { std::fprintf(stderr, "position beyond the stream\n"); return 2; }
        const uint64_t t = unrle_seek_tile(&scan[5 * n1], n_tiles, p);
        std::memset(tile.data(), (int)(((t % 5) << 5) | (1 + t % 31)), tile.size());
        ch.load(tile, 0, kUnrleLanes);
        const uint32_t rel = (uint32_t)(p - scan[5 * n1 + t]);
        const UnitAt at = unrle_locate(ch.bytes(), ch.starts.data(), kUnrleLanes, rel);
        uint64_t o[7] = {t * kUnrleTile + at.unit, at.off, 0, 0, 0, 0, 0};
        for(int k = 0; k < 5; ++k) o[2 + k] = scan[k * n1 + t];
        for(uint32_t l = 0; l < kUnrleLanes; ++l) {
            uint32_t c[5];
            units16_before(ch.units[l], ch.n[l], ch.starts[l], rel, c);
            for(int k = 0; k < 5; ++k) o[2 + k] += c[k];
        }
        std::fwrite(o, 8, 7, stdout);
    }
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if(argc == 5 && !std::strcmp(argv[1], "pack")) return pack_main(std::atoi(argv[2]) != 0, std::atoi(argv[3]) != 0, std::strtoull(argv[4], nullptr, 10));
    if(argc == 3 && !std::strcmp(argv[1], "seek")) return seek_main(std::strtoull(argv[2], nullptr, 10));
    std::fprintf(stderr, "usage: unrle_driver pack <wide> <small> <N> < units | unrle_driver seek <n_tiles> < positions\n");
    return 2;
}
