// rle_driver.cpp -- the device RL encoder's per-lane functions (csrc/fm_rle.h) compiled for the CPU, beside the sequential rule.
//
//   rle_driver encode <small: 0|1> < codes     (N bytes, BWT codes $=0 A=1 C=2 G=3 T=4)
//
// runs the encoder's four phases in the order of fm_rle.hip (stretch_summary per lane joined per tile, inclusive scan of the
// tiles with rle_combine, stretch_count per lane + exclusive sum, stretch_emit per lane into a staging row at the output's
// 16-byte phase) with the kernels' tile (small = 0) or with a tile of one Block32, 12 lanes of 16 symbols (small = 1), and the
// loop of lrsc_build_bwt on the same codes.  Writes both to stdout, the encoder's first: u64 n_units, the units.
//
//   rle_driver decode <wide: 0|1> < codes      (kSyms bytes)
//
// packs the first n_valid codes with pack_block and unpacks them with unpack_block, for n_valid = 0..kSyms, and writes the
// kSyms + 1 decoded blocks of kSyms bytes each.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../longreadselfcorrect_amd/csrc/fm_rle.h"

using namespace lrsc;

template <uint32_t kLanes, uint32_t kChunks>
static std::vector<uint8_t> encode_tiled(const std::vector<uint8_t>& codes)
{
    constexpr uint32_t kStretch = kChunks * 16, kTile = kLanes * kStretch;
    const uint64_t N = codes.size();
    const uint64_t n_tiles = (N + kTile - 1) / kTile;
    // a tile and its halo as the kernels see them in LDS, anything at or beyond N arbitrary
    std::vector<Sym16> syms(kTile / 16 + kRleHalo / 16);
    auto load = [&](uint64_t t) {
        std::memset(syms.data(), 0xA5, syms.size() * sizeof(Sym16));
        const uint64_t base = t * kTile, have = N - base < kTile + kRleHalo ? N - base : kTile + kRleHalo;
        std::memcpy(syms.data(), codes.data() + base, have);
    };
    auto n_valid = [&](uint64_t t, uint32_t lane) {
        const uint64_t base = t * kTile + (uint64_t)lane * kStretch;
        return base >= N ? 0u : (uint32_t)(N - base < kStretch ? N - base : kStretch);
    };
    const RunSummary none{0, 0, 0, 0};
    // 1. summaries
    std::vector<RunSummary> sum(n_tiles, none);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        load(t);
        for(uint32_t l = 0; l < kLanes; ++l) sum[t] = rle_combine(sum[t], stretch_summary<kChunks>(&syms[l * kChunks], n_valid(t, l)));
    }
    // 2. inclusive scan
    for(uint64_t t = 1; t < n_tiles; ++t) sum[t] = rle_combine(sum[t - 1], sum[t]);
    // 3. counts and their exclusive sum
    std::vector<uint64_t> off(n_tiles + 1, 0);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        load(t);
        RunSummary before = t ? sum[t - 1] : none;
        for(uint32_t l = 0; l < kLanes; ++l) {
            off[t] += stretch_count<kChunks>(&syms[l * kChunks], n_valid(t, l), before);
            before = rle_combine(before, stretch_summary<kChunks>(&syms[l * kChunks], n_valid(t, l)));
        }
    }
    uint64_t total = 0;
    for(uint64_t& x : off) { const uint64_t h = x; x = total; total += h; }
    // 4. emit, allocated at the exact size
    std::vector<uint8_t> out(total);
    std::vector<uint8_t> stage(kTile + 16);
    for(uint64_t t = 0; t < n_tiles; ++t) {
        load(t);
        std::memset(stage.data(), 0xEE, stage.size());
        const uint32_t phase = (uint32_t)(off[t] & 15);
        RunSummary before = t ? sum[t - 1] : none;
        uint32_t first = 0;
        for(uint32_t l = 0; l < kLanes; ++l) {
            const uint32_t nv = n_valid(t, l);
            const uint64_t end = t * kTile + (uint64_t)(l + 1) * kStretch;
            const uint32_t n_after = end < N ? (uint32_t)(N - end < kRleMaxRun - 1 ? N - end : kRleMaxRun - 1) : 0u;
            const uint32_t n = stretch_count<kChunks>(&syms[l * kChunks], nv, before);
            if(n) stretch_emit<kChunks>(&syms[l * kChunks], nv, before, n_after, &stage[phase + first]);
            first += n;
            before = rle_combine(before, stretch_summary<kChunks>(&syms[l * kChunks], nv));
        }
        if(first != off[t + 1] - off[t]) { std::fprintf(stderr, "tile %llu: count and emit disagree\n", (unsigned long long)t); std::exit(1); }
        std::memcpy(out.data() + off[t], &stage[phase], first);
    }
    return out;
}

static void dump(const std::vector<uint8_t>& u)
{
    const uint64_t n = u.size();
    std::fwrite(&n, 8, 1, stdout);
    std::fwrite(u.data(), 1, u.size(), stdout);
}

template <class Block>
static void decode_all(const std::vector<uint8_t>& codes)
{
    constexpr uint32_t kChunks = Block::kSyms / 16;
    const uint64_t base = 5ull * Block::kSyms + (1ull << 33);      // the block sits anywhere in the BWT
    const uint64_t before[4] = {11, 22, 33, 44};
    for(uint32_t nv = 0; nv <= Block::kSyms; ++nv) {
        Sym16 in[kChunks], out[kChunks];
        std::memset(in, 0xA5, sizeof in);
        std::memset(out, 0xEE, sizeof out);
        std::memcpy(in, codes.data(), nv);
        const Block b = pack_block<Block>(in, nv, before);
        std::vector<uint64_t> dollars;
        for(uint32_t i = 0; i < nv; ++i) if(codes[i] == 0) dollars.push_back(base + i);
        dollars.push_back(base + Block::kSyms);                    // the next block's: ignored
        const bool flagged = has_dollar_flag(b);
        if(flagged != (dollars.size() > 1)) { std::fprintf(stderr, "flag\n"); std::exit(1); }
        unpack_block<Block>(b, base, dollars.data(), flagged ? dollars.size() : 0, nv, out);
        std::fwrite(out, 1, sizeof out, stdout);
    }
}

int main(int argc, char** argv)
{
    if(argc != 3) { std::fprintf(stderr, "usage: rle_driver encode <small> | decode <wide> < codes\n"); return 2; }
    const bool flag = std::atoi(argv[2]) != 0;
    std::vector<uint8_t> codes;
    uint8_t buf[4096];
    for(size_t got; (got = std::fread(buf, 1, sizeof buf, stdin)) > 0;) codes.insert(codes.end(), buf, buf + got);
    for(uint8_t c : codes) if(c > 4) { std::fprintf(stderr, "code %u\n", c); return 2; }
    if(codes.empty()) { std::fprintf(stderr, "no codes\n"); return 2; }

    if(std::strcmp(argv[1], "decode") == 0) {
        if(codes.size() != (flag ? Block64::kSyms : Block32::kSyms)) { std::fprintf(stderr, "decode takes one block of codes\n"); return 2; }
        if(flag) decode_all<Block64>(codes); else decode_all<Block32>(codes);
        return 0;
    }
    static_assert(kRleLanes * kRleChunks * 16 == kRleTile, "the kernels' tile");
    dump(flag ? encode_tiled<12, 1>(codes) : encode_tiled<kRleLanes, kRleChunks>(codes));

    // the yardstick: the loop of lrsc_build_bwt (run < 31 extends)
    std::vector<uint8_t> units;
    uint8_t prev = 0xFF; unsigned run = 0;
    for(uint8_t c : codes) {
        if(c == prev && run < 31) units.back() = (uint8_t)((c << 5) | ++run);
        else { prev = c; run = 1; units.push_back((uint8_t)((c << 5) | 1)); }
    }
    dump(units);
    return 0;
}
