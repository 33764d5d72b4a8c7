// pack_driver.cpp -- the device packer's per-block functions (csrc/fm_pack.h) compiled for the CPU, beside the host builder.
//
//   pack_driver <wide: 0|1> < codes        (N bytes, BWT codes $=0 A=1 C=2 G=3 T=4)
//
// runs the packer's steps in the order of fm_pack.hip (block_hist per block, exclusive scan, pack_block per block, '$' list,
// dollar_dir_entry per group) and build_strand_image (fm_layout.cpp) on the RL units of the same codes, and writes both images
// to stdout, the packer's first: u64 n_blocks, the blocks, u64 n_dollars, the list, u64 n_dir, the directory, pred[5].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../longreadselfcorrect_amd/csrc/fm_layout.h"
#include "../../longreadselfcorrect_amd/csrc/fm_pack.h"

using namespace lrsc;

template <class Block>
static void pack_host(const std::vector<uint8_t>& codes, StrandImage& out)
{
    const uint64_t N = codes.size();
    const uint64_t n_blocks = N / Block::kSyms + 1;
    // the symbols as the kernels see them in LDS: whole blocks of 16-byte pieces, anything at or beyond N arbitrary
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

static void dump(const StrandImage& im)
{
    const uint64_t n[3] = {im.n_blocks, im.dollars.size(), im.dollar_dir.size()};
    std::fwrite(&n[0], 8, 1, stdout);
    std::fwrite(im.blocks.data(), 1, im.blocks.size(), stdout);
    std::fwrite(&n[1], 8, 1, stdout);
    std::fwrite(im.dollars.data(), 8, im.dollars.size(), stdout);
    std::fwrite(&n[2], 8, 1, stdout);
    std::fwrite(im.dollar_dir.data(), 4, im.dollar_dir.size(), stdout);
    std::fwrite(im.pred, 8, 5, stdout);
}

int main(int argc, char** argv)
{
    if(argc != 2) { std::fprintf(stderr, "usage: pack_driver <wide> < codes\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    std::vector<uint8_t> codes;
    uint8_t buf[4096];
    for(size_t got; (got = std::fread(buf, 1, sizeof buf, stdin)) > 0;) codes.insert(codes.end(), buf, buf + got);
    for(uint8_t c : codes) if(c > 4) { std::fprintf(stderr, "code %u\n", c); return 2; }
    if(codes.empty()) { std::fprintf(stderr, "no codes\n"); return 2; }

    StrandImage packed;
    if(wide) pack_host<Block64>(codes, packed); else pack_host<Block32>(codes, packed);

    // the yardstick: RL units as lrsc_build_bwt writes them (run < 31 extends), through the host builder
    std::vector<uint8_t> units;
    uint8_t prev = 0xFF; unsigned run = 0;
    for(uint8_t c : codes) {
        if(c == prev && run < 31) units.back() = (uint8_t)((c << 5) | ++run);
        else { prev = c; run = 1; units.push_back((uint8_t)((c << 5) | 1)); }
    }
    StrandImage built;
    std::string err;
    if(build_strand_image(units.data(), units.size(), codes.size(), wide, built, err) != 0) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    dump(packed);
    dump(built);
    return 0;
}
