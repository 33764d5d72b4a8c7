// locate_driver.cpp -- the device locate's per-lane functions (csrc/fm_locate.h) compiled for the CPU and run in the kernels' order.
//
//   locate_driver <wide: 0|1> <rate> < input
//
// input:  u64 N, u64 n_units, the RL units of the strand's BWT.
// The image comes from build_strand_image (fm_layout.cpp), Block64 where wide, as lrsc_index_upload would hold it.  Then, as
// fm_locate.hip does: the tables start as 0xFF bytes, locate_prepare_read for every read, locate_fix_sample for every sample,
// locate_row for every row of the strand.  A walk that reports kWalkBroken, a table entry written twice or never, ends the run.
// output: u64 n, order[] as u32; u64 n, read_len[] as u32; u64 n_samples, the samples as (u32 read, u32 pos); u64 N, the located
// (u32 read, u32 pos) of every row; u64 1, the LF steps of all locate walks as u64.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../longreadselfcorrect_amd/csrc/fm_layout.h"
#include "../../longreadselfcorrect_amd/csrc/fm_locate.h"

using namespace lrsc;

static void die(const char* what)
{
    std::fprintf(stderr, "locate_driver: %s\n", what);
    std::exit(1);
}

static FmStrand strand_of(const StrandImage& im, bool wide)
{
    FmStrand fs;
    fs.blocks = im.blocks.data();
    fs.dollars = im.dollars.data();
    fs.dollar_dir = im.dollar_dir.data();
    fs.dollar_group_syms = (uint64_t)(wide ? Block64::kSyms : Block32::kSyms) << kDollarDirShift;
    fs.n_dollars = im.dollars.size();
    fs.n_symbols = im.n_symbols;
    fs.n_blocks = im.n_blocks;
    for(int c = 0; c < 5; ++c) fs.pred[c] = im.pred[c];
    return fs;
}

template <class T>
static void dump(const std::vector<T>& v)
{
    const uint64_t n = v.size();
    std::fwrite(&n, 8, 1, stdout);
    if(n) std::fwrite(v.data(), sizeof(T), v.size(), stdout);
}

template <class Block>
static void locate(const StrandImage& im, bool wide, uint32_t rate)
{
    const FmStrand fs = strand_of(im, wide);
    const StrandView<Block> S = strand_view<Block>(fs);
    std::vector<uint32_t> mtab(MaskTab<Block>::kWords);
    for(uint32_t i = 0; i < mtab.size(); ++i) mtab[i] = mask_word<Block>(i);
    const uint64_t n = S.n_dollars, N = S.N;
    if(n == 0) die("the strand holds no read");

    // 1. the walks
    const SaElem unset{kLocateUnset, kLocateUnset};
    std::vector<SaElem> samples(locate_sample_count(N, rate), unset);
    std::vector<uint32_t> order(n, kLocateUnset), read_len(n, kLocateUnset);
    for(uint64_t read = 0; read < n; ++read)
        if(locate_prepare_read<Block>(S, mtab.data(), (uint32_t)read, rate, samples.data(), order.data(), read_len.data()) != kWalkOk)
            die("a prepare walk did not end");
    uint64_t total = n;
    for(uint64_t i = 0; i < n; ++i) {
        if(order[i] == kLocateUnset || read_len[i] == kLocateUnset) die("an order / length entry never written");
        total += read_len[i];
    }
    if(total != N) die("the walks do not cover the strand");

    // 2. the fix-up
    for(uint64_t slot = 0; slot < samples.size(); ++slot)
        if(locate_fix_sample(samples[slot], slot, rate, N, read_len.data(), n) != kWalkOk) die("a sample never written");

    // 3. locate of every row
    std::vector<SaElem> located(N);
    uint64_t steps = 0;
    for(uint64_t row = 0; row < N; ++row) {
        uint32_t st = 0;
        if(locate_row<Block>(S, mtab.data(), row, rate, samples.data(), order.data(), located[row], st) != kWalkOk) die("a locate walk did not end");
        steps += st;
    }
    SaElem e;
    uint32_t st = 0;
    if(locate_row<Block>(S, mtab.data(), N, rate, samples.data(), order.data(), e, st) != kWalkBroken) die("a row beyond the strand was located");
    dump(order);
    dump(read_len);
    dump(samples);
    dump(located);
    dump(std::vector<uint64_t>(1, steps));
}

int main(int argc, char** argv)
{
    if(argc != 3) { std::fprintf(stderr, "usage: locate_driver <wide> <rate> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    const uint32_t rate = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    uint64_t hdr[2];
    if(std::fread(hdr, 8, 2, stdin) != 2) die("short input");
    std::vector<uint8_t> units(hdr[1]);
    if(hdr[1] && std::fread(units.data(), 1, hdr[1], stdin) != hdr[1]) die("short input");
    StrandImage im;
    std::string err;
    if(build_strand_image(units.data(), units.size(), hdr[0], wide, im, err) != 0) die(err.c_str());
    if(wide) locate<Block64>(im, true, rate);
    else locate<Block32>(im, false, rate);
    return 0;
}
