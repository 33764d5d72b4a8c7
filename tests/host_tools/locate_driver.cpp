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
static const char kDriver[] = "locate_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_locate.h"

using namespace lrsc;

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
    const std::vector<uint32_t> mtab = mask_table<Block>();
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
    StrandImage im;
    read_image(wide, im);
    if(wide) locate<Block64>(im, true, rate);
    else locate<Block32>(im, false, rate);
    return 0;
}
