// fmwalk_driver.cpp -- the device FM-index walk's per-lane and per-pair code (csrc/fm_fmwalk.h) compiled for the CPU and run in the kernel's
// order.
//
//   fmwalk_driver <wide: 0|1> < input
//
// input:  twice (u64 N, u64 n_units, the RL units), of .bwt and of .rbwt; i32 kmer_length, kmer_threshold, min_overlap, max_overlap,
//         max_insert, max_leaves; u64 n_pairs, 2 * n_pairs + 1 offsets as u64, the bases as codes 0..3, one per byte.
// The images come from build_strand_image (fm_layout.cpp), Block64 where wide, as lrsc_index_upload would hold them.  Every pair is
// one fw_merge_pair, as one wavefront of fm_fmwalk.hip runs it: a phase is the kFwLanes lanes one after the other.  The workspace
// of a pair is an allocation of exactly fw_workspace_bytes, its reads and its merged string allocations of their own.
// output: n_pairs records of 48 bytes (lrsc_fmwalk_result), n_pairs rows of max(max_insert + 1, min_overlap) codes (0xFF where
//         nothing was written), then u64 Occ queries, u64 block loads.  A broken interval ends the run with "FORMAT" and status 3.
static const char kDriver[] = "fmwalk_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_fmwalk.h"

using namespace lrsc;

template <class Block>
static int run(const StrandImage im[2], bool wide)
{
    static_assert(sizeof(FwResult) == 48 && sizeof(FwParams) == 24, "lrsc_fmwalk_result, lrsc_fmwalk_params");
    const FmStrand fs[2] = {strand_of(im[0], wide), strand_of(im[1], wide)};
    const StrandView<Block> views[2] = {strand_view<Block>(fs[0]), strand_view<Block>(fs[1])};
    const std::vector<uint32_t> mtab = mask_table<Block>();
    FwParams p;
    read_exact(&p, sizeof(p));
    if(p.kmer_length <= 0 || p.kmer_threshold <= 0 || p.min_overlap < 2 || (p.max_overlap <= 0 && p.max_overlap != -1) || p.max_insert <= 0 || p.max_leaves <= 0 ||
       (uint32_t)p.max_leaves > kFwMaxLeaves || (uint32_t)p.max_insert > kFwMaxInsert || (uint32_t)p.min_overlap > kFwMaxOverlap || (uint32_t)p.kmer_length > kFwMaxKmer)
        die("the parameters");
    uint64_t n = 0, totals[2] = {0, 0};
    read_exact(&n, 8);
    std::vector<uint64_t> off(2 * n + 1);
    read_exact(off.data(), off.size() * 8);
    const uint64_t total = off[2 * n];
    std::vector<uint8_t> codes(total);
    read_exact(codes.data(), total);
    const uint64_t stride = (uint64_t)(p.max_insert + 1 > p.min_overlap ? p.max_insert + 1 : p.min_overlap);
    std::vector<FwResult> res(n);
    std::vector<uint8_t> out(n * stride, 0xFF);
    for(uint64_t r = 0; r < n; ++r) {
        if(off[2 * r + 1] <= off[2 * r] || off[2 * r + 2] <= off[2 * r + 1]) die("an empty read");
        // the pair's own bytes, so that a step beyond them is one beyond an allocation
        const std::vector<uint8_t> r1(codes.begin() + (long)off[2 * r], codes.begin() + (long)off[2 * r + 1]);
        const std::vector<uint8_t> r2(codes.begin() + (long)off[2 * r + 1], codes.begin() + (long)off[2 * r + 2]);
        std::vector<uint64_t> state(fw_workspace_bytes(p) / 8, 0xA5A5A5A5A5A5A5A5ull);
        const FwWork ws = fw_work_at(reinterpret_cast<uint8_t*>(state.data()), p);
        std::vector<uint8_t> merged(stride, 0xFF);
        SerialWave w;
        uint32_t n_rank = 0, n_blk = 0, bad = 0;
        fw_merge_pair<Block>(views, mtab.data(), r1.data(), (uint32_t)r1.size(), r2.data(), (uint32_t)r2.size(), p, ws, w, merged.data(), res[r], bad, n_rank,
                             n_blk);
        if(bad) {
            std::fwrite("FORMAT", 1, 6, stdout);
            return 3;
        }
        std::memcpy(out.data() + r * stride, merged.data(), stride);
        totals[0] += n_rank;
        totals[1] += n_blk;
    }
    if(n) std::fwrite(res.data(), sizeof(FwResult), n, stdout);
    if(n) std::fwrite(out.data(), 1, out.size(), stdout);
    std::fwrite(totals, 8, 2, stdout);
    return 0;
}

int main(int argc, char** argv)
{
    if(argc != 2) { std::fprintf(stderr, "usage: fmwalk_driver <wide> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    StrandImage im[2];
    for(int s = 0; s < 2; ++s) read_image(wide, im[s]);
    return wide ? run<Block64>(im, true) : run<Block32>(im, false);
}
