// overlap_driver.cpp -- the device overlap's per-chain and per-read code (csrc/fm_overlap.h) compiled for the CPU and run in the kernels'
// order.
//
//   overlap_driver <wide: 0|1> < input
//
// input:  twice (u64 N, u64 n_units, the RL units), of .bwt and of .rbwt; i32 min_overlap; u64 n_reads, n_reads + 1 offsets as u64,
//         the bases as codes 0..3, one per byte.
// The images come from build_strand_image (fm_layout.cpp), Block64 where wide, as lrsc_index_upload would hold them.  Every read is
// one ov_overlap_read: its four chains a lane each, then the reduction as one wavefront of fm_overlap.hip runs it, a phase being
// the kOvLanes lanes one after the other.  A read's workspace is an allocation of exactly ov_workspace_bytes, and its bases, chain
// heads, chain blocks and output blocks are allocations of their own.
// output: n_reads records of 24 bytes (lrsc_overlap_read), the blocks of all reads back to back, 24 bytes each
//         (lrsc_overlap_block), then u64 Occ queries, u64 block loads.  A broken interval ends the run with "FORMAT" and status 3.
static const char kDriver[] = "overlap_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_overlap.h"

using namespace lrsc;

template <class Block>
static int run(const StrandImage im[2], bool wide)
{
    const FmStrand fs[2] = {strand_of(im[0], wide), strand_of(im[1], wide)};
    const StrandView<Block> views[2] = {strand_view<Block>(fs[0]), strand_view<Block>(fs[1])};
    const std::vector<uint32_t> mtab = mask_table<Block>();
    int32_t m = 0;
    read_exact(&m, 4);
    if(m < 2 || (uint32_t)m > kOvMaxMinOverlap) die("the parameters");
    uint64_t n = 0, totals[2] = {0, 0};
    read_exact(&n, 8);
    std::vector<uint64_t> off(n + 1);
    read_exact(off.data(), off.size() * 8);
    std::vector<uint8_t> codes(off[n]);
    read_exact(codes.data(), codes.size());
    OvParams p{(uint32_t)m, 0u};
    for(uint64_t r = 0; r < n; ++r) {
        if(off[r + 1] <= off[r]) die("an empty read");
        if(off[r + 1] - off[r] > kOvMaxRead) die("a read above the limit");
        p.max_len = std::max<uint32_t>(p.max_len, (uint32_t)(off[r + 1] - off[r]));
    }
    const uint32_t slots = ov_slots(p);
    std::vector<OvOutRead> res(n);
    std::vector<OvOutBlock> all;
    for(uint64_t r = 0; r < n; ++r) {
        const std::vector<uint8_t> seq(codes.begin() + (long)off[r], codes.begin() + (long)off[r + 1]);
        std::vector<uint64_t> state(ov_workspace_bytes(p) / 8, 0xA5A5A5A5A5A5A5A5ull);
        const OvWork ws = ov_work_at(reinterpret_cast<uint8_t*>(state.data()), p);
        std::vector<OvChainHead> heads(kOvChains);
        std::vector<OvBlock> chain_blocks((size_t)kOvChains * slots);
        std::vector<OvOutBlock> out(kOvOutCap);
        std::memset(heads.data(), 0xA5, heads.size() * sizeof(OvChainHead));
        SerialWave w;
        uint32_t n_rank = 0, n_blk = 0, bad = 0;
        ov_overlap_read<Block>(views, mtab.data(), seq.data(), (uint32_t)seq.size(), p, heads.data(), chain_blocks.data(), ws, w, out.data(), res[r], bad, n_rank, n_blk);
        if(bad) {
            std::fwrite("FORMAT", 1, 6, stdout);
            return 3;
        }
        res[r].first_block = all.size();
        all.insert(all.end(), out.begin(), out.begin() + res[r].n_blocks);
        totals[0] += n_rank;
        totals[1] += n_blk;
    }
    if(n) std::fwrite(res.data(), sizeof(OvOutRead), n, stdout);
    if(!all.empty()) std::fwrite(all.data(), sizeof(OvOutBlock), all.size(), stdout);
    std::fwrite(totals, 8, 2, stdout);
    return 0;
}

int main(int argc, char** argv)
{
    if(argc != 2) { std::fprintf(stderr, "usage: overlap_driver <wide> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    StrandImage im[2];
    for(int s = 0; s < 2; ++s) read_image(wide, im[s]);
    return wide ? run<Block64>(im, true) : run<Block32>(im, false);
}
