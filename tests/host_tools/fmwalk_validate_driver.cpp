// fmwalk_validate_driver.cpp -- fmwalk's validate algorithm (csrc/fm_validate.h) compiled for the CPU and run in the kernels' order.
//
//   fmwalk_validate_driver <wide: 0|1> < input
//
// input:  twice (u64 N, u64 n_units, the RL units), of .bwt and of .rbwt; then i32 kmer_length, kmer_threshold, min_overlap,
//         max_overlap, max_insert (read and not used), max_leaves; u64 n_reads, n_reads + 1 offsets as u64, the bases as codes 0..3,
//         one per byte.  A kmer_threshold of 0, which lrsc_fmwalk_validate refuses, is taken: the split's threshold then wraps.
// The images come from build_strand_image (fm_layout.cpp), Block64 where wide.  Every read is one vd_read, as the wavefronts of
// fm_validate.hip and the entry run it between them: a phase is the kVdLanes lanes one after the other.  The workspaces are
// allocations of exactly fw_workspace_bytes, with max_insert = vd_depth of the longest read as the entry sets it, and
// km_workspace_bytes of the read; the read, its sequence and its pieces are allocations of their own.
// output: n_reads records of 80 bytes (lrsc_fmwalk_validate_result), n_reads rows of vd_depth(longest) + 1 codes (0xFF where nothing
// was written), the piece slots of all reads (12 bytes each, 0xFF where nothing was written), then u64 Occ queries, u64 block
// loads.  A broken interval ends the run with "FORMAT" and status 3.
static const char kDriver[] = "fmwalk_validate_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_validate.h"

using namespace lrsc;

template <class Block>
static int run(const StrandImage im[2], bool wide)
{
    static_assert(sizeof(VdResult) == 80 && sizeof(KmPiece) == 12, "lrsc_fmwalk_validate_result, lrsc_fmwalk_piece");
    const FmStrand fs[2] = {strand_of(im[0], wide), strand_of(im[1], wide)};
    const StrandView<Block> views[2] = {strand_view<Block>(fs[0]), strand_view<Block>(fs[1])};
    const std::vector<uint32_t> mtab = mask_table<Block>();
    FwParams p;
    uint64_t n = 0;
    read_exact(&p, sizeof(p));
    if(p.kmer_length <= 0 || p.kmer_threshold < 0 || p.min_overlap < 2 || (p.max_overlap <= 0 && p.max_overlap != -1) || p.max_leaves <= 0 ||
       (uint32_t)p.max_leaves > kFwMaxLeaves || (uint32_t)p.min_overlap > kFwMaxOverlap || (uint32_t)p.kmer_length > kFwMaxKmer)
        die("the parameters");
    read_exact(&n, 8);
    std::vector<uint64_t> off(n + 1), slot(n + 1, 0);
    read_exact(off.data(), off.size() * 8);
    std::vector<uint8_t> codes(off[n]);
    read_exact(codes.data(), codes.size());
    const uint32_t k = (uint32_t)p.kmer_length;
    uint64_t longest = 0;
    for(uint64_t i = 0; i < n; ++i) {
        if(off[i + 1] <= off[i]) die("an empty read");
        const uint64_t len = off[i + 1] - off[i];
        if(vd_depth((uint32_t)len) + 1 > kFwMaxInsert) die("a read above the limit");
        longest = len > longest ? len : longest;
        slot[i + 1] = slot[i] + (len >= k ? len - k + 1 : 0);
    }
    p.max_insert = (int32_t)vd_depth((uint32_t)longest);
    const uint64_t stride = (uint64_t)p.max_insert + 1;
    std::vector<VdResult> res(n);
    std::vector<uint8_t> out(n * stride, 0xFF);
    std::vector<KmPiece> pieces(slot[n], KmPiece{~0u, ~0u, ~0u});
    uint64_t totals[2] = {0, 0};
    for(uint64_t r = 0; r < n; ++r) {
        // the read's own bytes, so that a step beyond them is one beyond an allocation
        const std::vector<uint8_t> read(codes.begin() + (long)off[r], codes.begin() + (long)off[r + 1]);
        std::vector<uint64_t> state(fw_workspace_bytes(p) / 8, 0xA5A5A5A5A5A5A5A5ull);
        std::vector<uint64_t> kstate(km_workspace_bytes((uint32_t)read.size()) / 8, 0xA5A5A5A5A5A5A5A5ull);
        const FwWork ws = fw_work_at(reinterpret_cast<uint8_t*>(state.data()), p);
        const KmWork kws = km_work_at(reinterpret_cast<uint8_t*>(kstate.data()), (uint32_t)read.size());
        std::vector<uint8_t> seq(stride, 0xFF);
        std::vector<KmPiece> own(slot[r + 1] - slot[r], KmPiece{~0u, ~0u, ~0u});
        SerialWave w;
        uint32_t n_rank = 0, n_blk = 0, bad = 0;
        vd_read<Block>(views, mtab.data(), read.data(), (uint32_t)read.size(), p, ws, kws, w, seq.data(), res[r], own.data(), bad, n_rank, n_blk);
        if(bad) {
            std::fwrite("FORMAT", 1, 6, stdout);
            return 3;
        }
        std::memcpy(out.data() + r * stride, seq.data(), stride);
        if(!own.empty()) std::memcpy(pieces.data() + slot[r], own.data(), own.size() * sizeof(KmPiece));
        totals[0] += n_rank;
        totals[1] += n_blk;
    }
    if(n) std::fwrite(res.data(), sizeof(VdResult), n, stdout);
    if(n) std::fwrite(out.data(), 1, out.size(), stdout);
    if(!pieces.empty()) std::fwrite(pieces.data(), sizeof(KmPiece), pieces.size(), stdout);
    std::fwrite(totals, 8, 2, stdout);
    return 0;
}

int main(int argc, char** argv)
{
    if(argc != 2) { std::fprintf(stderr, "usage: fmwalk_validate_driver <wide> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    StrandImage im[2];
    for(int s = 0; s < 2; ++s) read_image(wide, im[s]);
    return wide ? run<Block64>(im, true) : run<Block32>(im, false);
}
