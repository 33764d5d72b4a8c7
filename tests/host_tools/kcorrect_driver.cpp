// kcorrect_driver.cpp -- the device k-mer corrector's per-lane and per-read code (csrc/fm_kcorrect.h) compiled for the CPU and run in the
// kernel's order.
//
//   kcorrect_driver <wide: 0|1> < input
//
// input:  u64 N, u64 n_units, the RL units of .bwt; i32 kmer_length, kmer_threshold, kmer_rounds, quality_cutoff; u64 n, n + 1
//         offsets as u64, the bases as codes 0..3, one per byte; u64 has_phred, then one score per base when it is 1.
// The image comes from build_strand_image (fm_layout.cpp), Block64 where wide, as lrsc_index_upload would hold it.  Every read is
// one kc_correct_read, as one wavefront of fm_kcorrect.hip runs it: a phase is the kKcLanes lanes one after the other.  The state
// of a read is an allocation of exactly kc_workspace_bytes of its length, whatever its length.
// output: n records of 16 bytes (lrsc_kcorrect_result), the corrected codes, then u64 Occ queries, u64 block loads.
//         A broken chain ends the run with "FORMAT" and status 3.
static const char kDriver[] = "kcorrect_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_kcorrect.h"

using namespace lrsc;

template <class Block>
static int run(const StrandImage& im, bool wide)
{
    static_assert(sizeof(KcResult) == 16 && sizeof(KcParams) == 16, "lrsc_kcorrect_result, lrsc_kcorrect_params");
    const FmStrand fs = strand_of(im, wide);
    const StrandView<Block> S = strand_view<Block>(fs);
    const std::vector<uint32_t> mtab = mask_table<Block>();
    KcParams p;
    read_exact(&p, sizeof(p));
    if(p.kmer_length <= 0 || p.kmer_threshold <= 0 || p.kmer_rounds <= 0) die("the parameters");
    uint64_t n = 0, has_phred = 0, totals[2] = {0, 0};
    read_exact(&n, 8);
    std::vector<uint64_t> off(n + 1);
    read_exact(off.data(), off.size() * 8);
    const uint64_t total = off[n];
    std::vector<uint8_t> codes(total), phred, out(total);
    read_exact(codes.data(), total);
    read_exact(&has_phred, 8);
    if(has_phred) {
        phred.resize(total);
        read_exact(phred.data(), total);
    }
    std::vector<KcResult> res(n);
    for(uint64_t r = 0; r < n; ++r) {
        if(off[r + 1] <= off[r] || off[r + 1] - off[r] >= (1ull << 31)) die("an empty read");
        const uint32_t len = (uint32_t)(off[r + 1] - off[r]);
        std::vector<uint32_t> state(kc_workspace_bytes(len) / 4, 0xA5A5A5A5u);
        const KcState st = kc_state_at(reinterpret_cast<uint8_t*>(state.data()), len);
        // the read's own bytes, so that a step beyond them is one beyond an allocation
        const std::vector<uint8_t> mine(codes.begin() + (long)off[r], codes.begin() + (long)off[r + 1]);
        std::vector<uint8_t> scores, corrected(len);
        if(has_phred) scores.assign(phred.begin() + (long)off[r], phred.begin() + (long)off[r + 1]);
        SerialWave w;
        uint32_t n_rank = 0, n_blk = 0;
        if(!kc_correct_read<Block>(S, mtab.data(), mine.data(), has_phred ? scores.data() : nullptr, len, p, st, w, corrected.data(), res[r], n_rank, n_blk)) {
            std::fwrite("FORMAT", 1, 6, stdout);
            return 3;
        }
        std::memcpy(out.data() + off[r], corrected.data(), len);
        totals[0] += n_rank;
        totals[1] += n_blk;
    }
    if(n) std::fwrite(res.data(), sizeof(KcResult), n, stdout);
    if(total) std::fwrite(out.data(), 1, total, stdout);
    std::fwrite(totals, 8, 2, stdout);
    return 0;
}

int main(int argc, char** argv)
{
    if(argc != 2) { std::fprintf(stderr, "usage: kcorrect_driver <wide> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    StrandImage im;
    read_image(wide, im);
    return wide ? run<Block64>(im, true) : run<Block32>(im, false);
}
