// dup_driver.cpp -- the device duplicate check's per-lane functions (csrc/fm_dup.h) compiled for the CPU and run in the kernels' order.
//
//   dup_driver <wide: 0|1> < input
//
// input:  for .bwt, then for .rbwt: u64 N, u64 n_units, the RL units of the strand's BWT; u64 n_calls; per call u64 n, n + 1
//         offsets as u64, the bases as codes 0..3, one per byte.
// The two images come from build_strand_image (fm_layout.cpp), Block64 where wide, as lrsc_index_upload would hold them.  One
// session (bit vector, winner words) serves all calls, as one lrsc_dupcheck does.  Per call, as fm_dup.hip does: dup_chain for
// every read, kind by kind; dup_combine and the claim of the slot for every read; dup_classify for every read; then the bits
// are set and the winner words released.  A broken chain or a winner word left claimed ends the run.
// output: per call n records of 40 bytes (lrsc_dup_result); then u64 Occ queries, u64 block loads of all chains.
static const char kDriver[] = "dup_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_dup.h"

using namespace lrsc;

template <class Block>
static void run(const StrandImage& i0, const StrandImage& i1, bool wide)
{
    static_assert(sizeof(DupResult) == 40, "lrsc_dup_result");
    const FmStrand f0 = strand_of(i0, wide), f1 = strand_of(i1, wide);
    const StrandView<Block> S[2] = {strand_view<Block>(f0), strand_view<Block>(f1)};
    const std::vector<uint32_t> mtab = mask_table<Block>();
    const uint64_t n_slots = S[0].n_dollars;
    if(n_slots == 0 || S[1].n_dollars != n_slots) die("the strands hold no reads, or not the same number");
    std::vector<uint32_t> bits((n_slots + 31) / 32, 0u), winner(n_slots, kDupNoWinner);
    uint64_t n_calls = 0, totals[2] = {0, 0};
    read_exact(&n_calls, 8);
    for(uint64_t call = 0; call < n_calls; ++call) {
        uint64_t n = 0;
        read_exact(&n, 8);
        std::vector<uint64_t> off(n + 1);
        read_exact(off.data(), off.size() * 8);
        const uint64_t total = off[n];
        std::vector<uint32_t> words(total / 4 + 1, 0xA5A5A5A5u);  // what lies behind the last base is anything
        read_exact(words.data(), total);
        // 1. the chains, kind by kind
        std::vector<DupChainOut> chains(kDupKinds * n);
        for(uint32_t kind = 0; kind < kDupKinds; ++kind)
            for(uint64_t r = 0; r < n; ++r) {
                if(off[r + 1] <= off[r] || off[r + 1] - off[r] >= (1ull << 32)) die("an empty read");
                uint32_t n_rank = 0, n_blk = 0;
                chains[kind * n + r] = dup_chain<Block>(S[dup_kind_strand(kind)], mtab.data(), words.data(), off[r], (uint32_t)(off[r + 1] - off[r]), kind,
                                                        n_rank, n_blk);
                totals[0] += n_rank;
                totals[1] += n_blk;
            }
        // 2. combine and claim
        std::vector<DupResult> res(n);
        std::vector<uint64_t> slots(n);
        for(uint64_t r = 0; r < n; ++r) {
            if(!dup_combine(dup_dollars(S[0]), S[0].N, chains[r], chains[n + r], chains[2 * n + r], chains[3 * n + r], n_slots, res[r], slots[r])) die("a broken chain");
            if(slots[r] < n_slots && (uint32_t)r < winner[slots[r]]) winner[slots[r]] = (uint32_t)r;
        }
        // 3. classify
        for(uint64_t r = 0; r < n; ++r)
            if(slots[r] < n_slots) res[r].cls = dup_classify(((bits[slots[r] >> 5] >> (slots[r] & 31)) & 1u) != 0, winner[slots[r]], (uint32_t)r);
        // 4. commit
        for(uint64_t r = 0; r < n; ++r)
            if(slots[r] < n_slots) {
                bits[slots[r] >> 5] |= 1u << (slots[r] & 31);
                winner[slots[r]] = kDupNoWinner;
            }
        for(uint32_t w : winner) if(w != kDupNoWinner) die("a winner word left claimed");
        if(n) std::fwrite(res.data(), sizeof(DupResult), n, stdout);
    }
    std::fwrite(totals, 8, 2, stdout);
}

int main(int argc, char** argv)
{
    if(argc != 2) { std::fprintf(stderr, "usage: dup_driver <wide> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    StrandImage i0, i1;
    read_image(wide, i0);
    read_image(wide, i1);
    if(wide) run<Block64>(i0, i1, true);
    else run<Block32>(i0, i1, false);
    return 0;
}
