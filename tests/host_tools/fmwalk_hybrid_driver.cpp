// fmwalk_hybrid_driver.cpp -- fmwalk's hybrid and kmerize algorithms and the sampled k-mer counts (csrc/fm_kmerize.h) compiled for the CPU
// and run in the kernels' order.
//
//   fmwalk_hybrid_driver <wide: 0|1> <hybrid|kmerize|sample|filters> < input
//
// input:  twice (u64 N, u64 n_units, the RL units), of .bwt and of .rbwt; then
//   hybrid   i32 kmer_length, kmer_threshold, min_overlap, max_overlap, max_insert, max_leaves; u64 repeat_kmer_freq; u64 n_pairs,
//            2 * n_pairs + 1 offsets as u64, the bases as codes 0..3, one per byte
//   kmerize  i32 kmer_length, kmer_threshold; u64 n_reads, n_reads + 1 offsets, the codes
//   sample   u32 len; u64 n, n rows as u64
//   filters  u64 n, n + 1 offsets, the codes of n strings (the images are read and not used)
// The images come from build_strand_image (fm_layout.cpp), Block64 where wide.  Every pair is one km_hybrid_pair and every read one
// km_split, as one wavefront of fm_kmerize.hip runs them: a phase is the kKmLanes lanes one after the other.  The workspaces of a
// pair or read are allocations of exactly fw_workspace_bytes and km_workspace_bytes, its reads, its merged string and its pieces
// allocations of their own.
// output:
//   hybrid   n_pairs records of 96 bytes (lrsc_fmwalk_hybrid_result), n_pairs rows of max(max_insert + 1, min_overlap) codes (0xFF
//            where nothing was written), the piece slots of all reads (12 bytes each, 0xFF where nothing was written)
//   kmerize  n_reads records of 24 bytes (lrsc_fmwalk_read_result), the piece slots
//   sample   n counts as u32
//   filters  per string u64 km_max_con, u64 km_low_complexity
// then u64 Occ queries, u64 block loads.  A broken interval ends the run with "FORMAT" and status 3.
static const char kDriver[] = "fmwalk_hybrid_driver";
#include "strand_driver.h"

#include "../../longreadselfcorrect_amd/csrc/fm_kmerize.h"

using namespace lrsc;

static int broken()
{
    std::fwrite("FORMAT", 1, 6, stdout);
    return 3;
}

struct Reads {
    std::vector<uint64_t> off, slot;
    std::vector<uint8_t> codes;
    // the read's own bytes, so that a step beyond them is one beyond an allocation
    std::vector<uint8_t> read(uint64_t i) const { return std::vector<uint8_t>(codes.begin() + (long)off[i], codes.begin() + (long)off[i + 1]); }
    uint64_t slots(uint64_t i) const { return slot[i + 1] - slot[i]; }
};
static Reads read_reads(uint64_t n, uint32_t k)
{
    Reads r;
    r.off.resize(n + 1);
    read_exact(r.off.data(), r.off.size() * 8);
    r.codes.resize(r.off[n]);
    read_exact(r.codes.data(), r.codes.size());
    r.slot.assign(n + 1, 0);
    for(uint64_t i = 0; i < n; ++i) {
        if(r.off[i + 1] <= r.off[i]) die("an empty read");
        const uint64_t len = r.off[i + 1] - r.off[i];
        r.slot[i + 1] = r.slot[i] + (len >= k ? len - k + 1 : 0);
    }
    return r;
}

template <class Block>
static int run_hybrid(const StrandView<Block>* views, const uint32_t* mtab, uint64_t totals[2])
{
    static_assert(sizeof(KmHybrid) == 96 && sizeof(KmRead) == 24 && sizeof(KmPiece) == 12, "lrsc_fmwalk_hybrid_result, _read_result, _piece");
    FwParams p;
    uint64_t repeat = 0, n = 0;
    read_exact(&p, sizeof(p));
    read_exact(&repeat, 8);
    if(p.kmer_length <= 0 || p.kmer_threshold <= 0 || p.min_overlap < 2 || (p.max_overlap <= 0 && p.max_overlap != -1) || p.max_insert <= 0 || p.max_leaves <= 0 ||
       (uint32_t)p.max_leaves > kFwMaxLeaves || (uint32_t)p.max_insert > kFwMaxInsert || (uint32_t)p.min_overlap > kFwMaxOverlap || (uint32_t)p.kmer_length > kFwMaxKmer)
        die("the parameters");
    read_exact(&n, 8);
    const Reads in = read_reads(2 * n, (uint32_t)p.kmer_length);
    const uint64_t stride = (uint64_t)(p.max_insert + 1 > p.min_overlap ? p.max_insert + 1 : p.min_overlap);
    std::vector<KmHybrid> res(n);
    std::vector<uint8_t> out(n * stride, 0xFF);
    std::vector<KmPiece> pieces(in.slot[2 * n], KmPiece{~0u, ~0u, ~0u});
    for(uint64_t r = 0; r < n; ++r) {
        const std::vector<uint8_t> r1 = in.read(2 * r), r2 = in.read(2 * r + 1);
        std::vector<uint64_t> state(fw_workspace_bytes(p) / 8, 0xA5A5A5A5A5A5A5A5ull);
        const uint32_t longest = (uint32_t)(r1.size() > r2.size() ? r1.size() : r2.size());
        std::vector<uint64_t> kstate(km_workspace_bytes(longest) / 8, 0xA5A5A5A5A5A5A5A5ull);
        const FwWork ws = fw_work_at(reinterpret_cast<uint8_t*>(state.data()), p);
        const KmWork kws = km_work_at(reinterpret_cast<uint8_t*>(kstate.data()), longest);
        std::vector<uint8_t> merged(stride, 0xFF);
        std::vector<KmPiece> own[2] = {std::vector<KmPiece>(in.slots(2 * r), KmPiece{~0u, ~0u, ~0u}), std::vector<KmPiece>(in.slots(2 * r + 1), KmPiece{~0u, ~0u, ~0u})};
        KmPiece* const to[2] = {own[0].data(), own[1].data()};
        SerialWave w;
        uint32_t n_rank = 0, n_blk = 0, bad = 0;
        km_hybrid_pair<Block>(views, mtab, r1.data(), (uint32_t)r1.size(), r2.data(), (uint32_t)r2.size(), p, repeat, ws, kws, w, merged.data(), res[r], to, bad, n_rank,
                              n_blk);
        if(bad) return broken();
        std::memcpy(out.data() + r * stride, merged.data(), stride);
        for(uint32_t e = 0; e < 2; ++e)
            if(!own[e].empty()) std::memcpy(pieces.data() + in.slot[2 * r + e], own[e].data(), own[e].size() * sizeof(KmPiece));
        totals[0] += n_rank;
        totals[1] += n_blk;
    }
    if(n) std::fwrite(res.data(), sizeof(KmHybrid), n, stdout);
    if(n) std::fwrite(out.data(), 1, out.size(), stdout);
    if(!pieces.empty()) std::fwrite(pieces.data(), sizeof(KmPiece), pieces.size(), stdout);
    return 0;
}

template <class Block>
static int run_kmerize(const StrandView<Block>* views, const uint32_t* mtab, uint64_t totals[2])
{
    int32_t kx[2];
    uint64_t n = 0;
    read_exact(kx, 8);
    if(kx[0] <= 0 || kx[1] <= 0 || (uint32_t)kx[0] > kFwMaxKmer) die("the parameters");
    read_exact(&n, 8);
    const uint32_t k = (uint32_t)kx[0];
    const Reads in = read_reads(n, k);
    std::vector<KmRead> res(n, KmRead{0u, 0, 0u, 0u, -1, 0u});
    std::vector<KmPiece> pieces(in.slot[n], KmPiece{~0u, ~0u, ~0u});
    for(uint64_t r = 0; r < n; ++r) {
        const std::vector<uint8_t> read = in.read(r);
        if(read.size() < k) continue;                             // KmerizeReads returns at once
        std::vector<uint64_t> kstate(km_workspace_bytes((uint32_t)read.size()) / 8, 0xA5A5A5A5A5A5A5A5ull);
        const KmWork kws = km_work_at(reinterpret_cast<uint8_t*>(kstate.data()), (uint32_t)read.size());
        std::vector<KmPiece> own(in.slots(r), KmPiece{~0u, ~0u, ~0u});
        uint32_t att[kKmLanes];
        SerialWave w;
        uint32_t n_rank = 0, n_blk = 0, bad = 0;
        res[r].length = (uint32_t)read.size();
        km_split<Block>(views[0], mtab, read.data(), (uint32_t)read.size(), k, (uint32_t)kx[1], false, kws, att, w, own.data(), res[r].n_pieces, res[r].main_piece, bad,
                        n_rank, n_blk);
        if(bad) return broken();
        res[r].kmerize = 1;
        std::memcpy(pieces.data() + in.slot[r], own.data(), own.size() * sizeof(KmPiece));
        totals[0] += n_rank;
        totals[1] += n_blk;
    }
    if(n) std::fwrite(res.data(), sizeof(KmRead), n, stdout);
    if(!pieces.empty()) std::fwrite(pieces.data(), sizeof(KmPiece), pieces.size(), stdout);
    return 0;
}

template <class Block>
static int run_sample(const StrandView<Block>* views, const uint32_t* mtab, uint64_t totals[2])
{
    uint32_t len = 0;
    uint64_t n = 0;
    read_exact(&len, 4);
    read_exact(&n, 8);
    if(len == 0 || len > kKmMaxSampleLength) die("the parameters");
    std::vector<uint64_t> rows(n);
    read_exact(rows.data(), n * 8);
    std::vector<uint32_t> counts(n);
    for(uint64_t i = 0; i < n; ++i) {
        if(rows[i] >= views[1].n_dollars) die("a row that is no string's");
        std::vector<uint8_t> row(len, 0xFF);                      // the sample's workspace row
        uint32_t n_rank = 0, n_blk = 0, bad = 0;
        counts[i] = (uint32_t)km_sample_count<Block>(views[1], mtab, rows[i], len, row.data(), bad, n_rank, n_blk);
        if(bad) return broken();
        totals[0] += n_rank;
        totals[1] += n_blk;
    }
    if(n) std::fwrite(counts.data(), 4, n, stdout);
    return 0;
}

static int run_filters()
{
    uint64_t n = 0;
    read_exact(&n, 8);
    const Reads in = read_reads(n, 1);
    std::vector<uint64_t> out(2 * n);
    for(uint64_t i = 0; i < n; ++i) {
        const std::vector<uint8_t> s = in.read(i);
        out[2 * i] = km_max_con(s.data(), (uint32_t)s.size());
        out[2 * i + 1] = km_low_complexity(s.data(), (uint32_t)s.size()) ? 1 : 0;
    }
    if(n) std::fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}

template <class Block>
static int run(const StrandImage im[2], bool wide, const std::string& mode)
{
    const FmStrand fs[2] = {strand_of(im[0], wide), strand_of(im[1], wide)};
    const StrandView<Block> views[2] = {strand_view<Block>(fs[0]), strand_view<Block>(fs[1])};
    const std::vector<uint32_t> mtab = mask_table<Block>();
    uint64_t totals[2] = {0, 0};
    int st = 2;
    if(mode == "hybrid") st = run_hybrid<Block>(views, mtab.data(), totals);
    else if(mode == "kmerize") st = run_kmerize<Block>(views, mtab.data(), totals);
    else if(mode == "sample") st = run_sample<Block>(views, mtab.data(), totals);
    else if(mode == "filters") st = run_filters();
    else die("the mode");
    if(st == 0) std::fwrite(totals, 8, 2, stdout);
    return st;
}

int main(int argc, char** argv)
{
    if(argc != 3) { std::fprintf(stderr, "usage: fmwalk_hybrid_driver <wide> <hybrid|kmerize|sample|filters> < input\n"); return 2; }
    const bool wide = std::atoi(argv[1]) != 0;
    StrandImage im[2];
    for(int s = 0; s < 2; ++s) read_image(wide, im[s]);
    return wide ? run<Block64>(im, true, argv[2]) : run<Block32>(im, false, argv[2]);
}
