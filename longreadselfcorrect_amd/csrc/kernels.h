// kernels.h -- launch wrappers of the gfx950 kernels (implemented in kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lrsc.h"
#include "fm_device.h"

namespace lrsc {

// device-side counters filled by the kernels.  One ctx owns kCtrShards of them, each on its own 64-byte
// line: every wavefront adds its totals to shard (blockIdx.x % kCtrShards).  (A single shared line was
// measured to throttle the grid kernel: ~49 M same-line atomics per launch at ~88 atomics/us.)
struct alignas(64) DevCounters {
    unsigned long long rank_queries;
    unsigned long long block_loads;
    unsigned long long table_loads;     // k-mer interval table look-ups (16-byte entries, one 64-byte line each)
    unsigned long long pad[5];
};
constexpr uint32_t kCtrShards = 1024;

constexpr uint32_t kMaxPool = 8;
constexpr uint32_t kChunkShift = 10;   // coarse position -> read table granularity (1024 bases)

struct GridArgs {
    const uint8_t* codes;         // one byte per base, 0..3 (A,C,G,T)
    const uint64_t* read_off;     // n_reads + 1
    const uint32_t* chunk_read;   // read containing position (chunk << kChunkShift)
    uint64_t total_bases;
    uint32_t n_reads;
    uint32_t n_k;
    uint8_t ks[kMaxPool];
    // full outputs (any may be null)
    lrsc_biinterval* out_iv;      // [pos * n_k + slot]
    uint8_t* out_size;            // [pos * n_k + slot]
    uint8_t* out_count;           // [(pos * n_k + slot) * 4]
    // compact outputs (any may be null): structure-of-arrays, slot-major
    int32_t* freq;                // [freq_index[slot] * total_bases + pos]  KmerFeature::getFreq() (-1 == fake)
    int8_t freq_index[kMaxPool];  // compact row of `freq` for a slot, -1 = not stored
    uint8_t* valid_mask;          // [pos] bit freq_index[slot] = both strands' intervals valid (KmerFeature::isValid)
    uint8_t* base_counted;        // [pos] chars counted by the base-slot search (<= ks[0])
    lrsc_biinterval* slot_iv;     // [slot * total_bases + pos] (only if non-null)
};

// LongReadProbe on the device (seeds.hip)
constexpr uint32_t kSeedInts = 8;   // seedStartPos, seedLen, maxFixedMerFreq, isRepeat, startBestK, endBestK, startKmerFreq, endKmerFreq
struct SeedArgs {
    const uint8_t* codes;
    const uint64_t* read_off;
    const uint32_t* chunk_read;
    uint64_t total_bases;
    uint32_t n_reads;
    // grid features (see GridArgs)
    const int32_t* freq;
    const uint8_t* valid_mask;
    const uint8_t* base_counted;
    int8_t row_of_k[64];          // freq row of a k-mer size, -1 if that size is not in the pool
    uint32_t base_k;
    // ProbeParameters (PacBio/LongReadProbe.h:7-40)
    int32_t start_kmer_len, scan_kmer_len, kmer_len_up_bound, pb_coverage, mode, manual, radius;
    int32_t offset[3];
    float hh_ratio;
    const float* thresholds;      // KmerThreshold table, [3][52]
    // scratch / outputs
    unsigned long long* flags;    // [pos] (repeat) | (garbage << 32), later its inclusive scan
    uint32_t* zeros;              // [pos] zero-frequency non-low-complexity scan k-mers, later its inclusive scan
    uint8_t* attribute;           // [pos] 1 unique / 2 repeat (LongReadProbe::getSeqAttribute)
    float* ratio;                 // [pos] the repeat ratio behind `attribute` (extend/<read>.log of --debugseed), or nullptr
    unsigned long long* start_bits;   // bit pos: the static k-mer at pos passes the scan's first-iteration tests (a seed can start here)
    int32_t* seeds;               // kSeedInts per seed, read r's slab starts at seed_slab(r)
    uint32_t* seed_count;         // [read]
    // --debugseed (both null otherwise): the seeds removeHitchhikingSeeds drops, same slab layout as `seeds`
    int32_t* outcasts;
    uint32_t* outcast_count;      // [read]
};
// first seed record of read r: reads can hold at most len/15 + 1 seeds (static k-mers are >= 15 long... any k >= 1: len + 1)
__host__ __device__ inline uint64_t seed_slab(uint64_t read_start, uint32_t r, uint32_t min_k) { return read_start / min_k + r; }

hipError_t launch_seed_modes(const SeedArgs& a, hipStream_t stream);
hipError_t launch_seed_attribute(const SeedArgs& a, hipStream_t stream);
hipError_t launch_seed_scan(const FmIndexDev& fm, const SeedArgs& a, uint32_t min_k, DevCounters* ctr, hipStream_t stream);
// inclusive scans of SeedArgs::flags / zeros in place (hipCUB); tmp is grown as needed
hipError_t scan_seed_flags(unsigned long long* flags, uint32_t* zeros, uint64_t n, void** tmp, size_t* tmp_cap, hipStream_t stream);

// fills a k-mer interval table (4^k uint4 entries) by running the k-step findBiInterval of every k-mer
hipError_t launch_ktab_build(const FmIndexDev& fm, uint32_t k, void* entries, uint32_t prev_k, const void* prev, hipStream_t stream);
hipError_t launch_rank(const FmIndexDev& fm, const lrsc_rank_query* q, uint64_t n, uint64_t* out,
                       DevCounters* ctr, hipStream_t stream);
// LF-walk (LongReadOverlap::retrieveStr, PacBio/LongReadOverlap.cpp:696-749): from BWT row `row` of `strand`,
// b = BWT[idx]; stop at '$' or after max_steps; idx = C[b] + Occ(b, idx - 1).  out codes (0..3), out_len.
struct LfJob { uint64_t row; uint64_t out_off; uint32_t max_steps; uint32_t strand; };
hipError_t launch_lf_walk(const FmIndexDev& fm, const LfJob* jobs, uint64_t n, uint8_t* out, uint32_t* out_len,
                          DevCounters* ctr, hipStream_t stream);
// SampledSuffixArray::calcSA of n rows of one strand (fm_locate.hip): out[i] = SA[rows[i]] from the strand's locate tables; *broken
// is set to 1 when a walk does not end (an index that is no BWT of a string set); the LF steps go to ctr->rank_queries
struct LocateTables;
struct SaElem;
hipError_t launch_locate(const FmStrand& s, bool wide, const LocateTables& t, const uint64_t* rows, uint64_t n, SaElem* out, uint32_t* broken,
                         DevCounters* ctr, hipStream_t stream);
// The duplicate check of n reads (fm_dup.hip): words = their codes, one per byte, in a buffer that can be read as 32-bit words up
// to the one that holds the last base; read_off = n + 1 offsets.  launch_dup_chains runs the four chains of every read into
// chains[kind * n + read]; launch_dup_classify joins them into results[] and slots[], lets the first read of the call claim each
// slot in winner[] (n_slots entries, all kDupNoWinner before and after), classifies against bits[] and then sets the claimed bits.
// *broken is set to 1 when an interval leaves the strand (an index that is no BWT of a string set).
struct DupChainOut;
struct DupResult;
hipError_t launch_dup_chains(const FmIndexDev& fm, const uint32_t* words, const uint64_t* read_off, uint32_t n, DupChainOut* chains, DevCounters* ctr,
                             hipStream_t stream);
hipError_t launch_dup_classify(const FmIndexDev& fm, const DupChainOut* chains, uint32_t n, uint64_t n_slots, DupResult* results, uint64_t* slots, uint32_t* winner,
                               uint32_t* bits, uint32_t* broken, hipStream_t stream);
// The k-mer correction of n reads (fm_kcorrect.hip), one wavefront each: codes and read_off as above, phred one score per base
// or nullptr (15 everywhere); corrected = the reads' codes after it, at the same offsets.  ws_off[read] is the read's place in
// the workspace ws (kc_workspace_bytes of its length) when it has more than kKcLdsBases bases, anything otherwise.  *broken is
// set to 1 when an interval leaves the strand.
struct KcParams;
struct KcResult;
hipError_t launch_kmer_correct(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, const uint8_t* phred, uint32_t n, const KcParams& p,
                               uint8_t* ws, const uint64_t* ws_off, uint8_t* corrected, KcResult* results, uint32_t* broken, DevCounters* ctr,
                               hipStream_t stream);
// The merge of n_pairs paired-end reads (fm_fmwalk.hip), reads 2i and 2i + 1 of codes / read_off being pair i.
// launch_fmwalk_trim, a wavefront per pair: trimmed[2i], [2i + 1] = the trimmed lengths, and where both reach min_overlap
// strs + i * 4 * m4 (m4 = min_overlap rounded up to a multiple of 4) = the four strings of the pair's walks.
// launch_fmwalk_walks, a wavefront per walk, walk 2i + w being pair i's walk w: `groups` workgroups of kFwThreads, every wavefront
// with its own ws_slice >= fw_workspace_bytes(p) bytes of ws, take the walks in turn; outs[walk] = its code, length, leaves and
// coverage (zeros for a pair the gate stopped), best + walk * stride = its string's codes.
// *broken is set to 1 when an interval leaves the strand.
struct FwParams;
struct FwWalkOut;
hipError_t launch_fmwalk_trim(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, uint8_t* strs,
                              uint32_t* trimmed, uint32_t* broken, DevCounters* ctr, hipStream_t stream);
hipError_t launch_fmwalk_walks(const FmIndexDev& fm, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, const uint8_t* strs, const uint32_t* trimmed,
                               uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint8_t* best, uint64_t stride, FwWalkOut* outs, uint32_t* broken, DevCounters* ctr,
                               hipStream_t stream);
// The hybrid and kmerize algorithms of fmwalk and the sampled k-mer counts (fm_kmerize.hip), codes / read_off as above.
// launch_kmerize_split, a wavefront per job: `groups` workgroups of kKmThreads, every wavefront with its own ws_slice >=
// km_workspace_bytes(longest job) bytes of ws, take the jobs in turn; outs[job] = the pieces' number and the main one,
// pieces + jobs[job].slot = the pieces, of which a job needs len - k + 1 slots at the most.
// launch_hybrid_gate, a wavefront per pair: gates[i] = the trims and what MergeAndKmerize decides before its walks, and for a
// pair that is to be walked strs + i * 4 * m4 = the four strings of its walks.  launch_hybrid_walks: launch_fmwalk_walks for the
// pairs whose gate says so, with MergeAndKmerize's maxOverlap.
// launch_kmer_sample, a lane per sample: counts[i] = the occurrences in .rbwt, on both strands, of the up to `len` bases before
// '$' row rows[i] < the index's strings; ws holds n * len bytes.
// *broken is set to 1 when an interval leaves the strand.
struct KmJob;
struct KmJobOut;
struct KmPiece;
struct KmGate;
hipError_t launch_kmerize_split(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, const KmJob* jobs, uint32_t n_jobs, uint32_t k, uint32_t threshold,
                                bool filters, uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint32_t longest, KmPiece* pieces, KmJobOut* outs, uint32_t* broken,
                                DevCounters* ctr, hipStream_t stream);
hipError_t launch_hybrid_gate(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, uint64_t repeat_kmer_freq,
                              uint8_t* strs, KmGate* gates, uint32_t* broken, DevCounters* ctr, hipStream_t stream);
hipError_t launch_hybrid_walks(const FmIndexDev& fm, const uint64_t* read_off, uint32_t n_pairs, const FwParams& p, const uint8_t* strs, const KmGate* gates,
                               uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint8_t* best, uint64_t stride, FwWalkOut* outs, uint32_t* broken, DevCounters* ctr,
                               hipStream_t stream);
hipError_t launch_kmer_sample(const FmIndexDev& fm, const uint64_t* rows, uint32_t n, uint32_t len, uint8_t* ws, uint32_t* counts, uint32_t* broken, DevCounters* ctr,
                              hipStream_t stream);
// The validate algorithm of fmwalk (fm_validate.hip), codes / read_off as above, single reads.
// launch_validate_walks, a wavefront per walk, walk 2i + w being read i's walk w (0: on the read, 1: on its reverse complement):
// `groups` workgroups of kVdThreads, every wavefront with its own ws_slice >= fw_workspace_bytes(p) bytes of ws, p.max_insert being
// vd_depth of the longest read and stride at least that + 1; outs[walk] and best + walk * stride as launch_fmwalk_walks leaves them,
// zeros for a read of min_overlap bases or fewer.
// launch_validate_split: launch_kmerize_split with splitRead(std::string&)'s rules and its 64-bit threshold.
// *broken is set to 1 when an interval leaves the strand.
hipError_t launch_validate_walks(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_reads, const FwParams& p, uint32_t groups, uint8_t* ws,
                                 uint64_t ws_slice, uint8_t* best, uint64_t stride, FwWalkOut* outs, uint32_t* broken, DevCounters* ctr, hipStream_t stream);
hipError_t launch_validate_split(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, const KmJob* jobs, uint32_t n_jobs, uint32_t k, uint64_t threshold,
                                 uint32_t groups, uint8_t* ws, uint64_t ws_slice, uint32_t longest, KmPiece* pieces, KmJobOut* outs, uint32_t* broken, DevCounters* ctr,
                                 hipStream_t stream);
// The exact irreducible overlaps of n_reads reads (fm_overlap.hip), codes / read_off as above, no read longer than p.max_len.
// launch_overlap_collect, a lane per chain and four chains per read: heads[4 r + c] and chain_blocks + (4 r + c) * ov_slots(p) =
// what chain c of read r found.  launch_overlap_reduce, a wavefront per read: `groups` workgroups of kOvThreads, every wavefront
// with its own ws_slice >= ov_workspace_bytes(p) bytes of ws, take the reads in turn; outs[r] = the read's result, its final
// blocks at pool + outs[r].first_block, a place taken from *pool_used (the caller zeroes it; pool_cap >= n_reads * kOvOutCap).
// *broken is set to 1 when an interval leaves the strand.
struct OvParams;
struct OvChainHead;
struct OvBlock;
struct OvOutRead;
struct OvOutBlock;
hipError_t launch_overlap_collect(const FmIndexDev& fm, const uint8_t* codes, const uint64_t* read_off, uint32_t n_reads, const OvParams& p, uint32_t groups,
                                  OvChainHead* heads, OvBlock* chain_blocks, uint32_t* broken, DevCounters* ctr, hipStream_t stream);
hipError_t launch_overlap_reduce(const FmIndexDev& fm, const uint64_t* read_off, uint32_t n_reads, const OvParams& p, const OvChainHead* heads, const OvBlock* chain_blocks,
                                 uint32_t groups, uint8_t* ws, uint64_t ws_slice, OvOutRead* outs, OvOutBlock* pool, uint64_t pool_cap, unsigned long long* pool_used,
                                 uint32_t* broken, DevCounters* ctr, hipStream_t stream);
// The merge of unambiguously overlapping reads (fm_fmmerge.hip) on the state s of fm_fmmerge.h, every array on the device.
// launch_fmmerge_links, a lane per read of the chunk [first, first + n_chunk) after its overlap launches: outs, pool, *pool_used
// and heads are that chunk's, order0 / order1 the strands' lexicographic orders; the reads' links and their words of the state;
// first_bad[kFmmBad...] = the lowest read that shows what the entry refuses (the caller sets them to kFmmNone).
// launch_fmmerge_init / _round / _cut, a lane per node: the nodes before the first round, a round of doubling from `in` to `out`,
// the cuts after the first ranking.  launch_fmmerge_place, a lane per read, after the second.  launch_fmmerge_scan, steps 0, 1,
// 2: the prefix sums over the keys, tile_seqs and tile_bases holding fmmerge_scan_tiles(n) words, totals two (sequences, bases).
// launch_fmmerge_finish: the records.  launch_fmmerge_assemble: the bases as characters, none at or behind n_bases.
struct FmmState;
struct FmmNode;
struct FmmOutRead;
struct FmmOutSeq;
hipError_t launch_fmmerge_links(const FmmState& s, uint32_t first, uint32_t n_chunk, uint32_t min_overlap, const OvOutRead* outs, const OvOutBlock* pool,
                                const unsigned long long* pool_used, const OvChainHead* heads, const uint32_t* order0, const uint32_t* order1, uint32_t* first_bad,
                                hipStream_t stream);
hipError_t launch_fmmerge_init(const FmmState& s, FmmNode* nodes, hipStream_t stream);
hipError_t launch_fmmerge_round(const FmmState& s, const FmmNode* in, FmmNode* out, hipStream_t stream);
hipError_t launch_fmmerge_cut(const FmmState& s, const FmmNode* nodes, hipStream_t stream);
hipError_t launch_fmmerge_place(const FmmState& s, const FmmNode* nodes, hipStream_t stream);
uint32_t fmmerge_scan_tiles(uint32_t n);
hipError_t launch_fmmerge_scan(const FmmState& s, int step, uint32_t* tile_seqs, unsigned long long* tile_bases, unsigned long long* totals, hipStream_t stream);
hipError_t launch_fmmerge_finish(const FmmState& s, FmmOutRead* per_read, FmmOutSeq* seqs, hipStream_t stream);
hipError_t launch_fmmerge_assemble(const FmmState& s, const uint8_t* codes, char* bases, uint64_t n_bases, hipStream_t stream);
hipError_t launch_bwt_chars(const FmIndexDev& fm, int strand, const uint64_t* idx, uint64_t n, char* out,
                            hipStream_t stream);
hipError_t launch_find_kmers(const FmIndexDev& fm, const uint8_t* kmer_codes, uint32_t k, uint64_t n,
                             lrsc_biinterval* out, DevCounters* ctr, hipStream_t stream);
hipError_t launch_kmer_grid(const FmIndexDev& fm, const GridArgs& a, DevCounters* ctr, hipStream_t stream);
// ASCII -> 2-bit code per byte; *bad set to 1 if a byte is not one of ACGT
hipError_t launch_encode(const char* ascii, uint8_t* codes, uint64_t n, int* bad, hipStream_t stream);
hipError_t launch_chunk_table(const uint64_t* read_off, uint32_t n_reads, uint64_t total_bases,
                              uint32_t* chunk_read, hipStream_t stream);

} // namespace lrsc
