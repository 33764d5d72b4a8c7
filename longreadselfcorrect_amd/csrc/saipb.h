// saipb.h -- what the host side (capi_saipb.cpp) and the kernels (saipb.hip, saipb_device.h) share about the hash-guided seed-pair merge:
// the job / seed records, the per-job workspace layout and the planner that sizes it from the seeds' intervals.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "../../include/lrsc.h"
#include "fm_device.h"

namespace lrsc {

constexpr uint32_t kSaipbMaxLeaves = 64;                    // frontier at the start of a step
constexpr uint32_t kSaipbFrontier = 4 * kSaipbMaxLeaves;    // children of one step
constexpr uint32_t kSaipbMaxResults = 32;                   // result list of one job (the sets of the tests reach 10)
constexpr uint32_t kSaipbMaxRows = 30;                      // rows LF-walked per strand per seed
constexpr uint32_t kSaipbBucket = 35;                       // positions per frequency bucket
constexpr uint32_t kSaipbMaxSeq = 32000;                    // longest single string of a job
// The alignment cells keep t = matches << 16 | columns.  An alignment of rawSeq against a candidate has at most raw_len + candidate
// length columns, and a candidate is at most max_length + 1 path bases plus dest beyond its first hash_kmer: a job is refused unless
// that sum fits the low half-word (matches are at most the shorter string, so they fit the high one).
constexpr uint32_t kSaipbMaxColumns = 65535;


struct SaipbSeed {               // one addHashBySingleSeed call; the seed's bases are codes[off .. off + len)
    uint64_t off;
    uint32_t len, large_kmer, max_length;
    int32_t expected_length;     // -1: source side
    uint32_t skip_repeat, pad;
};
struct SaipbSeedInfo {           // findBiInterval of the seed's last large_kmer bases, and what the call returns
    uint64_t flo, fhi, rlo, rhi;
    uint64_t freq;
};
struct SaipbJob {
    uint64_t raw_off, src_off, dest_off;
    uint32_t raw_len, src_len, dest_len;
    uint32_t seed_first, n_seeds;
    uint32_t hash_kmer, max_leaves, min_length, max_length, expected_length, min_sa;
    // the job's slice of the chunk's workspace and output (filled by the planner)
    uint32_t hash_slots, pool_words, node_cap, str_cap;
    uint64_t ws_off, out_off;
};
struct SaipbOut {
    int32_t code;
    uint32_t status, steps, max_used_leaves, n_results, hash_entries, out_len, pad;
};

struct SaipbLeaf { uint64_t stem, flo, fhi, rlo, rhi, count; uint32_t node, pad; };
struct SaipbCand { uint64_t flo, fhi, rlo, rhi; uint32_t ok, pad; };
struct SaipbRes { uint64_t count; uint32_t node, len; };
struct SaipbCell { int32_t m, i, d; uint32_t tm, ti, td; };          // scores of the three layers; t = matches << 16 | columns
struct SaipbMeta { uint32_t off, nb; };

// ---- workspace layout of one job (bytes, every part 16-byte aligned) ----------------------------------------------------------
struct SaipbLayout { uint64_t keys, meta, maxavg, pool, nodes, leaves, cands, res, ctl, str, rows, total; };
LRSC_HD uint64_t saipb_align16(uint64_t x) { return (x + 15) & ~15ull; }
LRSC_HD SaipbLayout saipb_layout(const SaipbJob& j)
{
    SaipbLayout l;
    uint64_t o = 0;
    l.keys = o;   o += saipb_align16((uint64_t)j.hash_slots * 8);
    l.meta = o;   o += saipb_align16((uint64_t)j.hash_slots * sizeof(SaipbMeta));
    l.maxavg = o; o += saipb_align16((uint64_t)j.hash_slots * 8);
    l.pool = o;   o += saipb_align16((uint64_t)j.pool_words * 4);
    l.nodes = o;  o += saipb_align16((uint64_t)j.node_cap * 4);
    l.leaves = o; o += saipb_align16((uint64_t)2 * kSaipbFrontier * sizeof(SaipbLeaf));
    l.cands = o;  o += saipb_align16((uint64_t)kSaipbMaxLeaves * 4 * sizeof(SaipbCand));
    l.res = o;    o += saipb_align16((uint64_t)kSaipbMaxResults * sizeof(SaipbRes));
    l.ctl = o;    o += 64;
    l.str = o;    o += saipb_align16((uint64_t)kSaipbMaxResults * j.str_cap);
    l.rows = o;   o += saipb_align16((uint64_t)kSaipbMaxResults * 2 * (j.raw_len + 1) * sizeof(SaipbCell));
    l.total = o;
    return l;
}
// Sizes of a job from its seeds' intervals: the record bound is sum of rows x (maxLength - seedLen + 1), every record may create one
// entry of the creating seed's bucket count; the table has at least twice as many slots as records can exist, so a probe ends.
// The path store holds one node per child ever created: at most max_leaves per continued step, 4 x max_leaves in the last one.
// False for a job whose counts do not fit the 32-bit fields (its table would not be a power of two any more): the caller gives it
// LRSC_SAIPB_HASH_LIMIT whatever the per-job budget says.
LRSC_HD bool saipb_plan_job(SaipbJob& j, const SaipbSeed* seeds, const SaipbSeedInfo* info)
{
    uint64_t records = 0, words = 0;
    for(uint32_t s = 0; s < j.n_seeds; ++s) {
        const SaipbSeed& sd = seeds[j.seed_first + s];
        const SaipbSeedInfo& si = info[j.seed_first + s];
        if(sd.skip_repeat && si.freq > 128) continue;
        uint64_t rows = 0;
        if(si.flo <= si.fhi) rows += (si.fhi - si.flo + 1 < kSaipbMaxRows) ? si.fhi - si.flo + 1 : kSaipbMaxRows;
        if(si.rlo <= si.rhi) rows += (si.rhi - si.rlo + 1 < kSaipbMaxRows) ? si.rhi - si.rlo + 1 : kSaipbMaxRows;
        const uint64_t per = sd.max_length > sd.len ? (uint64_t)(sd.max_length - sd.len) + 1 : 1;
        records += rows * per;
        words += rows * per * (sd.max_length / kSaipbBucket + 1);
    }
    uint64_t slots = 64;
    while(slots < 2 * records) slots <<= 1;
    const uint64_t steps = j.max_length >= j.src_len ? (uint64_t)(j.max_length - j.src_len) + 2 : 1;
    const uint64_t nodes = steps * j.max_leaves + 4ull * j.max_leaves + 2;
    const uint64_t cap = 0xFFFFFFFFull;
    if(slots > (1ull << 31) || words > cap || nodes > cap) { j.hash_slots = j.pool_words = j.node_cap = j.str_cap = 0; return false; }
    j.hash_slots = (uint32_t)slots;                                // a power of two: the probe masks with hash_slots - 1
    j.pool_words = (uint32_t)words;
    j.node_cap = (uint32_t)nodes;
    j.str_cap = (uint32_t)saipb_align16((uint64_t)j.max_length + j.src_len + j.dest_len + 4);
    return true;
}

// The ABI's records as the kernels read them; the checks are where the reference would throw (substr beyond the string) or divide by
// zero (an empty rawSeq), and the caps of this implementation.  Returns an lrsc_status; *why names the reason.
inline int saipb_from_abi(const lrsc_saipb_seed* seeds, uint32_t n_seeds, const lrsc_saipb_job& a, uint64_t seq_len, SaipbSeed* dseeds, SaipbJob& j,
                          const char** why)
{
    *why = "";
    if(a.hash_kmer < 2 || a.hash_kmer > 31) { *why = "hash_kmer must be 2..31"; return LRSC_ERR_UNSUPPORTED; }
    if(a.max_leaves < 1 || a.max_leaves > kSaipbMaxLeaves) { *why = "max_leaves must be 1..64"; return LRSC_ERR_UNSUPPORTED; }
    if(a.raw_len == 0) { *why = "empty rawSeq"; return LRSC_ERR_ARG; }
    if(a.src_len < a.hash_kmer || a.dest_len < a.hash_kmer) { *why = "src / dest shorter than hash_kmer"; return LRSC_ERR_ARG; }
    if(a.raw_off + a.raw_len > seq_len || a.src_off + a.src_len > seq_len || a.dest_off + a.dest_len > seq_len) { *why = "job string outside seq"; return LRSC_ERR_ARG; }
    if((uint64_t)a.seed_first + a.n_seeds > n_seeds) { *why = "job seeds outside the seed list"; return LRSC_ERR_ARG; }
    if(a.raw_len > kSaipbMaxSeq || a.max_length > kSaipbMaxSeq || a.src_len > kSaipbMaxSeq || a.dest_len > kSaipbMaxSeq) {
        *why = "strings beyond 32000 bases"; return LRSC_ERR_UNSUPPORTED;
    }
    if((uint64_t)a.raw_len + a.max_length + a.dest_len + 1 > kSaipbMaxColumns) {
        *why = "raw_len + max_length + dest_len beyond 65534 (alignment columns)"; return LRSC_ERR_UNSUPPORTED;
    }
    for(uint32_t s = 0; s < a.n_seeds; ++s) {
        const lrsc_saipb_seed& sd = seeds[a.seed_first + s];
        if(sd.large_kmer == 0 || sd.len < sd.large_kmer || sd.len < a.hash_kmer) { *why = "seed shorter than large_kmer / hash_kmer"; return LRSC_ERR_ARG; }
        if(sd.seq_off + sd.len > seq_len) { *why = "seed outside seq"; return LRSC_ERR_ARG; }
        if(sd.max_length > kSaipbMaxSeq || sd.len > kSaipbMaxSeq) { *why = "strings beyond 32000 bases"; return LRSC_ERR_UNSUPPORTED; }
        SaipbSeed& d = dseeds[a.seed_first + s];
        d.off = sd.seq_off; d.len = sd.len; d.large_kmer = sd.large_kmer; d.max_length = sd.max_length;
        d.expected_length = sd.expected_length; d.skip_repeat = sd.skip_repeat; d.pad = 0;
    }
    j = SaipbJob{};
    j.raw_off = a.raw_off; j.src_off = a.src_off; j.dest_off = a.dest_off;
    j.raw_len = a.raw_len; j.src_len = a.src_len; j.dest_len = a.dest_len;
    j.seed_first = a.seed_first; j.n_seeds = a.n_seeds;
    j.hash_kmer = a.hash_kmer; j.max_leaves = a.max_leaves; j.min_length = a.min_length; j.max_length = a.max_length;
    j.expected_length = a.expected_length; j.min_sa = a.min_sa_threshold;
    return LRSC_OK;
}

hipError_t launch_saipb_seed_info(const FmIndexDev& fm, const uint8_t* codes, const SaipbSeed* seeds, uint32_t n, SaipbSeedInfo* info,
                                  hipStream_t stream);
// one wavefront per job of the chunk: jobs[first .. first + n)
hipError_t launch_saipb_merge(const FmIndexDev& fm, const uint8_t* codes, const SaipbSeed* seeds, const SaipbSeedInfo* info,
                              const SaipbJob* jobs, uint32_t n, uint8_t* ws, char* out, SaipbOut* results, hipStream_t stream);

} // namespace lrsc
