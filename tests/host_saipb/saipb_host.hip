// saipb_host.hip -- TEST INFRASTRUCTURE ONLY (never linked into or loaded by the product).
//
// Runs the product's hash-guided seed-pair merge -- longreadselfcorrect_amd/csrc/saipb_device.h, the very source saipb_merge_kernel
// compiles for gfx950 -- on the CPU with one lane, over the same rank-block image and k-mer tables the device uses, so that
// `pytest -m "not gpu"` can hold it against the CPU oracle without a device.  The header is compiled with LRSC_SAIPB_FN =
// __host__ __device__ (tests/host_saipb/Makefile); in the product it is __device__ only and nothing there can reach this code.
// No HIP runtime call is made.  Jobs and seeds come in as the public ABI's records (include/lrsc.h) and pass through the same
// conversion, checks and planner as in lrsc_saipb_merge.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../longreadselfcorrect_amd/csrc/fm_layout.h"
#include "../../longreadselfcorrect_amd/csrc/saipb_device.h"

using namespace lrsc;

struct HostIndex {
    StrandImage image[2];
    bool wide = false;
    FmIndexDev dev{};
    std::vector<std::vector<uint8_t>> tables;
    std::vector<uint32_t> mtab;
};

template <bool WIDE>
static void build_tables(HostIndex* ix, const int* ks, int n)
{
    using P = typename Lay<WIDE>::pos_t;
    ix->mtab.resize(MaskTabSize<WIDE>::value);
    fill_mask_table_serial<WIDE>(ix->mtab.data());
    const StrandC<P> sF = strand_consts<P>(ix->dev.strand[LRSC_RBWT]);
    const StrandC<P> sR = strand_consts<P>(ix->dev.strand[LRSC_BWT]);
    for(int i = 0; i < n && ix->tables.size() < 5; ++i) {
        const uint32_t k = (uint32_t)ks[i];
        if(k == 0 || k > 12) continue;
        const uint64_t n_codes = 1ull << (2 * k);
        const size_t eb = WIDE ? 32 : 16;
        std::vector<uint8_t> buf(n_codes * eb);
        for(uint64_t code = 0; code < n_codes; ++code) {
            WalkState<P> st = walk_init<P>();
            for(uint32_t t = 0; t < k; ++t) {
                const uint32_t c = (uint32_t)(code >> (2 * (k - 1 - t))) & 3u;
                st = walk_step<WIDE>(sF, sR, c, 1u << 30, st, ix->mtab.data());
            }
            if(WIDE) {
                uint64_t e[4] = {(uint64_t)st.fwd.lo, (uint64_t)st.fwd.hi, (uint64_t)st.rvc.lo, (uint64_t)st.rvc.hi};
                std::memcpy(buf.data() + code * 32, e, 32);
            } else {
                uint32_t e[4] = {(uint32_t)st.fwd.lo, (uint32_t)st.fwd.hi, (uint32_t)st.rvc.lo, (uint32_t)st.rvc.hi};
                std::memcpy(buf.data() + code * 16, e, 16);
            }
        }
        ix->tables.push_back(std::move(buf));
    }
    // tables become visible only now: walk_step above must not consult a half-built one
    int slot = 0;
    for(int i = 0; i < n && slot < (int)ix->tables.size(); ++i) {
        const uint32_t k = (uint32_t)ks[i];
        if(k == 0 || k > 12) continue;
        ix->dev.ktab[slot].entries = ix->tables[slot].data();
        ix->dev.ktab[slot].k = k;
        ++slot;
    }
}

extern "C" void* hs_index_create(const uint8_t* bwt_units, uint64_t n0, const uint8_t* rbwt_units, uint64_t n1, uint64_t num_symbols,
                                 int wide, const int* table_ks, int n_tables)
{
    HostIndex* ix = new HostIndex();
    ix->wide = wide != 0;
    std::string err;
    if(build_strand_image(bwt_units, n0, num_symbols, ix->wide, ix->image[0], err) != 0 ||
       build_strand_image(rbwt_units, n1, num_symbols, ix->wide, ix->image[1], err) != 0) { delete ix; return nullptr; }
    std::memset(&ix->dev, 0, sizeof(ix->dev));
    ix->dev.wide = ix->wide ? 1u : 0u;
    for(int s = 0; s < 2; ++s) {
        FmStrand& fs = ix->dev.strand[s];
        fs.blocks = ix->image[s].blocks.data();
        fs.dollars = ix->image[s].dollars.data();
        fs.dollar_dir = ix->image[s].dollar_dir.data();
        fs.dollar_group_syms = (uint64_t)(ix->wide ? Block64::kSyms : Block32::kSyms) << kDollarDirShift;
        fs.n_dollars = ix->image[s].dollars.size();
        fs.n_symbols = ix->image[s].n_symbols;
        fs.n_blocks = ix->image[s].n_blocks;
        for(int c = 0; c < 5; ++c) fs.pred[c] = ix->image[s].pred[c];
    }
    if(ix->wide) build_tables<true>(ix, table_ks, n_tables); else build_tables<false>(ix, table_ks, n_tables);
    return ix;
}
extern "C" void hs_index_free(void* h) { delete static_cast<HostIndex*>(h); }

template <bool WIDE>
static int run_jobs(HostIndex* ix, const uint8_t* codes, uint64_t seq_len, const lrsc_saipb_seed* seeds, uint32_t n_seeds, const lrsc_saipb_job* jobs,
                    uint32_t n_jobs, lrsc_saipb_result* results, uint64_t* seed_freq, char* out, uint64_t out_cap, uint64_t* out_used)
{
    using P = typename Lay<WIDE>::pos_t;
    SaipbCtx<WIDE> c;
    c.sF = strand_consts<P>(ix->dev.strand[LRSC_RBWT]);
    c.sR = strand_consts<P>(ix->dev.strand[LRSC_BWT]);
    c.fm = &ix->dev;
    c.mtab = ix->mtab.data();
    c.codes = codes;
    std::vector<SaipbSeed> dseeds(n_seeds);
    std::vector<SaipbSeedInfo> info(n_seeds);
    std::vector<SaipbJob> djobs(n_jobs);
    for(uint32_t j = 0; j < n_jobs; ++j) {
        const char* why;
        const int st = saipb_from_abi(seeds, n_seeds, jobs[j], seq_len, dseeds.data(), djobs[j], &why);
        if(st != LRSC_OK) return st;
    }
    uint64_t used = 0;
    std::vector<uint8_t> ws;
    for(uint32_t j = 0; j < n_jobs; ++j) {
        SaipbJob& job = djobs[j];
        for(uint32_t s = 0; s < job.n_seeds; ++s) {
            info[job.seed_first + s] = saipb_seed_info<WIDE>(c, dseeds[job.seed_first + s]);
            if(seed_freq) seed_freq[job.seed_first + s] = info[job.seed_first + s].freq;
        }
        if(!saipb_plan_job(job, dseeds.data(), info.data())) {
            results[j] = lrsc_saipb_result{};
            results[j].status = LRSC_SAIPB_HASH_LIMIT;
            continue;
        }
        job.ws_off = 0;
        job.out_off = 0;
        const SaipbLayout lay = saipb_layout(job);
        ws.assign(lay.total + 64, 0xA5);                              // nothing may rely on a zeroed workspace
        std::vector<char> o(job.str_cap);
        SaipbOut r;
        saipb_run_job<WIDE>(c, job, dseeds.data(), info.data(), ws.data(), o.data(), r, 0u, 1u);
        for(size_t t = lay.total; t < ws.size(); ++t) if(ws[t] != 0xA5) return -1000;     // wrote beyond its slice
        lrsc_saipb_result& res = results[j];
        res.code = r.code; res.status = (int32_t)r.status; res.steps = r.steps; res.max_used_leaves = r.max_used_leaves;
        res.n_results = r.n_results; res.hash_entries = r.hash_entries; res.out_off = used; res.out_len = r.out_len; res.pad = 0;
        if(used + r.out_len > out_cap) return LRSC_ERR_CAPACITY;
        std::memcpy(out + used, o.data(), r.out_len);
        used += r.out_len;
    }
    *out_used = used;
    return LRSC_OK;
}

// seq: 0..3 codes
extern "C" int hs_saipb_merge(void* h, const uint8_t* codes, uint64_t seq_len, const lrsc_saipb_seed* seeds, uint32_t n_seeds,
                              const lrsc_saipb_job* jobs, uint32_t n_jobs, lrsc_saipb_result* results, uint64_t* seed_freq, char* out,
                              uint64_t out_cap, uint64_t* out_used)
{
    HostIndex* ix = static_cast<HostIndex*>(h);
    return ix->wide ? run_jobs<true>(ix, codes, seq_len, seeds, n_seeds, jobs, n_jobs, results, seed_freq, out, out_cap, out_used)
                    : run_jobs<false>(ix, codes, seq_len, seeds, n_seeds, jobs, n_jobs, results, seed_freq, out, out_cap, out_used);
}

// the device alignment helper alone: a, b as 0..3 codes -> {matches, score, columns}
extern "C" void hs_saipb_align(const uint8_t* a, int n1, const uint8_t* b, int n2, int* out3)
{
    std::vector<SaipbCell> r0((size_t)n1 + 1), r1((size_t)n1 + 1);
    saipb_global_align(a, n1, b, n2, r0.data(), r1.data(), out3[0], out3[1], out3[2]);
}
