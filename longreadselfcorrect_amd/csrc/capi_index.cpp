// capi_index.cpp -- the index object (open / from units, on the host or on the device / build from reads / upload with its
// k-mer tables / close), the
// device BWT build, the merge of two resident indexes, the locate tables of a resident copy, its RL units and the file writer.
#include <chrono>
#include <thread>

#include "capi_internal.h"
#include "fm_locate.h"
#include "fm_merge.h"
#include "fm_pack.h"
#include "fm_rle.h"
#include "fm_unrle.h"

using namespace lrsc;

bool lrsc::index_is_wide(uint64_t num_symbols) { return num_symbols >= (1ull << 31) || std::getenv("LRSC_FORCE_WIDE") != nullptr; }

static int index_from_units_impl(const uint8_t* u0, uint64_t n0, const uint8_t* u1, uint64_t n1,
                                 uint64_t num_strings, uint64_t num_symbols, lrsc_index** out)
{
    lrsc_index* idx = new(std::nothrow) lrsc_index();
    if(!idx) return fail(LRSC_ERR_NOMEM, "lrsc_index");
    idx->num_strings = num_strings;
    idx->num_symbols = num_symbols;
    idx->wide = index_is_wide(num_symbols);
    int st[2] = {LRSC_OK, LRSC_OK};
    std::string err[2];
    const uint8_t* us[2] = {u0, u1};
    const uint64_t ns[2] = {n0, n1};
    // the two strands are independent: build them on two host threads
    std::thread t([&]() { st[1] = build_strand_image(us[1], ns[1], num_symbols, idx->wide, idx->image[1], err[1]); });
    st[0] = build_strand_image(us[0], ns[0], num_symbols, idx->wide, idx->image[0], err[0]);
    t.join();
    for(int s = 0; s < 2; ++s)
        if(st[s] != LRSC_OK) { const int r = fail(st[s], err[s]); delete idx; return r; }
    if(idx->image[0].dollars.size() != num_strings || idx->image[1].dollars.size() != num_strings) {
        delete idx;
        return fail(LRSC_ERR_FORMAT, "number of '$' rows differs from the number of strings in the header");
    }
    *out = idx;
    return LRSC_OK;
}

extern "C" int lrsc_index_from_units(const uint8_t* bwt_units, uint64_t n_bwt_units, const uint8_t* rbwt_units,
                                     uint64_t n_rbwt_units, uint64_t num_strings, uint64_t num_symbols,
                                     lrsc_index** out)
{
    if(!bwt_units || !rbwt_units || !out || num_symbols == 0) return fail(LRSC_ERR_ARG, "null/empty index input");
    return index_from_units_impl(bwt_units, n_bwt_units, rbwt_units, n_rbwt_units, num_strings, num_symbols, out);
}

extern "C" int lrsc_index_open(const char* bwt_path, const char* rbwt_path, lrsc_index** out)
{
    if(!bwt_path || !rbwt_path || !out) return fail(LRSC_ERR_ARG, "null path");
    std::vector<uint8_t> u[2];
    uint64_t nstr[2] = {0, 0}, nsym[2] = {0, 0};
    std::string err;
    int st = read_bwt_file(bwt_path, u[0], nstr[0], nsym[0], err);
    if(st != LRSC_OK) return fail(st, err);
    st = read_bwt_file(rbwt_path, u[1], nstr[1], nsym[1], err);
    if(st != LRSC_OK) return fail(st, err);
    if(nstr[0] != nstr[1] || nsym[0] != nsym[1]) return fail(LRSC_ERR_FORMAT, ".bwt and .rbwt disagree on strings/symbols");
    return index_from_units_impl(u[0].data(), u[0].size(), u[1].data(), u[1].size(), nstr[0], nsym[0], out);
}

extern "C" int lrsc_index_info_get(const lrsc_index* idx, lrsc_index_info* out)
{
    if(!idx || !out) return fail(LRSC_ERR_ARG, "null");
    std::memset(out, 0, sizeof(*out));
    out->num_strings = idx->num_strings;
    out->num_symbols = idx->num_symbols;
    for(int s = 0; s < 2; ++s) {
        out->num_runs[s] = idx->image[s].n_runs;
        for(int c = 0; c < 5; ++c) out->pred_count[s][c] = idx->image[s].pred[c];
        out->device_bytes += idx->image[s].blocks.size() + idx->image[s].dollars.size() * 8 + idx->image[s].dollar_dir.size() * 4;
    }
    out->block_bytes = 64;
    out->block_symbols = idx->wide ? Block64::kSyms : Block32::kSyms;
    return LRSC_OK;
}

void lrsc::free_device_copy(DeviceCopy& dc)
{
    for(int s = 0; s < 2; ++s) {
        if(dc.blocks[s]) (void)hipFree(dc.blocks[s]);
        if(dc.dollars[s]) (void)hipFree(dc.dollars[s]);
        if(dc.dollar_dir[s]) (void)hipFree(dc.dollar_dir[s]);
        dc.blocks[s] = nullptr; dc.dollars[s] = nullptr; dc.dollar_dir[s] = nullptr;
    }
    for(int t = 0; t < 5; ++t) { if(dc.ktab[t]) (void)hipFree(dc.ktab[t]); dc.ktab[t] = nullptr; }
    for(int s = 0; s < 2; ++s) locate_free_device(dc.locate[s]);
    dc.located = false;
}

// first half of an upload: the host image of both strands -> the current device
static int copy_image(const lrsc_index* idx, DeviceCopy& dc)
{
    for(int s = 0; s < 2; ++s) {
        const StrandImage& im = idx->image[s];
        HIP_TRY(hipMalloc(&dc.blocks[s], im.blocks.size()));
        HIP_TRY(hipMemcpy(dc.blocks[s], im.blocks.data(), im.blocks.size(), hipMemcpyHostToDevice));
        const size_t db = std::max<size_t>(im.dollars.size(), 1) * sizeof(uint64_t);
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dc.dollars[s]), db));
        if(!im.dollars.empty())
            HIP_TRY(hipMemcpy(dc.dollars[s], im.dollars.data(), im.dollars.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dc.dollar_dir[s]), im.dollar_dir.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(dc.dollar_dir[s], im.dollar_dir.data(), im.dollar_dir.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return LRSC_OK;
}

// second half: describe the image that dc holds on the current device (copied there, or packed there by lrsc_index_build),
// build its k-mer tables and enter it as `device`'s copy.  The caller holds idx->mu and frees dc on failure.
int lrsc::register_copy(lrsc_index* idx, int device, DeviceCopy& dc)
{
    dc.dev.wide = idx->wide ? 1u : 0u;
    for(int s = 0; s < 2; ++s) {
        const StrandImage& im = idx->image[s];
        FmStrand& fs = dc.dev.strand[s];
        fs.blocks = dc.blocks[s];
        fs.dollars = dc.dollars[s];
        fs.dollar_dir = dc.dollar_dir[s];
        fs.dollar_group_syms = (uint64_t)(idx->wide ? Block64::kSyms : Block32::kSyms) << kDollarDirShift;
        fs.n_dollars = im.dollars.size();
        fs.n_symbols = im.n_symbols;
        fs.n_blocks = im.n_blocks;
        for(int c = 0; c < 5; ++c) fs.pred[c] = im.pred[c];
    }
    // k-mer interval tables (narrow indexes): sizes 5 and 9 (the walk's 5-mer / idmer look-ups), T = floor(log4 N) clamped
    // to [9, 13] -- up to there practically every k-mer occurs in the index -- and T + 2, where most chance matches have
    // died (16 bytes x 4^k: 1.07 GB at 13, 17.2 GB at 15, taken only if it fits a quarter of the free HBM).
    // LRSC_KTAB_K overrides T (0 disables all tables), LRSC_KTAB_K2 the fourth size (0 disables it).
    {
        const size_t entry_bytes = idx->wide ? 32 : 16;          // 4 x u64 for Block64 indexes
        int T = 0;
        for(uint64_t n = idx->num_symbols; n >= 4; n >>= 2) ++T;
        T = std::max(9, std::min(13, T));
        if(const char* e = std::getenv("LRSC_KTAB_K")) T = std::atoi(e);
        int T2 = T > 0 ? std::min(15, T + 2) : 0;
        if(const char* e = std::getenv("LRSC_KTAB_K2")) T2 = std::atoi(e);
        // LRSC_KTAB_K3 (experimental, default off): a fifth table of T + 3 (16-mers: 69 GB)
        int T3 = 0;
        if(const char* e = std::getenv("LRSC_KTAB_K3")) T3 = std::atoi(e);
        uint32_t want[5] = {5, 9, (uint32_t)T, (uint32_t)T2, (uint32_t)T3};
        uint32_t ks[5] = {0, 0, 0, 0, 0};
        uint32_t n_t = 0;
        for(int i = 0; i < 5 && T > 0; ++i) {
            if(want[i] == 0 || want[i] > 16 || (n_t > 0 && want[i] <= ks[n_t - 1])) continue;
            const size_t bytes = entry_bytes << (2 * want[i]);
            if(i >= 3) {
                size_t free_b = 0, total_b = 0;
                HIP_TRY(hipMemGetInfo(&free_b, &total_b));
                if(bytes > free_b / (i == 3 ? 4 : 3)) continue;
            }
            HIP_TRY(hipMalloc(&dc.ktab[n_t], bytes));
            // each table starts from the previous (smaller) one; dc.dev.ktab[].k stays 0 until all are built so that the
            // builder's own walk_step never consults a table
            hipError_t e2 = launch_ktab_build(dc.dev, want[i], dc.ktab[n_t], n_t ? ks[n_t - 1] : 0, n_t ? dc.ktab[n_t - 1] : nullptr, nullptr);
            if(e2 != hipSuccess) return hip_fail(e2, "ktab build");
            dc.dev.ktab[n_t].entries = dc.ktab[n_t];
            dc.dev.ktab[n_t].k = 0;
            ks[n_t] = want[i];
            ++n_t;
        }
        HIP_TRY(hipDeviceSynchronize());
        for(uint32_t i = 0; i < n_t; ++i) dc.dev.ktab[i].k = ks[i];
    }
    idx->copies[device] = dc;
    return LRSC_OK;
}

extern "C" int lrsc_index_upload(lrsc_index* idx, int device)
{
    if(!idx) return fail(LRSC_ERR_ARG, "null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    if(idx->copies.count(device)) return LRSC_OK;
    HIP_TRY(hipSetDevice(device));
    DeviceCopy dc;
    int st = copy_image(idx, dc);
    if(st == LRSC_OK) st = register_copy(idx, device, dc);
    if(st != LRSC_OK) free_device_copy(dc);
    return st;
}

extern "C" void lrsc_index_close(lrsc_index* idx)
{
    if(!idx) return;
    for(auto& kv : idx->copies) {
        if(hipSetDevice(kv.first) != hipSuccess) continue;
        free_device_copy(kv.second);
    }
    delete idx;
}

// ---------------------------------------------------------------------------------------
// index construction
// ---------------------------------------------------------------------------------------
namespace lrsc {
int build_bwt_device(const char* reads, const uint64_t* off, uint32_t n_reads, int reverse_reads, int device,
                     std::vector<uint8_t>& bwt_out, uint32_t* rounds_out, std::string& err);
int build_bwt_resident(const char* reads, const uint64_t* off, uint32_t n_reads, int reverse_reads, int device,
                       uint8_t** d_bwt_out, uint32_t* rounds_out, std::string& err);
}

// device units -> a malloc'ed host copy; d_units is released either way
static int units_to_host(uint8_t* d_units, uint64_t n_units, uint8_t** units_out, uint64_t* n_units_out)
{
    uint8_t* units = static_cast<uint8_t*>(std::malloc(n_units ? n_units : 1));
    hipError_t e = hipSuccess;
    if(units && n_units) e = hipMemcpy(units, d_units, n_units, hipMemcpyDeviceToHost);
    if(d_units) (void)hipFree(d_units);
    if(!units) return fail(LRSC_ERR_NOMEM, "RL units");
    if(e != hipSuccess) { std::free(units); return hip_fail(e, "copy of the RL units to the host"); }
    *units_out = units;
    *n_units_out = n_units;
    return LRSC_OK;
}

extern "C" int lrsc_build_bwt(const char* reads, const uint64_t* read_off, uint32_t n_reads, int reverse_reads,
                              int device, uint8_t** units_out, uint64_t* n_units_out)
{
    if(!reads || !units_out || !n_units_out || n_reads == 0) return fail(LRSC_ERR_ARG, "null / empty read set");
    int st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    std::string err;
    const char* host_rle = std::getenv("LRSC_BWT_HOST_RLE");
    if(!host_rle || std::atoi(host_rle) == 0) {
        // RL-encode where the BWT lies (fm_rle.hip); only the units cross to the host
        uint8_t* d_bwt = nullptr;
        st = build_bwt_resident(reads, read_off, n_reads, reverse_reads, device, &d_bwt, nullptr, err);
        if(st != LRSC_OK) return fail(st, err);
        const auto t0 = std::chrono::steady_clock::now();
        uint8_t* d_units = nullptr;
        uint64_t n_units = 0;
        st = rle_bwt_device(d_bwt, read_off[n_reads] + n_reads, &d_units, &n_units, err);
        (void)hipFree(d_bwt);
        if(st != LRSC_OK) return fail(st, err);
        if(std::getenv("LRSC_BWT_PROFILE"))
            std::fprintf(stderr, "[lrsc] RL encode on the device: %.3f ms, %llu units\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), (unsigned long long)n_units);
        return units_to_host(d_units, n_units, units_out, n_units_out);
    }
    // LRSC_BWT_HOST_RLE=1: the BWT comes to the host at a byte per symbol and one thread encodes it (the encoder's A/B)
    std::vector<uint8_t> bwt;
    st = build_bwt_device(reads, read_off, n_reads, reverse_reads, device, bwt, nullptr, err);
    if(st != LRSC_OK) return fail(st, err);
    // RL-encode as BWTWriterBinary::writeBWChar does: same symbol and run < 31 extends the run
    uint64_t n_units = 0;
    {
        uint8_t prev = 0xFF; unsigned run = 0;
        for(uint8_t c : bwt) {
            if(c == prev && run < 31) ++run;
            else { ++n_units; prev = c; run = 1; }
        }
    }
    uint8_t* units = static_cast<uint8_t*>(std::malloc(n_units ? n_units : 1));
    if(!units) return fail(LRSC_ERR_NOMEM, "RL units");
    {
        uint64_t u = 0; uint8_t prev = 0xFF; unsigned run = 0;
        for(uint8_t c : bwt) {
            if(c == prev && run < 31) { ++run; units[u - 1] = (uint8_t)((c << 5) | run); }
            else { prev = c; run = 1; units[u++] = (uint8_t)((c << 5) | 1); }
        }
    }
    *units_out = units;
    *n_units_out = n_units;
    return LRSC_OK;
}

extern "C" void lrsc_buffer_free(void* p) { std::free(p); }

// the host image of a strand that was packed on the device: a copy of the packed arrays (a third of a byte per symbol)
int lrsc::image_from_device(const PackedStrand& ps, uint64_t N, uint64_t n_runs, StrandImage& im, std::string& err)
{
    im.n_blocks = ps.n_blocks;
    im.n_symbols = N;
    im.n_runs = n_runs;
    for(int c = 0; c < 5; ++c) im.pred[c] = ps.pred[c];
    im.blocks.resize(ps.n_blocks * 64);
    im.dollars.resize(ps.n_dollars);
    im.dollar_dir.resize(ps.n_dir);
    hipError_t e = hipMemcpy(im.blocks.data(), ps.blocks, im.blocks.size(), hipMemcpyDeviceToHost);
    if(e == hipSuccess && ps.n_dollars) e = hipMemcpy(im.dollars.data(), ps.dollars, ps.n_dollars * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if(e == hipSuccess) e = hipMemcpy(im.dollar_dir.data(), ps.dollar_dir, ps.n_dir * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if(e != hipSuccess) { err = std::string("copy of the packed index to the host: ") + hipGetErrorString(e); return LRSC_ERR_DEVICE; }
    return LRSC_OK;
}

int lrsc::adopt_packed(const PackedStrand& ps, uint64_t N, uint64_t n_runs, int s, DeviceCopy& dc, StrandImage& im, std::string& err)
{
    dc.blocks[s] = ps.blocks;
    dc.dollars[s] = ps.dollars;
    dc.dollar_dir[s] = ps.dollar_dir;
    return image_from_device(ps, N, n_runs, im, err);
}

int lrsc::adopt_packed(uint8_t* d_bwt, uint64_t N, bool wide, int s, DeviceCopy& dc, StrandImage& im, double& pack_ms, std::string& err)
{
    const auto t0 = std::chrono::steady_clock::now();
    PackedStrand ps;
    const int st = pack_strand_device(d_bwt, N, wide, ps, err);
    (void)hipFree(d_bwt);
    if(st != LRSC_OK) return st;
    pack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return adopt_packed(ps, N, 0, s, dc, im, err);
}

// profile_fmt is applied to ms[0], ms[1], ms[2], ms[3]: it may consume at most those four doubles, in that order, and nothing else
int lrsc::finish_index(lrsc_index* idx, int device, DeviceCopy& dc, int st, uint64_t n_dollars, int bad_status, const char* bad_msg, double ms[4],
                       int tables_slot, const char* profile_fmt)
{
    if(st == LRSC_OK && bad_msg && (idx->image[0].dollars.size() != n_dollars || idx->image[1].dollars.size() != n_dollars))
        st = fail(bad_status, bad_msg);
    if(st == LRSC_OK) {
        const auto t0 = std::chrono::steady_clock::now();
        std::lock_guard<std::mutex> lock(idx->mu);
        st = register_copy(idx, device, dc);
        ms[tables_slot] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if(st != LRSC_OK) { free_device_copy(dc); delete idx; return st; }
    if(std::getenv("LRSC_BWT_PROFILE")) std::fprintf(stderr, profile_fmt, ms[0], ms[1], ms[2], ms[3]);
    return LRSC_OK;
}

// One strand of lrsc_index_build: BWT on the device -> packed image on the device (dc.*[s]) -> host image.  d_bwt is gone before
// the next strand starts.
static int build_strand(const char* reads, const uint64_t* off, uint32_t n_reads, int s, int device, bool wide, StrandImage& im,
                        DeviceCopy& dc, double ms[2], std::string& err)
{
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t* d_bwt = nullptr;
    const int st = build_bwt_resident(reads, off, n_reads, s, device, &d_bwt, nullptr, err);
    if(st != LRSC_OK) return st;
    ms[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return adopt_packed(d_bwt, off[n_reads] + n_reads, wide, s, dc, im, ms[1], err);
}

extern "C" int lrsc_index_build(const char* reads, const uint64_t* read_off, uint32_t n_reads, int device, lrsc_index** out)
{
    if(!reads || !out || n_reads == 0) return fail(LRSC_ERR_ARG, "null / empty read set");
    int st = check_offsets(read_off, n_reads);
    if(st != LRSC_OK) return st;
    lrsc_index* idx = new(std::nothrow) lrsc_index();
    if(!idx) return fail(LRSC_ERR_NOMEM, "lrsc_index");
    idx->num_strings = n_reads;
    idx->num_symbols = read_off[n_reads] + n_reads;
    idx->wide = index_is_wide(idx->num_symbols);
    DeviceCopy dc;
    double ms[4] = {0., 0., 0., 0.};
    std::string err;
    for(int s = 0; s < 2 && st == LRSC_OK; ++s) {
        st = build_strand(reads, read_off, n_reads, s, device, idx->wide, idx->image[s], dc, ms, err);
        if(st != LRSC_OK) st = fail(st, err);
    }
    st = finish_index(idx, device, dc, st, n_reads, LRSC_OK, nullptr, ms, 2, "[lrsc] index build: bwt %.3f ms, pack %.3f ms, tables %.3f ms\n");
    if(st != LRSC_OK) return st;
    *out = idx;
    return LRSC_OK;
}

// ---------------------------------------------------------------------------------------
// two resident indexes merged on the device (fm_merge.hip)
// ---------------------------------------------------------------------------------------
// One strand of lrsc_index_merge: walk + interleave -> BWT of the union on the device -> packed image on the device (dc.*[s]) ->
// host image (adopt_packed).  rank[] goes once the origin is read from it, the BWT once it is packed.
// ms: walk, interleave, pack.
static int merge_strand(const FmStrand& a, bool wide_a, const FmStrand& b, bool wide_b, int s, bool wide, uint8_t* origin, StrandImage& im,
                        DeviceCopy& dc, double ms[3], std::string& err)
{
    uint8_t* d_bwt = nullptr;
    uint64_t* d_rank = nullptr;
    int st = merge_strand_device(a, wide_a, b, wide_b, &d_bwt, &d_rank, ms, err);
    if(st != LRSC_OK) return st;
    if(origin) st = merge_origin_device(a, b, d_rank, origin, err);
    (void)hipFree(d_rank);
    if(st != LRSC_OK) { (void)hipFree(d_bwt); return st; }
    return adopt_packed(d_bwt, a.n_symbols + b.n_symbols, wide, s, dc, im, ms[2], err);
}

// the strands of idx's copy on `device`
int lrsc::resident_strands(lrsc_index* idx, int device, FmStrand fs[2], bool& wide)
{
    std::lock_guard<std::mutex> lock(idx->mu);
    auto it = idx->copies.find(device);
    if(it == idx->copies.end()) return fail(LRSC_ERR_DEVICE, "index not uploaded to this device (call lrsc_index_upload)");
    fs[0] = it->second.dev.strand[0];
    fs[1] = it->second.dev.strand[1];
    wide = idx->wide;
    return LRSC_OK;
}

extern "C" int lrsc_index_merge(lrsc_index* a, lrsc_index* b, int device, lrsc_index** out, uint8_t* dollar_origin)
{
    if(!a || !b || !out) return fail(LRSC_ERR_ARG, "null");
    FmStrand fa[2], fb[2];
    bool wide_a = false, wide_b = false;
    int st = resident_strands(a, device, fa, wide_a);
    if(st == LRSC_OK) st = resident_strands(b, device, fb, wide_b);
    if(st != LRSC_OK) return st;
    const uint64_t n_reads = a->num_strings + b->num_strings;
    if(n_reads >= (1ull << 32)) return fail(LRSC_ERR_UNSUPPORTED, "more than 2^32 reads");
    HIP_TRY(hipSetDevice(device));
    lrsc_index* idx = new(std::nothrow) lrsc_index();
    if(!idx) return fail(LRSC_ERR_NOMEM, "lrsc_index");
    idx->num_strings = n_reads;
    idx->num_symbols = a->num_symbols + b->num_symbols;
    idx->wide = index_is_wide(idx->num_symbols);
    std::vector<uint8_t> origin(dollar_origin ? 2 * n_reads : 0);
    DeviceCopy dc;
    double ms[4] = {0., 0., 0., 0.};
    std::string err;
    for(int s = 0; s < 2 && st == LRSC_OK; ++s) {
        st = merge_strand(fa[s], wide_a, fb[s], wide_b, s, idx->wide, dollar_origin ? origin.data() + s * n_reads : nullptr, idx->image[s], dc, ms, err);
        if(st != LRSC_OK) st = fail(st, err);
    }
    st = finish_index(idx, device, dc, st, n_reads, LRSC_ERR_DEVICE, "index merge: the '$' rows of the result are not those of its inputs", ms, 3,
                      "[lrsc] index merge: walk %.3f ms, interleave %.3f ms, pack %.3f ms, tables %.3f ms\n");
    if(st != LRSC_OK) return st;
    if(dollar_origin) std::memcpy(dollar_origin, origin.data(), origin.size());
    *out = idx;
    return LRSC_OK;
}

// ---------------------------------------------------------------------------------------
// a saved index, decoded on the device (fm_unrle.hip)
// ---------------------------------------------------------------------------------------
// One strand of the device route: units -> device -> packed image on the device (dc.*[s]) -> host image by a copy of the packed
// arrays.  The units are gone from the device before the next strand starts.  ms: copy of the units, decode + pack.
static int unrle_strand(const uint8_t* units, uint64_t n_units, uint64_t N, int s, bool wide, StrandImage& im, DeviceCopy& dc, double ms[2],
                        std::string& err)
{
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    uint8_t* d_units = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_units), std::max<uint64_t>(n_units, 1));
    if(e == hipSuccess && n_units) e = hipMemcpy(d_units, units, n_units, hipMemcpyHostToDevice);
    if(e != hipSuccess) {
        if(d_units) (void)hipFree(d_units);
        err = std::string("copy of the RL units to the device: ") + hipGetErrorString(e);
        return LRSC_ERR_DEVICE;
    }
    const auto t1 = clk::now();
    PackedStrand ps;
    const int st = pack_units_device(d_units, n_units, N, wide, ps, nullptr, err);
    (void)hipFree(d_units);
    if(st != LRSC_OK) return st;
    ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms[1] += std::chrono::duration<double, std::milli>(clk::now() - t1).count();
    return adopt_packed(ps, N, n_units, s, dc, im, err);
}

static int index_from_units_device_impl(const uint8_t* u0, uint64_t n0, const uint8_t* u1, uint64_t n1, uint64_t num_strings,
                                        uint64_t num_symbols, int device, lrsc_index** out)
{
    HIP_TRY(hipSetDevice(device));
    lrsc_index* idx = new(std::nothrow) lrsc_index();
    if(!idx) return fail(LRSC_ERR_NOMEM, "lrsc_index");
    idx->num_strings = num_strings;
    idx->num_symbols = num_symbols;
    idx->wide = index_is_wide(num_symbols);
    const uint8_t* us[2] = {u0, u1};
    const uint64_t ns[2] = {n0, n1};
    DeviceCopy dc;
    double ms[4] = {0., 0., 0., 0.};
    std::string err;
    int st = LRSC_OK;
    for(int s = 0; s < 2 && st == LRSC_OK; ++s) {
        const auto t0 = std::chrono::steady_clock::now();
        st = unrle_strand(us[s], ns[s], num_symbols, s, idx->wide, idx->image[s], dc, ms, err);
        if(st != LRSC_OK) st = fail(st, err);
        ms[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    ms[2] -= ms[0] + ms[1];                                       // what the strands took beyond the copy and the pack
    st = finish_index(idx, device, dc, st, num_strings, LRSC_ERR_FORMAT, "number of '$' rows differs from the number of strings in the header", ms, 3,
                      "[lrsc] index open on the device: units to the device %.3f ms, decode + pack %.3f ms, image to the host %.3f ms, tables %.3f ms\n");
    if(st != LRSC_OK) return st;
    *out = idx;
    return LRSC_OK;
}

extern "C" int lrsc_index_from_units_device(const uint8_t* bwt_units, uint64_t n_bwt_units, const uint8_t* rbwt_units,
                                            uint64_t n_rbwt_units, uint64_t num_strings, uint64_t num_symbols, int device,
                                            lrsc_index** out)
{
    if(!bwt_units || !rbwt_units || !out || num_symbols == 0) return fail(LRSC_ERR_ARG, "null/empty index input");
    return index_from_units_device_impl(bwt_units, n_bwt_units, rbwt_units, n_rbwt_units, num_strings, num_symbols, device, out);
}

extern "C" int lrsc_index_open_device(const char* bwt_path, const char* rbwt_path, int device, lrsc_index** out)
{
    if(!bwt_path || !rbwt_path || !out) return fail(LRSC_ERR_ARG, "null path");
    std::vector<uint8_t> u[2];
    uint64_t nstr[2] = {0, 0}, nsym[2] = {0, 0};
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    int st = read_bwt_file(bwt_path, u[0], nstr[0], nsym[0], err);
    if(st != LRSC_OK) return fail(st, err);
    st = read_bwt_file(rbwt_path, u[1], nstr[1], nsym[1], err);
    if(st != LRSC_OK) return fail(st, err);
    if(nstr[0] != nstr[1] || nsym[0] != nsym[1]) return fail(LRSC_ERR_FORMAT, ".bwt and .rbwt disagree on strings/symbols");
    if(std::getenv("LRSC_BWT_PROFILE"))
        std::fprintf(stderr, "[lrsc] index open on the device: file read %.3f ms\n",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return index_from_units_device_impl(u[0].data(), u[0].size(), u[1].data(), u[1].size(), nstr[0], nsym[0], device, out);
}

// ---------------------------------------------------------------------------------------
// the locate tables of a resident copy (fm_locate.hip)
// ---------------------------------------------------------------------------------------
// Builds both strands' tables of dc at `rate` on the current device.  The caller holds idx->mu; on an error dc has none.
static int locate_prepare_copy(const lrsc_index* idx, DeviceCopy& dc, uint32_t rate)
{
    std::string err;
    for(int s = 0; s < 2; ++s) {
        const int st = locate_prepare_device(dc.dev.strand[s], idx->wide, rate, dc.locate[s], err);
        if(st != LRSC_OK) {
            for(int u = 0; u < s; ++u) locate_free_device(dc.locate[u]);
            return fail(st, err);
        }
    }
    dc.located = true;
    return LRSC_OK;
}

extern "C" int lrsc_index_locate_prepare(lrsc_index* idx, int device, uint32_t sample_rate)
{
    if(!idx) return fail(LRSC_ERR_ARG, "null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    auto it = idx->copies.find(device);
    if(it == idx->copies.end()) return fail(LRSC_ERR_DEVICE, "index not uploaded to this device (call lrsc_index_upload)");
    DeviceCopy& dc = it->second;
    if(dc.located) {
        if(dc.locate[0].rate == sample_rate) return LRSC_OK;
        return fail(LRSC_ERR_ARG, "locate tables already prepared with rate " + std::to_string(dc.locate[0].rate));
    }
    HIP_TRY(hipSetDevice(device));
    return locate_prepare_copy(idx, dc, sample_rate);
}

extern "C" int lrsc_index_lexico_order(lrsc_index* idx, int strand, int device, uint32_t* order, uint32_t* read_len)
{
    if(!idx || !order) return fail(LRSC_ERR_ARG, "null");
    if(strand != LRSC_BWT && strand != LRSC_RBWT) return fail(LRSC_ERR_ARG, "strand must be LRSC_BWT or LRSC_RBWT");
    std::lock_guard<std::mutex> lock(idx->mu);
    auto it = idx->copies.find(device);
    if(it == idx->copies.end()) return fail(LRSC_ERR_DEVICE, "index not uploaded to this device (call lrsc_index_upload)");
    DeviceCopy& dc = it->second;
    HIP_TRY(hipSetDevice(device));
    if(!dc.located) {
        const int st = locate_prepare_copy(idx, dc, 0);
        if(st != LRSC_OK) return st;
    }
    const LocateTables& t = dc.locate[strand];
    HIP_TRY(hipMemcpy(order, t.order, idx->num_strings * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if(read_len) HIP_TRY(hipMemcpy(read_len, t.read_len, idx->num_strings * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return LRSC_OK;
}

extern "C" int lrsc_index_units(lrsc_index* idx, int strand, int device, uint8_t** units_out, uint64_t* n_units_out)
{
    if(!idx || !units_out || !n_units_out) return fail(LRSC_ERR_ARG, "null");
    if(strand != LRSC_BWT && strand != LRSC_RBWT) return fail(LRSC_ERR_ARG, "strand must be LRSC_BWT or LRSC_RBWT");
    FmStrand fs;
    bool wide;
    {
        std::lock_guard<std::mutex> lock(idx->mu);
        auto it = idx->copies.find(device);
        if(it == idx->copies.end()) return fail(LRSC_ERR_DEVICE, "index not uploaded to this device (call lrsc_index_upload)");
        fs = it->second.dev.strand[strand];
        wide = idx->wide;
    }
    HIP_TRY(hipSetDevice(device));
    uint8_t* d_units = nullptr;
    uint64_t n_units = 0;
    std::string err;
    const int st = rle_strand_device(fs, wide, &d_units, &n_units, err);
    if(st != LRSC_OK) return fail(st, err);
    return units_to_host(d_units, n_units, units_out, n_units_out);
}

extern "C" int lrsc_index_write(lrsc_index* idx, int device, const char* bwt_path, const char* rbwt_path)
{
    if(!idx || !bwt_path || !rbwt_path) return fail(LRSC_ERR_ARG, "null");
    const char* paths[2] = {bwt_path, rbwt_path};
    for(int s = 0; s < 2; ++s) {
        uint8_t* units = nullptr;
        uint64_t n_units = 0;
        int st = lrsc_index_units(idx, s, device, &units, &n_units);
        if(st != LRSC_OK) return st;
        st = lrsc_write_bwt_file(paths[s], units, n_units, idx->num_strings, idx->num_symbols);
        std::free(units);
        if(st != LRSC_OK) return st;
    }
    return LRSC_OK;
}

extern "C" int lrsc_write_bwt_file(const char* path, const uint8_t* units, uint64_t n_units, uint64_t num_strings,
                                   uint64_t num_symbols)
{
    if(!path || (!units && n_units)) return fail(LRSC_ERR_ARG, "null");
    std::FILE* f = std::fopen(path, "wb");
    if(!f) return fail(LRSC_ERR_IO, std::string("cannot open ") + path);
    uint8_t hdr[30];
    const uint16_t magic = 0xCACA;
    const int32_t flag = 0;   // BWF_NOFMI
    std::memcpy(hdr, &magic, 2);
    std::memcpy(hdr + 2, &num_strings, 8);
    std::memcpy(hdr + 10, &num_symbols, 8);
    std::memcpy(hdr + 18, &n_units, 8);
    std::memcpy(hdr + 26, &flag, 4);
    bool ok = std::fwrite(hdr, 1, 30, f) == 30;
    ok = ok && std::fwrite(units, 1, n_units, f) == n_units;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? LRSC_OK : fail(LRSC_ERR_IO, std::string("short write to ") + path);
}
