// begin_host.hip -- TEST INFRASTRUCTURE ONLY (never linked into or loaded by the product).
//
// Runs Walk::begin_static of longreadselfcorrect_amd/csrc/walk_device.h -- the source wp_begin_kernel, walk_extend_kernel and the
// wide kernels compile for gfx950 -- on the CPU over interval lists given directly (query codes + one key per offset and strand),
// so that the rule "sort only a list with a repeated idmer code" can be held against "sort every list" without an index or a
// device.  hb_check builds the tables of one query three ways and compares them:
//   forced   sort_always = true (LRSC_WP_BEGIN_SORT): every list takes the introsort
//   default  the sort only where a code repeats among the valid entries
//   legacy   a restatement, in this file, of the build as it was when every list was sorted (compact, introsort, chains with a tail array)
// Built twice by the Makefile: as a shared library for pytest, and with HB_MAIN as a stand-alone program under
// -fsanitize=address,undefined that runs hb_check over a file of cases.  No HIP runtime call is made.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../longreadselfcorrect_amd/csrc/walk_device.h"

using namespace lrsc;

namespace {

struct Tables {
    std::vector<SortItem> it[2];
    std::vector<uint16_t> next[2], head;          // head: [0, 256) fwd, [256, 512) rvc
    uint32_t n[2] = {0, 0}, rep = 0;
};

uint32_t code_at(const uint8_t* q, uint32_t i, uint32_t seed)
{
    uint32_t c = 0;
    for(uint32_t t = 0; t < seed; ++t) c = (c << 2) | q[i + t];
    return c;
}

void fill_items(Tables& T, const uint8_t* q, uint32_t lq, uint32_t seed, const uint64_t* keyf, const uint64_t* keyr)
{
    const uint32_t n9 = lq >= seed ? lq - seed + 1 : 0;
    for(int s = 0; s < 2; ++s) {
        // slack behind the arrays is filled with a pattern: nothing may be written past n9 entries
        T.it[s].assign(n9 + 1, SortItem{0x5151515151515151ull, 0x51515151u, 0x51515151u});
        T.next[s].assign(n9 + 1, 0x5151u);
        for(uint32_t i = 0; i < n9; ++i) T.it[s][i] = SortItem{s ? keyr[i] : keyf[i], i, code_at(q, i, seed)};
    }
    T.head.assign(512, 0x5151u);
}

void build(Tables& T, const uint8_t* q, uint32_t lq, uint32_t seed, const uint64_t* keyf, const uint64_t* keyr, bool force)
{
    fill_items(T, q, lq, seed, keyf, keyr);
    const uint32_t n5 = lq >= 5 ? lq - 4 : 0;
    std::vector<uint16_t> head5(1024), next5(n5 + 1);
    std::vector<uint8_t> flags5(n5 + 1, 0);
    Walk<false> W;
    W.q = q; W.Lq = lq; W.seedSize = seed; W.minOverlap = 13; W.initk = 0; W.path_len = 0; W.n_term = 0;
    W.it9f = T.it[0].data(); W.it9r = T.it[1].data();
    W.next9f = T.next[0].data(); W.next9r = T.next[1].data();
    W.head9f = T.head.data(); W.head9r = T.head.data() + 256;
    W.head5 = head5.data(); W.next5 = next5.data(); W.flags5 = flags5.data();
    W.sort_always = force;
    W.begin_static();
    T.n[0] = W.n9f; T.n[1] = W.n9r; T.rep = W.rep9;
}

// the build of one list as it was before: every list sorted
uint32_t legacy_build9(SortItem* it, uint32_t n_all, uint16_t* head, uint16_t* next)
{
    uint32_t n = 0;
    for(uint32_t i = 0; i < n_all; ++i)
        if(it[i].key != kNoKey) { if(n != i) it[n] = it[i]; ++n; }
    introsort(it, (int64_t)n);
    for(uint32_t b = 0; b < 256; ++b) head[b] = 0xFFFFu;
    uint16_t tail[256];
    for(uint32_t j = 0; j < n; ++j) {
        const uint32_t code = it[j].pad;
        const uint32_t hb = (code ^ (code >> 9)) & 255u;
        next[j] = 0xFFFFu;
        if(head[hb] == 0xFFFFu) head[hb] = (uint16_t)j; else next[tail[hb]] = (uint16_t)j;
        tail[hb] = (uint16_t)j;
    }
    return n;
}

void build_legacy(Tables& T, const uint8_t* q, uint32_t lq, uint32_t seed, const uint64_t* keyf, const uint64_t* keyr)
{
    fill_items(T, q, lq, seed, keyf, keyr);
    const uint32_t n9 = lq >= seed ? lq - seed + 1 : 0;
    for(int s = 0; s < 2; ++s) T.n[s] = legacy_build9(T.it[s].data(), n9, T.head.data() + 256 * s, T.next[s].data());
}

// what seed_support_core reads for `code`: val of the chain's entries that carry it, in chain order; false on a broken chain
bool chain_vals(const Tables& T, int s, uint32_t code, std::vector<uint32_t>& out)
{
    out.clear();
    const uint32_t hb = (code ^ (code >> 9)) & 255u;
    uint32_t steps = 0;
    for(uint32_t j = T.head[256 * s + hb]; j != 0xFFFFu; j = T.next[s][j]) {
        if(j >= T.n[s] || ++steps > T.n[s]) return false;
        if(T.it[s][j].pad == code) out.push_back(T.it[s][j].val);
    }
    return true;
}

bool same_arrays(const Tables& A, const Tables& B, int s, uint32_t n9)
{
    // the whole item array (the stale entries behind the compacted ones too), the bucket heads and next[] of the chained entries
    if(A.n[s] != B.n[s]) return false;
    if(std::memcmp(A.it[s].data(), B.it[s].data(), (size_t)(n9 + 1) * sizeof(SortItem)) != 0) return false;
    if(std::memcmp(A.head.data() + 256 * s, B.head.data() + 256 * s, 256 * sizeof(uint16_t)) != 0) return false;
    return std::memcmp(A.next[s].data(), B.next[s].data(), (size_t)A.n[s] * sizeof(uint16_t)) == 0;
}

} // namespace

// -> 0, or 10 * property + strand of the first check that fails:
//   1 forced != legacy arrays          2 default's repeat flag != a repeated code among the valid entries (counted here)
//   3 list with a repeat: default != forced arrays, byte for byte
//   4 a chain is broken / leaves its list            5 filtered val sequence of some code differs between default and forced
//   6 the filtered entries of a code are not exactly the valid offsets that carry it      7 an array was written past its end
// n_valid[2], repeated[2]: per strand, valid entries and whether some code repeats among them
extern "C" int hb_check(const uint8_t* q, uint32_t lq, uint32_t seed, const uint64_t* keyf, const uint64_t* keyr, uint32_t* n_valid,
                        uint32_t* repeated)
{
    const uint32_t n9 = lq >= seed ? lq - seed + 1 : 0;
    Tables F, D, G;
    build(F, q, lq, seed, keyf, keyr, true);
    build(D, q, lq, seed, keyf, keyr, false);
    build_legacy(G, q, lq, seed, keyf, keyr);
    std::vector<uint32_t> vf, vd;
    for(int s = 0; s < 2; ++s) {
        const uint64_t* key = s ? keyr : keyf;
        // valid offsets by code, ascending
        std::vector<std::pair<uint32_t, uint32_t>> byc;
        for(uint32_t i = 0; i < n9; ++i)
            if(key[i] != kNoKey) byc.push_back({code_at(q, i, seed), i});
        std::sort(byc.begin(), byc.end());
        bool rep = false;
        for(size_t k = 1; k < byc.size(); ++k) rep |= byc[k].first == byc[k - 1].first;
        n_valid[s] = (uint32_t)byc.size();
        repeated[s] = rep ? 1u : 0u;

        if(F.n[s] != byc.size() || !same_arrays(F, G, s, n9)) return 10 + s;
        if((((D.rep >> s) & 1u) != 0) != rep || D.n[s] != byc.size()) return 20 + s;
        if(rep && !same_arrays(D, F, s, n9)) return 30 + s;
        for(const Tables* T : {&F, &D}) {
            const SortItem& e = T->it[s][n9];
            if(e.key != 0x5151515151515151ull || e.val != 0x51515151u || e.pad != 0x51515151u || T->next[s][n9] != 0x5151u) return 70 + s;
        }
        for(size_t k = 0; k < byc.size();) {
            size_t k1 = k;
            while(k1 < byc.size() && byc[k1].first == byc[k].first) ++k1;
            if(!chain_vals(F, s, byc[k].first, vf) || !chain_vals(D, s, byc[k].first, vd)) return 40 + s;
            if(vf != vd) return 50 + s;
            std::sort(vd.begin(), vd.end());
            if(vd.size() != k1 - k) return 60 + s;
            for(size_t t = 0; t < vd.size(); ++t)
                if(vd[t] != byc[k + t].second) return 60 + s;
            k = k1;
        }
    }
    return 0;
}

#ifdef HB_MAIN
// cases file: u32 count, then per case u32 lq, u32 seed, lq code bytes, n9 fwd keys, n9 rvc keys (u64, n9 = lq - seed + 1 or 0)
int main(int argc, char** argv)
{
    if(argc != 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if(!f) { std::perror(argv[1]); return 2; }
    uint32_t count = 0;
    if(std::fread(&count, 4, 1, f) != 1) return 2;
    uint32_t lists = 0, with_repeat = 0;
    for(uint32_t c = 0; c < count; ++c) {
        uint32_t hdr[2];
        if(std::fread(hdr, 4, 2, f) != 2) return 2;
        const uint32_t lq = hdr[0], seed = hdr[1], n9 = lq >= seed ? lq - seed + 1 : 0;
        std::vector<uint8_t> q(lq);
        std::vector<uint64_t> kf(n9), kr(n9);
        if(lq && std::fread(q.data(), 1, lq, f) != lq) return 2;
        if(n9 && (std::fread(kf.data(), 8, n9, f) != n9 || std::fread(kr.data(), 8, n9, f) != n9)) return 2;
        uint32_t nv[2], rp[2];
        const int r = hb_check(q.data(), lq, seed, kf.data(), kr.data(), nv, rp);
        if(r != 0) { std::fprintf(stderr, "case %u: hb_check = %d\n", c, r); return 1; }
        lists += 2; with_repeat += rp[0] + rp[1];
    }
    std::fclose(f);
    std::printf("%u cases ok: %u lists, %u with a repeated code\n", count, lists, with_repeat);
    return 0;
}
#endif
