// TEST INFRASTRUCTURE ONLY: csrc/dp_msa_layout.h on the host.  One line per (lq, n_str, nw, global): the request's capacities as
// DpStage::size_requests derives them, every offset of MsaLayout and its two totals, and the new-column ceiling of the variant.
// tests/test_msa_layout_host.py restates the sizes and the byte counts of the host's two functions and checks the lines.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "dp_msa_layout.h"

int main()
{
    const uint32_t lqs[] = {1, 63, 64, 65, 250, 1024, 3500}, strs[] = {0, 1, 7, 64, 1000}, nws[] = {1, 2, 4, 8};
    for(uint32_t lq : lqs)
        for(uint32_t n_str : strs)
            for(uint32_t nw : nws)
                for(int global = 0; global < 2; ++global) {
                    // DpStage::size_requests (capi_dp.cpp) and dp_msa_columns (dp_dev.h); the seed length cannot exceed the query's
                    const uint32_t k = std::min(lq, 15u);
                    const uint32_t max_len = (uint32_t)(size_t)(lq * 1.1 + 20);
                    const uint32_t str_cap = (std::max(max_len, k) + 3) & ~3u;
                    const uint32_t ops_cap = (lq + str_cap + 1 + 3) & ~3u;
                    const uint32_t w_cols = 3 * lq + 128;
                    const lrsc::MsaLayout L = lrsc::msa_layout(w_cols, lq, str_cap, ops_cap, n_str, nw, global != 0);
                    std::printf("lq=%u n_str=%u nw=%u global=%d w_cols=%u str_cap=%u ops_cap=%u max_ins=%u xchg_words=%u "
                                "xchg=%u insx=%u insg=%u inss=%u lead=%u size=%u small_total=%u cnt=%u bpos=%u T=%u Rw=%u S=%u ops=%u total=%u\n",
                                lq, n_str, nw, global, w_cols, str_cap, ops_cap, lrsc::msa_max_ins(global != 0, nw), lrsc::kXchgWords,
                                L.xchg, L.insx, L.insg, L.inss, L.lead, L.size, L.small_total, L.cnt, L.bpos, L.T, L.Rw, L.S, L.ops, L.total);
                }
    return 0;
}
