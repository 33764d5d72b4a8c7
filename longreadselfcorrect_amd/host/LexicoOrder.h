// LexicoOrder.h -- the host route to .sai / .rsai: lexicographic rank -> read index by a sort of whole reads (`stride index`,
// `--save-index`); the device route is lrsc_index_lexico_order, from the index alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace stride {

// SampledSuffixArray::buildLexicoIndex (SuffixTools/SampledSuffixArray.cpp:158-190) LF-walks each read back to its '$' row;
// that row's rank among the '$' rows is the rank of the read among all reads compared as strings ('$' < A < C < G < T, so a
// proper prefix sorts first) with equal reads in input order (sentinel order MR_SO_IO) -- computed directly here.  Read i is
// B[off[i], off[i + 1]), read backwards when rev.
inline std::vector<uint32_t> lexicoOrder(const char* B, const uint64_t* off, uint32_t n, bool rev)
{
    std::vector<uint32_t> order(n);
    for(uint32_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const uint64_t lx = off[x + 1] - off[x], ly = off[y + 1] - off[y];
        const uint64_t m = lx < ly ? lx : ly;
        for(uint64_t t = 0; t < m; ++t) {
            const char cx = rev ? B[off[x + 1] - 1 - t] : B[off[x] + t], cy = rev ? B[off[y + 1] - 1 - t] : B[off[y] + t];
            if(cx != cy) return cx < cy;
        }
        if(lx != ly) return lx < ly;
        return x < y;
    });
    return order;
}

} // namespace stride
