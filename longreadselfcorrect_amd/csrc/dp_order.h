// dp_order.h -- the order in which the align launches (dp_align.hip) hand out their alignments: one list of job indices per
// staging-size class, back to back in one array, each in index order.  Host code without HIP (the classes are defined here for that
// reason; dp_dev.h includes this header), so that tests/test_dp_order_host.py compiles it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace lrsc {

// bytes of sequence staging one alignment needs (LDS or global slice)
constexpr uint32_t dp_align_stage_bytes(uint32_t s1_len, uint32_t s2_len) { return ((s1_len + 2 + 3) & ~3u) + 264u + ((s2_len + 3) & ~3u) + 16u; }
constexpr uint32_t kDpAlignLdsCap = 64u * 1024u;
// upper bounds of the staging-size classes that run from LDS; what is beyond the last one runs from the global workspace
constexpr uint32_t kDpAlignClasses = 3;
constexpr uint32_t kDpAlignClassCap[kDpAlignClasses] = {4u * 1024u, 16u * 1024u, kDpAlignLdsCap};
constexpr uint32_t dp_align_class(uint32_t stage_bytes)
{
    uint32_t c = 0;
    while(c < kDpAlignClasses && stage_bytes > kDpAlignClassCap[c]) ++c;
    return c;                     // kDpAlignClasses = the global-workspace launch
}

// Jobs first .. first + n - 1, all of one class: the retrieved strings of one DP request (the class is that of the request's
// capacities), or one job of lrsc_dp_align.  The lists are put together from these runs: a launch of 6 x 10^6 alignments has some
// 10^5 requests.
struct DpOrderRun {
    uint32_t cls;                 // dp_align_class(..) of the run's jobs
    uint32_t first, n;
};

struct DpOrder {
    std::vector<uint32_t> list;                  // class k's jobs: list[begin[k] .. begin[k + 1])
    uint32_t begin[kDpAlignClasses + 2] = {};
    uint32_t size(uint32_t k) const { return begin[k + 1] - begin[k]; }
};

// `runs` is reordered: by class, inside a class by job index.  Index order is the measured choice ("Alignments
// from a queue"): with the longest alignments first, so that a launch would not end on one of them, the large launches ran 11-12 %
// longer.  The runs' jobs are taken to be disjoint.
inline DpOrder dp_order_build(std::vector<DpOrderRun>& runs)
{
    std::sort(runs.begin(), runs.end(), [](const DpOrderRun& x, const DpOrderRun& y) { return x.cls != y.cls ? x.cls < y.cls : x.first < y.first; });
    DpOrder o;
    uint64_t total = 0;
    for(const DpOrderRun& r : runs) total += r.n;
    o.list.reserve(total);
    uint32_t k = 0;
    for(const DpOrderRun& r : runs) {
        while(k < r.cls && k <= kDpAlignClasses) o.begin[++k] = (uint32_t)o.list.size();
        for(uint32_t s = 0; s < r.n; ++s) o.list.push_back(r.first + s);
    }
    while(k <= kDpAlignClasses) o.begin[++k] = (uint32_t)o.list.size();
    return o;
}

} // namespace lrsc
