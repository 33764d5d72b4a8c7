// dp_deal.h -- how the MSA launches of one pass (one per LDS-size bucket, capi_dp.cpp) are dealt to the DP stage's side streams.
// A stream runs its launches one after the other, so a pass lasts as long as its most loaded stream: the launches go out by
// estimated work, the largest first, each to the stream that has the least so far.  Host code without HIP, like dp_order.h, so that
// tests/test_dp_deal_host.py compiles it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace lrsc {

struct DpDealLaunch {
    uint64_t work;                // estimate of the launch's work: sum over its requests of query length x strings
    uint32_t lds;                 // LDS of one of its workgroups (0: it holds none)
};

// Launch indices per stream, in the order the stream runs them; every launch appears exactly once.  Ties of work go by index, ties
// of load to the stream with fewer launches (launches of requests without strings weigh nothing), then to the lowest stream, so the
// deal depends on nothing but its arguments and no stream gets a second launch while another has none.  Inside a stream the widest LDS goes first: a
// launch that needs most of a CU is placed while little else of the pass is resident.  n_streams = 0 deals nothing.
inline std::vector<std::vector<uint32_t>> dp_deal(const std::vector<DpDealLaunch>& launches, uint32_t n_streams)
{
    std::vector<std::vector<uint32_t>> out(n_streams);
    if(n_streams == 0) return out;
    std::vector<uint32_t> by_work(launches.size());
    for(uint32_t i = 0; i < by_work.size(); ++i) by_work[i] = i;
    std::sort(by_work.begin(), by_work.end(), [&](uint32_t x, uint32_t y) {
        return launches[x].work != launches[y].work ? launches[x].work > launches[y].work : x < y;
    });
    std::vector<uint64_t> load(n_streams, 0);
    for(uint32_t i : by_work) {
        uint32_t s = 0;
        for(uint32_t t = 1; t < n_streams; ++t)
            if(load[t] < load[s] || (load[t] == load[s] && out[t].size() < out[s].size())) s = t;
        out[s].push_back(i);
        const uint64_t w = launches[i].work;
        load[s] = load[s] > UINT64_MAX - w ? UINT64_MAX : load[s] + w;
    }
    for(std::vector<uint32_t>& st : out)
        std::sort(st.begin(), st.end(), [&](uint32_t x, uint32_t y) {
            return launches[x].lds != launches[y].lds ? launches[x].lds > launches[y].lds : x < y;
        });
    return out;
}

} // namespace lrsc
