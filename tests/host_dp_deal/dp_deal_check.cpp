// dp_deal_check.cpp -- csrc/dp_deal.h against its contract, as a program of its own (tests/test_dp_deal_host.py builds it with
// -fsanitize=address,undefined and runs it).  For seeded random launch sets and the edge cases (no launches, one launch, more streams
// than launches, equal weights, no streams, a weight sum beyond 64 bits): every launch is dealt exactly once; a stream's launches go
// widest LDS first; the deal is the greedy one (largest work first to the least loaded stream), so the most loaded stream carries
// at most the mean load plus the largest launch.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "dp_deal.h"

using namespace lrsc;

namespace {
int fails = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if(!(cond)) { std::printf("FAIL %s: ", what); std::printf(__VA_ARGS__); std::printf("\n"); if(++fails > 20) std::exit(1); } \
    } while(0)

void check(const char* what, const std::vector<DpDealLaunch>& ls, uint32_t n_streams, bool sums_fit = true)
{
    const std::vector<std::vector<uint32_t>> d = dp_deal(ls, n_streams);
    CHECK(d.size() == n_streams, "%zu streams for %u", d.size(), n_streams);
    std::vector<uint32_t> seen(ls.size(), 0);
    std::vector<uint64_t> load(n_streams, 0);
    size_t dealt = 0;
    for(uint32_t s = 0; s < d.size(); ++s) {
        for(size_t t = 0; t < d[s].size(); ++t) {
            const uint32_t i = d[s][t];
            CHECK(i < ls.size(), "stream %u holds launch %u of %zu", s, i, ls.size());
            if(i >= ls.size()) continue;
            ++seen[i]; ++dealt;
            load[s] += sums_fit ? ls[i].work : 0;
            if(t) {
                const DpDealLaunch& p = ls[d[s][t - 1]];
                CHECK(p.lds > ls[i].lds || (p.lds == ls[i].lds && d[s][t - 1] < i), "stream %u: launch %u (lds %u) after %u (lds %u)", s, i,
                      ls[i].lds, d[s][t - 1], p.lds);
            }
        }
    }
    if(n_streams == 0) { CHECK(dealt == 0, "%zu launches dealt to no stream", dealt); return; }
    CHECK(dealt == ls.size(), "%zu of %zu launches dealt", dealt, ls.size());
    for(size_t i = 0; i < ls.size(); ++i) CHECK(seen[i] == 1, "launch %zu dealt %u times", i, seen[i]);
    if(!sums_fit || ls.empty()) return;
    // more streams than launches: nobody waits behind another launch
    if(ls.size() <= n_streams) for(uint32_t s = 0; s < n_streams; ++s) CHECK(d[s].size() <= 1, "stream %u holds %zu of %zu launches", s, d[s].size(), ls.size());
    // the greedy bound: when the last launch of the most loaded stream was dealt, that stream was the least loaded one
    uint64_t total = 0, w_max = 0, l_max = 0;
    for(const DpDealLaunch& l : ls) { total += l.work; w_max = l.work > w_max ? l.work : w_max; }
    for(uint64_t l : load) l_max = l > l_max ? l : l_max;
    CHECK(l_max <= total / n_streams + w_max, "most loaded stream %llu, mean %llu, largest launch %llu", (unsigned long long)l_max,
          (unsigned long long)(total / n_streams), (unsigned long long)w_max);
    // and it depends on nothing but its arguments
    CHECK(dp_deal(ls, n_streams) == d, "a second deal differs");
}
} // namespace

int main()
{
    check("no launches", {}, 3);
    check("no launches, no streams", {}, 0);
    check("no streams", {{5, 100}, {7, 200}}, 0);
    check("one launch", {{1000, 4096}}, 3);
    check("one launch, one stream", {{1000, 4096}}, 1);
    check("more streams than launches", {{10, 8192}, {30, 0}}, 8);
    check("equal weights", std::vector<DpDealLaunch>(10, DpDealLaunch{77, 12288}), 3);
    check("equal weights, different LDS", {{5, 100}, {5, 300}, {5, 200}, {5, 300}, {5, 0}, {5, 100}}, 2);
    check("zero weights", std::vector<DpDealLaunch>(7, DpDealLaunch{0, 64}), 3);
    check("weights beyond 64 bits together", {{UINT64_MAX, 1}, {UINT64_MAX, 2}, {UINT64_MAX - 1, 3}, {5, 4}}, 2, false);
    {   // equal weights go out round robin in index order: the deal is fully determined
        const char* what = "equal weights, the deal itself";
        const auto d = dp_deal(std::vector<DpDealLaunch>(5, DpDealLaunch{9, 0}), 2);
        CHECK((d == std::vector<std::vector<uint32_t>>{{0, 2, 4}, {1, 3}}), "not {0,2,4},{1,3}");
    }
    {   // the bucket ladder of a pass: the heaviest launch alone, the rest shared, widest first inside a stream
        const char* what = "a pass of five buckets";
        const auto d = dp_deal({{100, 8192}, {900, 16384}, {300, 69120}, {250, 138240}, {50, 0}}, 3);
        CHECK((d == std::vector<std::vector<uint32_t>>{{1}, {2, 4}, {3, 0}}), "not {1},{2,4},{3,0}");
    }
    std::mt19937_64 rng(0x5EED);
    for(int round = 0; round < 2000; ++round) {
        std::vector<DpDealLaunch> ls(rng() % 14);
        for(DpDealLaunch& l : ls) { l.work = rng() % (round % 3 ? 1000000 : 4); l.lds = (uint32_t)(rng() % 5) * 32768u; }
        check("random launches", ls, (uint32_t)(rng() % 6));
    }
    if(fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok: dp_deal.h holds its contract\n");
    return 0;
}
