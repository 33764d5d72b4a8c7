// dp_order_check.cpp -- csrc/dp_order.h against its contract, as a program of its own (tests/test_dp_order_host.py builds it with
// -fsanitize=address,undefined and runs it): for seeded random request sets and the edge cases, every job index appears exactly once,
// class k's list holds exactly the jobs of class k, and every list is in index order.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "dp_order.h"

using namespace lrsc;

namespace {
static_assert(dp_align_class(0) == 0 && dp_align_class(4096) == 0 && dp_align_class(4097) == 1 && dp_align_class(16384) == 1 &&
              dp_align_class(16385) == 2 && dp_align_class(65536) == 2 && dp_align_class(65537) == 3 && dp_align_class(~0u) == 3,
              "the staging-size classes: 4 KB, 16 KB and 64 KB of LDS, then the global workspace");
static_assert(dp_align_stage_bytes(1, 3812) == 4096 && dp_align_stage_bytes(1, 3813) == 4100, "staging bytes of an alignment");

struct Req { uint32_t lq, cap2, n_str; };       // a DP request: its jobs are lq columns by up to cap2 rows, n_str of them

int fails = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if(!(cond)) { std::printf("FAIL %s: ", what); std::printf(__VA_ARGS__); std::printf("\n"); if(++fails > 20) std::exit(1); } \
    } while(0)

// jobs are numbered request by request, as plan_chunk numbers them (DpRequest::job_first)
void check(const char* what, const std::vector<Req>& reqs, uint32_t* class_seen)
{
    std::vector<DpOrderRun> runs;
    std::vector<uint32_t> cls_of;
    for(const Req& r : reqs) {
        const uint32_t k = dp_align_class(dp_align_stage_bytes(r.lq, r.cap2));
        if(r.n_str) runs.push_back({k, (uint32_t)cls_of.size(), r.n_str});
        for(uint32_t s = 0; s < r.n_str; ++s) cls_of.push_back(k);
    }
    // the order of the runs must not matter
    std::mt19937 sh(12345u + (uint32_t)reqs.size());
    std::shuffle(runs.begin(), runs.end(), sh);
    const DpOrder o = dp_order_build(runs);
    const size_t n = cls_of.size();
    CHECK(o.list.size() == n, "list of %zu for %zu jobs", o.list.size(), n);
    CHECK(o.begin[0] == 0 && o.begin[kDpAlignClasses + 1] == n, "lists span %u .. %u of %zu", o.begin[0], o.begin[kDpAlignClasses + 1], n);
    std::vector<uint32_t> seen(n, 0);
    for(uint32_t k = 0; k <= kDpAlignClasses; ++k) {
        CHECK(o.begin[k] <= o.begin[k + 1] && o.begin[k + 1] <= o.list.size(), "class %u: list %u .. %u", k, o.begin[k], o.begin[k + 1]);
        if(!(o.begin[k] <= o.begin[k + 1] && o.begin[k + 1] <= o.list.size())) return;
        uint64_t want = 0;
        for(size_t j = 0; j < n; ++j) want += cls_of[j] == k;
        CHECK(o.size(k) == want, "class %u: %u jobs listed, %llu exist", k, o.size(k), (unsigned long long)want);
        if(o.size(k)) class_seen[k] = 1;
        for(uint32_t t = o.begin[k]; t < o.begin[k + 1]; ++t) {
            const uint32_t j = o.list[t];
            CHECK(j < n, "class %u: job %u of %zu", k, j, n);
            if(j >= n) continue;
            ++seen[j];
            CHECK(cls_of[j] == k, "job %u of class %u in the list of class %u", j, cls_of[j], k);
            if(t > o.begin[k]) CHECK(o.list[t - 1] < j, "class %u: job %u before job %u", k, o.list[t - 1], j);
        }
    }
    for(size_t j = 0; j < n; ++j) CHECK(seen[j] == 1, "job %zu listed %u times", j, seen[j]);
}

// capacity of a request's retrieved strings (DpStage::size_requests)
uint32_t str_cap(uint32_t lq) { return ((uint32_t)(lq * 1.1 + 20) + 3) & ~3u; }
} // namespace

int main()
{
    uint32_t class_seen[kDpAlignClasses + 1] = {};
    uint32_t none[kDpAlignClasses + 1] = {};
    int sets = 0;
    for(uint32_t seed = 1; seed <= 60; ++seed, ++sets) {
        std::mt19937 rng(seed);
        const uint32_t n_req = 1 + rng() % 300;
        std::vector<Req> reqs;
        for(uint32_t i = 0; i < n_req; ++i) {
            // column counts over all four classes (4 KB, 16 KB, 64 KB of staging and beyond), many of them equal
            static const uint32_t top[4] = {1700, 7400, 31000, 60000};
            const uint32_t hi = top[rng() % 4];
            uint32_t lq = 1 + rng() % hi;
            if(rng() % 3 == 0) lq = lq / 500 * 500 + 17;
            reqs.push_back({lq, str_cap(lq), (uint32_t)(rng() % 41)});
        }
        check("random requests", reqs, class_seen);
        // the same as single jobs with their own second length, as lrsc_dp_align passes them
        for(Req& r : reqs) { r.n_str = 1; r.cap2 = rng() % (2 * r.lq + 1); }
        check("random single jobs", reqs, class_seen);
    }
    for(uint32_t k = 0; k <= kDpAlignClasses; ++k)
        if(!class_seen[k]) { std::printf("FAIL: no random set had a job of class %u\n", k); ++fails; }
    check("empty set", {}, none);
    check("requests without strings", {{100, str_cap(100), 0}, {9000, str_cap(9000), 0}}, none);
    check("one job", {{5000, str_cap(5000), 1}}, none);
    check("one job beyond the LDS", {{40000, str_cap(40000), 1}}, none);
    check("a class with no jobs", {{100, str_cap(100), 3}, {20000, str_cap(20000), 2}, {0, 0, 0}, {120, str_cap(120), 40}}, none);
    check("all jobs in one class", {{100, str_cap(100), 7}, {300, str_cap(300), 1}, {100, str_cap(100), 2}, {1500, str_cap(1500), 40}, {300, str_cap(300), 5}}, none);
    check("class bounds", {{0, 0, 1}, {1, 4096 - 4 - 264 - 16, 1}, {1, 4096 - 4 - 264 - 16 + 1, 1}, {2, 65536 - 4 - 264 - 16, 1}, {2, 65536 - 4 - 264 - 16 + 1, 1}}, none);
    sets += 7;
    if(fails) return 1;
    std::printf("ok: %d sets\n", sets);
    return 0;
}
