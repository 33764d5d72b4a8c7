// walk_host_groups.hip -- TEST INFRASTRUCTURE ONLY (never linked into or loaded by the product).
//
// tests/host_walk/walk_host.hip once more, compiled with the walk's trace hook (walk_device.h: LRSC_WALK_TRACE) defined, so that
// tests/test_host_walk_groups.py can tell which shapes of the general step -- frontier sizes, children per step, threshold
// retries by leaf index, SelectFreqsOfrange calls by leaf count -- its inputs have reached.  Same entry points as the plain
// harness, plus hw_trace_reset / hw_trace_get.
#include <cstdint>
#include <cstring>

struct GroupTrace {
    uint64_t steps_by_leaves[40];      // general steps by n_cur (39 = more)
    uint64_t retries_by_leaf[40];      // threshold retries by the leaf's index in cur[]
    uint64_t selects_by_leaves[40];    // SelectFreqsOfrange calls by their leaf count (39 = more)
    uint64_t max_children;             // most children extendLeaves has made in a step
    uint64_t steps_over_64_children;
    uint64_t children_overflows;
};
static GroupTrace g_trace;

static inline void lrsc_walk_trace(int kind, uint32_t a, uint32_t b)
{
    (void)b;
    const uint32_t k = a < 39 ? a : 39;
    if(kind == 0) g_trace.steps_by_leaves[k]++;
    else if(kind == 1) { if(a > g_trace.max_children) g_trace.max_children = a; if(a > 64) g_trace.steps_over_64_children++; }
    else if(kind == 2) g_trace.retries_by_leaf[k]++;
    else if(kind == 3) g_trace.selects_by_leaves[k]++;
    else if(kind == 4) g_trace.children_overflows++;
}
#if defined(__HIP_DEVICE_COMPILE__)
#define LRSC_WALK_TRACE(kind, a, b)
#else
#define LRSC_WALK_TRACE(kind, a, b) lrsc_walk_trace((kind), (uint32_t)(a), (uint32_t)(b))
#endif

#include "../host_walk/walk_host.hip"

extern "C" void hw_trace_reset() { std::memset(&g_trace, 0, sizeof(g_trace)); }
extern "C" void hw_trace_get(uint64_t* out) { std::memcpy(out, &g_trace, sizeof(g_trace)); }
extern "C" uint32_t hw_trace_words() { return (uint32_t)(sizeof(g_trace) / sizeof(uint64_t)); }
