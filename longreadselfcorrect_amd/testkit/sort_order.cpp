// sort_order.cpp -- test hook: runs the product's emulation of libstdc++'s std::sort (csrc/introsort_emul.h, the tie order
// of the interval-tree build in the FM-extend engine) on the host, so that tests can compare it with the real std::sort and
// with the reference's object code; and the host route to .sai / .rsai (host/LexicoOrder.h), so that tools can time it.
#include <cstdint>
#include <vector>

#include "../csrc/introsort_emul.h"
#include "../host/LexicoOrder.h"
#include "lrsc_testkit.h"

using namespace lrsc;

extern "C" int lrsc_debug_sort_order(const uint64_t* keys, uint32_t n, uint32_t* perm_out)
{
    if((!keys || !perm_out) && n) return -1;
    std::vector<SortItem> v(n);
    for(uint32_t i = 0; i < n; ++i) { v[i].key = keys[i]; v[i].val = i; v[i].pad = 0; }
    introsort(v.data(), (int64_t)n);
    for(uint32_t i = 0; i < n; ++i) perm_out[i] = v[i].val;
    return 0;
}

extern "C" int lrsc_host_lexico_order(const char* bases, const uint64_t* off, uint32_t n_reads, int reverse_reads, uint32_t* order_out)
{
    if(!bases || !off || !order_out) return -1;
    const std::vector<uint32_t> order = stride::lexicoOrder(bases, off, n_reads, reverse_reads != 0);
    for(uint32_t i = 0; i < n_reads; ++i) order_out[i] = order[i];
    return 0;
}
