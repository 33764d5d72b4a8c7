// fm_launch.h -- what the .hip units of the index tools share around their kernels: the layout of a WIDE flag, the mask table in
// LDS, a wavefront's sum into a counter, and on the host the device allocations of one call and the error check of a HIP call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "fm_strand.h"
#include "kernels.h"

namespace lrsc {

template <bool WIDE> struct BlockOf { using type = Block32; };
template <> struct BlockOf<true> { using type = Block64; };

// the layout's mask table (fm_strand.h's MaskTab), filled by the whole workgroup; the caller synchronises
template <class Block>
__device__ __forceinline__ void fill_mask_table(uint32_t* tab)
{
    for(uint32_t i = threadIdx.x; i < MaskTab<Block>::kWords; i += blockDim.x) tab[i] = mask_word<Block>(i);
}

// The sum of v over the wavefront, in its lane 0.  Every lane of the wavefront has to be here.
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for(int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// a wavefront's Occ queries and block loads, as wave_sum left them -> the counter shard of its workgroup
__device__ __forceinline__ void wave_count(DevCounters* ctr, unsigned long long rank_queries, unsigned long long block_loads)
{
    if(ctr != nullptr && (threadIdx.x & 63) == 0 && rank_queries) {
        DevCounters* shard = ctr + (blockIdx.x & (kCtrShards - 1));
        atomicAdd(&shard->rank_queries, rank_queries);
        atomicAdd(&shard->block_loads, block_loads);
    }
}
// The device allocations of one call: freed when it ends, except those the call hands to its caller (keep).
struct Owned {
    std::vector<void*> ptrs;
    ~Owned() { for(void* p : ptrs) (void)hipFree(p); }
    template <class T> hipError_t alloc(T** p, size_t n)
    {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
        if(e == hipSuccess) { ptrs.push_back(q); *p = static_cast<T*>(q); }
        return e;
    }
    void keep(void* p) { ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), p), ptrs.end()); }
};

// In a function that returns an lrsc_status and has `std::string& err`: a HIP error leaves with the expression and HIP's text in
// err.  The unit says before its first use what running out of device memory answers: `constexpr int kOomStatus = ...;`.
#define DEV_TRY(expr)                                                                \
    do {                                                                             \
        hipError_t _e = (expr);                                                      \
        if(_e != hipSuccess) {                                                       \
            err = std::string(#expr) + ": " + hipGetErrorString(_e);                 \
            return _e == hipErrorOutOfMemory ? kOomStatus : LRSC_ERR_DEVICE;         \
        }                                                                            \
    } while(0)

} // namespace lrsc
