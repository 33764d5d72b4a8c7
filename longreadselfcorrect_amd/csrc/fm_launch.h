// fm_launch.h -- what the .hip units of the index tools share around their kernels: the layout of a WIDE flag, the mask table in
// LDS, a wavefront's sum into a counter, the wavefront of fm_wave.h (WaveExec), and on the host the device allocations of one call
// and the error check of a HIP call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "fm_strand.h"
#include "fm_wave.h"
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

// fm_wave.h's wavefront on the device: a phase is every lane's call and then the wavefront's agreement on memory.
struct WaveExec {
    __device__ __forceinline__ static void sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    // The lane of a phase, opaque to the compiler: what a phase asks of its lane (is it below 4, odd, which base) would otherwise
    // be computed once, before the first phase, and held through all of them as a mask in two scalar registers each.
    __device__ __forceinline__ static uint32_t lane()
    {
        uint32_t l = threadIdx.x & (kWaveLanes - 1);
        asm volatile("" : "+v"(l));
        return l;
    }
    // a value that every lane holds alike, in scalar registers
    __device__ __forceinline__ static uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ static uint64_t uniform64(uint64_t v) { return ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v); }
    template <class F> __device__ __forceinline__ void each(F&& f)
    {
        f(lane());
        sync();
    }
    template <class F> __device__ __forceinline__ uint32_t min_over(F&& f)
    {
        uint32_t v = f(lane());
        sync();
#pragma unroll
        for(int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
        return uniform(v);
    }
    template <class F> __device__ __forceinline__ uint32_t sum_over(F&& f)
    {
        uint32_t v = f(lane());
        sync();
#pragma unroll
        for(int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
        return uniform(v);
    }
    template <class F> __device__ __forceinline__ uint64_t sum64_over(F&& f)
    {
        unsigned long long v = f(lane());
        sync();
#pragma unroll
        for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return uniform64(v);
    }
    template <class F, class G> __device__ __forceinline__ uint32_t scan(F&& f, G&& g)
    {
        const uint32_t l = lane(), mine = f(l);
        uint32_t incl = mine;
#pragma unroll
        for(int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
            incl += l >= (uint32_t)o ? up : 0u;
        }
        g(l, incl - mine, mine);
        sync();
        return uniform((uint32_t)__shfl((int)incl, 63, 64));
    }
};
static_assert(kWaveLanes == 64, "WaveExec's shuffles and wave_sum are a 64-lane wavefront's");

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
