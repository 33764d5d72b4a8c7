// saipb.hip -- kernels of lrsc_saipb_merge (the reference's SAIPBSelfCorrectTree): the job itself is
// saipb_run_job() in saipb_device.h, the source the CPU test harness compiles for the host as well.
//   saipb_seed_kernel   one lane per addHashBySingleSeed call: findBiInterval of the seed's large k-mer and the repeat guard's
//                       frequency.  The host sizes every job's table from these before any chunk starts.
//   saipb_merge_kernel  one wavefront per job (blocks of 64): collect, tree and result choice with no host step in between.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "saipb_device.h"

namespace lrsc {

template <bool WIDE>
__device__ __forceinline__ SaipbCtx<WIDE> saipb_ctx(const FmIndexDev& fm, const uint32_t* mtab, const uint8_t* codes)
{
    using P = typename Lay<WIDE>::pos_t;
    SaipbCtx<WIDE> c;
    c.sF = strand_consts<P>(fm.strand[LRSC_RBWT]);
    c.sR = strand_consts<P>(fm.strand[LRSC_BWT]);
    c.fm = &fm;
    c.mtab = mtab;
    c.codes = codes;
    return c;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void saipb_seed_kernel(FmIndexDev fm, const uint8_t* __restrict__ codes, const SaipbSeed* __restrict__ seeds,
                                                         uint32_t n, SaipbSeedInfo* __restrict__ info)
{
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTabSize<WIDE>::value];
    init_mask_table<WIDE>(mtab);
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if(i >= n) return;
    const SaipbCtx<WIDE> c = saipb_ctx<WIDE>(fm, mtab, codes);
    info[i] = saipb_seed_info<WIDE>(c, seeds[i]);
}

template <bool WIDE>
__global__ __launch_bounds__(64) void saipb_merge_kernel(FmIndexDev fm, const uint8_t* __restrict__ codes, const SaipbSeed* __restrict__ seeds,
                                                         const SaipbSeedInfo* __restrict__ info, const SaipbJob* __restrict__ jobs, uint32_t n,
                                                         uint8_t* ws, char* out, SaipbOut* __restrict__ results)
{
    __shared__ __attribute__((aligned(16))) uint32_t mtab[MaskTabSize<WIDE>::value];
    init_mask_table<WIDE>(mtab);
    const uint32_t j = blockIdx.x;
    if(j >= n) return;
    const SaipbCtx<WIDE> c = saipb_ctx<WIDE>(fm, mtab, codes);
    const SaipbJob job = jobs[j];
    SaipbOut r;
    saipb_run_job<WIDE>(c, job, seeds, info, ws, out, r, threadIdx.x, 64u);
    if(threadIdx.x == 0) results[j] = r;
}

hipError_t launch_saipb_seed_info(const FmIndexDev& fm, const uint8_t* codes, const SaipbSeed* seeds, uint32_t n, SaipbSeedInfo* info,
                                  hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    const uint32_t blocks = (n + 255) / 256;
    if(fm.wide) hipLaunchKernelGGL(saipb_seed_kernel<true>, dim3(blocks), dim3(256), 0, stream, fm, codes, seeds, n, info);
    else        hipLaunchKernelGGL(saipb_seed_kernel<false>, dim3(blocks), dim3(256), 0, stream, fm, codes, seeds, n, info);
    return hipGetLastError();
}

hipError_t launch_saipb_merge(const FmIndexDev& fm, const uint8_t* codes, const SaipbSeed* seeds, const SaipbSeedInfo* info,
                              const SaipbJob* jobs, uint32_t n, uint8_t* ws, char* out, SaipbOut* results, hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    if(fm.wide) hipLaunchKernelGGL(saipb_merge_kernel<true>, dim3(n), dim3(64), 0, stream, fm, codes, seeds, info, jobs, n, ws, out, results);
    else        hipLaunchKernelGGL(saipb_merge_kernel<false>, dim3(n), dim3(64), 0, stream, fm, codes, seeds, info, jobs, n, ws, out, results);
    return hipGetLastError();
}

} // namespace lrsc
