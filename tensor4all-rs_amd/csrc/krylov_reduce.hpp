// krylov_reduce.hpp — the fixed reduction tree of the Krylov vector kernels (kernels_linsolve.hip, kernels_dmrg.hip): 256 threads,
// the 64 lanes of a wave folded by a shuffle tree, then the four waves in ascending order.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace t4a {

constexpr int GS_THREADS = 256;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v; // lane 0
}

// sum of `v` over the workgroup, valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s4)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

} // namespace t4a
