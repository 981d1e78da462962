// kernels_tdvp.hip — the projections of a Gram–Schmidt pass for short vectors with many basis vectors: what the Krylov exponential of a
// TDVP step (tdvp.hpp) launches where gs_dots of kernels_linsolve.hip would leave the card idle.  A one-site region holds chi d chi
// elements (2048 at chi = 32): gs_workgroups gives it 2 workgroups, each of which walks all nb basis vectors one after the other.
// gs_dots_wide spreads the basis over a second grid dimension: workgroup (g, y) handles the GS_WIDE vectors from GS_WIDE y of element
// group g in ONE pass over the elements, w read once and kept in a register, GS_WIDE independent accumulators per thread.
// The partition and the order of every sum are those of gs_dots: thread t of element group g owns g*256 + t + k*(256*G), summed
// k-ascending, G = gs_workgroups(len); lanes by the fixed shuffle tree, the four waves ((s0 + s1) + s2) + s3.  Each part[i + nb g] is
// the same chain of separately rounded multiplies and adds (-ffp-contract=off), hence the same bits; no atomics.
#include "krylov_reduce.hpp"
#include "linsolve.hpp"

namespace t4a {

namespace {

// part[i + nb g] = sum over the elements of element group g = blockIdx.x of V[e + ld i] w[e], for the vectors i of blockIdx.y
__global__ void __launch_bounds__(256) gs_dots_wide_kernel(const double* __restrict__ V, long long ld, int nb, const double* __restrict__ w,
                                                           long long len, double* __restrict__ part)
{
    __shared__ double sred[4][GS_WIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = (int)blockIdx.y * GS_WIDE;
    const int nv = min(GS_WIDE, nb - i0); // >= 1: the grid has ceil(nb / GS_WIDE) rows
    const long long first = (long long)blockIdx.x * GS_THREADS + tid, stride = (long long)gridDim.x * GS_THREADS;
    const double* v0 = V + ld * i0;
    double acc[GS_WIDE];
#pragma unroll
    for (int ii = 0; ii < GS_WIDE; ++ii) acc[ii] = 0.0;
    if (nv == GS_WIDE) {
        for (long long e = first; e < len; e += stride) {
            const double we = w[e];
#pragma unroll
            for (int ii = 0; ii < GS_WIDE; ++ii) acc[ii] = acc[ii] + v0[e + ld * ii] * we;
        }
    } else {
        for (long long e = first; e < len; e += stride) {
            const double we = w[e];
#pragma unroll
            for (int ii = 0; ii < GS_WIDE; ++ii)
                if (ii < nv) acc[ii] = acc[ii] + v0[e + ld * ii] * we;
        }
    }
#pragma unroll
    for (int ii = 0; ii < GS_WIDE; ++ii) {
        const double s = wave_sum(acc[ii]);
        if (lane == 0) sred[wave][ii] = s;
    }
    __syncthreads();
    if (tid < nv) part[(i0 + tid) + (long long)nb * blockIdx.x] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}

} // namespace

void gs_dots_wide_launch(const double* V, size_t ld, int nb, const double* w, size_t len, double* part, hipStream_t stream)
{
    if (nb <= 0 || len == 0) return;
    const dim3 grid((unsigned)gs_workgroups(len), (unsigned)((nb + GS_WIDE - 1) / GS_WIDE));
    hipLaunchKernelGGL(gs_dots_wide_kernel, grid, dim3(GS_THREADS), 0, stream, V, (long long)ld, nb, w, (long long)len, part);
}

} // namespace t4a
