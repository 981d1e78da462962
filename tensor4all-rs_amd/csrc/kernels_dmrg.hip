// kernels_dmrg.hip — what the Lanczos eigensolver of a two-site DMRG step (dmrg.hpp) adds to the launches of the linear solver:
//   * the Ritz vector out = sum_i c[i] V[:, i] over the whole basis (krylov_combine), the coefficients staged in LDS, every load
//     along the fast index of a basis vector, with the shares of |out|^2 from the same pass,
//   * the eigen-residual r = Hv - lambda v with the shares of |r|^2, <v, Hv> and <v, v> from one read of v and Hv (eig_residual):
//     the true residual of a finalise and, with lambda = 0 and no r, the two sums of the final Rayleigh quotient,
//   * a finishing launch that folds the shares of the workgroups in ascending order (krylov_finish).
// The partition is that of kernels_linsolve.hip: thread t of workgroup g owns the elements g*256 + t + k*(256*G), summed k-ascending,
// G = gs_workgroups(len); lanes by the fixed shuffle tree, the four waves and then the workgroups ascending.  No atomics; multiply and
// add are rounded separately (-ffp-contract=off): two runs give the same bits.
#include "dmrg.hpp"
#include "krylov_reduce.hpp"

#include <algorithm>
#include <string>

namespace t4a {

namespace {

// out[e] = (..(c[0] V[e, 0] + c[1] V[e, 1]) + ..) + c[nb-1] V[e, nb-1];  npart[g] = this workgroup's share of |out|^2
__global__ void __launch_bounds__(256) krylov_combine_kernel(const double* __restrict__ V, long long ld, int nb, const double* __restrict__ c,
                                                             double* __restrict__ out, long long len, double* __restrict__ npart)
{
    extern __shared__ double sc[];
    __shared__ double s4[4];
    const int tid = threadIdx.x;
    for (int i = tid; i < nb; i += GS_THREADS) sc[i] = c[i];
    __syncthreads();
    const long long first = (long long)blockIdx.x * GS_THREADS + tid, stride = (long long)gridDim.x * GS_THREADS;
    double acc = 0.0;
    for (long long e = first; e < len; e += stride) {
        double t = sc[0] * V[e];
        for (int i = 1; i < nb; ++i) t = t + sc[i] * V[e + ld * i];
        out[e] = t;
        acc = acc + t * t;
    }
    acc = block_sum(acc, s4);
    if (tid == 0) npart[blockIdx.x] = acc;
}

// r[e] = hv[e] - lambda v[e] (r may be null);  part[3 g + (0, 1, 2)] = this workgroup's shares of |r|^2, <v, hv>, <v, v>
__global__ void __launch_bounds__(256) eig_residual_kernel(const double* __restrict__ v, const double* __restrict__ hv, double lambda,
                                                           double* __restrict__ r, long long len, double* __restrict__ part)
{
    __shared__ double s12[3][4];
    const long long first = (long long)blockIdx.x * GS_THREADS + threadIdx.x, stride = (long long)gridDim.x * GS_THREADS;
    double rr = 0.0, vh = 0.0, vv = 0.0;
    for (long long e = first; e < len; e += stride) {
        const double a = v[e], b = hv[e];
        const double t = b - lambda * a;
        if (r) r[e] = t;
        rr = rr + t * t;
        vh = vh + a * b;
        vv = vv + a * a;
    }
    rr = wave_sum(rr);
    vh = wave_sum(vh);
    vv = wave_sum(vv);
    if ((threadIdx.x & 63) == 0) {
        const int wave = threadIdx.x >> 6;
        s12[0][wave] = rr;
        s12[1][wave] = vh;
        s12[2][wave] = vv;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double* s = s12[threadIdx.x];
        part[3 * (long long)blockIdx.x + threadIdx.x] = ((s[0] + s[1]) + s[2]) + s[3];
    }
}

// out[q] = sum_g part[q + nq g], g < n_part ascending, q < nq: one thread per sum
__global__ void __launch_bounds__(64) krylov_finish_kernel(const double* __restrict__ part, int n_part, int nq, double* __restrict__ out)
{
    const int q = threadIdx.x;
    if (q >= nq) return;
    double s = part[q];
    for (int g = 1; g < n_part; ++g) s = s + part[q + (long long)nq * g];
    out[q] = s;
}

} // namespace

void krylov_combine_launch(const double* V, size_t ld, int nb, const double* c, double* out, size_t len, double* npart, hipStream_t stream)
{
    if (nb <= 0 || len == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "krylov_combine: len and nb must be positive");
    hipLaunchKernelGGL(krylov_combine_kernel, dim3(gs_workgroups(len)), dim3(GS_THREADS), sizeof(double) * (size_t)nb, stream, V, (long long)ld, nb, c,
                       out, (long long)len, npart);
}

void eig_residual_launch(const double* v, const double* hv, double lambda, double* r, size_t len, double* part3, hipStream_t stream)
{
    if (len == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "eig_residual: len must be positive");
    hipLaunchKernelGGL(eig_residual_kernel, dim3(gs_workgroups(len)), dim3(GS_THREADS), 0, stream, v, hv, lambda, r, (long long)len, part3);
}

void krylov_finish_launch(const double* part, int n_part, int nq, double* out, hipStream_t stream)
{
    if (n_part <= 0 || nq <= 0 || nq > 64) throw Error(T4A_GPU_INVALID_ARGUMENT, "krylov_finish: n_part must be positive and nq in 1 .. 64");
    hipLaunchKernelGGL(krylov_finish_kernel, dim3(1), dim3(64), 0, stream, part, n_part, nq, out);
}

} // namespace t4a
