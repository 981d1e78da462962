// kernels_linsolve.hip — what a two-site linear solve (linsolve.hpp) spends outside its GEMMs:
//   * the half operators HL = L·A_i and HR = A_{i+1}·R of a bond step, written straight into the stacked layouts the projected
//     apply reads as plain matrices (one output element per thread, the operator bond summed ascending, stores along the fast index),
//   * the Gram–Schmidt launches of an Arnoldi step: all projections of a pass from one launch (gs_dots), the update of w with the
//     running Hessenberg column and the partial sums of |w|^2 (gs_update), the normalisation that reads its norm from device
//     memory (gs_normalize),
//   * the affine residual b - (a0 x + a1 A x) and a scaled copy.
// Every reduction has a fixed partition that depends on the vector length alone: thread t of workgroup g owns the elements
// g*256 + t + k*(256*G), summed k-ascending; lanes are folded by a fixed shuffle tree, the four waves and then the workgroups in
// ascending order.  No atomics; multiply and add are rounded separately (-ffp-contract=off): two runs give the same bits.
#include "krylov_reduce.hpp"
#include "linsolve.hpp"

#include <algorithm>

namespace t4a {

namespace {

constexpr int GS_PER_THREAD = 4;  // elements per thread the grid is sized for
constexpr int GS_BATCH = 32;      // basis vectors per barrier of gs_dots

// HL[(beta + chi s1) + M wm, (alpha + chi t1)] = sum_wl L[beta, wl, alpha] A[wl, s1, t1, wm],  M = chi d, leading dimension W M
__global__ void __launch_bounds__(256) linsolve_hl_kernel(const double* __restrict__ L, const double* __restrict__ A, double* __restrict__ HL,
                                                          int chi, int Wl, int d, int W)
{
    const long long M = (long long)chi * d, rows = M * W, total = rows * M;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long r = e % rows, c = e / rows;
        const int beta = (int)(r % chi), s1 = (int)((r / chi) % d), wm = (int)(r / M);
        const int alpha = (int)(c % chi), t1 = (int)(c / chi);
        const double* l = L + beta + (long long)chi * Wl * alpha;
        const double* a = A + (long long)Wl * (s1 + (long long)d * (t1 + (long long)d * wm));
        double acc = 0.0;
        for (int wl = 0; wl < Wl; ++wl) acc = acc + l[(long long)chi * wl] * a[wl];
        HL[e] = acc;
    }
}

// HR[wm + W (t2 + d alpha), (s2 + d beta)] = sum_wr A[wm, s2, t2, wr] R[beta, wr, alpha],  N = d chi, leading dimension W N
__global__ void __launch_bounds__(256) linsolve_hr_kernel(const double* __restrict__ A, const double* __restrict__ R, double* __restrict__ HR,
                                                          int chi, int W, int d, int Wr)
{
    const long long N = (long long)chi * d, rows = N * W, total = rows * N;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long r = e % rows, c = e / rows;
        const int wm = (int)(r % W), t2 = (int)((r / W) % d), alpha = (int)(r / ((long long)W * d));
        const int s2 = (int)(c % d), beta = (int)(c / d);
        const double* a = A + wm + (long long)W * (s2 + (long long)d * t2);
        const double* rr = R + beta + (long long)chi * Wr * alpha;
        const long long sa = (long long)W * d * d;
        double acc = 0.0;
        for (int wr = 0; wr < Wr; ++wr) acc = acc + a[sa * wr] * rr[(long long)chi * wr];
        HR[e] = acc;
    }
}

// part[i + nb g] = sum over the elements of workgroup g of V[e + ld i] w[e], i < nb
__global__ void __launch_bounds__(256) gs_dots_kernel(const double* __restrict__ V, long long ld, int nb, const double* __restrict__ w, long long len,
                                                      double* __restrict__ part)
{
    __shared__ double sred[4][GS_BATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long first = (long long)blockIdx.x * GS_THREADS + tid, stride = (long long)gridDim.x * GS_THREADS;
    for (int i0 = 0; i0 < nb; i0 += GS_BATCH) {
        const int nbb = min(GS_BATCH, nb - i0);
        for (int ii = 0; ii < nbb; ++ii) {
            const double* v = V + ld * (i0 + ii);
            double acc = 0.0;
            for (long long e = first; e < len; e += stride) acc = acc + v[e] * w[e];
            acc = wave_sum(acc);
            if (lane == 0) sred[wave][ii] = acc;
        }
        __syncthreads();
        if (tid < nbb) part[(i0 + tid) + (long long)nb * blockIdx.x] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
        __syncthreads();
    }
}

// c[i] = sum_g part[i + nb g] (g ascending, every workgroup forms the same values);  w[e] <- (..(w[e] - c[0] V[e, 0]) - ..) - c[nb-1] V[e, nb-1];
// npart[g] = this workgroup's share of |w|^2.  Workgroup 0 also keeps the books: hcol[i] = c[i] (first pass) or hcol[i] + c[i], hpass[i] = c[i].
__global__ void __launch_bounds__(256) gs_update_kernel(const double* __restrict__ V, long long ld, int nb, double* __restrict__ w, long long len,
                                                        const double* __restrict__ part, int n_part, double* __restrict__ hcol, int first_pass,
                                                        double* __restrict__ hpass, double* __restrict__ npart)
{
    extern __shared__ double sc[];
    __shared__ double s4[4];
    const int tid = threadIdx.x;
    for (int i = tid; i < nb; i += GS_THREADS) {
        double c = part[i];
        for (int g = 1; g < n_part; ++g) c = c + part[i + (long long)nb * g];
        sc[i] = c;
        if (blockIdx.x == 0) {
            if (hcol) hcol[i] = first_pass ? c : hcol[i] + c;
            if (hpass) hpass[i] = c;
        }
    }
    __syncthreads();
    const long long first = (long long)blockIdx.x * GS_THREADS + tid, stride = (long long)gridDim.x * GS_THREADS;
    double acc = 0.0;
    for (long long e = first; e < len; e += stride) {
        double t = w[e];
        for (int i = 0; i < nb; ++i) t = t - sc[i] * V[e + ld * i];
        w[e] = t;
        acc = acc + t * t;
    }
    acc = block_sum(acc, s4);
    if (tid == 0) npart[blockIdx.x] = acc;
}

// npart[g] = this workgroup's share of |w|^2
__global__ void __launch_bounds__(256) gs_norm2_kernel(const double* __restrict__ w, long long len, double* __restrict__ npart)
{
    __shared__ double s4[4];
    const long long first = (long long)blockIdx.x * GS_THREADS + threadIdx.x, stride = (long long)gridDim.x * GS_THREADS;
    double acc = 0.0;
    for (long long e = first; e < len; e += stride) acc = acc + w[e] * w[e];
    acc = block_sum(acc, s4);
    if (threadIdx.x == 0) npart[blockIdx.x] = acc;
}

// nrm = sqrt(sum_g npart[g]) (g ascending, every workgroup alike); out[e] = w[e] * (1 / nrm) unless out is null; *norm_out = nrm
__global__ void __launch_bounds__(256) gs_normalize_kernel(const double* w, long long len, const double* __restrict__ npart, int n_part, double* out,
                                                           double* __restrict__ norm_out)
{
    __shared__ double s_inv;
    if (threadIdx.x == 0) {
        double s = npart[0];
        for (int g = 1; g < n_part; ++g) s = s + npart[g];
        const double nrm = sqrt(s);
        s_inv = 1.0 / nrm;
        if (blockIdx.x == 0 && norm_out) *norm_out = nrm;
    }
    __syncthreads();
    if (!out) return;
    const double inv = s_inv;
    const long long first = (long long)blockIdx.x * GS_THREADS + threadIdx.x, stride = (long long)gridDim.x * GS_THREADS;
    for (long long e = first; e < len; e += stride) out[e] = w[e] * inv;
}

// r[e] = b[e] - (a0 x[e] + a1 ax[e]);  npart[g] = this workgroup's share of |r|^2
__global__ void __launch_bounds__(256) linsolve_residual_kernel(const double* __restrict__ b, const double* __restrict__ x, const double* __restrict__ ax,
                                                                double a0, double a1, double* __restrict__ r, long long len, double* __restrict__ npart)
{
    __shared__ double s4[4];
    const long long first = (long long)blockIdx.x * GS_THREADS + threadIdx.x, stride = (long long)gridDim.x * GS_THREADS;
    double acc = 0.0;
    for (long long e = first; e < len; e += stride) {
        const double aff = a0 * x[e] + a1 * ax[e];
        const double t = b[e] - aff;
        r[e] = t;
        acc = acc + t * t;
    }
    acc = block_sum(acc, s4);
    if (threadIdx.x == 0) npart[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256) linsolve_scale_kernel(const double* __restrict__ in, double alpha, double* __restrict__ out, long long len)
{
    const long long stride = (long long)gridDim.x * GS_THREADS;
    for (long long e = (long long)blockIdx.x * GS_THREADS + threadIdx.x; e < len; e += stride) out[e] = in[e] * alpha;
}

unsigned builder_blocks(long long total) { return (unsigned)std::min<long long>((total + 255) / 256, 8192); }

} // namespace

int gs_workgroups(size_t len)
{
    const size_t per = (size_t)GS_THREADS * GS_PER_THREAD;
    return (int)std::max<size_t>(1, std::min<size_t>((len + per - 1) / per, GS_MAX_WORKGROUPS));
}

void linsolve_hl_launch(const double* L, const double* A, double* HL, int chi, int Wl, int d, int W, hipStream_t stream)
{
    const long long total = (long long)chi * d * W * chi * d;
    if (total <= 0) return;
    hipLaunchKernelGGL(linsolve_hl_kernel, dim3(builder_blocks(total)), dim3(256), 0, stream, L, A, HL, chi, Wl, d, W);
}

void linsolve_hr_launch(const double* A, const double* R, double* HR, int chi, int W, int d, int Wr, hipStream_t stream)
{
    const long long total = (long long)chi * d * W * chi * d;
    if (total <= 0) return;
    hipLaunchKernelGGL(linsolve_hr_kernel, dim3(builder_blocks(total)), dim3(256), 0, stream, A, R, HR, chi, W, d, Wr);
}

void gs_dots_launch(const double* V, size_t ld, int nb, const double* w, size_t len, double* part, hipStream_t stream)
{
    if (nb <= 0 || len == 0) return;
    hipLaunchKernelGGL(gs_dots_kernel, dim3(gs_workgroups(len)), dim3(GS_THREADS), 0, stream, V, (long long)ld, nb, w, (long long)len, part);
}

void gs_update_launch(const double* V, size_t ld, int nb, double* w, size_t len, const double* part, int n_part, double* hcol, bool first_pass,
                      double* hpass, double* npart, hipStream_t stream)
{
    if (len == 0) return;
    hipLaunchKernelGGL(gs_update_kernel, dim3(gs_workgroups(len)), dim3(GS_THREADS), sizeof(double) * (size_t)std::max(nb, 0), stream, V, (long long)ld,
                       nb, w, (long long)len, part, n_part, hcol, first_pass ? 1 : 0, hpass, npart);
}

void gs_norm2_launch(const double* w, size_t len, double* npart, hipStream_t stream)
{
    if (len == 0) return;
    hipLaunchKernelGGL(gs_norm2_kernel, dim3(gs_workgroups(len)), dim3(GS_THREADS), 0, stream, w, (long long)len, npart);
}

void gs_normalize_launch(const double* w, size_t len, const double* npart, double* out, double* norm_out, hipStream_t stream)
{
    if (len == 0) return;
    const int g = gs_workgroups(len);
    hipLaunchKernelGGL(gs_normalize_kernel, dim3(out ? g : 1), dim3(GS_THREADS), 0, stream, w, (long long)len, npart, g, out, norm_out);
}

void linsolve_residual_launch(const double* b, const double* x, const double* ax, double a0, double a1, double* r, size_t len, double* npart,
                              hipStream_t stream)
{
    if (len == 0) return;
    hipLaunchKernelGGL(linsolve_residual_kernel, dim3(gs_workgroups(len)), dim3(GS_THREADS), 0, stream, b, x, ax, a0, a1, r, (long long)len, npart);
}

void linsolve_scale_launch(const double* in, double alpha, double* out, size_t len, hipStream_t stream)
{
    if (len == 0) return;
    hipLaunchKernelGGL(linsolve_scale_kernel, dim3(gs_workgroups(len)), dim3(GS_THREADS), 0, stream, in, alpha, out, (long long)len);
}

} // namespace t4a
