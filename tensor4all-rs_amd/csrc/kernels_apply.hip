// kernels_apply.hip — the local products of an operator applied to a state on a subset of its sites (linop.hpp).  A state site the
// operator does not act on (a gap site) carries the operator bond through unchanged: the identity delta_{aa'} delta_{yx} it stands for
// is never formed and never multiplied.
//
// 1. apply_site_kernel: every site of the chain in ONE launch, ragged like mpo_site_contract_kernel (kernels_mpo.hip), one output
//    element per thread.  At an operator site x ascends, multiply and add are rounded separately (the file is built with
//    -ffp-contract=off) and the sum starts from 0.0: the chain of operations of mpo_site_contract_kernel with t = 1, so with full
//    coverage the bits are its bits.  At a gap site an element is a copy of the state's (a == a') or 0.0.
//
// 2. apply_gap_half_kernel: the half product of a gap site for zip-up and fit,
//      left   P[n, x, a, d] = sum_b E[n, a, b] X[b, x, d]        right   Q[a, b, x, n] = sum_d X[b, x, d] E[a, d, n]
//    one kernel, the mirrors selected through strides: out[n, x, a, c] = sum_k E[n, a, k] X[k, x, c].  A workgroup owns one (a, x),
//    16 values of n and 64 of c, a wavefront one 16 x 16 tile of that strip.  A tile that lies inside the matrix (which needs both
//    output bonds from 16 up) runs on the f64 matrix cores (v_mfma_f64_16x16x4_f64), the summed index in chunks of four, ascending, the
//    last chunk zero-padded in registers; operand roles as in kernels_fit_sum.hip: first operand indexed by the output column, second
//    by the output row, acc[reg] = out[row = lane & 15][col = (lane >> 4) + 4 reg].  A ragged or small tile is one element per thread
//    (four per lane) with the summed index ascending, multiply and add rounded separately.  No summed index is split across
//    workgroups and nothing is added atomically: two runs give the same bits.  The output is written once, in the layout the SVD
//    (zip-up) or the Theta GEMM (fit) behind it reads; nothing is permuted before or after the launch.  An Outside site is M == 1.
//    First version, not tuned: a lane loads its operand element straight from global memory.
#include "linop.hpp"

#include <algorithm>
#include <climits>

namespace t4a {

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

__global__ void __launch_bounds__(256) apply_site_kernel(const ApplySiteJob* __restrict__ jobs, int n_jobs, unsigned long long total)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        // the site whose output range holds e: the last job with off <= e (offsets ascend, jobs[0].off == 0)
        int lo = 0, hi = n_jobs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].off <= e) lo = mid;
            else hi = mid - 1;
        }
        const ApplySiteJob& j = jobs[lo];
        // every site's input and output holds at most INT_MAX elements (checked on the host)
        int q = (int)(e - j.off);
        const int Lc = j.ml * j.lb;
        const int row = q % Lc;
        q /= Lc;
        const int s = q % j.s1;
        const int col = q / j.s1;
        const int ia = row / j.lb, ib = row % j.lb;
        const int ra = col / j.rb, rb = col % j.rb;
        double acc = 0.0;
        if (j.gap) {
            // X[ib, s, rb] at ib + Lb (s + K rb)
            if (ia == ra) acc = j.X[ib + j.lb * (s + j.k * rb)];
        } else {
            // O[ia, s, x, ra] at ia + Ml (s + S1 (x + K ra)); X[ib, x, rb] at ib + Lb (x + K rb)
            const double* o = j.O + ia + j.ml * (s + j.s1 * j.k * ra);
            const double* x = j.X + ib + j.lb * j.k * rb;
            const int so = j.ml * j.s1, sx = j.lb;
            for (int k = 0; k < j.k; ++k) acc = acc + o[so * k] * x[sx * k];
        }
        j.Y[e - j.off] = acc;
    }
}

constexpr int GH_THREADS = 256; // four wavefronts, one 16 x 16 tile each
constexpr int GH_TN = 16;       // values of n per workgroup
constexpr int GH_TC = 64;       // values of c per workgroup

__global__ void __launch_bounds__(GH_THREADS) apply_gap_half_kernel(const ApplyGapHalfDesc d)
{
    // workgroup -> (n tile, c strip, a, x), n fastest
    const int nt = (d.N + GH_TN - 1) / GH_TN, ct = (d.C + GH_TC - 1) / GH_TC;
    unsigned blk = blockIdx.x;
    const int in = (int)(blk % (unsigned)nt);
    blk /= (unsigned)nt;
    const int ic = (int)(blk % (unsigned)ct);
    blk /= (unsigned)ct;
    const int a = (int)(blk % (unsigned)d.M);
    const int x = (int)(blk / (unsigned)d.M);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = in * GH_TN, c0 = ic * GH_TC + 16 * wave;
    if (c0 >= d.C) return; // a wavefront past the last column tile of the strip
    const double* E = d.E + (long long)a * d.ea;
    const double* X = d.X + (long long)x * d.xx;
    double* out = d.out + (long long)a * d.oa + (long long)x * d.ox;
    if (n0 + 16 <= d.N && c0 + 16 <= d.C) {
        const int lr = lane & 15, lk = lane >> 4;
        const double* ep = E + (long long)(n0 + lr) * d.en;
        const double* xp = X + (long long)(c0 + lr) * d.xc;
        double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < d.K; k0 += 4) {
            const int k = k0 + lk;
            const bool k_ok = k < d.K;
            const double ev = k_ok ? ep[(long long)k * d.ek] : 0.0;
            const double xv = k_ok ? xp[(long long)k * d.xk] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, ev, acc, 0, 0, 0);
        }
        double* op = out + (long long)(n0 + lr) * d.on;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) op[(long long)(c0 + lk + 4 * reg) * d.oc] = acc[reg];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = lane + 64 * q;
            const int n = n0 + (e & 15), c = c0 + (e >> 4);
            if (n < d.N && c < d.C) {
                const double* ep = E + (long long)n * d.en;
                const double* xp = X + (long long)c * d.xc;
                double v = 0.0;
                for (int k = 0; k < d.K; ++k) {
                    const double prod = ep[(long long)k * d.ek] * xp[(long long)k * d.xk];
                    v = v + prod;
                }
                out[(long long)n * d.on + (long long)c * d.oc] = v;
            }
        }
    }
}

} // namespace

void apply_site_launch(const ApplySiteJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream)
{
    if (n_jobs <= 0 || total == 0) return;
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(apply_site_kernel, dim3(blocks), dim3(256), 0, stream, d_jobs, n_jobs, total);
}

bool apply_gap_half_launch(const ApplyGapHalfDesc& d, hipStream_t stream)
{
    if (d.N <= 0 || d.M <= 0 || d.S <= 0 || d.K <= 0 || d.C <= 0) return true; // nothing to write
    const unsigned long long nt = (d.N + GH_TN - 1) / GH_TN, ct = (d.C + GH_TC - 1) / GH_TC;
    // never more workgroups than output elements, which the host bounds by INT_MAX; the products are formed so that none can wrap
    if (nt * ct > INT_MAX || (unsigned long long)d.M * (unsigned long long)d.S > INT_MAX) return false;
    const unsigned long long blocks = nt * ct * (unsigned long long)d.M * (unsigned long long)d.S;
    if (blocks > INT_MAX) return false;
    hipLaunchKernelGGL(apply_gap_half_kernel, dim3((unsigned)blocks), dim3(GH_THREADS), 0, stream, d);
    return true;
}

} // namespace t4a
