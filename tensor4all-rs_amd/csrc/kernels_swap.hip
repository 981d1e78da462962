// kernels_swap.hip — the step of swap_site_indices (swap.hpp) and the leg reordering of a leg train.
//
// 1. swap_theta_kernel: two neighbouring cores A[l, x, m] and B[m, y, r] of a chain, in chain order, are contracted over their bond
//    and the result is written with the site legs of the pair redistributed between the two sides, as the column-major matrix the
//    SVD of the step reads:
//      out[(l_idx + l xa) + M (xb + Cb r_idx)] = sum_m A[l_idx, x, m] B[m, y, r_idx],   M = l Ra,  N = Cb r,
//    where (x, y) <-> (xa, xb) is the redistribution: every leg of the pair is one digit of x or of y and one digit of xa or of xb
//    (SwapThetaDesc, kernels.hpp; at most SWAP_MAX_LEGS legs, the table travels in the launch descriptor).  There is no
//    intermediate two-site tensor and no permutation launch.
//    For a fixed pair (x, y) this is an l x r product over m.  A wavefront owns one pair and one 16 x 16 tile of (l, r); a workgroup
//    is four wavefronts with consecutive work items (tile row fastest, then tile column, then the pair), so its wavefronts share
//    the pair, or neighbouring ones, and read the same panels of A and B.  A tile that lies inside l x r runs on the f64 matrix
//    cores (v_mfma_f64_16x16x4_f64), m in chunks of four ascending, the last chunk padded with zeros; the operands of four chunks
//    are loaded before their four matrix-core steps issue, as in mpo_partial_half_kernel.  An edge tile, and every tile of a bond
//    below 16, is four elements per lane with m ascending and multiply and add rounded separately.  Which route an element takes
//    depends on (l, r) and its position alone, the order of its sum on nothing else: no sum is split over wavefronts, nothing is
//    added atomically, two runs give the same bits.  Lanes of a wavefront write 16 consecutive rows of `out`.
//    The kernel always sees the left core first; a left-moving step differs only in which factor of the SVD keeps S.
//
// 2. leg_reorder_kernel: the legs of the fused site index of every named site in a new order, one launch for all of them, one
//    element per thread (ragged job list searched as in mpo_partial_site_kernel).
#include "kernels.hpp"

#include <algorithm>
#include <climits>

namespace t4a {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int SW_T = 16;        // tile edge in l and in r
constexpr int SW_WAVES = 4;     // wavefronts (work items) per workgroup
constexpr int SW_UA = 4;        // chunks of four values of m whose loads issue together

__global__ void __launch_bounds__(64 * SW_WAVES) swap_theta_kernel(const SwapThetaDesc d, unsigned long long n_items)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long item = (unsigned long long)blockIdx.x * SW_WAVES + wave;
    if (item >= n_items) return; // no barrier below: a wavefront may leave alone
    const int nlt = (d.l + SW_T - 1) / SW_T, nrt = (d.r + SW_T - 1) / SW_T;
    const int lt = (int)(item % (unsigned)nlt);
    const unsigned long long rest = item / (unsigned)nlt;
    const int rt = (int)(rest % (unsigned)nrt);
    const int pair = (int)(rest / (unsigned)nrt); // < X * Y <= INT_MAX (host)
    const int x = pair % d.X, y = pair / d.X;
    int xa = 0, xb = 0;
    for (int j = 0; j < d.n_legs; ++j) {
        const int digit = ((d.from_right[j] ? y : x) / d.src[j]) % d.dim[j];
        if (d.to_col[j]) xb += digit * d.dst[j];
        else xa += digit * d.dst[j];
    }
    const int l0 = lt * SW_T, r0 = rt * SW_T;
    const int lr = lane & 15, lk = lane >> 4;
    const long long M = (long long)d.l * d.Ra;
    // A[l_idx + l (x + X mi)], B[mi + m (y + Y r_idx)]
    const double* a = d.A + (long long)d.l * x;
    const long long a_m = (long long)d.l * d.X;
    const double* b = d.B + (long long)d.m * y;
    const long long b_r = (long long)d.m * d.Y;
    double* o = d.out + (long long)d.l * xa + M * xb;
    const long long o_r = M * d.Cb;

    if (l0 + SW_T <= d.l && r0 + SW_T <= d.r) {
        // first operand indexed by the row of the result it makes (r = lane & 15), second by the column (l = lane & 15), both at the
        // summed index lane >> 4; acc[reg] = C[l0 + (lane & 15)][r0 + (lane >> 4) + 4 reg]  (operand roles as in kernels_partial.hip)
        double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
        const double* ap = a + (l0 + lr);
        const double* bp = b + b_r * (r0 + lr);
        for (int m0 = 0; m0 < d.m; m0 += 4 * SW_UA) {
            double pv[SW_UA], qv[SW_UA];
#pragma unroll
            for (int u = 0; u < SW_UA; ++u) {
                const int mi = m0 + 4 * u + lk;
                const bool ok = mi < d.m;
                pv[u] = ok ? ap[a_m * mi] : 0.0;
                qv[u] = ok ? bp[mi] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < SW_UA; ++u)
                if (m0 + 4 * u < d.m) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[u], pv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o[(l0 + lr) + o_r * (r0 + lk + 4 * reg)] = acc[reg];
        return;
    }
    // edge tile / small bond: element (l0 + lr, r0 + lk + 4 reg) per lane and reg
    const int li = l0 + lr;
    if (li >= d.l) return;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int ri = r0 + lk + 4 * reg;
        if (ri >= d.r) continue;
        const double* ap = a + li;
        const double* bp = b + b_r * ri;
        double v = 0.0;
        for (int mi = 0; mi < d.m; ++mi) {
            const double prod = ap[a_m * mi] * bp[mi];
            v = v + prod;
        }
        o[li + o_r * ri] = v;
    }
}

__global__ void __launch_bounds__(256) leg_reorder_kernel(const LegReorderJob* __restrict__ jobs, int n_jobs, unsigned long long total)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        int lo = 0, hi = n_jobs - 1; // the last job with off <= e (offsets ascend, jobs[0].off == 0)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].off <= e) lo = mid;
            else hi = mid - 1;
        }
        const LegReorderJob& j = jobs[lo];
        int q = (int)(e - j.off); // a site holds at most INT_MAX elements (host)
        const int li = q % j.l;
        q /= j.l;
        int s = q % j.s;
        const int ri = q / j.s;
        int f = 0;
        for (int k = 0; k < j.n_legs; ++k) {
            f += (s % j.dim[k]) * j.stride[k];
            s /= j.dim[k];
        }
        j.dst[e - j.off] = j.src[li + (long long)j.l * (f + (long long)j.s * ri)];
    }
}

} // namespace

int swap_theta_route(int l, int r)
{
    int route = 0;
    if (l >= SW_T && r >= SW_T) route |= SWAP_ROUTE_MFMA;
    if (l % SW_T != 0 || r % SW_T != 0) route |= SWAP_ROUTE_SCALAR;
    return route;
}

bool swap_theta_launch(const SwapThetaDesc& d, hipStream_t stream)
{
    if (d.l <= 0 || d.X <= 0 || d.m <= 0 || d.Y <= 0 || d.r <= 0) return true; // nothing to write
    const unsigned long long nlt = (d.l + SW_T - 1) / SW_T, nrt = (d.r + SW_T - 1) / SW_T;
    const unsigned long long items = nlt * nrt * (unsigned long long)d.X * (unsigned long long)d.Y;
    const unsigned long long blocks = (items + SW_WAVES - 1) / SW_WAVES;
    if (blocks > INT_MAX) return false;
    hipLaunchKernelGGL(swap_theta_kernel, dim3((unsigned)blocks), dim3(64 * SW_WAVES), 0, stream, d, items);
    return true;
}

void leg_reorder_launch(const LegReorderJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream)
{
    if (n_jobs <= 0 || total == 0) return;
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(leg_reorder_kernel, dim3(blocks), dim3(256), 0, stream, d_jobs, n_jobs, total);
}

} // namespace t4a
