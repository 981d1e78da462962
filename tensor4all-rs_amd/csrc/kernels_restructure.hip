// kernels_restructure.hip — one round of fuse_to (restructure.hpp) for every group of a chain at once.
//
// fuse_round_kernel: per job the accumulated core A[l, x, m] of a group and its next member B[m, y, r] are contracted over their
// bond and written as the core of the fused site index,
//   out[l_idx + l (f + X Y r_idx)] = sum_m A[l_idx, x, m] B[m, y, r_idx],
// where f is x + X y read through the job's leg table: leg k (chain order, first fastest) is the digit (x + X y) / prod_{k' < k} dim[k']
// % dim[k] and contributes digit * dst[k].  A table of no legs is the chain order itself (f = x + X y): the intermediate rounds of a
// group, and a last round whose target order is the chain order.  The legs of a group's last round land in the target's order; there
// is no permutation launch.
// The jobs of a round are a ragged table in device memory (FuseRoundJob, kernels.hpp): job k owns the work items off[k] .. off[k + 1]
// and a wavefront finds its job by binary search, as leg_reorder_kernel does per element.  Inside a job a work item is one pair
// (x, y) and one 16 x 16 tile of (l, r), tile row fastest, then tile column, then the pair — exactly the items of swap_theta_kernel
// (kernels_swap.hip), and the arithmetic is that kernel's statement by statement: a tile inside l x r runs on the f64 matrix cores
// (v_mfma_f64_16x16x4_f64), m in ascending chunks of four, the last chunk padded with zeros; an edge tile, and every tile when l or r
// is below 16, is four elements per lane with m ascending and multiply and add rounded separately.  The route of an element depends
// on (l, r) of its job and its position alone: no sum is split over wavefronts, nothing is added atomically, two runs give the same
// bits, and the bits of a job do not depend on the other jobs of the launch.  On one job with the chain order the output is bit for
// bit what swap_theta_kernel writes with every leg sent to the left side.
#include "kernels.hpp"

#include <climits>

namespace t4a {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int FR_T = 16;    // tile edge in l and in r
constexpr int FR_WAVES = 4; // wavefronts (work items) per workgroup
constexpr int FR_UA = 4;    // chunks of four values of m whose loads issue together

__global__ void __launch_bounds__(64 * FR_WAVES) fuse_round_kernel(const FuseRoundJob* __restrict__ jobs, int n_jobs, unsigned long long n_items)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // uniform: the job is read with scalar loads
    const unsigned long long item = (unsigned long long)blockIdx.x * FR_WAVES + wave;
    if (item >= n_items) return; // no barrier below: a wavefront may leave alone
    int lo = 0, hi = n_jobs - 1; // the last job with off <= item (offsets ascend, jobs[0].off == 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].off <= item) lo = mid;
        else hi = mid - 1;
    }
    const FuseRoundJob& j = jobs[lo];
    const int l = j.l, X = j.X, m = j.m, Y = j.Y, r = j.r;
    const unsigned long long q = item - j.off;
    const int nlt = (l + FR_T - 1) / FR_T, nrt = (r + FR_T - 1) / FR_T;
    const int lt = (int)(q % (unsigned)nlt);
    const unsigned long long rest = q / (unsigned)nlt;
    const int rt = (int)(rest % (unsigned)nrt);
    const int pair = (int)(rest / (unsigned)nrt); // < X * Y <= 65535 (host)
    const int x = pair % X, y = pair / X;
    int f = pair;
    if (j.n_legs > 0) {
        f = 0;
        int p = pair;
        for (int k = 0; k < j.n_legs; ++k) {
            f += (p % j.dim[k]) * j.dst[k];
            p /= j.dim[k];
        }
    }
    const int l0 = lt * FR_T, r0 = rt * FR_T;
    const int lr = lane & 15, lk = lane >> 4;
    // A[l_idx + l (x + X mi)], B[mi + m (y + Y r_idx)]
    const double* a = j.A + (long long)l * x;
    const long long a_m = (long long)l * X;
    const double* b = j.B + (long long)m * y;
    const long long b_r = (long long)m * Y;
    double* o = j.out + (long long)l * f;
    const long long o_r = (long long)l * X * Y;

    if (l0 + FR_T <= l && r0 + FR_T <= r) {
        // operand roles as in swap_theta_kernel: acc[reg] = C[l0 + (lane & 15)][r0 + (lane >> 4) + 4 reg]
        double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
        const double* ap = a + (l0 + lr);
        const double* bp = b + b_r * (r0 + lr);
        for (int m0 = 0; m0 < m; m0 += 4 * FR_UA) {
            double pv[FR_UA], qv[FR_UA];
#pragma unroll
            for (int u = 0; u < FR_UA; ++u) {
                const int mi = m0 + 4 * u + lk;
                const bool ok = mi < m;
                pv[u] = ok ? ap[a_m * mi] : 0.0;
                qv[u] = ok ? bp[mi] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < FR_UA; ++u)
                if (m0 + 4 * u < m) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[u], pv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o[(l0 + lr) + o_r * (r0 + lk + 4 * reg)] = acc[reg];
        return;
    }
    // edge tile / small bond: element (l0 + lr, r0 + lk + 4 reg) per lane and reg
    const int li = l0 + lr;
    if (li >= l) return;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int ri = r0 + lk + 4 * reg;
        if (ri >= r) continue;
        const double* ap = a + li;
        const double* bp = b + b_r * ri;
        double v = 0.0;
        for (int mi = 0; mi < m; ++mi) {
            const double prod = ap[a_m * mi] * bp[mi];
            v = v + prod;
        }
        o[li + o_r * ri] = v;
    }
}

} // namespace

int fuse_round_route(int l, int r)
{
    int route = 0;
    if (l >= FR_T && r >= FR_T) route |= FUSE_ROUTE_MFMA;
    if (l % FR_T != 0 || r % FR_T != 0) route |= FUSE_ROUTE_SCALAR;
    return route;
}

unsigned long long fuse_round_items(int l, int X, int Y, int r)
{
    if (l <= 0 || X <= 0 || Y <= 0 || r <= 0) return 0;
    const unsigned long long nlt = (l + FR_T - 1) / FR_T, nrt = (r + FR_T - 1) / FR_T;
    return nlt * nrt * (unsigned long long)X * (unsigned long long)Y;
}

bool fuse_round_launch(const FuseRoundJob* d_jobs, int n_jobs, unsigned long long n_items, hipStream_t stream)
{
    if (n_jobs <= 0 || n_items == 0) return true; // nothing to write
    const unsigned long long blocks = (n_items + FR_WAVES - 1) / FR_WAVES;
    if (blocks > INT_MAX) return false;
    hipLaunchKernelGGL(fuse_round_kernel, dim3((unsigned)blocks), dim3(64 * FR_WAVES), 0, stream, d_jobs, n_jobs, n_items);
    return true;
}

} // namespace t4a
