// kernels_pmpo.hip — the launches of a partitioned MPO (tensor4all-partitionedtt/src/subdomain_tt.rs:171-443 project / contract,
// partitioned_tt.rs:305-340 contract): the projection of every site of every patch, and the site products of every task of a
// patch-wise contraction with the projection of both operands folded in,
//   C[(la*Lb+lb), s, t, (ra*Rb+rb)] = [s in s-mask][t in t-mask] sum_{k0 <= k < k1} A[la, s, k, ra] * B[lb, k, t, rb].
// The third launch is the direct sum of all patches of to_mpo (partitioned_tt.rs:460-480): every site of the result in one launch.
// Like kernels_mpo.hip each thread forms one output element as a k-ascending sum with separately rounded multiply and add (built with
// -ffp-contract=off): on finite operands the bits are those of mpo_site_contract_kernel applied to operands that were masked
// beforehand, because the products it adds outside [k0, k1) are +-0.0 and leave a sum that starts at +0.0 unchanged.  No atomics,
// int indexing inside a site (the host checks every site against INT_MAX).  Site tensors are column-major [left, s1, s2, right].
#include "kernels.hpp"

#include <algorithm>

namespace t4a {

namespace {

// the job whose range holds e: the last one with off <= e (offsets ascend, jobs[0].off == 0)
template <class Job> __device__ __forceinline__ int find_job(const Job* __restrict__ jobs, int n_jobs, unsigned long long e)
{
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].off <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) pmpo_mask_kernel(const PmpoMaskJob* __restrict__ jobs, int n_jobs, unsigned long long total)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const PmpoMaskJob& j = jobs[find_job(jobs, n_jobs, e)];
        const int q = (int)(e - j.off) / j.l;
        const int s1 = q % j.s1, s2 = (q / j.s1) % j.s2;
        // a store of zero, never a product: a non-finite value outside the subdomain disappears (mask_index)
        if ((j.m1 >= 0 && s1 != j.m1) || (j.m2 >= 0 && s2 != j.m2)) j.X[e - j.off] = 0.0;
    }
}

__global__ void __launch_bounds__(256) pmpo_pair_contract_kernel(const PmpoPairJob* __restrict__ jobs, int n_jobs, unsigned long long total)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const PmpoPairJob& j = jobs[find_job(jobs, n_jobs, e)];
        int q = (int)(e - j.off);
        const int Lc = j.la * j.lb;
        const int row = q % Lc;
        q /= Lc;
        const int s = q % j.s1;
        q /= j.s1;
        const int t = q % j.t;
        const int col = q / j.t;
        double acc = 0.0;
        if ((j.sm < 0 || s == j.sm) && (j.tm < 0 || t == j.tm)) {
            const int ia = row / j.lb, ib = row % j.lb;
            const int ra = col / j.rb, rb = col % j.rb;
            // A[ia, s, k, ra] at ia + La (s + S1 (k + K ra)); B[ib, k, t, rb] at ib + Lb (k + K (t + T rb))
            const double* a = j.A + ia + j.la * (s + j.s1 * j.k * ra);
            const double* b = j.B + ib + j.lb * j.k * (t + j.t * rb);
            const int sa = j.la * j.s1, sb = j.lb;
            for (int k = j.k0; k < j.k1; ++k) acc = acc + a[sa * k] * b[sb * k];
        }
        j.C[e - j.off] = acc;
    }
}

// the patch whose range [o[g], o[g + 1]) holds x (offsets strictly ascend, o[0] == 0, x < o[G])
__device__ __forceinline__ int find_patch(const int* __restrict__ o, int G, int x)
{
    int lo = 0, hi = G - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (o[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) pmpo_direct_sum_kernel(const PmpoSumJob* __restrict__ jobs, int n_jobs, unsigned long long total)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const PmpoSumJob& j = jobs[find_job(jobs, n_jobs, e)];
        int q = (int)(e - j.off);
        const int row = q % j.L;
        q /= j.L;
        const int s = q % j.S;
        const int col = q / j.S;
        // the block is found by its rows, at the first site (one row for every patch) by its columns
        const int g = j.first ? find_patch(j.col0, j.G, col) : find_patch(j.row0, j.G, row);
        const int r0 = j.first ? 0 : j.row0[g], lg = j.first ? 1 : j.row0[g + 1] - r0;
        const int c0 = j.last ? 0 : j.col0[g], c1 = j.last ? 1 : j.col0[g + 1];
        double v = 0.0;
        if (col >= c0 && col < c1) v = j.src[g][(row - r0) + lg * (s + j.S * (col - c0))];
        j.dst[e - j.off] = v;
    }
}

} // namespace

// One resident pass of the chip: 256 CUs x 8 blocks of four waves (32 waves per CU, which both kernels reach with their fewer than 64
// VGPRs); larger totals go round the grid-stride loop.  The output is written once and the operands of a patch are a few KiB that stay
// in L2, so there is nothing a smaller grid would save.
unsigned pmpo_launch_blocks(unsigned long long total) { return (unsigned)std::min<unsigned long long>((total + 255) / 256, 2048); }

void pmpo_mask_launch(const PmpoMaskJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream)
{
    if (n_jobs <= 0 || total == 0) return;
    hipLaunchKernelGGL(pmpo_mask_kernel, dim3(pmpo_launch_blocks(total)), dim3(256), 0, stream, d_jobs, n_jobs, total);
}

void pmpo_pair_contract_launch(const PmpoPairJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream)
{
    if (n_jobs <= 0 || total == 0) return;
    hipLaunchKernelGGL(pmpo_pair_contract_kernel, dim3(pmpo_launch_blocks(total)), dim3(256), 0, stream, d_jobs, n_jobs, total);
}

void pmpo_direct_sum_launch(const PmpoSumJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream)
{
    if (n_jobs <= 0 || total == 0) return;
    hipLaunchKernelGGL(pmpo_direct_sum_kernel, dim3(pmpo_launch_blocks(total)), dim3(256), 0, stream, d_jobs, n_jobs, total);
}

} // namespace t4a
