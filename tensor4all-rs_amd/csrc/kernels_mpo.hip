// kernels_mpo.hip — MPO site contraction of the naive MPO-MPO product (tensor4all-simplett/src/mpo/contract_naive.rs:41-98,
// contract_site_tensors environment.rs:37-80):
//   C[(la*Lb+lb), s1, t, (ra*Rb+rb)] = sum_k A[la, s1, k, ra] * B[lb, k, t, rb]
// for every site of the chain in ONE launch.  The shared index k is the physical dimension (typically 2): an MFMA tile would
// mostly hold padding, so each thread forms one output element as a k-ascending sum (separately rounded multiply and add,
// built with -ffp-contract=off).  Site tensors are column-major [left, s1, s2, right].
#include "kernels.hpp"

#include <algorithm>

namespace t4a {

namespace {

__global__ void __launch_bounds__(256) mpo_site_contract_kernel(const MpoSiteJob* __restrict__ jobs, int n_jobs,
                                                                unsigned long long total)
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
        const MpoSiteJob& j = jobs[lo];
        // every site's input and output holds at most INT_MAX elements (checked on the host)
        int q = (int)(e - j.off);
        const int Lc = j.la * j.lb;
        const int row = q % Lc;
        q /= Lc;
        const int s = q % j.s1;
        q /= j.s1;
        const int t = q % j.t;
        const int col = q / j.t;
        const int ia = row / j.lb, ib = row % j.lb;
        const int ra = col / j.rb, rb = col % j.rb;
        // A[ia, s, k, ra] at ia + La (s + S1 (k + K ra)); B[ib, k, t, rb] at ib + Lb (k + K (t + T rb))
        const double* a = j.A + ia + j.la * (s + j.s1 * j.k * ra);
        const double* b = j.B + ib + j.lb * j.k * (t + j.t * rb);
        const int sa = j.la * j.s1, sb = j.lb;
        double acc = 0.0;
        for (int k = 0; k < j.k; ++k) acc = acc + a[sa * k] * b[sb * k];
        j.C[e - j.off] = acc;
    }
}

} // namespace

void mpo_site_contract_launch(const MpoSiteJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream)
{
    if (n_jobs <= 0 || total == 0) return;
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(mpo_site_contract_kernel, dim3(blocks), dim3(256), 0, stream, d_jobs, n_jobs, total);
}

} // namespace t4a
