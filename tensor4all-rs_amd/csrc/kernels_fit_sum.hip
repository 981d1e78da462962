// kernels_fit_sum.hip — the half products of a bond step of fit_sum (fit_sum.hpp) for ALL targets in one launch.  A job is one target's
// block, O = X Y with every operand addressed by a row and a column stride, so an environment block and a core are read in place in
// either orientation and the block lands at its offset of P or Q.  The job table lives in device memory (the number of targets is not
// bounded by a by-value argument); a workgroup finds its job by a binary search of the first tiles.
//
// Arithmetic, chosen per job by the host (mfma): the summed and both output dimensions from FIT_SUM_MFMA_MIN up take 16 x 16 output
// tiles on v_mfma_f64_16x16x4_f64, a workgroup a strip of 16 rows x 64 columns (one tile per wavefront), the summed index in chunks of
// four, ascending, edge tiles and the last chunk zero-padded in registers (operand roles as in kernels_gse.hip /
// kernels_contraction.hip: first operand indexed by the output column, second by the output row, acc[reg] = out[row = lane & 15]
// [col = (lane >> 4) + 4 reg]).  Otherwise one output element per thread, the summed index ascending, multiply and add rounded
// separately (the file is built with -ffp-contract=off).  First version, not tuned: a lane loads its operand element straight from
// global memory.  There is no floating-point atomic and no split of a summed index: the bits of an output depend on the operands and
// the job's shape alone, not on the other jobs of the launch.
#include "fit_sum.hpp"

namespace t4a {

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr int FIT_SUM_THREADS = 256;

__global__ void __launch_bounds__(FIT_SUM_THREADS) fit_sum_half_kernel(const FitSumJob* __restrict__ jobs, int n_jobs)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    int lo = 0, hi = n_jobs - 1; // the last job whose first tile is <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const FitSumJob J = jobs[lo];
    const int t = b - J.tile0;
    if (J.mfma) {
        const int nrt = (J.m + 15) >> 4;
        const int m0 = (t % nrt) << 4, ct = ((t / nrt) << 2) + (tid >> 6);
        if ((ct << 4) >= J.n) return; // a wavefront past the last column tile of the strip
        const int lane = tid & 63, lr = lane & 15, lk = lane >> 4;
        const int row = m0 + lr, c = (ct << 4) + lr;
        const bool row_ok = row < J.m, c_ok = c < J.n;
        double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < J.k; k0 += 4) {
            const int k = k0 + lk;
            const bool k_ok = k < J.k;
            const double xv = (row_ok && k_ok) ? J.X[(long long)row * J.xrs + (long long)k * J.xcs] : 0.0;
            const double yv = (c_ok && k_ok) ? J.Y[(long long)k * J.yrs + (long long)c * J.ycs] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(yv, xv, acc, 0, 0, 0);
        }
        if (!row_ok) return;
        const long long ro = (long long)(row % J.rdiv) * J.ors + (long long)(row / J.rdiv) * J.ors2;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int cc = (ct << 4) + lk + 4 * reg;
            if (cc < J.n) J.O[ro + (long long)cc * J.ocs] = acc[reg];
        }
    } else {
        const long long e = (long long)t * FIT_SUM_THREADS + tid;
        if (e >= (long long)J.m * J.n) return;
        const int row = (int)(e % J.m), c = (int)(e / J.m);
        const double* x = J.X + (long long)row * J.xrs;
        const double* y = J.Y + (long long)c * J.ycs;
        double s = 0.0;
        for (int k = 0; k < J.k; ++k) s = s + x[(long long)k * J.xcs] * y[(long long)k * J.yrs];
        J.O[(long long)(row % J.rdiv) * J.ors + (long long)(row / J.rdiv) * J.ors2 + (long long)c * J.ocs] = s;
    }
}

} // namespace

void fit_sum_half_launch(const FitSumJob* d_jobs, int n_jobs, int n_tiles, hipStream_t stream)
{
    if (n_jobs <= 0 || n_tiles <= 0) return;
    hipLaunchKernelGGL(fit_sum_half_kernel, dim3((unsigned)n_tiles), dim3(FIT_SUM_THREADS), 0, stream, d_jobs, n_jobs);
}

} // namespace t4a
