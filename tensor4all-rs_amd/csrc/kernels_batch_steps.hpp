// kernels_batch_steps.hpp — the device routines the batched site steps share (kernels_batch_compress.hip: the compress stage;
// kernels_batch_truncate.hip: the budgeted truncation): the non-finite / magnitude scan, the Householder QR of one workgroup with its
// reflector application, and the one-sided Jacobi on a square factor of at most 64 x 64 in the LDS.  One workgroup of BC_T threads per
// item.  Units that include it are compiled with -ffp-contract=fast (build.py), as kernels_jacobi_common.hpp asks.
#pragma once

#include "kernels.hpp"
#include "kernels_jacobi_common.hpp"
#include "batch_compress.hpp"

namespace t4a {

namespace {

constexpr int BC_T = 512; // threads of a workgroup: 32 pair slots of 16 lanes, the 32 pairs of a 64-column tournament round
constexpr int BC_LD = BATCH_COMPRESS_BMAX;
constexpr double BC_TINY = 1.4916681462400413e-154; // sqrt(DBL_MIN): below it a squared norm underflows

// Inf / NaN flag and the largest magnitude of `count` values; the same on every thread.  s_bad and s_amax are zeroed here.
__device__ inline bool bc_scan(const double* __restrict__ x, int count, int* s_bad, unsigned long long* s_amax, double* amax)
{
    const int tid = threadIdx.x;
    if (tid == 0) {
        *s_bad = 0;
        *s_amax = 0ull;
    }
    __syncthreads();
    int bad = 0;
    double mx = 0.0;
    for (int e = tid; e < count; e += BC_T) {
        const double v = fabs(x[e]);
        if (!(v <= 1.79769313486231570e308)) bad = 1;
        else if (v > mx) mx = v;
    }
    if (bad) *s_bad = 1;
    if (mx > 0.0) atomicMax(s_amax, (unsigned long long)__double_as_longlong(mx)); // (non-negative doubles order like their bit patterns)
    __syncthreads();
    *amax = __longlong_as_double((long long)*s_amax);
    return *s_bad != 0;
}

// Householder QR of G (m x n, column-major, leading dimension m) in place by the whole workgroup, k = min(m, n) reflectors
// H_j = I - tau_j v_j v_j^T (alpha = -sign(x0) |x|, v = x - alpha e_j unnormalised, tau = 2 / v.v, as qr_panel_kernel):
// R[a, b] = G[a + m b] for a < b and diag[a] for a == b; v_j = (v0s[j], G[j + 1 .., j]).  A column whose norm underflows is left alone
// (tau = 0).  Ends behind a barrier.
__device__ void bc_house_qr(double* G, int m, int n, double* diag, double* tau, double* v0s, double* red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = BC_T / 64;
    const int k = m < n ? m : n;
    for (int j = 0; j < k; ++j) {
        double* col = G + (size_t)m * j;
        double ss = 0.0;
        for (int r = j + tid; r < m; r += BC_T) ss += col[r] * col[r];
        ss = block_sum(ss, red);
        const double x0 = col[j];
        const double nrm = sqrt(ss);
        double alpha = x0, v0 = 0.0, t = 0.0;
        if (nrm > BC_TINY) {
            alpha = x0 >= 0.0 ? -nrm : nrm;
            v0 = x0 - alpha;
            t = 1.0 / (nrm * (nrm + fabs(x0))); // v.v = 2 |x| (|x| + |x0|)
        }
        if (tid == 0) {
            diag[j] = alpha;
            tau[j] = t;
            v0s[j] = v0;
        }
        if (t != 0.0) {
            const int r0 = (j & ~63) + lane; // a lane keeps its rows from step to step
            for (int c = j + 1 + wave; c < n; c += nw) {
                double* cc = G + (size_t)m * c;
                double d = 0.0;
                for (int r = r0; r < m; r += 64)
                    if (r >= j) d += (r == j ? v0 : col[r]) * cc[r];
                d = wave_sum(d) * t;
                for (int r = r0; r < m; r += 64)
                    if (r >= j) cc[r] -= d * (r == j ? v0 : col[r]);
            }
        }
        __syncthreads();
    }
}

// E (m x nc, leading dimension m) <- H_0 H_1 .. H_{k-1} E with the reflectors bc_house_qr left in G: one wave per column, a lane owns the
// rows lane, lane + 64, .. of its column throughout, so no barrier is needed between the reflectors.
__device__ void bc_apply_q(const double* G, int m, int k, const double* tau, const double* v0s, double* E, int nc)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = BC_T / 64;
    for (int c = wave; c < nc; c += nw) {
        double* cc = E + (size_t)m * c;
        for (int j = k - 1; j >= 0; --j) {
            const double t = tau[j];
            if (t == 0.0) continue;
            const double* col = G + (size_t)m * j;
            const double v0 = v0s[j];
            const int r0 = (j & ~63) + lane;
            double d = 0.0;
            for (int r = r0; r < m; r += 64)
                if (r >= j) d += (r == j ? v0 : col[r]) * cc[r];
            d = wave_sum(d) * t;
            for (int r = r0; r < m; r += 64)
                if (r >= j) cc[r] -= d * (r == j ? v0 : col[r]);
        }
    }
}

// One-sided Jacobi on the n x n matrix W (LDS, leading dimension 64, rows n .. 16 MR - 1 zero) with V accumulating the rotations: the
// loop of jacobi_groups_kernel (a group of 16 lanes per column pair, a lane owns MR rows of both columns of W and of V).
template <int MR> __device__ void bc_jacobi(double* W, double* V, int n, int* s_rot)
{
    constexpr int G = 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & (G - 1);
    const int k = wave * (64 / G) + lane / G;
    const int np = n + (n & 1), q = np - 1;
    const bool slot = k < np / 2;
    const double tol = jacobi_tol(n);
    for (int sweep = 0; sweep < 60; ++sweep) {
        // three flags in rotation, as in jacobi_groups_kernel
        if (tid == 0) s_rot[(sweep + 1) % 3] = 0;
        int* rotated = &s_rot[sweep % 3];
        for (int round = 0; round < q; ++round) {
            int x, y;
            if (k == 0) {
                x = q;
                y = round;
            } else {
                x = round + k;
                if (x >= q) x -= q;
                y = round - k;
                if (y < 0) y += q;
            }
            const int i = x < y ? x : y, j = x < y ? y : x;
            if (slot && j < n) {
                double* wi = W + i * BC_LD + sub;
                double* wj = W + j * BC_LD + sub;
                double* vi = V + i * BC_LD + sub;
                double* vj = V + j * BC_LD + sub;
                double xv[MR], yv[MR], vx[MR], vy[MR];
#pragma unroll
                for (int t = 0; t < MR; ++t) {
                    xv[t] = wi[G * t];
                    yv[t] = wj[G * t];
                    vx[t] = vi[G * t];
                    vy[t] = vj[G * t];
                }
                double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
                for (int t = 0; t < MR; ++t) {
                    a += xv[t] * xv[t];
                    b += yv[t] * yv[t];
                    g += xv[t] * yv[t];
                }
                a = group_sum<G>(a);
                b = group_sum<G>(b);
                g = group_sum<G>(g);
                const Rot rot = jacobi_rotation_fast(a, b, g, tol);
                if (rot.apply) {
                    if (sub == 0) *rotated = 1;
#pragma unroll
                    for (int t = 0; t < MR; ++t) {
                        wi[G * t] = rot.c * xv[t] - rot.s * yv[t];
                        wj[G * t] = rot.s * xv[t] + rot.c * yv[t];
                        vi[G * t] = rot.c * vx[t] - rot.s * vy[t];
                        vj[G * t] = rot.s * vx[t] + rot.c * vy[t];
                    }
                }
            }
            __syncthreads();
        }
        if (!*rotated) break;
    }
}

} // namespace

} // namespace t4a
