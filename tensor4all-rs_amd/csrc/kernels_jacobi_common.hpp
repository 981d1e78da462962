// kernels_jacobi_common.hpp — the device helpers the one-sided Jacobi kernels share (kernels_linalg.hip: the SVD of one matrix;
// kernels_batch_compress.hip: the site steps of a batch of chains): DPP sums over a wave or a group of lanes, the workgroup sum, the
// circle-method tournament and the rotation arithmetic.  Units that include it are compiled with -ffp-contract=fast (build.py).
#pragma once

#include <hip/hip_runtime.h>

namespace t4a {

namespace {

// Wave sum through DPP row reductions (no LDS crossbar traffic): every lane of the wave ends with the total.
template <int CTRL> __device__ inline double dpp_mov_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xFFFFFFFFll), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ inline double wave_sum_dpp(double v)
{
    v += dpp_mov_f64<0xB1>(v);  // quad_perm [1,0,3,2]
    v += dpp_mov_f64<0x4E>(v);  // quad_perm [2,3,0,1]
    v += dpp_mov_f64<0x141>(v); // row_half_mirror
    v += dpp_mov_f64<0x140>(v); // row_mirror: every lane of a row of 16 holds the row sum
    // rows -> wave: lanes 15, 31, 47, 63 hold the four row sums
    const long long b = __double_as_longlong(v);
    double t = 0.0;
#pragma unroll
    for (int l = 15; l < 64; l += 16) {
        const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
        t += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    }
    return t;
}

// (round 5: the shuffle form — six __shfl_down = twelve ds_bpermute round trips + a broadcast — is gone: block_sum sits in front of
// every Householder column of the QR panel and of every rank count of the SVD's sort)
__device__ inline double wave_sum(double v) { return wave_sum_dpp(v); }

// Sum over the whole workgroup, identical on every thread.  `red` holds one slot per wave.
__device__ inline double block_sum(double v, double* red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += red[w];
    __syncthreads();
    return t;
}

// circle-method tournament: pair `k` of round `r` among np (even) players
__device__ inline void rr_pair(int np, int r, int k, int* a, int* b)
{
    const int q = np - 1;
    int x, y;
    if (k == 0) {
        x = q;
        y = r % q;
    } else {
        x = (r + k) % q;
        y = (r - k + q) % q;
    }
    *a = x < y ? x : y;
    *b = x < y ? y : x;
}

struct Rot {
    double c, s;
    int apply;
};
// A pair rotates when the cosine of the angle between its columns exceeds tol = sqrt(m) * eps — the stopping rule of LAPACK's one-sided
// Jacobi (dgesvj: "TOL = SQRT(M) * EPS").  Round 5: with tol = eps the last two sweeps of every decomposition found 1 - 200 of the 32 640
// pairs of a 256-column matrix to rotate (angles of a few eps); singular values and vectors agree to the same 1e-14 either way.
// The scale of the pair test, sqrt(alpha beta).  Where the product of the two squared norms leaves the normal range (columns of norm
// below ~1e-77 inside a matrix that is not rescaled: alpha * beta underflowed to 0 and EVERY pair with a nonzero gamma passed the test,
// so the iteration never converged) the product of the two square roots; in the normal range the same expression as before, bit for bit.
__device__ inline double pair_scale(double alpha, double beta)
{
    const double ab = alpha * beta;
    if (ab >= 2.2250738585072014e-308 && ab <= 1.79769313486231570e308) return sqrt(ab);
    return sqrt(alpha) * sqrt(beta);
}
__device__ inline Rot jacobi_rotation(double alpha, double beta, double gamma, double tol)
{
    Rot r;
    r.c = 1.0;
    r.s = 0.0;
    r.apply = 0;
    if (gamma == 0.0 || !(fabs(gamma) > tol * pair_scale(alpha, beta))) return r;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    // |zeta| > 1e154: zeta * zeta overflows and t = 0 — the identity, which must not count as a rotation (the sweep would never converge)
    if (t == 0.0) return r;
    // c = (1 + t^2)^(-1/2), |t| <= 1: the hardware estimate and two Newton steps (y <- y (3 - x y^2) / 2) instead of a square root and a
    // division in the longest dependent chain of a local round
    const double x = 1.0 + t * t;
    double y = __builtin_amdgcn_rsq(x);
    y = y * (1.5 - 0.5 * x * y * y);
    y = y * (1.5 - 0.5 * x * y * y);
    r.c = y;
    r.s = r.c * t;
    r.apply = 1;
    return r;
}
__device__ inline double jacobi_tol(int m) { return 2.220446049250313e-16 * sqrt((double)m); }

// Sum over an aligned group of G = 8 or 16 lanes (DPP inside a row of 16, no readlane): every lane of the group ends with bitwise the same
// total (the two operands of every addition are the same pair of partial sums in every lane, in either order).
template <int G> __device__ inline double group_sum(double v)
{
    v += dpp_mov_f64<0xB1>(v);  // quad_perm [1,0,3,2]
    v += dpp_mov_f64<0x4E>(v);  // quad_perm [2,3,0,1]
    v += dpp_mov_f64<0x141>(v); // row_half_mirror: the sum of 8 lanes
    if (G == 16) v += dpp_mov_f64<0x140>(v); // row_mirror
    return v;
}

// jacobi_rotation with the divisions and square roots replaced by the hardware reciprocal / reciprocal-square-root estimates and Newton
// steps (the rotation arithmetic is the longest dependent chain of a round of jacobi_groups_kernel).  The ANGLE (zeta, t) is computed to
// ~2^-46: an error there leaves a residual inner product of that relative size, which the next sweep removes; the COSINE keeps both
// Newton steps (c^2 + s^2 = 1 to rounding: every rotation stays orthogonal).  Out-of-range intermediates (|zeta| > 1e154, subnormal
// gamma) surface as a NaN and hand the pair to the exact jacobi_rotation.
__device__ inline Rot jacobi_rotation_fast(double alpha, double beta, double gamma, double tol)
{
    Rot r;
    r.c = 1.0;
    r.s = 0.0;
    r.apply = 0;
    if (gamma == 0.0) return r;
    const double ab = alpha * beta;
    // sqrt(alpha beta) to 2^-23: a threshold (outside the normal range of alpha * beta the exact scale: pair_scale)
    const double sq = (ab >= 2.2250738585072014e-308 && ab <= 1.79769313486231570e308) ? ab * __builtin_amdgcn_rsq(ab) : pair_scale(alpha, beta);
    if (!(fabs(gamma) > tol * sq)) return r;
    const double den = 2.0 * gamma;
    double rd = __builtin_amdgcn_rcp(den);
    rd = rd * (2.0 - den * rd);
    const double zeta = (beta - alpha) * rd;
    const double x = 1.0 + zeta * zeta;
    double y = __builtin_amdgcn_rsq(x);
    y = y * (1.5 - 0.5 * x * y * y);
    const double d2 = fabs(zeta) + x * y; // |zeta| + sqrt(1 + zeta^2) >= 1
    double rt = __builtin_amdgcn_rcp(d2);
    rt = rt * (2.0 - d2 * rt);
    const double t = zeta >= 0.0 ? rt : -rt;
    const double x2 = 1.0 + t * t;
    double c = __builtin_amdgcn_rsq(x2);
    c = c * (1.5 - 0.5 * x2 * c * c);
    c = c * (1.5 - 0.5 * x2 * c * c);
    const double sn = c * t;
    // a pair that passed the test but whose estimates left the range (a subnormal gamma: rcp(2 gamma) overflows; |zeta| > 1e154): the
    // exact rotation, with IEEE division and square roots (skipping it left live columns of norm ~1e-150 un-orthogonalised, silently)
    if (!(c == c) || !(sn == sn)) return jacobi_rotation(alpha, beta, gamma, tol);
    r.c = c;
    r.s = sn;
    r.apply = 1;
    return r;
}

} // namespace

} // namespace t4a
