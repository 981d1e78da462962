// kernels_batch_compress.hip — the site steps of the compress stage for a ragged batch of chains (batch_compress.hpp): ONE WORKGROUP PER
// CHAIN, one launch per site of either sweep whatever the number of chains, no host round trip inside a sweep.
//
// Right step (bc_right_step_kernel): thin Householder QR of the transposed l x (s r) matricisation in the item's scratch, Q^T into the new
// site, R^T absorbed into the left neighbour.  Every shape follows from the input shapes, so the whole right sweep is queued at once.
// Left step (bc_left_step_kernel), one launch: the (l s) x r matricisation A with the ACTUAL l read from the device rank array
//   tall or square (l s >= r):  A = Q R,    Jacobi on W = R^T:  W V = U_L S,  A = (Q V) S U_L^T:  U = Q [V; 0],  S Vt = (W V)^T
//   wide (l s < r):             A^T = Q R,  Jacobi on W = R:    W V = U_R S,  A = V S (Q U_R)^T:  U = V,         S Vt = (Q [W V; 0])^T
// so in either orientation the reflectors sit in the scratch, the one-sided Jacobi runs on a square factor of at most 64 x 64 in the LDS
// (W and V, 64 KiB: two workgroups per compute unit), U is a product of reflectors and rotations (an isometry whatever the rank: a zero
// matrix forced to rank 1 keeps e_1 and a zero right factor, no dead column has to be completed) and diag(S) Vt needs no division.  The
// rank rule of factorize runs on the device; U[:, :rank] and the absorbed next site are written compactly with the actual dims.
// Safeguards of the serial SVD: an Inf / NaN sets the item's flag and ends the item's steps; a matrix whose largest entry is outside
// 2^-200 .. 2^200 is scaled exactly by a power of two (pow2_scale_exponent); the sweep cap is 60, running into it is accepted.
// Every sum has a fixed order per output element (per-thread sums, DPP sums of fixed shape, no floating-point atomics): two runs give
// the same bits, and an item's bits do not depend on the batch around it.
#include "kernels.hpp"
#include "kernels_jacobi_common.hpp"
#include "batch_compress.hpp"

#include <algorithm>
#include <mutex>
#include <vector>

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

__global__ void __launch_bounds__(BC_T) bc_right_step_kernel(const BcRightJob* __restrict__ jobs, int* flags)
{
    __shared__ double red[BC_T / 64];
    __shared__ unsigned long long s_amax;
    __shared__ int s_bad;
    const BcRightJob jb = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    if (flags[blockIdx.x]) return;
    const int l = jb.l, m = jb.sr, k = jb.k, pl = jb.pl; // T^T is m x l
    double amax;
    if (bc_scan(jb.T, l * m, &s_bad, &s_amax, &amax)) {
        if (tid == 0) flags[blockIdx.x] = 1;
        return;
    }
    const int e2 = pow2_scale_exponent(amax);
    double* G = jb.scratch;
    double* E = G + (size_t)m * l;
    double* diag = E + (size_t)m * k;
    double* tau = diag + k;
    double* v0s = tau + k;
    for (int e = tid; e < l * m; e += BC_T) {
        const int b = e / l, a = e - b * l; // T[a, b]
        const double v = jb.T[e];
        G[b + (size_t)m * a] = e2 != 0 ? ldexp(v, -e2) : v;
    }
    __syncthreads();
    bc_house_qr(G, m, l, diag, tau, v0s, red);
    for (int e = tid; e < m * k; e += BC_T) {
        const int c = e / m, r = e - c * m;
        E[e] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    bc_apply_q(G, m, k, tau, v0s, E, k);
    __syncthreads();
    // the site: Q^T (k x m)
    for (int e = tid; e < k * m; e += BC_T) {
        const int c = e / k, a = e - c * k;
        jb.Z[e] = E[c + (size_t)m * a];
    }
    // the left neighbour: Y[p, a] = sum_{b >= a} P[p, b] R[a, b], the terms in ascending b
    for (int e = tid; e < pl * k; e += BC_T) {
        const int a = e / pl, p = e - a * pl;
        double sum = jb.P[p + (size_t)pl * a] * diag[a];
        for (int b = a + 1; b < l; ++b) sum += jb.P[p + (size_t)pl * b] * G[a + (size_t)m * b];
        jb.Y[e] = e2 != 0 ? ldexp(sum, e2) : sum;
    }
}

__global__ void __launch_bounds__(BC_T) bc_left_step_kernel(const BcLeftJob* __restrict__ jobs, int* ranks, int* flags, double tolerance, int cap)
{
    // all of the LDS in the dynamic region, every carve a multiple of 16 bytes
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* W = (double*)smem_raw;
    double* V = W + BC_LD * BC_LD;
    double* sig = V + BC_LD * BC_LD;
    double* red = sig + BC_LD;
    unsigned long long* s_amax = (unsigned long long*)(red + BC_T / 64);
    int* idx = (int*)(s_amax + 2);
    int* s_i = idx + BC_LD; // [0..2] rotation flags, [3] non-finite, [4] rank
    const BcLeftJob jb = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    if (flags[blockIdx.x]) return;
    const int l = jb.prev < 0 ? 1 : ranks[jb.prev];
    const int M = l * jb.s, N = jb.r;
    double amax;
    if (bc_scan(jb.C, M * N, &s_i[3], s_amax, &amax)) {
        if (tid == 0) flags[blockIdx.x] = 1;
        return;
    }
    const int e2 = pow2_scale_exponent(amax);
    const bool tall = M >= N;
    const int m = tall ? M : N, n = tall ? N : M; // the QR is that of an m x n matrix, n <= 64
    double* G = jb.scratch;
    double* RT = G + (size_t)jb.lb * jb.s * jb.r;
    double* diag = RT + BC_LD * BC_LD;
    double* tau = diag + BC_LD;
    double* v0s = tau + BC_LD;
    for (int e = tid; e < M * N; e += BC_T) {
        const double v = e2 != 0 ? ldexp(jb.C[e], -e2) : jb.C[e];
        if (tall) {
            G[e] = v;
        } else {
            const int b = e / M, a = e - b * M; // A[a, b] -> A^T[b, a]
            G[b + (size_t)N * a] = v;
        }
    }
    if (tid < 3) s_i[tid] = 0;
    if (tid < BC_LD) idx[tid] = tid;
    __syncthreads();
    bc_house_qr(G, m, n, diag, tau, v0s, red);
    // W = R^T (tall) or R (wide), V = I
    for (int e = tid; e < BC_LD * BC_LD; e += BC_T) {
        const int b = e / BC_LD, a = e - b * BC_LD; // W[a, b]
        double w = 0.0;
        if (a < n && b < n) {
            const int lo = tall ? b : a, hi = tall ? a : b; // R[lo, hi] with lo <= hi
            if (lo == hi) w = diag[lo];
            else if (lo < hi) w = G[lo + (size_t)m * hi];
        }
        W[e] = w;
        V[e] = (a == b && a < n) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (n >= 2) {
        if (n <= 16) bc_jacobi<1>(W, V, n, s_i);
        else if (n <= 32) bc_jacobi<2>(W, V, n, s_i);
        else if (n <= 48) bc_jacobi<3>(W, V, n, s_i);
        else bc_jacobi<4>(W, V, n, s_i);
    }
    __syncthreads();
    // singular values (of the scaled matrix: the rank rule is relative), sorted non-increasing, ties by index
    if (tid < n) {
        double a = 0.0;
        for (int r = 0; r < n; ++r) a += W[r + tid * BC_LD] * W[r + tid * BC_LD];
        sig[tid] = sqrt(a);
    }
    __syncthreads();
    if (tid < n) {
        const double sj = sig[tid];
        int pos = 0;
        for (int i = 0; i < n; ++i) {
            const double si = sig[i];
            if (si > sj || (si == sj && i < tid)) ++pos;
        }
        idx[pos] = tid;
    }
    __syncthreads();
    if (tid == 0) {
        // factorize: cutoff = tolerance * s_max, values kept while rank < cap and s >= cutoff; a zero matrix is floored to rank 1
        const double s_max = sig[idx[0]];
        int rank = 0;
        if (s_max > 0.0) {
            const double cutoff = tolerance * s_max;
            for (int p = 0; p < n; ++p) {
                if (cap != 0 && rank >= cap) break;
                if (sig[idx[p]] < cutoff) break;
                ++rank;
            }
        }
        if (rank < 1) rank = 1;
        s_i[4] = rank;
        ranks[jb.cur] = rank;
    }
    __syncthreads();
    const int rank = s_i[4];
    // U (M x rank) and RT = (diag(S) Vt)^T (N x rank)
    for (int e = tid; e < M * rank; e += BC_T) {
        const int kk = e / M, a = e - kk * M;
        jb.U[e] = a < n ? V[a + idx[kk] * BC_LD] : 0.0;
    }
    for (int e = tid; e < N * rank; e += BC_T) {
        const int kk = e / N, j = e - kk * N;
        double w = 0.0;
        if (j < n) {
            w = W[j + idx[kk] * BC_LD];
            if (e2 != 0) w = ldexp(w, e2);
        }
        RT[e] = w;
    }
    __syncthreads();
    if (tall) bc_apply_q(G, M, n, tau, v0s, jb.U, rank);
    else bc_apply_q(G, N, n, tau, v0s, RT, rank);
    __syncthreads();
    // the next site: Nout[k, c] = sum_j RT[j, k] Nx[j, c], the terms in ascending j; RT goes through the LDS (W and V are done)
    double* RTs = W;
    for (int e = tid; e < N * rank; e += BC_T) {
        const int kk = e / N, j = e - kk * N;
        RTs[j * BC_LD + kk] = RT[e];
    }
    __syncthreads();
    const int total = rank * jb.rest;
    for (int e = tid; e < total; e += BC_T) {
        const int c = e / rank, kk = e - c * rank;
        const double* x = jb.Nx + (size_t)N * c;
        double sum = 0.0;
        for (int j = 0; j < N; ++j) sum += RTs[j * BC_LD + kk] * x[j];
        jb.Nout[e] = sum;
    }
}

constexpr size_t BC_LEFT_LDS = sizeof(double) * (2 * BC_LD * BC_LD + BC_LD + BC_T / 64) + sizeof(unsigned long long) * 2 + sizeof(int) * (BC_LD + 8);

} // namespace

void bc_right_step_launch(const BcRightJob* d_jobs, int n_items, int* d_flags, hipStream_t stream)
{
    if (n_items <= 0) return;
    hipLaunchKernelGGL(bc_right_step_kernel, dim3((unsigned)n_items), dim3(BC_T), 0, stream, d_jobs, d_flags);
}

void bc_left_step_launch(const BcLeftJob* d_jobs, int n_items, int* d_ranks, int* d_flags, double tolerance, int cap, hipStream_t stream)
{
    if (n_items <= 0) return;
    // the kernel needs more dynamic LDS than the default limit; the attribute belongs to the device, so it is set once per device, and a
    // failure is reported here, not as a launch error later
    static std::mutex attr_mutex;
    static std::vector<int> attr_devices;
    {
        int dev = 0;
        T4A_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lock(attr_mutex);
        if (std::find(attr_devices.begin(), attr_devices.end(), dev) == attr_devices.end()) {
            T4A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&bc_left_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)BC_LEFT_LDS));
            attr_devices.push_back(dev);
        }
    }
    hipLaunchKernelGGL(bc_left_step_kernel, dim3((unsigned)n_items), dim3(BC_T), BC_LEFT_LDS, stream, d_jobs, d_ranks, d_flags, tolerance, cap);
}

} // namespace t4a
