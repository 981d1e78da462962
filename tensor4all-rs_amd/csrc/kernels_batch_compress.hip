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
#include "kernels_batch_steps.hpp"

#include <algorithm>
#include <mutex>
#include <vector>

namespace t4a {

namespace {

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
