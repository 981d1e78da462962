// kernels_batch_truncate.hip — the site steps of the budgeted truncation of a ragged batch of chains (batch_truncate.hpp): ONE WORKGROUP PER
// CHAIN, one launch per site and sweep whatever the number of chains, no host round trip inside a sweep.
//
// QR step (bt_qr_step_kernel): thin Householder QR of the (l s) x r matricisation as it lies in memory, Q into the new site, R absorbed
// into the right neighbour — the mirror of bc_right_step_kernel.  Every shape follows from the input shapes.  The last step also sums
// the squares of the centre site it writes: per-thread sums in element order, then the workgroup sum of fixed shape.
// SVD step (bt_svd_step_kernel<LEFT>): the algorithm of bc_left_step_kernel (QR of the longer side, one-sided Jacobi on the square factor
// of at most 64 x 64 in the LDS, U a product of reflectors and rotations, diag(S) Vt without a division) on the matrix A (M x N) whose
// N side is the bond under truncation:
//   rightward  A[a, b] = C[a + M b]   (the site as (l s) x r),  U -> site (l, s, rank),  Nout[k, c] = sum_j (S Vt)[k, j] Nb[j, c]
//   leftward   A[a, b] = C[b + N a]   (the site as l x (s r)),  U^T -> site (rank, s, r),  Nout[p, k] = sum_j Nb[p, j] (S Vt)[k, j]
// Every dimension an earlier SVD step decided is read from the rank array; a value outside the bound the host planned for sets the
// item's flag to 2 and ends its steps (nothing is written past a buffer).  The rank rule is svd_retained_rank (tensorops.hip) statement
// by statement on the unscaled singular values, then the cap and the floor of one.
#include "kernels_batch_steps.hpp"
#include "batch_truncate.hpp"

#include <algorithm>
#include <mutex>
#include <vector>

namespace t4a {

namespace {

__global__ void __launch_bounds__(BC_T) bt_qr_step_kernel(const BtQrJob* __restrict__ jobs, int* flags)
{
    __shared__ double red[BC_T / 64];
    __shared__ unsigned long long s_amax;
    __shared__ int s_bad;
    const BtQrJob jb = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    if (flags[blockIdx.x]) return;
    const int M = jb.ls, r = jb.r, k = jb.k, rest = jb.rest;
    double amax;
    if (bc_scan(jb.T, M * r, &s_bad, &s_amax, &amax)) {
        if (tid == 0) flags[blockIdx.x] = 1;
        return;
    }
    if (jb.norm2) { // the last step: the last site is read by no later QR step, so it is scanned here (its values enter the norm)
        __syncthreads();
        double amax_nx;
        if (bc_scan(jb.Nx, r * rest, &s_bad, &s_amax, &amax_nx)) {
            if (tid == 0) flags[blockIdx.x] = 1;
            return;
        }
    }
    const int e2 = pow2_scale_exponent(amax);
    double* G = jb.scratch;
    double* E = G + (size_t)M * r;
    double* diag = E + (size_t)M * k;
    double* tau = diag + k;
    double* v0s = tau + k;
    for (int e = tid; e < M * r; e += BC_T) G[e] = e2 != 0 ? ldexp(jb.T[e], -e2) : jb.T[e];
    __syncthreads();
    bc_house_qr(G, M, r, diag, tau, v0s, red);
    for (int e = tid; e < M * k; e += BC_T) {
        const int c = e / M, a = e - c * M;
        E[e] = a == c ? 1.0 : 0.0;
    }
    __syncthreads();
    bc_apply_q(G, M, k, tau, v0s, E, k);
    __syncthreads();
    for (int e = tid; e < M * k; e += BC_T) jb.Q[e] = E[e];
    // the right neighbour: Y[a, c] = sum_{b >= a} R[a, b] Nx[b, c], the terms in ascending b
    double acc = 0.0;
    for (int e = tid; e < k * rest; e += BC_T) {
        const int c = e / k, a = e - c * k;
        const double* x = jb.Nx + (size_t)r * c;
        double sum = diag[a] * x[a];
        for (int b = a + 1; b < r; ++b) sum += G[a + (size_t)M * b] * x[b];
        const double y = e2 != 0 ? ldexp(sum, e2) : sum;
        jb.Y[e] = y;
        acc += y * y;
    }
    if (jb.norm2) {
        acc = block_sum(acc, red);
        if (tid == 0) *jb.norm2 = acc;
    }
}

template <bool LEFT> __global__ void __launch_bounds__(BC_T) bt_svd_step_kernel(const BtSvdJob* __restrict__ jobs, const BtRule* __restrict__ rules, int* ranks, int* flags)
{
    // all of the LDS in the dynamic region, every carve a multiple of 16 bytes
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* W = (double*)smem_raw;
    double* V = W + BC_LD * BC_LD;
    double* sig = V + BC_LD * BC_LD;
    double* srt = sig + BC_LD; // the singular values, sorted and unscaled
    double* mv = srt + BC_LD;  // their measure: the value or its square
    double* red = mv + BC_LD;
    unsigned long long* s_amax = (unsigned long long*)(red + BC_T / 64);
    int* idx = (int*)(s_amax + 2);
    int* s_i = idx + BC_LD; // [0..2] rotation flags, [3] non-finite, [4] rank
    const BtSvdJob jb = jobs[blockIdx.x];
    const BtRule rl = rules[blockIdx.x];
    const int tid = threadIdx.x;
    if (flags[blockIdx.x] || rl.skip) return;
    const int outer = jb.outer_idx < 0 ? jb.outer_dim : ranks[jb.outer_idx];
    const int N = jb.trunc_idx < 0 ? jb.trunc_dim : ranks[jb.trunc_idx];
    const int far_ = jb.far_idx < 0 ? jb.far_dim : ranks[jb.far_idx];
    if (outer < 1 || outer > jb.outer_dim || N < 1 || N > jb.trunc_dim || N > BC_LD || far_ < 1 || far_ > jb.far_dim) {
        if (tid == 0) flags[blockIdx.x] = 2;
        return;
    }
    const int M = outer * jb.s, rest = far_ * jb.nb_s;
    double amax;
    if (bc_scan(jb.C, M * N, &s_i[3], s_amax, &amax)) {
        if (tid == 0) flags[blockIdx.x] = 1;
        return;
    }
    const int e2 = pow2_scale_exponent(amax);
    const bool tall = M >= N;
    const int m = tall ? M : N, n = tall ? N : M; // the QR is that of an m x n matrix, n <= 64
    double* G = jb.scratch;
    double* RT = G + (size_t)jb.outer_dim * jb.s * jb.trunc_dim;
    double* diag = RT + BC_LD * BC_LD;
    double* tau = diag + BC_LD;
    double* v0s = tau + BC_LD;
    double* E = v0s + BC_LD;
    double* Ub = LEFT ? E : jb.U; // U (M x rank, column-major); leftward it is written out transposed
    for (int e = tid; e < M * N; e += BC_T) {
        const double v = e2 != 0 ? ldexp(jb.C[e], -e2) : jb.C[e];
        int a, b;
        if (LEFT) {
            a = e / N;
            b = e - a * N;
        } else {
            b = e / M;
            a = e - b * M;
        }
        G[tall ? a + (size_t)M * b : b + (size_t)N * a] = v;
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
    // singular values of the scaled matrix, sorted non-increasing, ties by index
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
    // the rule reads the singular values of the matrix itself: a threshold may be absolute
    if (tid < BC_LD) {
        double sv = 0.0;
        if (tid < n) {
            sv = sig[idx[tid]];
            if (e2 != 0) sv = ldexp(sv, e2);
        }
        srt[tid] = sv;
        mv[tid] = rl.measure == 0 ? sv : sv * sv;
        if (jb.sv) jb.sv[tid] = sv;
    }
    __syncthreads();
    if (tid == 0) {
        // svd_retained_rank: one thread, the sums in the order of the host's loops
        const double thr = rl.threshold;
        bool all_zero = true;
        for (int p = 0; p < n; ++p)
            if (mv[p] != 0.0) all_zero = false;
        int keep = 0;
        if (all_zero) {
            keep = 1;
        } else if (rl.rule == 0) {
            if (rl.scale == 0) {
                double ref = 0.0;
                for (int p = 0; p < n; ++p) ref = mv[p] > ref ? mv[p] : ref;
                while (keep < n && ref > 0.0 && mv[keep] / ref > thr) ++keep;
            } else {
                while (keep < n && mv[keep] > thr) ++keep;
            }
        } else {
            double total = 0.0;
            for (int p = 0; p < n; ++p) total += mv[p];
            if (rl.scale == 0 && total == 0.0) {
                keep = 1;
            } else {
                double discarded = 0.0;
                keep = n;
                for (int p = n - 1; p >= 0; --p) {
                    const double t = discarded + mv[p];
                    const bool ok = rl.scale == 0 ? t / total <= thr : t <= thr;
                    if (!ok) break;
                    discarded = t;
                    keep = p;
                }
            }
        }
        if (rl.cap != 0 && keep > rl.cap) keep = rl.cap;
        if (keep < 1) keep = 1;
        if (keep > n) keep = n;
        s_i[4] = keep;
        ranks[jb.cur] = keep;
    }
    __syncthreads();
    const int rank = s_i[4];
    // U (M x rank) and RT = (diag(S) Vt)^T (N x rank)
    for (int e = tid; e < M * rank; e += BC_T) {
        const int kk = e / M, a = e - kk * M;
        Ub[e] = a < n ? V[a + idx[kk] * BC_LD] : 0.0;
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
    if (tall) bc_apply_q(G, M, n, tau, v0s, Ub, rank);
    else bc_apply_q(G, N, n, tau, v0s, RT, rank);
    __syncthreads();
    if (LEFT) {
        for (int e = tid; e < M * rank; e += BC_T) {
            const int a = e / rank, kk = e - a * rank;
            jb.U[e] = E[a + (size_t)M * kk];
        }
    }
    // the neighbour; RT goes through the LDS (W and V are done)
    double* RTs = W;
    for (int e = tid; e < N * rank; e += BC_T) {
        const int kk = e / N, j = e - kk * N;
        RTs[j * BC_LD + kk] = RT[e];
    }
    __syncthreads();
    const int total = rank * rest;
    if (LEFT) {
        // Nout[p, k] = sum_j Nb[p, j] RT[j, k], the terms in ascending j
        for (int e = tid; e < total; e += BC_T) {
            const int kk = e / rest, p = e - kk * rest;
            double sum = 0.0;
            for (int j = 0; j < N; ++j) sum += jb.Nb[p + (size_t)rest * j] * RTs[j * BC_LD + kk];
            jb.Nout[e] = sum;
        }
    } else {
        // Nout[k, c] = sum_j RT[j, k] Nb[j, c], the terms in ascending j
        for (int e = tid; e < total; e += BC_T) {
            const int c = e / rank, kk = e - c * rank;
            const double* x = jb.Nb + (size_t)N * c;
            double sum = 0.0;
            for (int j = 0; j < N; ++j) sum += RTs[j * BC_LD + kk] * x[j];
            jb.Nout[e] = sum;
        }
    }
}

constexpr size_t BT_SVD_LDS = sizeof(double) * (2 * BC_LD * BC_LD + 3 * BC_LD + BC_T / 64) + sizeof(unsigned long long) * 2 + sizeof(int) * (BC_LD + 8);

// the kernels need more dynamic LDS than the default limit; the attribute belongs to the device, so it is set once per device and
// instantiation, and a failure is reported here, not as a launch error later
template <bool LEFT> void bt_svd_attr()
{
    static std::mutex attr_mutex;
    static std::vector<int> attr_devices;
    int dev = 0;
    T4A_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(attr_mutex);
    if (std::find(attr_devices.begin(), attr_devices.end(), dev) == attr_devices.end()) {
        T4A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&bt_svd_step_kernel<LEFT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)BT_SVD_LDS));
        attr_devices.push_back(dev);
    }
}

} // namespace

void bt_qr_step_launch(const BtQrJob* d_jobs, int n_items, int* d_flags, hipStream_t stream)
{
    if (n_items <= 0) return;
    hipLaunchKernelGGL(bt_qr_step_kernel, dim3((unsigned)n_items), dim3(BC_T), 0, stream, d_jobs, d_flags);
}

void bt_svd_step_launch(bool leftward, const BtSvdJob* d_jobs, int n_items, const BtRule* d_rules, int* d_ranks, int* d_flags, hipStream_t stream)
{
    if (n_items <= 0) return;
    if (leftward) {
        bt_svd_attr<true>();
        hipLaunchKernelGGL(bt_svd_step_kernel<true>, dim3((unsigned)n_items), dim3(BC_T), BT_SVD_LDS, stream, d_jobs, d_rules, d_ranks, d_flags);
    } else {
        bt_svd_attr<false>();
        hipLaunchKernelGGL(bt_svd_step_kernel<false>, dim3((unsigned)n_items), dim3(BC_T), BT_SVD_LDS, stream, d_jobs, d_rules, d_ranks, d_flags);
    }
}

} // namespace t4a
