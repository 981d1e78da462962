// kernels_contraction.hip — left / right environments of the lazy product of two MPOs (tensor4all-simplett/src/mpo/contraction.rs:
// evaluate_left :262-314, evaluate_right :324-383) for a batch of unique index halves, one workgroup per half.
// At the end of the file: contraction_pair_kernel, every left environment of a cut paired with every right one (a candidate matrix).
//
// An environment of the product A·B is a matrix over the bond pair (a, b), held column-major [a + dim_a * b].  A site step
//   L'[ra, rb] = sum_{la, lb, k} L[la, lb] A[la, i, k, ra] B[lb, k, j, rb]      (contraction.rs:288-308)
//   R'[la, lb] = sum_{ra, rb, k} R[ra, rb] A[la, i, k, ra] B[lb, k, j, rb]      (contraction.rs:357-377)
// is done as two small matrix products instead of the five-deep loop:
//   left :  T_k[ra, lb] = sum_la A[la, i, k, ra] L[la, lb]   for every shared index k,   L'[ra, rb] = sum_k sum_lb T_k[ra, lb] B[lb, k, j, rb]
//   right:  T_k[la, rb] = sum_ra A[la, i, k, ra] R[ra, rb]   for every shared index k,   R'[la, lb] = sum_k sum_rb T_k[la, rb] B[lb, k, j, rb]
// (k ascending in the second product), K ra lb (la + rb) multiply-adds instead of K la lb ra rb.
//
// Which arithmetic a product takes is decided per product from its OUTPUT shape M x N:
//   M >= 16 and N >= 16  -> f64 matrix cores (v_mfma_f64_16x16x4_f64), one 16 x 16 output tile per wavefront at a time, edge tiles
//                           and the summed dimension zero-padded in registers;
//   otherwise            -> one output element per thread, summed index ascending, multiply and add rounded separately (the file is
//                           built with -ffp-contract=off), as in kernels_mpo.hip.
// For the left walk that is: product 1 on the cores where ra >= 16 and lb >= 16, product 2 where ra >= 16 and rb >= 16; for the right
// walk: product 1 where la >= 16 and rb >= 16, product 2 where la >= 16 and lb >= 16.  Operators with every bond below 16 (the quantics
// transform operators, bonds 1 - 4) never touch the cores; a product with bonds 32 and 24 runs both products of every inner site on them.
// The matrix-core branch is a first version and not tuned: every lane loads its one operand element per instruction straight from global
// memory or the LDS (the A operand with stride la*s1*K across lanes), a tile's operands are not reused across tiles, and one wavefront
// works on a tile.  At the sizes measured the calls are bound by the host, not by these kernels.
//
// The current environment, the next one (double buffered) and the K intermediate matrices T_k are the working set of a workgroup:
// 2 * env_cap + t_cap doubles.  The launcher places it in the LDS when it fits CONTRACTION_LDS_DOUBLES (64 KiB, what a workgroup gets
// without opting into more) and otherwise in a slice of global scratch per workgroup — the same walk, every step through memory.
#include "kernels.hpp"

#include <algorithm>

namespace t4a {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

// C[m + ldc * n] = sum_{k1 < K1} sum_{x < K2} P[m * psm + k1 * psk1 + x * psk2] * Q[n * qsn + k1 * qsk1 + x * qsk2]   (k1 outer, both ascending)
// for 0 <= m < M, 0 <= n < N, by the whole workgroup.  The caller synchronises before (operands written) and after (C complete).
__device__ __forceinline__ void wg_product(int M, int N, int K1, int K2, const double* P, int psm, int psk1, int psk2, const double* Q,
                                           int qsn, int qsk1, int qsk2, double* C, int ldc)
{
    const int tid = threadIdx.x, T = blockDim.x;
    if (M >= 16 && N >= 16) {
        // MFMA operand roles as in gemm_kernel (kernels_dense.hip): first operand = Q^T (lane: n = lane & 15, k = lane >> 4), second
        // operand = P (lane: m = lane & 15, k = lane >> 4); acc[reg] = C[m = lane & 15][n = (lane >> 4) + 4 reg]
        const int lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
        const int lr = lane & 15, lk = lane >> 4;
        const int mt = (M + 15) >> 4, nt = (N + 15) >> 4;
        for (int t = wave; t < mt * nt; t += nwaves) {
            const int m0 = (t % mt) << 4, n0 = (t / mt) << 4;
            const bool m_ok = m0 + lr < M, n_ok = n0 + lr < N;
            const double* p = P + (size_t)(m_ok ? m0 + lr : 0) * psm;
            const double* q = Q + (size_t)(n_ok ? n0 + lr : 0) * qsn;
            double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
            for (int k1 = 0; k1 < K1; ++k1)
                for (int x0 = 0; x0 < K2; x0 += 4) {
                    const int x = x0 + lk;
                    const bool x_ok = x < K2;
                    const double pv = (m_ok && x_ok) ? p[(size_t)k1 * psk1 + (size_t)x * psk2] : 0.0;
                    const double qv = (n_ok && x_ok) ? q[(size_t)k1 * qsk1 + (size_t)x * qsk2] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qv, pv, acc, 0, 0, 0);
                }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int n = n0 + lk + 4 * reg;
                if (m_ok && n < N) C[(m0 + lr) + (size_t)ldc * n] = acc[reg];
            }
        }
    } else {
        for (int e = tid; e < M * N; e += T) {
            const int m = e % M, n = e / M;
            const double* p = P + (size_t)m * psm;
            const double* q = Q + (size_t)n * qsn;
            double acc = 0.0;
            for (int k1 = 0; k1 < K1; ++k1)
                for (int x = 0; x < K2; ++x) {
                    const double prod = p[(size_t)k1 * psk1 + (size_t)x * psk2] * q[(size_t)k1 * qsk1 + (size_t)x * qsk2];
                    acc = acc + prod;
                }
            C[m + (size_t)ldc * n] = acc;
        }
    }
}

__device__ __forceinline__ double* working_set(double* lds, double* scratch, size_t ws_doubles)
{
    return scratch ? scratch + (size_t)blockIdx.x * ws_doubles : lds;
}

// idx: n_items x (2 n_walk) uint32, [i_0, j_0, i_1, j_1, ...] of sites 0 .. n_walk-1; out: n_items x ld, item `it` holds the
// ra x rb environment behind site n_walk-1, column-major.
__global__ void __launch_bounds__(256) contraction_env_left_kernel(const ContractionSiteDesc* __restrict__ sites, int n_walk,
                                                                   const uint32_t* __restrict__ idx, int n_items, double* __restrict__ out,
                                                                   int ld, int env_cap, int t_cap, double* scratch)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* ws = working_set((double*)smem_raw, scratch, (size_t)2 * env_cap + t_cap);
    double* cur = ws;
    double* nxt = ws + env_cap;
    double* tk = ws + 2 * (size_t)env_cap;
    const int tid = threadIdx.x, T = blockDim.x;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const uint32_t* my = idx + (size_t)it * 2 * n_walk;
        if (tid == 0) cur[0] = 1.0; // the environment left of site 0 (contraction.rs:269-273)
        __syncthreads();
        for (int s = 0; s < n_walk; ++s) {
            const ContractionSiteDesc d = sites[s];
            const int i = (int)my[2 * s], j = (int)my[2 * s + 1];
            // A[la, i, k, ra] at la + La (i + S1 (k + K ra));  B[lb, k, j, rb] at lb + Lb (k + K (j + S2 rb))
            const double* a = d.A + (size_t)d.la * i;
            const double* b = d.B + (size_t)d.lb * d.k * j;
            const int a_k = d.la * d.s1, a_r = d.la * d.s1 * d.k;
            const int b_k = d.lb, b_r = d.lb * d.k * d.s2;
            const int tsz = d.ra * d.lb;
            // T_k[ra, lb] (ld ra) = sum_la A[la, i, k, ra] L[la, lb]
            for (int k = 0; k < d.k; ++k)
                wg_product(d.ra, d.lb, 1, d.la, a + (size_t)a_k * k, a_r, 0, 1, cur, d.la, 0, 1, tk + (size_t)tsz * k, d.ra);
            __syncthreads();
            // L'[ra, rb] (ld ra) = sum_k sum_lb T_k[ra, lb] B[lb, k, j, rb]
            wg_product(d.ra, d.rb, d.k, d.lb, tk, 1, tsz, d.ra, b, b_r, b_k, 1, nxt, d.ra);
            __syncthreads();
            double* t = cur;
            cur = nxt;
            nxt = t;
        }
        const ContractionSiteDesc last = sites[n_walk - 1];
        const int len = last.ra * last.rb;
        for (int e = tid; e < len; e += T) out[(size_t)it * ld + e] = cur[e];
        __syncthreads();
    }
}

// idx: n_items x (2 (n_sites - first)) uint32 of sites first .. n_sites-1; out: n_items x ld, item `it` holds the la x lb environment
// in front of site `first`, column-major.
__global__ void __launch_bounds__(256) contraction_env_right_kernel(const ContractionSiteDesc* __restrict__ sites, int n_sites, int first,
                                                                    const uint32_t* __restrict__ idx, int n_items, double* __restrict__ out,
                                                                    int ld, int env_cap, int t_cap, double* scratch)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* ws = working_set((double*)smem_raw, scratch, (size_t)2 * env_cap + t_cap);
    double* cur = ws;
    double* nxt = ws + env_cap;
    double* tk = ws + 2 * (size_t)env_cap;
    const int tid = threadIdx.x, T = blockDim.x;
    const int w = n_sites - first;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const uint32_t* my = idx + (size_t)it * 2 * w;
        if (tid == 0) cur[0] = 1.0; // the environment right of the last site (contraction.rs:332-336)
        __syncthreads();
        for (int s = n_sites - 1; s >= first; --s) {
            const ContractionSiteDesc d = sites[s];
            const int i = (int)my[2 * (s - first)], j = (int)my[2 * (s - first) + 1];
            const double* a = d.A + (size_t)d.la * i;
            const double* b = d.B + (size_t)d.lb * d.k * j;
            const int a_k = d.la * d.s1, a_r = d.la * d.s1 * d.k;
            const int b_k = d.lb, b_r = d.lb * d.k * d.s2;
            const int tsz = d.la * d.rb;
            // T_k[la, rb] (ld la) = sum_ra A[la, i, k, ra] R[ra, rb]
            for (int k = 0; k < d.k; ++k)
                wg_product(d.la, d.rb, 1, d.ra, a + (size_t)a_k * k, 1, 0, a_r, cur, d.ra, 0, 1, tk + (size_t)tsz * k, d.la);
            __syncthreads();
            // R'[la, lb] (ld la) = sum_k sum_rb T_k[la, rb] B[lb, k, j, rb]
            wg_product(d.la, d.lb, d.k, d.rb, tk, 1, tsz, d.la, b, 1, b_k, b_r, nxt, d.la);
            __syncthreads();
            double* t = cur;
            cur = nxt;
            nxt = t;
        }
        const ContractionSiteDesc head = sites[first];
        const int len = head.la * head.lb;
        for (int e = tid; e < len; e += T) out[(size_t)it * ld + e] = cur[e];
        __syncthreads();
    }
}

// out[r, c] = sum_k L[r * K + k] * R[c * K + k]: every left environment paired with every right environment of a cut (a candidate
// matrix of a cross interpolation of A·B).  One workgroup computes a PAIR_TILE x PAIR_TILE tile of the output: the K range is staged
// through the LDS in panels of PAIR_KC (rows of both operands are contiguous in k, so a panel is read in 256-byte runs), wavefront w
// owns columns [16 w, 16 w + 16) of the tile and walks its four 16 x 16 row blocks with the R operand held in a register.
//
// The bits of an entry depend on its two environments alone: every output goes through the same instruction sequence — K in chunks of
// four, ascending, one v_mfma_f64_16x16x4_f64 per chunk, the last chunk zero-padded — whatever the shape of the request, the position
// of the entry in it or the order of the output.  There is no split of K, no atomic and no separate arithmetic for small shapes: rows
// and columns beyond the request are zero operands of the same instructions.
//
// Operand roles as in wg_product above: first operand = R (lane: c = lane & 15, k = lane >> 4), second = L (lane: r = lane & 15,
// k = lane >> 4), acc[reg] = out[r = lane & 15][c = (lane >> 4) + 4 reg].  The LDS rows are PAIR_KC + 2 doubles apart: the 32 lanes of
// a half-wavefront (16 rows, two k) then read 32 different 8-byte banks.
constexpr int PAIR_TILE = 64;
constexpr int PAIR_KC = 32;
constexpr int PAIR_LDS_LD = PAIR_KC + 2;

__global__ void __launch_bounds__(256) contraction_pair_kernel(const double* __restrict__ L, int n_rows, const double* __restrict__ R,
                                                               int n_cols, int K, double* __restrict__ out, size_t ld, int transposed)
{
    __shared__ double Ls[PAIR_TILE * PAIR_LDS_LD];
    __shared__ double Rs[PAIR_TILE * PAIR_LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int r0 = blockIdx.x * PAIR_TILE, c0 = blockIdx.y * PAIR_TILE;
    double4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += PAIR_KC) {
        for (int e = tid; e < PAIR_TILE * PAIR_KC; e += 256) {
            const int row = e / PAIR_KC, kk = e % PAIR_KC;
            const bool k_ok = k0 + kk < K;
            Ls[row * PAIR_LDS_LD + kk] = (k_ok && r0 + row < n_rows) ? L[(size_t)(r0 + row) * K + k0 + kk] : 0.0;
            Rs[row * PAIR_LDS_LD + kk] = (k_ok && c0 + row < n_cols) ? R[(size_t)(c0 + row) * K + k0 + kk] : 0.0;
        }
        __syncthreads();
        const int kend = min(PAIR_KC, K - k0); // (chunks behind the last one that holds an element of K are not issued)
        for (int kk = 0; kk < kend; kk += 4) {
            const double rv = Rs[(16 * wave + lr) * PAIR_LDS_LD + kk + lk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double lv = Ls[(16 * t + lr) * PAIR_LDS_LD + kk + lk];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(rv, lv, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = r0 + 16 * t + lr, c = c0 + 16 * wave + lk + 4 * reg;
            if (r < n_rows && c < n_cols) out[transposed ? (size_t)c + ld * r : (size_t)r + ld * c] = acc[t][reg];
        }
}

} // namespace

void contraction_pair_launch(const double* d_left, int n_rows, const double* d_right, int n_cols, int K, double* d_out, size_t ld,
                             bool transposed, hipStream_t stream)
{
    if (n_rows <= 0 || n_cols <= 0 || K <= 0) return;
    const dim3 grid((unsigned)((n_rows + PAIR_TILE - 1) / PAIR_TILE), (unsigned)((n_cols + PAIR_TILE - 1) / PAIR_TILE));
    hipLaunchKernelGGL(contraction_pair_kernel, grid, dim3(256), 0, stream, d_left, n_rows, d_right, n_cols, K, d_out, ld,
                       transposed ? 1 : 0);
}

void contraction_env_left_launch(const ContractionSiteDesc* d_sites, int n_walk, const uint32_t* d_idx, int n_items, double* d_out, int ld,
                                 int env_cap, int t_cap, double* d_scratch, int blocks, hipStream_t stream)
{
    if (n_items <= 0 || n_walk <= 0 || blocks <= 0) return;
    const size_t lds = d_scratch ? 0 : ((size_t)2 * env_cap + t_cap) * sizeof(double);
    hipLaunchKernelGGL(contraction_env_left_kernel, dim3(std::min(blocks, n_items)), dim3(256), lds, stream, d_sites, n_walk, d_idx,
                       n_items, d_out, ld, env_cap, t_cap, d_scratch);
}

void contraction_env_right_launch(const ContractionSiteDesc* d_sites, int n_sites, int first, const uint32_t* d_idx, int n_items,
                                  double* d_out, int ld, int env_cap, int t_cap, double* d_scratch, int blocks, hipStream_t stream)
{
    if (n_items <= 0 || first >= n_sites || blocks <= 0) return;
    const size_t lds = d_scratch ? 0 : ((size_t)2 * env_cap + t_cap) * sizeof(double);
    hipLaunchKernelGGL(contraction_env_right_kernel, dim3(std::min(blocks, n_items)), dim3(256), lds, stream, d_sites, n_sites, first,
                       d_idx, n_items, d_out, ld, env_cap, t_cap, d_scratch);
}

} // namespace t4a
