// kernels_tdvp.hip — the projections of a Gram–Schmidt pass for short vectors with many basis vectors: what the Krylov exponential of a
// TDVP step (tdvp.hpp) launches where gs_dots of kernels_linsolve.hip would leave the card idle.  A one-site region holds chi d chi
// elements (2048 at chi = 32): gs_workgroups gives it 2 workgroups, each of which walks all nb basis vectors one after the other.
// gs_dots_wide spreads the basis over a second grid dimension: workgroup (g, y) handles the GS_WIDE vectors from GS_WIDE y of element
// group g in ONE pass over the elements, w read once and kept in a register, GS_WIDE independent accumulators per thread.
// The partition and the order of every sum are those of gs_dots: thread t of element group g owns g*256 + t + k*(256*G), summed
// k-ascending, G = gs_workgroups(len); lanes by the fixed shuffle tree, the four waves ((s0 + s1) + s2) + s3.  Each part[i + nb g] is
// the same chain of separately rounded multiplies and adds (-ffp-contract=off), hence the same bits; no atomics.
//
// tdvp_bond_apply_kernel — the bond-centre (zero-site) apply of one-site TDVP in ONE launch:
//   Y[b, b'] = sum_w sum_a sum_a' La[b, w, a] C[a, a'] Rb[b', w, a'],   La[k_a, W, k_a], Rb[k_b, W, k_b], C and Y k_a x k_b (column-major).
// A workgroup owns BOND_TILE = 16 rows b.  Stage 1 forms T[b, j] = sum_a La[b, w, a] C[a, a'] for its rows and every j = w + W a' into the
// LDS (16 W k_b doubles: the envelope of the launch is W k_b <= 512, 64 KiB); stage 2 is Y[b, b'] = sum_j T[b, j] Rb[b', j], Rb read as the
// k_b x (W k_b) matrix it is in memory.  No workgroup reads another one's T, so nothing but the LDS carries the intermediate.
// Arithmetic, as in kernels_gse.hip: from k_a, k_b >= 16 a wavefront owns a 16 x 16 tile at a time on v_mfma_f64_16x16x4_f64, the summed
// index in chunks of four, ascending, edge tiles and the last chunk zero-padded in registers; below, one element per thread, the summed
// index ascending.  The operands of BOND_DEPTH chunks are loaded per trip with indices clamped into the operand (the value replaced by
// zero afterwards), so that the loads are unconditional and their latencies overlap; a chunk past the end adds zeros.
// The order of every sum is fixed by its output element and the shape: the same bits on every run and for every grid.
#include "krylov_reduce.hpp"
#include "tdvp.hpp"

#include <climits>
#include <string>

namespace t4a {

typedef double bond_double4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr int BOND_TILE = 16, BOND_THREADS = 256, BOND_DEPTH = 8;

__global__ void __launch_bounds__(BOND_THREADS) tdvp_bond_apply_kernel(const double* __restrict__ La, const double* __restrict__ C, const double* __restrict__ Rb,
                                                                      double* __restrict__ Y, int ka, int kb, int W, int mfma)
{
    extern __shared__ double T[]; // T[row + 16 j], j = w + W a' < W kb
    const int tid = threadIdx.x, m0 = (int)blockIdx.x * BOND_TILE;
    const int J = W * kb;
    const long long lda = (long long)ka * W; // La[b + ka w + lda a]
    if (mfma) {
        const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
        const int row = m0 + lr;
        const bool row_ok = row < ka;
        const int nct = (kb + 15) >> 4;
        // operand roles as in kernels_gse.hip: first operand indexed by the output column, second by the output row,
        // acc[reg] = out[row = lane & 15][col = (lane >> 4) + 4 reg]
        for (int t = wave; t < W * nct; t += BOND_THREADS / 64) {
            const int w = t % W, ct = t / W;
            const int c = (ct << 4) + lr;
            const bool c_ok = c < kb;
            const double* Lw = La + (long long)ka * w;
            bond_double4_t acc = (bond_double4_t){0.0, 0.0, 0.0, 0.0};
            // BOND_DEPTH chunks of four per trip: the loads are unconditional (indices clamped into the operand, the value
            // replaced by zero afterwards), so that they are issued together and their latencies overlap
            const int rowc = min(row, ka - 1), cc0 = min(c, kb - 1);
            for (int k0 = 0; k0 < ka; k0 += 4 * BOND_DEPTH) {
                double xv[BOND_DEPTH], yv[BOND_DEPTH];
#pragma unroll
                for (int u = 0; u < BOND_DEPTH; ++u) {
                    const int kc = min(k0 + 4 * u + lk, ka - 1);
                    xv[u] = Lw[rowc + lda * kc];
                    yv[u] = C[kc + (long long)ka * cc0];
                }
#pragma unroll
                for (int u = 0; u < BOND_DEPTH; ++u) {
                    const bool k_ok = k0 + 4 * u + lk < ka; // a chunk past the end adds zeros: the sum does not change
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((c_ok && k_ok) ? yv[u] : 0.0, (row_ok && k_ok) ? xv[u] : 0.0, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int cc = (ct << 4) + lk + 4 * reg;
                if (cc < kb) T[lr + BOND_TILE * (w + W * cc)] = acc[reg]; // rows past ka hold zeros
            }
        }
        __syncthreads();
        for (int ct = wave; ct < nct; ct += BOND_THREADS / 64) {
            const int c = (ct << 4) + lr;
            const bool c_ok = c < kb;
            bond_double4_t acc = (bond_double4_t){0.0, 0.0, 0.0, 0.0};
            const int cc0 = min(c, kb - 1);
            for (int j0 = 0; j0 < J; j0 += 4 * BOND_DEPTH) {
                double xv[BOND_DEPTH], yv[BOND_DEPTH];
#pragma unroll
                for (int u = 0; u < BOND_DEPTH; ++u) {
                    const int jc = min(j0 + 4 * u + lk, J - 1);
                    xv[u] = T[lr + BOND_TILE * jc];
                    yv[u] = Rb[cc0 + (long long)kb * jc];
                }
#pragma unroll
                for (int u = 0; u < BOND_DEPTH; ++u) {
                    const bool j_ok = j0 + 4 * u + lk < J;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((c_ok && j_ok) ? yv[u] : 0.0, j_ok ? xv[u] : 0.0, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int cc = (ct << 4) + lk + 4 * reg;
                if (row_ok && cc < kb) Y[row + (long long)ka * cc] = acc[reg];
            }
        }
    } else {
        for (int e = tid; e < BOND_TILE * J; e += BOND_THREADS) {
            const int row = m0 + (e & (BOND_TILE - 1)), j = e / BOND_TILE;
            const int w = j % W, c = j / W;
            double s = 0.0;
            if (row < ka)
                for (int k = 0; k < ka; ++k) s = s + La[row + (long long)ka * w + lda * k] * C[k + (long long)ka * c];
            T[e] = s;
        }
        __syncthreads();
        for (int e = tid; e < BOND_TILE * kb; e += BOND_THREADS) {
            const int r = e & (BOND_TILE - 1), c = e / BOND_TILE, row = m0 + r;
            if (row >= ka) continue;
            double s = 0.0;
            for (int j = 0; j < J; ++j) s = s + T[r + BOND_TILE * j] * Rb[c + (long long)kb * j];
            Y[row + (long long)ka * c] = s;
        }
    }
}

// part[i + nb g] = sum over the elements of element group g = blockIdx.x of V[e + ld i] w[e], for the vectors i of blockIdx.y
__global__ void __launch_bounds__(256) gs_dots_wide_kernel(const double* __restrict__ V, long long ld, int nb, const double* __restrict__ w,
                                                           long long len, double* __restrict__ part)
{
    __shared__ double sred[4][GS_WIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = (int)blockIdx.y * GS_WIDE;
    const int nv = min(GS_WIDE, nb - i0); // >= 1: the grid has ceil(nb / GS_WIDE) rows
    const long long first = (long long)blockIdx.x * GS_THREADS + tid, stride = (long long)gridDim.x * GS_THREADS;
    const double* v0 = V + ld * i0;
    double acc[GS_WIDE];
#pragma unroll
    for (int ii = 0; ii < GS_WIDE; ++ii) acc[ii] = 0.0;
    if (nv == GS_WIDE) {
        for (long long e = first; e < len; e += stride) {
            const double we = w[e];
#pragma unroll
            for (int ii = 0; ii < GS_WIDE; ++ii) acc[ii] = acc[ii] + v0[e + ld * ii] * we;
        }
    } else {
        for (long long e = first; e < len; e += stride) {
            const double we = w[e];
#pragma unroll
            for (int ii = 0; ii < GS_WIDE; ++ii)
                if (ii < nv) acc[ii] = acc[ii] + v0[e + ld * ii] * we;
        }
    }
#pragma unroll
    for (int ii = 0; ii < GS_WIDE; ++ii) {
        const double s = wave_sum(acc[ii]);
        if (lane == 0) sred[wave][ii] = s;
    }
    __syncthreads();
    if (tid < nv) part[(i0 + tid) + (long long)nb * blockIdx.x] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}

} // namespace

void gs_dots_wide_launch(const double* V, size_t ld, int nb, const double* w, size_t len, double* part, hipStream_t stream)
{
    if (nb <= 0 || len == 0) return;
    const dim3 grid((unsigned)gs_workgroups(len), (unsigned)((nb + GS_WIDE - 1) / GS_WIDE));
    hipLaunchKernelGGL(gs_dots_wide_kernel, grid, dim3(GS_THREADS), 0, stream, V, (long long)ld, nb, w, (long long)len, part);
}

bool tdvp_bond_apply_fused_admits(size_t ka, size_t kb, size_t W)
{
    if (ka == 0 || kb == 0 || W == 0 || ka > (size_t)INT_MAX || kb > TDVP_BOND_FUSED_MAX_PANEL || W > TDVP_BOND_FUSED_MAX_PANEL) return false;
    return W * kb <= TDVP_BOND_FUSED_MAX_PANEL;
}

void tdvp_bond_apply_launch(const double* La, const double* C, const double* Rb, double* Y, int ka, int kb, int W, hipStream_t stream)
{
    if (!tdvp_bond_apply_fused_admits((size_t)ka, (size_t)kb, (size_t)W))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_bond_apply: the fused launch holds 16 W k_b doubles in the LDS: W k_b must be at most " +
                                                  std::to_string(TDVP_BOND_FUSED_MAX_PANEL));
    const size_t lds = sizeof(double) * BOND_TILE * (size_t)W * (size_t)kb;
    const int mfma = ka >= TDVP_BOND_MFMA_MIN && kb >= TDVP_BOND_MFMA_MIN;
    hipLaunchKernelGGL(tdvp_bond_apply_kernel, dim3((unsigned)((ka + BOND_TILE - 1) / BOND_TILE)), dim3(BOND_THREADS), lds, stream, La, C, Rb, Y, ka, kb, W, mfma);
}

} // namespace t4a
