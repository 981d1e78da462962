// kernels_mpo_fit.hip — the half product of the variational fit of an MPO-MPO product (mpo_fit.hip): an environment of A·B against
// the fitted MPO, times one site of A and one site of B, in ONE launch and without a permutation before or behind it:
//   out[n, s, t, c, d] = sum_{k < K} sum_{b < Lb} X[n, c, k, b] * B[b, k, t, d],     X[n, c, k, b] = sum_{a < La} E[n, a, b] * A[a, s, k, c]
// Every operand and the output are addressed through element strides (MpoFitHalfDesc), so the left half product P_i (E = L_i, natural
// strides) and the right half product Q_i (E = R_{i+1}, the bond strides of both sites exchanged, output written as [a, b, s, t, c'])
// are the same kernel, and the output lands in the layout the following GEMM reads.
//
// A workgroup owns one s, 16 values of n, 16 values of c and 48 values of the fused column index j = t + T d.  The inner sum X never goes
// to global memory: it is formed for one k and a panel of 8 values of b at a time, [16 n][16 c][8 b] doubles = 16 KiB of LDS (well
// inside the 64 KiB a workgroup gets without opting in), consumed by the second product, and overwritten by the next panel.  The
// output accumulates in registers over all K * ceil(Lb / 8) panels and is written once.  No summed index is split across workgroups,
// nothing is accumulated with atomics: an output element is one fixed chain of operations, k outer, b and a ascending, so two runs
// give the same bits.
//
// Which arithmetic a product takes is decided per 16 x 16 tile of its OUTPUT (as in kernels_contraction.hip, but an edge tile is not
// padded onto the cores):
//   first product, tile [16 n] x [16 c] of X at one (k, b):   all 16 n and all 16 c inside N and C
//       -> f64 matrix cores (v_mfma_f64_16x16x4_f64), a in chunks of four ascending, the last chunk zero-padded in registers;
//   second product, tile [16 n] x [16 j] of out at one (s, c): all 16 n and all 16 j inside N and T D
//       -> f64 matrix cores, b in chunks of four ascending inside a panel (values of b past Lb are zeros);
//   every other tile (N, C or T D below 16, and the ragged last tile of each) -> one element per thread, summed index ascending,
//       multiply and add rounded separately (the file is built with -ffp-contract=off), as in kernels_mpo.hip.
// So a call whose N is 17 runs rows 0 .. 15 on the cores and row 16 per thread; bonds below 16 never touch the cores.
// A first version, not tuned: an MFMA operand element is one load per lane and instruction (B straight from global memory, reused
// over the four values of c a wavefront owns), and X is recomputed for every 48 columns of (t, d).
#include "kernels.hpp"

#include <algorithm>
#include <climits>

namespace t4a {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int FIT_TN = 16;             // values of n per workgroup (the rows of every tile)
constexpr int FIT_TC = 16;             // values of c per workgroup
constexpr int FIT_PB = 8;              // values of b per panel of X
constexpr int FIT_JT = 3;              // 16-column tiles of j = t + T d per workgroup
constexpr int FIT_JW = 16 * FIT_JT;    // columns per workgroup
constexpr int FIT_THREADS = 256;       // four wavefronts; wavefront w owns c = 4 w .. 4 w + 3 in the second product
constexpr int FIT_XC = FIT_PB * FIT_TN; // X[nn + 16 bb + 128 cc]

// NFULL: all 16 rows n of the workgroup are inside N.  Then full column tiles run on the cores and only the ragged last tile (at
// most 15 columns) is summed per thread; otherwise all (at most 48) columns are.  The per-thread sums of a thread are the columns
// js0 .. jv-1 of its one (n, c) = (tid & 15, tid >> 4).
template <bool NFULL>
__device__ __forceinline__ void fit_half_body(const MpoFitHalfDesc& d, double* X, int s, int n0, int nv, int c0, int cv, int j0, int jv)
{
    constexpr int SJ = NFULL ? 16 : FIT_JW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int jfull = NFULL ? (jv >> 4) : 0;
    const int js0 = jfull << 4;
    const bool c_full = cv == FIT_TC;
    const int nn = tid & 15, cc_own = tid >> 4;
    const bool own_ok = nn < nv && cc_own < cv && js0 < jv;

    double4_t acc[4][FIT_JT];
    double sacc[SJ];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int jt = 0; jt < FIT_JT; ++jt) acc[ci][jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int jj = 0; jj < SJ; ++jj) sacc[jj] = 0.0;

    const double* As = d.A + (long long)s * d.as;
    for (int k = 0; k < d.K; ++k) {
        for (int b0 = 0; b0 < d.Lb; b0 += FIT_PB) {
            const int pb = min(FIT_PB, d.Lb - b0);
            // ---- first product: X[nn, cc, bb] = sum_a E[n0 + nn, a, b0 + bb] A[a, s, k, c0 + cc]; zeros outside N, C, Lb
            if (NFULL && c_full) {
                // MFMA operand roles as in kernels_contraction.hip: first operand indexed by the column (cc = lane & 15), second by the
                // row (nn = lane & 15), both at summed index lane >> 4; x[reg] = X[nn = lane & 15][cc = (lane >> 4) + 4 reg]
                for (int bb = wave; bb < FIT_PB; bb += 4) {
                    double4_t x = (double4_t){0.0, 0.0, 0.0, 0.0};
                    if (bb < pb) {
                        const double* e = d.E + (long long)(n0 + lr) * d.en + (long long)(b0 + bb) * d.eb;
                        const double* a = As + (long long)k * d.ak + (long long)(c0 + lr) * d.ac;
                        for (int a0 = 0; a0 < d.La; a0 += 4) {
                            const int ai = a0 + lk;
                            const bool ok = ai < d.La;
                            const double pv = ok ? e[(long long)ai * d.ea] : 0.0;
                            const double qv = ok ? a[(long long)ai * d.aa] : 0.0;
                            x = __builtin_amdgcn_mfma_f64_16x16x4f64(qv, pv, x, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) X[(lk + 4 * reg) * FIT_XC + bb * FIT_TN + lr] = x[reg];
                }
            } else {
                for (int e = tid; e < FIT_TC * FIT_XC; e += FIT_THREADS) {
                    const int xn = e & 15, bb = (e >> 4) % FIT_PB, xc = e / FIT_XC;
                    double v = 0.0;
                    if (xn < nv && xc < cv && bb < pb) {
                        const double* ep = d.E + (long long)(n0 + xn) * d.en + (long long)(b0 + bb) * d.eb;
                        const double* ap = As + (long long)k * d.ak + (long long)(c0 + xc) * d.ac;
                        for (int ai = 0; ai < d.La; ++ai) {
                            const double prod = ep[(long long)ai * d.ea] * ap[(long long)ai * d.aa];
                            v = v + prod;
                        }
                    }
                    X[e] = v;
                }
            }
            __syncthreads();
            // ---- second product on the cores: out[nn, (cc), j] += sum_bb X[nn, cc, bb] B[b0 + bb, k, t(j), d(j)]
            if (NFULL) {
#pragma unroll
                for (int jt = 0; jt < FIT_JT; ++jt) {
                    if (jt < jfull) {
                        const int j = j0 + (jt << 4) + lr;
                        const double* bp = d.B + (long long)k * d.bk + (long long)(j % d.T) * d.bt + (long long)(j / d.T) * d.bd;
                        for (int x0 = 0; x0 < pb; x0 += 4) {
                            const int bb = x0 + lk; // X holds zeros for bb >= pb
                            const double qv = bb < pb ? bp[(long long)(b0 + bb) * d.bb] : 0.0;
#pragma unroll
                            for (int ci = 0; ci < 4; ++ci) {
                                const int cc = wave * 4 + ci;
                                if (cc < cv) {
                                    const double pv = X[cc * FIT_XC + bb * FIT_TN + lr];
                                    acc[ci][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv, pv, acc[ci][jt], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
            }
            // ---- second product per thread: the columns no full tile covers
            if (own_ok) {
                const double* xp = X + cc_own * FIT_XC + nn;
#pragma unroll
                for (int jj = 0; jj < SJ; ++jj) {
                    if (js0 + jj < jv) {
                        const int j = j0 + js0 + jj;
                        const double* bp = d.B + (long long)k * d.bk + (long long)(j % d.T) * d.bt + (long long)(j / d.T) * d.bd +
                                           (long long)b0 * d.bb;
                        double v = sacc[jj];
                        for (int bb = 0; bb < pb; ++bb) {
                            const double prod = xp[bb * FIT_TN] * bp[(long long)bb * d.bb];
                            v = v + prod;
                        }
                        sacc[jj] = v;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- the output, written once
    double* os = d.out + (long long)s * d.os;
    if (NFULL) {
#pragma unroll
        for (int jt = 0; jt < FIT_JT; ++jt) {
            if (jt < jfull) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = j0 + (jt << 4) + lk + 4 * reg;
                    double* op = os + (long long)(n0 + lr) * d.on + (long long)(j % d.T) * d.ot + (long long)(j / d.T) * d.od;
#pragma unroll
                    for (int ci = 0; ci < 4; ++ci) {
                        const int cc = wave * 4 + ci;
                        if (cc < cv) op[(long long)(c0 + cc) * d.oc] = acc[ci][jt][reg];
                    }
                }
            }
        }
    }
    if (own_ok) {
        double* op = os + (long long)(n0 + nn) * d.on + (long long)(c0 + cc_own) * d.oc;
#pragma unroll
        for (int jj = 0; jj < SJ; ++jj) {
            if (js0 + jj < jv) {
                const int j = j0 + js0 + jj;
                op[(long long)(j % d.T) * d.ot + (long long)(j / d.T) * d.od] = sacc[jj];
            }
        }
    }
}

__global__ void __launch_bounds__(FIT_THREADS) mpo_fit_half_kernel(const MpoFitHalfDesc d)
{
    __shared__ __attribute__((aligned(16))) double X[FIT_TC * FIT_XC];
    // workgroup -> (n tile, c tile, s, column group), n fastest
    const int nt = (d.N + FIT_TN - 1) / FIT_TN, ct = (d.C + FIT_TC - 1) / FIT_TC;
    unsigned blk = blockIdx.x;
    const int in = (int)(blk % (unsigned)nt);
    blk /= (unsigned)nt;
    const int ic = (int)(blk % (unsigned)ct);
    blk /= (unsigned)ct;
    const int s = (int)(blk % (unsigned)d.S);
    const int ig = (int)(blk / (unsigned)d.S);
    const int n0 = in * FIT_TN, c0 = ic * FIT_TC, j0 = ig * FIT_JW;
    const int nv = min(FIT_TN, d.N - n0), cv = min(FIT_TC, d.C - c0), jv = min(FIT_JW, d.T * d.D - j0);
    if (nv == FIT_TN) fit_half_body<true>(d, X, s, n0, nv, c0, cv, j0, jv);
    else fit_half_body<false>(d, X, s, n0, nv, c0, cv, j0, jv);
}

} // namespace

bool mpo_fit_half_launch(const MpoFitHalfDesc& d, hipStream_t stream)
{
    if (d.N <= 0 || d.La <= 0 || d.Lb <= 0 || d.S <= 0 || d.K <= 0 || d.T <= 0 || d.C <= 0 || d.D <= 0) return true; // nothing to write
    const unsigned long long nt = (d.N + FIT_TN - 1) / FIT_TN, ct = (d.C + FIT_TC - 1) / FIT_TC;
    const unsigned long long jg = ((unsigned long long)d.T * d.D + FIT_JW - 1) / FIT_JW;
    const unsigned long long blocks = nt * ct * (unsigned long long)d.S * jg; // each factor < 2^32 and the first three <= out size
    if ((unsigned long long)d.T * d.D > INT_MAX || blocks > INT_MAX) return false;
    hipLaunchKernelGGL(mpo_fit_half_kernel, dim3((unsigned)blocks), dim3(FIT_THREADS), 0, stream, d);
    return true;
}

} // namespace t4a
