// kernels_partial.hip — the local products of the partial contraction of two MPOs (mpo.hpp: mpo_partial_contract).  At a site the
// legs of A[a, x0, x1, a'] and B[b, y0, y1, b'] fall into three fused groups (first leg fastest, an empty group has dimension 1):
//   s: the legs of A in no contract pair     kappa: the contract pairs     t: the legs of B in no pair
// and a leg of B that is diagonally paired takes its value from s.  Both kernels address a site through the bond stride times a
// fused-site-index offset that is linear in the (at most two) legs of every group,
//   fA(s, kappa) = (s % s0) as0 + (s / s0) as1 + (kappa % k0) ak0 + (kappa / k0) ak1
//   fB(s, kappa, t) = (s % s0) bs0 + (s / s0) bs1 + (kappa % k0) bk0 + (kappa / k0) bk1 + (t % t0) bt0 + (t / t0) bt1
// (s0, k0, t0: the dimension of the first leg of the group), so nothing is packed or permuted first and no copy tensor is multiplied
// into A: a diagonal pair is a non-zero bs0 / bs1.
//
// 1. mpo_partial_site_kernel: every site of the chain in ONE launch, ragged like mpo_site_contract_kernel (kernels_mpo.hip), one
//    output element per thread, kappa ascending, multiply and add rounded separately (the file is built with -ffp-contract=off):
//      C[(a Lb + b), s, t, (a' Rb + b')] = sum_kappa A[a, fA(s, kappa), a'] * B[b, fB(s, kappa, t), b']
//    On the matrix-product plan this is the chain of operations of mpo_site_contract_kernel, so the bits are its bits.
//
// 2. mpo_partial_half_kernel: the half product of zip-up and fit for a plan,
//      out[n, s, t, c, d] = sum_kappa sum_b ( sum_a E[n, a, b] A[a, fA(s, kappa), c] ) B[b, fB(s, kappa, t), d]
//    and its right-hand mirror through other strides.  It is the sibling of mpo_fit_half_kernel (kernels_mpo_fit.hip) and keeps what
//    that file documents: a workgroup owns one s, 16 values of n, 16 of c and 48 of the fused column index j = t + T d; the inner
//    sum X is formed for one kappa and a panel of 8 values of b in 16 KiB of LDS and never goes to global memory; a 16 x 16 tile
//    of either product that lies inside its matrix runs on the f64 matrix cores (v_mfma_f64_16x16x4_f64, summed index in chunks of
//    four ascending), every ragged or small tile is one element per thread with the summed index ascending; no summed index is
//    split across workgroups and nothing is added atomically, so two runs give the same bits; the output is written once, in the
//    layout the SVD (zip-up) or the GEMM (fit) behind it reads.  Because a workgroup owns one s, the value a diagonal leg of B takes
//    is uniform over the workgroup: it moves the base pointer of B and costs nothing in the loops.  On the matrix-product plan the
//    operation chain is that of mpo_fit_half_kernel, which keeps its own code and callers.  Two things differ from that kernel in how
//    operands are fetched, not in what is added: the first product loads the operands of four chunks of a before it issues their four
//    matrix-core steps (the one-chunk loop waits for two dependent global loads per step: 156 us against 84 us for a 128 x 64 x 64
//    environment at a 32 x 32 output bond pair), and the operand of B of the second product is loaded before the
//    first product of the same panel runs.  Nothing is packed or permuted before the launch.
#include "kernels.hpp"

#include <algorithm>
#include <climits>

namespace t4a {

namespace {

__global__ void __launch_bounds__(256) mpo_partial_site_kernel(const MpoPartialSiteJob* __restrict__ jobs, int n_jobs,
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
        const MpoPartialSiteJob& j = jobs[lo];
        // every site's input and output holds at most INT_MAX elements (checked on the host)
        int q = (int)(e - j.off);
        const int Lc = j.la * j.lb;
        const int row = q % Lc;
        q /= Lc;
        const int s = q % j.S;
        q /= j.S;
        const int t = q % j.T;
        const int col = q / j.T;
        const int ia = row / j.lb, ib = row % j.lb;
        const int ra = col / j.rb, rb = col % j.rb;
        const int fa = (s % j.s0) * j.as0 + (s / j.s0) * j.as1;
        const int fb = (s % j.s0) * j.bs0 + (s / j.s0) * j.bs1 + (t % j.t0) * j.bt0 + (t / j.t0) * j.bt1;
        // A[ia, f, ra] at ia + La (f + FA ra); B[ib, f, rb] at ib + Lb (f + FB rb)
        const double* a = j.A + ia + (long long)j.la * (fa + (long long)j.FA * ra);
        const double* b = j.B + ib + (long long)j.lb * (fb + (long long)j.FB * rb);
        double acc = 0.0;
        for (int k = 0; k < j.K; ++k) {
            const int k0 = k % j.k0, k1 = k / j.k0;
            acc = acc + a[(long long)j.la * (k0 * j.ak0 + k1 * j.ak1)] * b[(long long)j.lb * (k0 * j.bk0 + k1 * j.bk1)];
        }
        j.C[e - j.off] = acc;
    }
}

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int PH_TN = 16;             // values of n per workgroup (the rows of every tile)
constexpr int PH_TC = 16;             // values of c per workgroup
constexpr int PH_PB = 8;              // values of b per panel of X
constexpr int PH_JT = 3;              // 16-column tiles of j = t + T d per workgroup
constexpr int PH_JW = 16 * PH_JT;     // columns per workgroup
constexpr int PH_THREADS = 256;       // four wavefronts; wavefront w owns c = 4 w .. 4 w + 3 in the second product
constexpr int PH_XC = PH_PB * PH_TN;  // X[nn + 16 bb + 128 cc]
constexpr int PH_UA = 4;              // chunks of four values of a whose loads the first product issues together

// offset of column j = t + T d of B, without the bond index b and the parts that s and kappa fix
__device__ __forceinline__ long long ph_bcol(const MpoPartialHalfDesc& d, int j)
{
    const int t = j % d.T, dd = j / d.T;
    return (long long)(t % d.t0) * d.bt0 + (long long)(t / d.t0) * d.bt1 + (long long)dd * d.bd;
}
// offset of column j of the output
__device__ __forceinline__ long long ph_ocol(const MpoPartialHalfDesc& d, int j)
{
    return (long long)(j % d.T) * d.ot + (long long)(j / d.T) * d.od;
}

// NFULL: all 16 rows n of the workgroup are inside N.  Then full column tiles run on the cores and only the ragged last tile (at
// most 15 columns) is summed per thread; otherwise all (at most 48) columns are.  The per-thread sums of a thread are the columns
// js0 .. jv-1 of its one (n, c) = (tid & 15, tid >> 4).
template <bool NFULL>
__device__ __forceinline__ void partial_half_body(const MpoPartialHalfDesc& d, double* X, int s, int n0, int nv, int c0, int cv, int j0,
                                                  int jv)
{
    constexpr int SJ = NFULL ? 16 : PH_JW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int jfull = NFULL ? (jv >> 4) : 0;
    const int js0 = jfull << 4;
    const bool c_full = cv == PH_TC;
    const int nn = tid & 15, cc_own = tid >> 4;
    const bool own_ok = nn < nv && cc_own < cv && js0 < jv;

    double4_t acc[4][PH_JT];
    double sacc[SJ];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int jt = 0; jt < PH_JT; ++jt) acc[ci][jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int jj = 0; jj < SJ; ++jj) sacc[jj] = 0.0;

    // s is uniform over the workgroup: the S legs of A, and the legs of B that are diagonally paired with them, move the bases
    const int sl = s % d.s0, sh = s / d.s0;
    const double* As = d.A + (long long)sl * d.as0 + (long long)sh * d.as1;
    const double* Bs = d.B + (long long)sl * d.bs0 + (long long)sh * d.bs1;
    // the columns of B this lane feeds to the cores, one per full tile
    long long bcol[PH_JT];
#pragma unroll
    for (int jt = 0; jt < PH_JT; ++jt) bcol[jt] = jt < jfull ? ph_bcol(d, j0 + (jt << 4) + lr) : 0;

    for (int k = 0; k < d.K; ++k) {
        const int kl = k % d.k0, kh = k / d.k0;
        const double* Ak = As + (long long)kl * d.ak0 + (long long)kh * d.ak1;
        const double* Bk = Bs + (long long)kl * d.bk0 + (long long)kh * d.bk1;
        for (int b0 = 0; b0 < d.Lb; b0 += PH_PB) {
            const int pb = min(PH_PB, d.Lb - b0);
            // the operand of B this lane feeds to the cores in the second product of this panel: loaded here, so that the loads are
            // in flight while the first product runs (zeros for b past the panel)
            double bq[PH_JT][PH_PB / 4];
            if (NFULL) {
#pragma unroll
                for (int jt = 0; jt < PH_JT; ++jt)
#pragma unroll
                    for (int h = 0; h < PH_PB / 4; ++h) {
                        const int bb = 4 * h + lk;
                        bq[jt][h] = jt < jfull && bb < pb ? Bk[bcol[jt] + (long long)(b0 + bb) * d.bb] : 0.0;
                    }
            }
            // ---- first product: X[nn, cc, bb] = sum_a E[n0 + nn, a, b0 + bb] A[a, fA(s, k), c0 + cc]; zeros outside N, C, Lb
            if (NFULL && c_full) {
                // MFMA operand roles as in kernels_mpo_fit.hip: first operand indexed by the column (cc = lane & 15), second by the
                // row (nn = lane & 15), both at summed index lane >> 4; x[reg] = X[nn = lane & 15][cc = (lane >> 4) + 4 reg]
                for (int bb = wave; bb < PH_PB; bb += 4) {
                    double4_t x = (double4_t){0.0, 0.0, 0.0, 0.0};
                    if (bb < pb) {
                        const double* e = d.E + (long long)(n0 + lr) * d.en + (long long)(b0 + bb) * d.eb;
                        const double* a = Ak + (long long)(c0 + lr) * d.ac;
                        // four chunks of a per trip: their eight loads are in flight together, the matrix-core steps then run in
                        // the ascending order of the one-chunk loop (a chunk wholly past La is not issued, as there)
                        for (int a0 = 0; a0 < d.La; a0 += 4 * PH_UA) {
                            double pv[PH_UA], qv[PH_UA];
#pragma unroll
                            for (int u = 0; u < PH_UA; ++u) {
                                const int ai = a0 + 4 * u + lk;
                                const bool ok = ai < d.La;
                                pv[u] = ok ? e[(long long)ai * d.ea] : 0.0;
                                qv[u] = ok ? a[(long long)ai * d.aa] : 0.0;
                            }
#pragma unroll
                            for (int u = 0; u < PH_UA; ++u)
                                if (a0 + 4 * u < d.La) x = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[u], pv[u], x, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) X[(lk + 4 * reg) * PH_XC + bb * PH_TN + lr] = x[reg];
                }
            } else {
                for (int e = tid; e < PH_TC * PH_XC; e += PH_THREADS) {
                    const int xn = e & 15, bb = (e >> 4) % PH_PB, xc = e / PH_XC;
                    double v = 0.0;
                    if (xn < nv && xc < cv && bb < pb) {
                        const double* ep = d.E + (long long)(n0 + xn) * d.en + (long long)(b0 + bb) * d.eb;
                        const double* ap = Ak + (long long)(c0 + xc) * d.ac;
                        for (int ai = 0; ai < d.La; ++ai) {
                            const double prod = ep[(long long)ai * d.ea] * ap[(long long)ai * d.aa];
                            v = v + prod;
                        }
                    }
                    X[e] = v;
                }
            }
            __syncthreads();
            // ---- second product on the cores: out[nn, (cc), j] += sum_bb X[nn, cc, bb] B[b0 + bb, fB(s, k, t(j)), d(j)]
            if (NFULL) {
#pragma unroll
                for (int jt = 0; jt < PH_JT; ++jt) {
                    if (jt < jfull) {
#pragma unroll
                        for (int h = 0; h < PH_PB / 4; ++h) {
                            if (4 * h < pb) {
                                const int bb = 4 * h + lk; // X holds zeros for bb >= pb
#pragma unroll
                                for (int ci = 0; ci < 4; ++ci) {
                                    const int cc = wave * 4 + ci;
                                    if (cc < cv) {
                                        const double pv = X[cc * PH_XC + bb * PH_TN + lr];
                                        acc[ci][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(bq[jt][h], pv, acc[ci][jt], 0, 0, 0);
                                    }
                                }
                            }
                        }
                    }
                }
            }
            // ---- second product per thread: the columns no full tile covers
            if (own_ok) {
                const double* xp = X + cc_own * PH_XC + nn;
#pragma unroll
                for (int jj = 0; jj < SJ; ++jj) {
                    if (js0 + jj < jv) {
                        const double* bp = Bk + ph_bcol(d, j0 + js0 + jj) + (long long)b0 * d.bb;
                        double v = sacc[jj];
                        for (int bb = 0; bb < pb; ++bb) {
                            const double prod = xp[bb * PH_TN] * bp[(long long)bb * d.bb];
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
        for (int jt = 0; jt < PH_JT; ++jt) {
            if (jt < jfull) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    double* op = os + (long long)(n0 + lr) * d.on + ph_ocol(d, j0 + (jt << 4) + lk + 4 * reg);
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
        for (int jj = 0; jj < SJ; ++jj)
            if (js0 + jj < jv) op[ph_ocol(d, j0 + js0 + jj)] = sacc[jj];
    }
}

__global__ void __launch_bounds__(PH_THREADS) mpo_partial_half_kernel(const MpoPartialHalfDesc d)
{
    __shared__ __attribute__((aligned(16))) double X[PH_TC * PH_XC];
    // workgroup -> (n tile, c tile, s, column group), n fastest
    const int nt = (d.N + PH_TN - 1) / PH_TN, ct = (d.C + PH_TC - 1) / PH_TC;
    unsigned blk = blockIdx.x;
    const int in = (int)(blk % (unsigned)nt);
    blk /= (unsigned)nt;
    const int ic = (int)(blk % (unsigned)ct);
    blk /= (unsigned)ct;
    const int s = (int)(blk % (unsigned)d.S);
    const int ig = (int)(blk / (unsigned)d.S);
    const int n0 = in * PH_TN, c0 = ic * PH_TC, j0 = ig * PH_JW;
    const int nv = min(PH_TN, d.N - n0), cv = min(PH_TC, d.C - c0), jv = min(PH_JW, d.T * d.D - j0);
    if (nv == PH_TN) partial_half_body<true>(d, X, s, n0, nv, c0, cv, j0, jv);
    else partial_half_body<false>(d, X, s, n0, nv, c0, cv, j0, jv);
}

} // namespace

void mpo_partial_site_launch(const MpoPartialSiteJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream)
{
    if (n_jobs <= 0 || total == 0) return;
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(mpo_partial_site_kernel, dim3(blocks), dim3(256), 0, stream, d_jobs, n_jobs, total);
}

bool mpo_partial_half_launch(const MpoPartialHalfDesc& d, hipStream_t stream)
{
    if (d.N <= 0 || d.La <= 0 || d.Lb <= 0 || d.S <= 0 || d.K <= 0 || d.T <= 0 || d.C <= 0 || d.D <= 0) return true; // nothing to write
    if (d.s0 <= 0 || d.k0 <= 0 || d.t0 <= 0) return false;
    const unsigned long long nt = (d.N + PH_TN - 1) / PH_TN, ct = (d.C + PH_TC - 1) / PH_TC;
    const unsigned long long jg = ((unsigned long long)d.T * d.D + PH_JW - 1) / PH_JW;
    const unsigned long long blocks = nt * ct * (unsigned long long)d.S * jg; // each factor < 2^32 and the first three <= out size
    if ((unsigned long long)d.T * d.D > INT_MAX || blocks > INT_MAX) return false;
    hipLaunchKernelGGL(mpo_partial_half_kernel, dim3((unsigned)blocks), dim3(PH_THREADS), 0, stream, d);
    return true;
}

} // namespace t4a
