// kernels_gse.hip — the two launches of an edge of the global subspace expansion (gse.hpp): project, N_j = R_j - (R_j B^T) B stacked
// over the references with the trace sum_j |R_j|_F^2, and absorb, parent_tau <- (parent_tau C_tau) B'^T over the target and the
// references.  Both are the same kernel: a workgroup owns GSE_TILE rows of the first operand of its job, forms T = A_tile M1 into the
// job's scratch (its own rows only: no workgroup reads another one's), and then O_tile = T M2 (or A_tile - T M2).  Every operand is
// addressed by a row and a column stride, so a core is read in place in either orientation.
//
// Arithmetic, chosen per job by the launcher (mfma): bonds below GSE_MFMA_MIN take one output element per thread, the summed index
// ascending, multiply and add rounded separately (the file is built with -ffp-contract=off); from GSE_MFMA_MIN up a wavefront owns a
// 16 x 16 output tile at a time on v_mfma_f64_16x16x4_f64, the summed index in chunks of four, ascending, edge tiles and the last chunk
// zero-padded in registers (operand roles as in kernels_contraction.hip: first operand indexed by the output column, second by the
// output row, acc[reg] = out[row = lane & 15][col = (lane >> 4) + 4 reg]).  First version, not tuned: a lane loads its operand element
// straight from global memory.  There is no floating-point atomic and no split of a summed index: the bits of an output depend on the
// operands and the shape alone.  The trace is summed per workgroup by a fixed tree, and the shares by the last workgroup to arrive
// (an integer ticket) in workgroup order.
#include "gse.hpp"

namespace t4a {

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr int GSE_THREADS = 256;

// O[row, c] for the GSE_TILE rows from m0, c < n: sum_k X[row, k] Y[k, c], k < K; X and Y by strides; minus: O = S[row, c] - sum
__device__ __forceinline__ void gse_tile_product(const double* X, long long xrs, long long xcs, const double* Y, long long yrs, long long ycs, int rows, int m0,
                                                 int K, int n, double* O, long long ors, long long ocs, const double* S, long long srs, long long scs, int mfma,
                                                 int tid)
{
    if (mfma) {
        const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
        const int row = m0 + lr;
        const bool row_ok = row < rows;
        const int nct = (n + 15) >> 4;
        for (int ct = wave; ct < nct; ct += GSE_THREADS / 64) {
            const int c = (ct << 4) + lr;
            const bool c_ok = c < n;
            double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < K; k0 += 4) {
                const int k = k0 + lk;
                const bool k_ok = k < K;
                const double xv = (row_ok && k_ok) ? X[(long long)row * xrs + (long long)k * xcs] : 0.0;
                const double yv = (c_ok && k_ok) ? Y[(long long)k * yrs + (long long)c * ycs] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(yv, xv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int cc = (ct << 4) + lk + 4 * reg;
                if (row_ok && cc < n) {
                    const double v = acc[reg];
                    O[(long long)row * ors + (long long)cc * ocs] = S ? S[(long long)row * srs + (long long)cc * scs] - v : v;
                }
            }
        }
    } else {
        for (int e = tid; e < GSE_TILE * n; e += GSE_THREADS) {
            const int row = m0 + (e & (GSE_TILE - 1)), c = e / GSE_TILE;
            if (row >= rows) continue;
            double s = 0.0;
            for (int k = 0; k < K; ++k) s = s + X[(long long)row * xrs + (long long)k * xcs] * Y[(long long)k * yrs + (long long)c * ycs];
            O[(long long)row * ors + (long long)c * ocs] = S ? S[(long long)row * srs + (long long)c * scs] - s : s;
        }
    }
}

// subtract: 0 O = T M2; 1 O = A - T M2 and the trace of A; 2 the trace alone (the GEMM route forms the products)
__global__ void __launch_bounds__(GSE_THREADS) gse_chain_kernel(const GseLaunch a)
{
    __shared__ double red[GSE_THREADS];
    __shared__ int s_last;
    const int tid = threadIdx.x, b = blockIdx.x;
    int j = 0;
    while (j + 1 < a.n_jobs && b >= a.job[j + 1].tile0) ++j;
    const GseJob J = a.job[j];
    const int m0 = (b - J.tile0) * GSE_TILE;
    if (a.subtract != 2) {
        gse_tile_product(J.A, J.ars, J.acs, J.M1, J.m1rs, J.m1cs, J.rows, m0, J.k1, J.n1, J.T, 1, J.rows, nullptr, 0, 0, J.mfma, tid);
        __threadfence_block(); // the rows of T this workgroup wrote are read by its own threads only
        __syncthreads();
        gse_tile_product(J.T, 1, J.rows, J.M2, J.m2rs, J.m2cs, J.rows, m0, J.n1, J.n2, J.O, J.ors, J.ocs, a.subtract ? J.A : nullptr, J.ars, J.acs, J.mfma, tid);
    }
    if (!a.subtract) return;
    double s = 0.0;
    for (int e = tid; e < GSE_TILE * J.k1; e += GSE_THREADS) {
        const int row = m0 + (e & (GSE_TILE - 1)), c = e / GSE_TILE;
        if (row < J.rows) {
            const double v = J.A[(long long)row * J.ars + (long long)c * J.acs];
            s = s + v * v;
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int w = GSE_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        a.trace_part[b] = red[0];
        __threadfence();
        const unsigned t = atomicAdd(a.ticket, 1u);
        s_last = (t == (unsigned)a.n_tiles - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last || tid != 0) return;
    __threadfence();
    const volatile double* part = a.trace_part;
    double t = 0.0;
    for (int g = 0; g < a.n_tiles; ++g) t = t + part[g];
    *a.trace = t;
}

void strides(int orient, int na, int q, long long& rs, long long& cs)
{
    rs = orient ? q : 1;
    cs = orient ? 1 : na;
}

} // namespace

void gse_chain_launch(const GseLaunch& a, hipStream_t stream)
{
    if (a.n_tiles <= 0) return;
    hipLaunchKernelGGL(gse_chain_kernel, dim3((unsigned)a.n_tiles), dim3(GSE_THREADS), 0, stream, a);
}

int gse_tiles(const int* rows, int n_jobs)
{
    int t = 0;
    for (int j = 0; j < n_jobs; ++j) t += (rows[j] + GSE_TILE - 1) / GSE_TILE;
    return t;
}

namespace {
GseLaunch project_args(int orient, int q, const double* const* refs, const int* rho, int K, const double* B, int kb, double* stack, double* scratch,
                       double* trace_part, unsigned* ticket, double* trace)
{
    GseLaunch a{};
    int P = 0;
    for (int j = 0; j < K; ++j) P += rho[j];
    long long brs, bcs;
    strides(orient, kb, q, brs, bcs);
    int off = 0, tile = 0;
    for (int j = 0; j < K; ++j) {
        GseJob& J = a.job[j];
        J.A = refs[j];
        strides(orient, rho[j], q, J.ars, J.acs);
        J.rows = rho[j];
        J.k1 = q;
        J.M1 = B; // B^T: q x kb
        J.m1rs = bcs;
        J.m1cs = brs;
        J.n1 = kb;
        J.M2 = B;
        J.m2rs = brs;
        J.m2cs = bcs;
        J.n2 = q;
        J.O = stack + (orient ? (size_t)q * off : (size_t)off);
        strides(orient, P, q, J.ors, J.ocs);
        J.T = scratch + (size_t)off * kb;
        J.tile0 = tile;
        J.mfma = kb >= GSE_MFMA_MIN;
        off += rho[j];
        tile += (rho[j] + GSE_TILE - 1) / GSE_TILE;
    }
    a.n_jobs = K;
    a.n_tiles = tile;
    a.subtract = 1;
    a.trace_part = trace_part;
    a.ticket = ticket;
    a.trace = trace;
    return a;
}
} // namespace

void gse_project_launch(int orient, int q, const double* const* refs, const int* rho, int K, const double* B, int kb, double* stack, double* scratch,
                        double* trace_part, unsigned* ticket, double* trace, hipStream_t stream)
{
    gse_chain_launch(project_args(orient, q, refs, rho, K, B, kb, stack, scratch, trace_part, ticket, trace), stream);
}

void gse_absorb_launch(int orient, int q, const double* const* child, const int* r, const double* const* parent, const int* L, int n_trains,
                       const double* Bn, int kn, double* const* out, double* scratch, hipStream_t stream)
{
    GseLaunch a{};
    int tile = 0;
    size_t soff = 0;
    for (int j = 0; j < n_trains; ++j) {
        GseJob& J = a.job[j];
        J.A = parent[j]; // orient 0: L x r; orient 1: r x L read as its transpose
        J.ars = orient ? r[j] : 1;
        J.acs = orient ? 1 : L[j];
        J.rows = L[j];
        J.k1 = r[j];
        J.M1 = child[j];
        strides(orient, r[j], q, J.m1rs, J.m1cs);
        J.n1 = q;
        J.M2 = Bn; // Bn^T: q x kn
        long long brs, bcs;
        strides(orient, kn, q, brs, bcs);
        J.m2rs = bcs;
        J.m2cs = brs;
        J.n2 = kn;
        J.O = out[j]; // orient 0: L x kn; orient 1: kn x L written as its transpose
        J.ors = orient ? kn : 1;
        J.ocs = orient ? 1 : L[j];
        J.T = scratch + soff;
        J.tile0 = tile;
        J.mfma = kn >= GSE_MFMA_MIN;
        soff += (size_t)L[j] * q;
        tile += (L[j] + GSE_TILE - 1) / GSE_TILE;
    }
    a.n_jobs = n_trains;
    a.n_tiles = tile;
    a.subtract = 0;
    gse_chain_launch(a, stream);
}

// ---- the GEMM composition
void gse_project_gemm(Engine& e, int orient, int q, const double* const* refs, const int* rho, int K, const double* B, int kb, double* stack, double* scratch,
                      double* trace_part, unsigned* ticket, double* trace)
{
    hipStream_t st = e.stream();
    int P = 0;
    for (int j = 0; j < K; ++j) P += rho[j];
    int off = 0;
    for (int j = 0; j < K; ++j) {
        double* G = scratch + (size_t)off * kb;
        if (!orient) { // R rho x q, B kb x q, stack rows off.. of P x q
            double* O = stack + off;
            T4A_HIP(hipMemcpy2DAsync(O, sizeof(double) * P, refs[j], sizeof(double) * rho[j], sizeof(double) * rho[j], (size_t)q, hipMemcpyDeviceToDevice, st));
            GemmDesc g = gemm_desc(rho[j], kb, q, refs[j], rho[j], B, kb, G, rho[j]); // G = R B^T
            g.transB = 1;
            gemm_launch(g, st);
            GemmDesc h = gemm_desc(rho[j], q, kb, G, rho[j], B, kb, O, P); // O = O - G B
            h.alpha = -1.0;
            h.beta = 1.0;
            gemm_launch(h, st);
        } else { // R^T q x rho, B^T q x kb, stack columns off.. of q x P
            double* O = stack + (size_t)q * off;
            T4A_HIP(hipMemcpyAsync(O, refs[j], sizeof(double) * (size_t)q * rho[j], hipMemcpyDeviceToDevice, st));
            GemmDesc g = gemm_desc(kb, rho[j], q, B, q, refs[j], q, G, kb); // G^T = B R^T (kb x rho)
            g.transA = 1;
            gemm_launch(g, st);
            GemmDesc h = gemm_desc(q, rho[j], kb, B, q, G, kb, O, q); // O = O - B^T G^T
            h.alpha = -1.0;
            h.beta = 1.0;
            gemm_launch(h, st);
        }
        off += rho[j];
    }
    GseLaunch a = project_args(orient, q, refs, rho, K, B, kb, stack, scratch, trace_part, ticket, trace);
    a.subtract = 2;
    gse_chain_launch(a, st);
}

void gse_absorb_gemm(Engine& e, int orient, int q, const double* const* child, const int* r, const double* const* parent, const int* L, int n_trains,
                     const double* Bn, int kn, double* const* out, double* scratch)
{
    hipStream_t st = e.stream();
    size_t soff = 0;
    for (int j = 0; j < n_trains; ++j) {
        double* G = scratch + soff;
        if (!orient) {
            GemmDesc g = gemm_desc(r[j], kn, q, child[j], r[j], Bn, kn, G, r[j]); // G = C Bn^T (r x kn)
            g.transB = 1;
            gemm_launch(g, st);
            gemm_launch(gemm_desc(L[j], kn, r[j], parent[j], L[j], G, r[j], out[j], L[j]), st); // out = parent G
        } else {
            GemmDesc g = gemm_desc(kn, r[j], q, Bn, q, child[j], q, G, kn); // G^T = Bn C^T (kn x r)
            g.transA = 1;
            gemm_launch(g, st);
            gemm_launch(gemm_desc(kn, L[j], r[j], G, kn, parent[j], r[j], out[j], kn), st); // out = G^T parent
        }
        soff += (size_t)r[j] * kn;
    }
}

} // namespace t4a
