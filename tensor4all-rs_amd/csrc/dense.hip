// dense.hip — see dense.hpp.
#include "dense.hpp"

#include <cmath>
#include <numeric>

#include "stdrng.hpp"

namespace t4a {

void trsm(Engine& e, double* dA, size_t na, double* dB, size_t bm, size_t bn, bool left_side, bool lower, bool transpose_a,
          bool unit_diagonal)
{
    hipStream_t st = e.stream();
    double* dAt = dA + na * na;
    double* dBt = dB + bm * bn;
    // reduce to a left-side solve with an untransposed triangular matrix T:  T Y = R
    //   left : op(A) X = B           -> T = op(A),   R = B
    //   right: X op(A) = B           -> T = op(A)^T, R = B^T, X = Y^T
    TrsmProblem tp{};
    tp.T = dA;
    tp.ldt = tp.n = (int)na;
    tp.B = dB;
    tp.ldb = (int)bm;
    tp.nrhs = (int)bn;
    tp.lower = lower ? 1 : 0;
    tp.unit_diag = unit_diagonal ? 1 : 0;
    if (left_side ? transpose_a : !transpose_a) {
        transpose_launch(dA, (int)na, (int)na, (int)na, dAt, (int)na, st);
        tp.T = dAt;
        tp.lower = lower ? 0 : 1;
    }
    if (!left_side) {
        transpose_launch(dB, (int)bm, (int)bn, (int)bm, dBt, (int)bn, st);
        tp.B = dBt;
        tp.ldb = (int)bn;
        tp.nrhs = (int)bm;
    }
    DevBuf<TrsmProblem> dprob;
    dprob.reserve(1);
    T4A_HIP(hipMemcpyAsync(dprob.get(), &tp, sizeof(tp), hipMemcpyHostToDevice, st));
    T4A_HIP(hipStreamSynchronize(st));
    trsm_left_batched_launch(dprob.get(), 1, (int)na, tp.nrhs, st);
    if (!left_side) transpose_launch(dBt, (int)bn, (int)bm, (int)bn, dB, (int)bm, st);
    T4A_HIP(hipGetLastError());
}

void solve(Engine& e, double* dA, size_t n, double* dB, size_t nrhs)
{
    hipStream_t st = e.stream();
    DevBuf<int> dpiv;
    dpiv.reserve(n + 1);
    DevBuf<LuProblem> dlp;
    dlp.reserve(1);
    DevBuf<TrsmProblem> dtp;
    dtp.reserve(2);
    LuProblem lp{};
    lp.A = dA;
    lp.lda = lp.n = lp.ldb = (int)n;
    lp.piv = dpiv.get();
    lp.info = dpiv.get() + n;
    lp.B = dB;
    lp.nrhs = (int)nrhs;
    const TrsmProblem t[2] = {lu_trsm_problem(lp, true), lu_trsm_problem(lp, false)};
    T4A_HIP(hipMemcpyAsync(dlp.get(), &lp, sizeof(lp), hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(dtp.get(), t, sizeof(t), hipMemcpyHostToDevice, st));
    T4A_HIP(hipStreamSynchronize(st));
    // (round 5) blocked LU + one fused launch for both triangular solves; outside its size range the two-step path
    const bool fused = lu_solve_blocked_launch(dlp.get(), 1, (int)n, (int)nrhs, st);
    const bool forward_done = fused || lu_forward_blocked_launch(dlp.get(), 1, (int)n, (int)nrhs, st);
    if (!forward_done) lu_batched_launch(dlp.get(), 1, (int)n, st);
    int info = 0;
    T4A_HIP(hipMemcpyAsync(&info, lp.info, sizeof(int), hipMemcpyDeviceToHost, st));
    T4A_HIP(hipStreamSynchronize(st));
    if (info != 0) throw Error(T4A_GPU_SINGULAR_MATRIX, "solve: matrix is singular");
    if (!fused) {
        if (!forward_done) trsm_left_batched_launch(dtp.get(), 1, (int)n, (int)nrhs, st);
        trsm_left_batched_launch(dtp.get() + 1, 1, (int)n, (int)nrhs, st);
    }
    T4A_HIP(hipGetLastError());
}

void RsvdBuffers::reserve(size_t m, size_t n, size_t l)
{
    A.reserve(m * n);
    omega.reserve(n * l);
    Y.reserve(m * l);
    Q.reserve(m * l);
    R.reserve(l * std::max(l, n));
    Z.reserve(n * l);
    B.reserve(l * n);
    Ub.reserve(l * l);
    S.reserve(l);
    Vt.reserve(l * n);
    U.reserve(m * l);
}

std::vector<double> rsvd_sketch(size_t n, size_t l, uint64_t seed)
{
    std::vector<double> omega(n * l);
    StdRng rng(seed);
    for (size_t i = 0; i < omega.size(); i += 2) {
        const double u1 = ((double)(rng.next_u64() >> 11) + 1.0) * (1.0 / 9007199254740992.0);
        const double u2 = (double)(rng.next_u64() >> 11) * (1.0 / 9007199254740992.0);
        const double rad = std::sqrt(-2.0 * std::log(u1));
        omega[i] = rad * std::cos(6.283185307179586 * u2);
        if (i + 1 < omega.size()) omega[i + 1] = rad * std::sin(6.283185307179586 * u2);
    }
    return omega;
}

void rsvd(Engine& e, RsvdBuffers& w, size_t m, size_t n, size_t l, size_t power_iters)
{
    const int M = (int)m, N = (int)n, L = (int)l;
    hipStream_t st = e.stream();
    auto gemm_ta = [&](GemmDesc g) { // op(A) = A^T
        g.transA = 1;
        gemm_launch(g, st);
    };
    const GemmDesc sketch = gemm_desc(M, L, N, w.A.get(), M, w.omega.get(), N, w.Y.get(), M);
    gemm_launch(sketch, st);                                                        // Y = A Omega
    e.qr(w.Y.get(), M, L, w.Q.get(), w.R.get());                                    // Q (m x l)
    for (size_t it = 0; it < power_iters; ++it) {
        gemm_ta(gemm_desc(N, L, M, w.A.get(), M, w.Q.get(), M, w.Z.get(), N));      // Z = A^T Q (n x l)
        e.qr(w.Z.get(), N, L, w.omega.get(), w.R.get());                            // orthonormal basis of Z in omega (n x l)
        gemm_launch(sketch, st);                                                    // Y = A Z
        e.qr(w.Y.get(), M, L, w.Q.get(), w.R.get());
    }
    gemm_ta(gemm_desc(L, N, M, w.Q.get(), M, w.A.get(), M, w.B.get(), L));          // B = Q^T A (l x n)
    e.svd(w.B.get(), L, N, w.Ub.get(), w.S.get(), w.Vt.get());                      // B = Ub S Vt, Ub l x l, Vt l x n
    gemm_launch(gemm_desc(M, L, L, w.Q.get(), M, w.Ub.get(), L, w.U.get(), M), st); // U = Q Ub
    T4A_HIP(hipGetLastError());
}

double* full_piv_lu_factors(Engine& e, const LuciResult& r, size_t n)
{
    const size_t count = n * n;
    e.d_tmp.reserve(2 * count);
    double* d_l = e.d_tmp.get();
    double* d_u = d_l + count;
    hipStream_t st = e.stream();
    set_identity_launch(d_l, (int)n, (int)n, (int)n, st);
    fill_launch(d_u, count, 0.0, st);
    if (r.rank > 0) {
        tri_extract_launch(e.lu_buf(), (int)n, (int)n, r.rank, 1, 1, d_l, (int)n, st);
        tri_extract_launch(e.lu_buf(), (int)n, r.rank, (int)n, 0, 0, d_u, (int)n, st);
    }
    T4A_HIP(hipGetLastError());
    return d_l;
}

RookSource rook_source_device(Engine& e, const double* d_a, double* d_at, size_t m, size_t n)
{
    hipStream_t st = e.stream();
    const size_t count = m * n;
    if (count) transpose_launch(d_a, (int)m, (int)n, (int)m, d_at, (int)n, st);
    RookSource src;
    src.M = (int)m;
    src.N = (int)n;
    src.column = [=](int c, double* d_out) {
        T4A_HIP(hipMemcpyAsync(d_out, d_a + (size_t)c * m, m * sizeof(double), hipMemcpyDeviceToDevice, st));
    };
    src.row = [=](int r, double* d_out) {
        T4A_HIP(hipMemcpyAsync(d_out, d_at + (size_t)r * n, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    };
    static const bool host_driven = std::getenv("T4A_ROOK_HOST") != nullptr; // (A/B and parity of the two search drivers)
    if (!host_driven)
        src.full = [=](double* d_out) { T4A_HIP(hipMemcpyAsync(d_out, d_a, count * sizeof(double), hipMemcpyDeviceToDevice, st)); };
    return src;
}

RookSource rook_source_blocks(Engine& e, size_t m, size_t n, t4a_gpu_fill_block_fn fill_block, void* ctx)
{
    hipStream_t st = e.stream();
    std::vector<size_t> all_rows(m), all_cols(n);
    std::iota(all_rows.begin(), all_rows.end(), (size_t)0);
    std::iota(all_cols.begin(), all_cols.end(), (size_t)0);
    RookSource src;
    src.M = (int)m;
    src.N = (int)n;
    auto to_device = [st](const std::vector<double>& h, double* d_out) {
        T4A_HIP(hipMemcpyAsync(d_out, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
        T4A_HIP(hipStreamSynchronize(st));
    };
    src.column = [=, hbuf = std::vector<double>(m)](int c, double* d_out) mutable {
        const size_t cc = (size_t)c;
        fill_block(ctx, all_rows.data(), m, &cc, 1, hbuf.data());
        to_device(hbuf, d_out);
    };
    src.row = [=, hbuf = std::vector<double>(n)](int r, double* d_out) mutable {
        const size_t rr = (size_t)r;
        fill_block(ctx, &rr, 1, all_cols.data(), n, hbuf.data());
        to_device(hbuf, d_out);
    };
    return src;
}

} // namespace t4a
