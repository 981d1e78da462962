// tt_chain.hip — the chain helpers of tt_chain.hpp.  Host code only; the floating-point work runs in the gfx950 kernels of
// kernels_linalg.hip (Householder QR), kernels_dense.hip (the f64-MFMA GEMM, gathers, transposes) and kernels_tt.hip (core reshapes).
#include "tt_chain.hpp"
#include "tensorops.hpp"

namespace t4a {

DevCore clone_core(const DevCore& src, hipStream_t st)
{
    DevCore c = DevCore::make(src.l, src.s, src.r);
    if (src.size()) T4A_HIP(hipMemcpyAsync(c.buf.get(), src.buf.get(), src.size() * sizeof(double), hipMemcpyDeviceToDevice, st));
    return c;
}

std::vector<DevCore> clone_cores(const std::vector<DevCore>& src, hipStream_t st)
{
    std::vector<DevCore> out;
    out.reserve(src.size());
    for (const DevCore& c : src) out.push_back(clone_core(c, st));
    return out;
}

std::vector<double> to_host(Engine& eng, const double* d_src, size_t count)
{
    std::vector<double> h(count);
    if (count) {
        T4A_HIP(hipMemcpyAsync(h.data(), d_src, count * sizeof(double), hipMemcpyDeviceToHost, eng.stream()));
        eng.sync();
    }
    return h;
}

DevCore QrSweep::factor_right(const DevCore& c)
{
    const int L = (int)c.l, rest = (int)(c.s * c.r);
    const int k = std::min(L, rest);
    grow(eng, m1, (size_t)rest * L);
    grow(eng, q, (size_t)rest * k);
    grow(eng, rr, (size_t)k * L);
    transpose_launch(c.buf.get(), L, rest, L, m1.get(), rest, st);
    eng.qr(m1.get(), rest, L, q.get(), rr.get());
    DevCore nc = DevCore::make(k, c.s, c.r);
    transpose_launch(q.get(), rest, k, rest, nc.buf.get(), k, st);
    return nc;
}

DevCore QrSweep::factor_left(const DevCore& c)
{
    const int rows = (int)(c.l * c.s), R = (int)c.r;
    const int k = std::min(rows, R);
    grow(eng, rr, (size_t)k * R);
    DevCore nc = DevCore::make(c.l, c.s, k);
    eng.qr(c.buf.get(), rows, R, nc.buf.get(), rr.get());
    return nc;
}

void QrSweep::right_step(std::vector<DevCore>& cores, size_t i)
{
    DevCore& c = cores[i];
    DevCore& p = cores[i - 1];
    DevCore nc = factor_right(c);
    const int L = (int)c.l, k = (int)nc.l;
    DevCore np = DevCore::make(p.l, p.s, k);
    const int pm = (int)(p.l * p.s);
    GemmDesc g = gemm_desc(pm, k, L, p.buf.get(), pm, rr.get(), k, np.buf.get(), pm);
    g.transB = 1; // prev (l s x L) * R^T (L x k)
    gemm_launch(g, st);
    T4A_HIP(hipGetLastError());
    eng.sync(); // the old cores are released below
    c = std::move(nc);
    p = std::move(np);
}

void QrSweep::left_step(std::vector<DevCore>& cores, size_t i)
{
    DevCore& c = cores[i];
    DevCore& nx = cores[i + 1];
    DevCore nc = factor_left(c);
    const int R = (int)c.r, k = (int)nc.r;
    DevCore nn = DevCore::make(k, nx.s, nx.r);
    const int rest = (int)(nx.s * nx.r);
    gemm_launch(gemm_desc(k, rest, R, rr.get(), k, nx.buf.get(), R, nn.buf.get(), k), st); // R (k x R) * next (R x s r)
    T4A_HIP(hipGetLastError());
    eng.sync();
    c = std::move(nc);
    nx = std::move(nn);
}

void QrSweep::canonicalize(std::vector<DevCore>& cores, size_t center)
{
    for (size_t i = 0; i < center; ++i) left_step(cores, i);
    for (size_t i = cores.size() - 1; i > center; --i) right_step(cores, i);
}

void split_two_site(hipStream_t st, const double* U, int ldU, const double* S, const double* Vt, int ldVt, int N, int keep, bool move_right,
                    DevCore& left, DevCore& right)
{
    const int M = ldU;
    if (move_right) {
        gather_launch(U, ldU, nullptr, M, nullptr, keep, left.buf.get(), M, st);
        diag_scale_launch(Vt, ldVt, keep, N, S, true, right.buf.get(), keep, st);
    } else {
        diag_scale_launch(U, ldU, M, keep, S, false, left.buf.get(), M, st);
        gather_launch(Vt, ldVt, nullptr, keep, nullptr, N, right.buf.get(), keep, st);
    }
}

DevCore core_from_left_factor(Engine& eng, size_t L, size_t S, size_t rk)
{
    DevCore c = DevCore::make(L, S, rk);
    core_reshape_launch(eng.left(), (int)L, (int)S, (int)rk, 1, c.buf.get(), eng.stream());
    return c;
}

DevCore core_from_right_factor(Engine& eng, size_t rk, size_t S, size_t R)
{
    DevCore c = DevCore::make(rk, S, R);
    core_reshape_launch(eng.right(), (int)rk, (int)S, (int)R, 3, c.buf.get(), eng.stream());
    return c;
}

DevCore absorb_right_into_next(Engine& eng, size_t rk, const DevCore& next, DevBuf<double>& m1, DevBuf<double>& m2)
{
    hipStream_t st = eng.stream();
    const int R = (int)next.l, S = (int)next.s, NR = (int)next.r;
    m1.reserve(std::max<size_t>(next.size(), 1));
    core_reshape_launch(next.buf.get(), R, S, NR, 2, m1.get(), st);
    m2.reserve(std::max<size_t>(rk * next.s * next.r, 1));
    gemm_launch(gemm_desc((int)rk, S * NR, R, eng.right(), (int)rk, m1.get(), R, m2.get(), (int)rk), st);
    DevCore c = DevCore::make(rk, next.s, next.r);
    core_reshape_launch(m2.get(), (int)rk, S, NR, 3, c.buf.get(), st);
    return c;
}

DevCore absorb_left_into_prev(Engine& eng, size_t rk, const DevCore& prev, DevBuf<double>& m1, DevBuf<double>& m2)
{
    hipStream_t st = eng.stream();
    const int PL = (int)prev.l, PS = (int)prev.s, L = (int)prev.r;
    m1.reserve(std::max<size_t>(prev.size(), 1));
    core_reshape_launch(prev.buf.get(), PL, PS, L, 0, m1.get(), st);
    m2.reserve(std::max<size_t>(prev.l * prev.s * rk, 1));
    gemm_launch(gemm_desc(PL * PS, (int)rk, L, m1.get(), PL * PS, eng.left(), L, m2.get(), PL * PS), st);
    DevCore c = DevCore::make(prev.l, prev.s, rk);
    core_reshape_launch(m2.get(), PL, PS, (int)rk, 1, c.buf.get(), st);
    return c;
}

} // namespace t4a
