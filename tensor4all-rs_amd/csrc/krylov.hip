// krylov.hip — the shared core of the Krylov solvers (see krylov.hpp).  The Jacobi of the small projected matrix and the Hermitian check
// are host work; every floating-point operation on a vector runs in the kernels of kernels_linsolve.hip, kernels_tdvp.hip and
// kernels_dmrg.hip.
#include "krylov.hpp"

#include <algorithm>
#include <cmath>
#include <string>

namespace t4a {

// ------------------------------------------------------------------------------------------------ the orthogonalisation step
void KrylovOrth::reserve(size_t nb_max)
{
    grow(eng_, part_, std::max<size_t>(nb_max, 1) * GS_MAX_WORKGROUPS);
    grow(eng_, npart_, 3 * GS_MAX_WORKGROUPS);
    grow(eng_, scal_, 4);
}

double KrylovOrth::norm(const double* d_w, size_t len, double* d_out)
{
    hipStream_t st = eng_.stream();
    double v = 0.0;
    gs_norm2_launch(d_w, len, npart_.get(), st);
    gs_normalize_launch(d_w, len, npart_.get(), d_out, scal_.get(), st);
    T4A_HIP(hipMemcpyAsync(&v, scal_.get(), sizeof(double), hipMemcpyDeviceToHost, st));
    eng_.sync();
    return v;
}

KrylovDotsRoute krylov_dots_route(size_t, int nb) { return nb > GS_WIDE ? KrylovDotsRoute::Wide : KrylovDotsRoute::Serial; }

void KrylovOrth::dots(const double* d_V, size_t ld, int nb, const double* d_w, size_t len)
{
    const KrylovDotsRoute r = route_ == KrylovDotsRoute::Auto ? krylov_dots_route(len, nb) : route_;
    if (r == KrylovDotsRoute::Wide) gs_dots_wide_launch(d_V, ld, nb, d_w, len, part_.get(), eng_.stream());
    else gs_dots_launch(d_V, ld, nb, d_w, len, part_.get(), eng_.stream());
}

void KrylovOrth::orth(const double* d_V, size_t ld, int nb, double* d_w, size_t len, double* d_hcol, double* d_hpass)
{
    hipStream_t st = eng_.stream();
    const int G = gs_workgroups(len);
    dots(d_V, ld, nb, d_w, len);
    gs_update_launch(d_V, ld, nb, d_w, len, part_.get(), G, d_hcol, true, d_hpass, npart_.get(), st);
    dots(d_V, ld, nb, d_w, len);
    gs_update_launch(d_V, ld, nb, d_w, len, part_.get(), G, d_hcol, false, d_hpass ? d_hpass + nb : nullptr, npart_.get(), st);
    gs_normalize_launch(d_w, len, npart_.get(), d_w, d_hcol + nb, st);
}

// ------------------------------------------------------------------------------------------------ the small eigenproblem
void jacobi_eigh(const std::vector<double>& a_in, size_t n, std::vector<double>& evals, std::vector<double>& v)
{
    std::vector<double> a(a_in);
    v.assign(n * n, 0.0);
    for (size_t i = 0; i < n; ++i) v[i + n * i] = 1.0;
    double fro = 0.0;
    for (double x : a) fro = fro + x * x;
    fro = std::sqrt(fro);
    const double tiny = 1e-19 * fro;
    for (int sweep = 0; sweep < 100; ++sweep) {
        bool rotated = false;
        for (size_t p = 0; p + 1 < n; ++p) {
            for (size_t q = p + 1; q < n; ++q) {
                const double apq = a[p + n * q];
                if (!(std::fabs(apq) > tiny)) continue;
                rotated = true;
                const double theta = (a[q + n * q] - a[p + n * p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                a[p + n * p] = a[p + n * p] - t * apq;
                a[q + n * q] = a[q + n * q] + t * apq;
                a[p + n * q] = a[q + n * p] = 0.0;
                for (size_t k = 0; k < n; ++k) {
                    if (k != p && k != q) {
                        const double akp = a[k + n * p], akq = a[k + n * q];
                        a[k + n * p] = a[p + n * k] = c * akp - s * akq;
                        a[k + n * q] = a[q + n * k] = s * akp + c * akq;
                    }
                    const double vkp = v[k + n * p], vkq = v[k + n * q];
                    v[k + n * p] = c * vkp - s * vkq;
                    v[k + n * q] = s * vkp + c * vkq;
                }
            }
        }
        if (!rotated) break;
    }
    evals.resize(n);
    for (size_t i = 0; i < n; ++i) evals[i] = a[i + n * i];
}

double jacobi_lowest_eigenpair(const std::vector<double>& a, size_t n, std::vector<double>& vec)
{
    std::vector<double> evals, v;
    jacobi_eigh(a, n, evals, v);
    size_t lo = 0;
    for (size_t i = 1; i < n; ++i)
        if (evals[i] < evals[lo]) lo = i;
    vec.assign(v.begin() + n * lo, v.begin() + n * (lo + 1));
    double nn = 0.0;
    for (double x : vec) nn = nn + x * x;
    nn = std::sqrt(nn);
    for (double& x : vec) x = x / nn;
    return evals[lo];
}

// ------------------------------------------------------------------------------------------------ the Hermitian Arnoldi step
void HermitianArnoldi::reserve(size_t len, size_t max_iter)
{
    grow(eng_, basis_, len * (max_iter + 1));
    gs_.reserve(max_iter + 1);
    grow(eng_, hcol_, max_iter + 2);
    grow(eng_, coef_, max_iter + 1);
}

double HermitianArnoldi::start(const double* d_x, size_t len)
{
    len_ = len;
    hcols_.clear();
    return gs_.norm(d_x, len, basis_.get());
}

double HermitianArnoldi::step(const GmresApply& apply, size_t j, double hermitian_tol, const char* who)
{
    double* V = basis_.get();
    double* w = V + len_ * (j + 1);
    apply(V + len_ * j, w);
    gs_.orth(V, len_, (int)(j + 1), w, len_, hcol_.get(), nullptr); // w is left normalised: v_{j+1}
    std::vector<double> hc(j + 2);
    T4A_HIP(hipMemcpyAsync(hc.data(), hcol_.get(), sizeof(double) * (j + 2), hipMemcpyDeviceToHost, eng_.stream()));
    eng_.sync();
    const double beta = hc[j + 1];
    hcols_.push_back(std::move(hc));
    // projected_matrix_from_columns: the upper-Hessenberg data, rows below the subdiagonal zero
    const size_t dim = j + 1;
    a_.assign(dim * dim, 0.0);
    for (size_t col = 0; col < dim; ++col)
        for (size_t row = 0; row < dim && row < hcols_[col].size(); ++row) a_[row + dim * col] = hcols_[col][row];
    for (size_t r = 0; r < dim; ++r)
        for (size_t c = r + 1; c < dim; ++c) {
            const double x = a_[r + dim * c], y = a_[c + dim * r];
            const double scale = std::max(1.0, std::max(std::fabs(x), std::fabs(y)));
            if (!(std::fabs(x - y) <= hermitian_tol * scale))
                throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": projected operator is not Hermitian: entries (" + std::to_string(r) + ", " +
                                                          std::to_string(c) + ") and its transpose differ by " + std::to_string(std::fabs(x - y)));
            a_[r + dim * c] = a_[c + dim * r] = 0.5 * (x + y);
        }
    return beta;
}

// ------------------------------------------------------------------------------------------------ probes and dense test hooks
void time_pieces(hipStream_t st, const std::function<void()>* pieces, int n, size_t reps, double* ms)
{
    EventTimer t;
    t.init();
    for (int k = 0; k < n; ++k) {
        pieces[k](); // warm-up
        T4A_HIP(hipGetLastError());
        T4A_HIP(hipEventRecord(t.a, st));
        for (size_t r = 0; r < reps; ++r) pieces[k]();
        T4A_HIP(hipEventRecord(t.b, st));
        T4A_HIP(hipEventSynchronize(t.b));
        T4A_HIP(hipGetLastError());
        float f = 0.0f;
        T4A_HIP(hipEventElapsedTime(&f, t.a, t.b));
        ms[k] = (double)f / (double)reps;
    }
}

DevBuf<double> upload_vector(hipStream_t st, const double* h, size_t count)
{
    DevBuf<double> d;
    d.reserve(count);
    T4A_HIP(hipMemcpyAsync(d.get(), h, sizeof(double) * count, hipMemcpyHostToDevice, st));
    return d;
}

GmresApply dense_apply(const double* dH, size_t n, hipStream_t st)
{
    return [=](const double* v, double* y) { gemm_launch(gemm_desc((int)n, 1, (int)n, dH, (int)n, v, (int)n, y, (int)n), st); };
}

} // namespace t4a
