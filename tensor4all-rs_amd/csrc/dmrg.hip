// dmrg.hip — two-site DMRG on the device (see dmrg.hpp).  Shape bookkeeping and the lowest eigenpair of the small projected matrix
// of Lanczos (a cyclic Jacobi) are host work; every other floating-point operation runs in gfx950 kernels: the projected apply and
// the orthogonalisation of linsolve.hpp, the Ritz combination, the eigen-residual and the finishing sums of kernels_dmrg.hip, the
// QR and the SVD behind QrSweep and tensor_svd.
#include "dmrg.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

namespace {

void require_tol(double v, const std::string& what)
{
    if (!std::isfinite(v) || v < 0.0) throw Error(T4A_GPU_INVALID_ARGUMENT, what);
}

std::vector<std::array<size_t, 3>> dims3_of(const std::vector<DevCore>& cores)
{
    std::vector<std::array<size_t, 3>> d;
    for (const DevCore& c : cores) d.push_back({c.l, c.s, c.r});
    return d;
}

} // namespace

// ------------------------------------------------------------------------------------------------ options and shapes
void LanczosOptions::validate() const
{
    const std::string who = "hermitian_lanczos_lowest_eigenpair: ";
    if (max_iter == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, who + "max_iter must be greater than zero");
    if (max_iter > LINSOLVE_RESTART_DIM_MAX)
        throw Error(T4A_GPU_INVALID_ARGUMENT, who + "max_iter above " + std::to_string(LINSOLVE_RESTART_DIM_MAX) + " is not supported");
    require_tol(rtol, who + "rtol must be finite and non-negative");
    require_tol(atol, who + "atol must be finite and non-negative");
    require_tol(breakdown_tol, who + "breakdown_tol must be finite and non-negative");
    require_tol(hermitian_tol, who + "hermitian_tol must be finite and non-negative");
}

double LanczosOptions::threshold(double eigenvalue) const { return std::max(atol, rtol * std::max(std::fabs(eigenvalue), 1.0)); }

void DmrgOptions::validate() const
{
    if (nsite != 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "DMRG supports only nsite=2 in this version, got nsite=" + std::to_string(nsite));
    if (nsweeps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid DMRG option nsweeps: must be greater than zero");
    if (has_max_bond_dim && max_bond_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid DMRG option max_bond_dim: must be greater than zero when set");
    if (has_energy_tol) require_tol(energy_tol, "invalid DMRG option energy_tol: must be finite and non-negative");
    require_tol(real_scalar_tol, "invalid DMRG option real_scalar_tol: must be finite and non-negative");
    lanczos.validate();
    if (has_svd_policy) {
        if (!std::isfinite(svd_policy.threshold) || svd_policy.threshold < 0.0)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid SVD truncation threshold: threshold must be finite and non-negative");
        if (svd_policy.scale < 0 || svd_policy.scale > 1 || svd_policy.measure < 0 || svd_policy.measure > 1 || svd_policy.rule < 0 || svd_policy.rule > 1)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "DmrgOptions::svd_policy: unknown scale, measure or rule");
    }
}

void dmrg_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter)
{
    const size_t n = state.size();
    if (op.size() != n)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "dmrg: lengths differ: the operator has " + std::to_string(op.size()) + " sites, the state " + std::to_string(n));
    if (n < 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "dmrg: two-site DMRG requires at least one state edge");
    for (size_t i = 0; i < n; ++i) {
        if (op[i][1] != op[i][2])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "dmrg: site " + std::to_string(i) + " of the operator is not square: (" + std::to_string(op[i][1]) + ", " +
                                                      std::to_string(op[i][2]) + ")");
        if (op[i][1] != state[i][1])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "dmrg: site " + std::to_string(i) + " of the operator has dimension " + std::to_string(op[i][1]) +
                                                      ", the state " + std::to_string(state[i][1]));
    }
    if (center >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "dmrg: center " + std::to_string(center) + " is not a state node (" + std::to_string(n) + " sites)");
    for (size_t i = 0; i + 1 < n; ++i) check_bond_step_dims("dmrg", i, state[i][0], state[i][1], state[i + 1][1], state[i + 1][2], op[i][3], max_iter);
}

// ------------------------------------------------------------------------------------------------ the small eigenproblem
double jacobi_lowest_eigenpair(const std::vector<double>& a_in, size_t n, std::vector<double>& vec)
{
    std::vector<double> a(a_in), v(n * n, 0.0);
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
    size_t lo = 0;
    for (size_t i = 1; i < n; ++i)
        if (a[i + n * i] < a[lo + n * lo]) lo = i;
    vec.assign(v.begin() + n * lo, v.begin() + n * (lo + 1));
    double nn = 0.0;
    for (double x : vec) nn = nn + x * x;
    nn = std::sqrt(nn);
    for (double& x : vec) x = x / nn;
    return a[lo + n * lo];
}

// ------------------------------------------------------------------------------------------------ Lanczos
void Lanczos::reserve(size_t len, size_t max_iter)
{
    grow(eng_, basis_, len * (max_iter + 1));
    grow(eng_, ax_, len);
    gs_.reserve(max_iter + 1);
    grow(eng_, hcol_, max_iter + 2);
    grow(eng_, coef_, max_iter + 1);
}

void Lanczos::residual_sums(const GmresApply& apply, size_t len, const double* d_v, double lambda, double sums[3])
{
    hipStream_t st = eng_.stream();
    grow(eng_, ax_, len);
    gs_.reserve(1);
    apply(d_v, ax_.get());
    eig_residual_launch(d_v, ax_.get(), lambda, nullptr, len, gs_.npart(), st);
    krylov_finish_launch(gs_.npart(), gs_workgroups(len), 3, gs_.scalars() + 1, st);
    T4A_HIP(hipGetLastError());
    T4A_HIP(hipMemcpyAsync(sums, gs_.scalars() + 1, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    eng_.sync();
}

LanczosResult Lanczos::solve(const GmresApply& apply, size_t len, double* d_x, const LanczosOptions& o)
{
    LanczosResult res;
    hipStream_t st = eng_.stream();
    const size_t m = o.max_iter;
    reserve(len, m);
    double* V = basis_.get();
    const double n0 = gs_.norm(d_x, len, V); // v_0 = theta_0 / |theta_0|
    if (!(n0 > o.breakdown_tol)) throw Error(T4A_GPU_INVALID_ARGUMENT, "hermitian_lanczos_lowest_eigenpair: the initial vector is numerically zero");

    std::vector<std::vector<double>> hcols;
    std::vector<double> a, coef;
    // the Ritz vector sum_i c_i v_i into d_x and its true residual
    auto finalise = [&](size_t dim, double lambda, const std::vector<double>& c) {
        T4A_HIP(hipMemcpyAsync(coef_.get(), c.data(), sizeof(double) * dim, hipMemcpyHostToDevice, st));
        // (the shares of |x|^2 that the combine leaves in npart are not read here: eig_residual below overwrites them with its own three
        // sums, and <v, v> comes from there)
        krylov_combine_launch(V, len, (int)dim, coef_.get(), d_x, len, gs_.npart(), st);
        double sums[3];
        residual_sums(apply, len, d_x, lambda, sums);
        ++res.apply_calls;
        res.eigenvalue = lambda;
        res.iterations = dim;
        res.residual_norm = std::sqrt(sums[0]);
        res.converged = res.residual_norm <= o.threshold(lambda);
    };
    double last_lambda = 0.0;
    for (size_t j = 0; j < m; ++j) {
        double* w = V + len * (j + 1);
        apply(V + len * j, w);
        ++res.apply_calls;
        gs_.orth(V, len, (int)(j + 1), w, len, hcol_.get(), nullptr); // w is left normalised: v_{j+1}
        std::vector<double> hc(j + 2);
        T4A_HIP(hipMemcpyAsync(hc.data(), hcol_.get(), sizeof(double) * (j + 2), hipMemcpyDeviceToHost, st));
        eng_.sync();
        const double beta = hc[j + 1];
        hcols.push_back(std::move(hc));
        // projected_matrix_from_columns: the upper-Hessenberg data, rows below the subdiagonal zero
        const size_t dim = j + 1;
        a.assign(dim * dim, 0.0);
        for (size_t col = 0; col < dim; ++col)
            for (size_t row = 0; row < dim && row < hcols[col].size(); ++row) a[row + dim * col] = hcols[col][row];
        for (size_t r = 0; r < dim; ++r)
            for (size_t c = r + 1; c < dim; ++c) {
                const double x = a[r + dim * c], y = a[c + dim * r];
                const double scale = std::max(1.0, std::max(std::fabs(x), std::fabs(y)));
                if (!(std::fabs(x - y) <= o.hermitian_tol * scale))
                    throw Error(T4A_GPU_INVALID_ARGUMENT, "hermitian_lanczos_lowest_eigenpair: projected operator is not Hermitian: entries (" +
                                                              std::to_string(r) + ", " + std::to_string(c) + ") and its transpose differ by " +
                                                              std::to_string(std::fabs(x - y)));
                a[r + dim * c] = a[c + dim * r] = 0.5 * (x + y);
            }
        const double lambda = jacobi_lowest_eigenpair(a, dim, coef);
        last_lambda = lambda;
        const double estimate = beta * std::fabs(coef[dim - 1]);
        const bool broke_down = beta <= o.breakdown_tol;
        if (estimate <= o.threshold(lambda) || broke_down) {
            finalise(dim, lambda, coef);
            if (res.converged || broke_down) return res;
        }
    }
    finalise(m, last_lambda, coef);
    return res;
}

void Lanczos::time_finalise(size_t len, size_t nb, size_t reps, double ms[3])
{
    hipStream_t st = eng_.stream();
    reserve(len, nb);
    DevBuf<double> x;
    x.reserve(len);
    fill_launch(basis_.get(), len * (nb + 1), 1.0 / std::sqrt((double)len), st);
    fill_launch(coef_.get(), nb, 1.0 / std::sqrt((double)nb), st);
    fill_launch(ax_.get(), len, 1.0, st);
    const int G = gs_workgroups(len);
    EventTimer t;
    t.init();
    const std::function<void()> pieces[3] = {
        [&] { krylov_combine_launch(basis_.get(), len, (int)nb, coef_.get(), x.get(), len, gs_.npart(), st); },
        [&] { eig_residual_launch(x.get(), ax_.get(), 0.5, nullptr, len, gs_.npart(), st); },
        [&] { krylov_finish_launch(gs_.npart(), G, 3, gs_.scalars() + 1, st); },
    };
    for (int k = 0; k < 3; ++k) {
        pieces[k](); // warm-up
        T4A_HIP(hipEventRecord(t.a, st));
        for (size_t r = 0; r < reps; ++r) pieces[k]();
        T4A_HIP(hipEventRecord(t.b, st));
        T4A_HIP(hipEventSynchronize(t.b));
        T4A_HIP(hipGetLastError());
        float f = 0.0f;
        T4A_HIP(hipEventElapsedTime(&f, t.a, t.b));
        ms[k] = (double)f / (double)reps;
    }
    eng_.sync();
}

// ------------------------------------------------------------------------------------------------ the sweeps
namespace {

// theta = x_i x_{i+1} as M x N into `theta`; -> len
size_t two_site_vector(ProjectedOperator& po, size_t i, DevBuf<double>& theta)
{
    Engine& e = po.engine();
    const auto ld = po.local_dims(i);
    const int M = (int)(ld[0] * ld[1]), N = (int)(ld[2] * ld[3]), mid = (int)po.x[i].r;
    const size_t len = (size_t)M * N;
    grow(e, theta, len);
    gemm_launch(gemm_desc(M, N, mid, po.x[i].buf.get(), M, po.x[i + 1].buf.get(), mid, theta.get(), M), e.stream());
    return len;
}

// the Rayleigh quotient at the region of `center` (rayleigh_region: the centre and a neighbour)
double rayleigh_quotient(ProjectedOperator& po, Lanczos& lz, size_t center, double real_scalar_tol)
{
    const size_t n = po.len();
    const size_t i = center + 1 < n ? center : center - 1;
    po.check_step(i, 1, "dmrg");
    DevBuf<double> theta;
    const size_t len = two_site_vector(po, i, theta);
    po.prepare(i);
    double sums[3];
    lz.residual_sums([&](const double* v, double* y) { po.apply_prepared(v, y); }, len, theta.get(), 0.0, sums);
    if (!(std::fabs(sums[2]) > real_scalar_tol)) throw Error(T4A_GPU_INVALID_ARGUMENT, "DMRG Rayleigh quotient denominator is zero");
    return sums[1] / sums[2];
}

} // namespace

DmrgResult dmrg(Mpo& op, TensorTrain& init, size_t center, const DmrgOptions& o)
{
    o.validate();
    dmrg_validate_shapes(op.dims4(), dims3_of(init.cores), center, o.lanczos.max_iter);
    DmrgResult out;
    ProjectedOperator po(op, init, nullptr);
    Engine& e = po.engine();
    hipStream_t st = e.stream();
    const size_t n = po.len();
    {
        QrSweep sw(e);
        sw.canonicalize(po.x, center);
    }
    Lanczos lz(e);
    DevBuf<double> theta;
    SvdOptions so;
    so.truncate = true;
    if (o.has_svd_policy) so.policy = o.svd_policy;
    so.has_max_bond_dim = o.has_max_bond_dim;
    so.max_bond_dim = o.max_bond_dim;
    double last_energy = 0.0;

    auto bond_step = [&](size_t i, bool move_right) {
        po.check_step(i, o.lanczos.max_iter, "dmrg");
        const size_t len = two_site_vector(po, i, theta); // theta_0 = x_i x_{i+1}
        lz.reserve(len, o.lanczos.max_iter);
        po.prepare(i);
        const LanczosResult lr = lz.solve([&](const double* v, double* y) { po.apply_prepared(v, y); }, len, theta.get(), o.lanczos);
        ++out.stats.local_solves;
        out.stats.lanczos_steps += lr.iterations;
        out.stats.apply_calls += lr.apply_calls;
        last_energy = lr.eigenvalue;
        out.max_residual_norm = std::max(out.max_residual_norm, lr.residual_norm);
        po.split_and_advance(i, theta.get(), so, move_right, "dmrg"); // the singular values go to the new centre, no renormalisation
        ++out.local_updates;
    };

    bool has_previous = false;
    double previous = 0.0;
    for (size_t sweep = 0; sweep < o.nsweeps; ++sweep) {
        for (size_t i = center; i + 1 < n; ++i) bond_step(i, true);
        for (size_t i = n - 1; i-- > 0;) bond_step(i, false);
        for (size_t i = 0; i < center; ++i) bond_step(i, true);
        out.sweeps_completed = sweep + 1;
        if (o.has_energy_tol) {
            if (has_previous && std::fabs(last_energy - previous) <= o.energy_tol) {
                out.converged = true;
                break;
            }
            previous = last_energy;
            has_previous = true;
        }
    }
    out.energy = rayleigh_quotient(po, lz, center, o.real_scalar_tol);
    e.sync();
    out.state = std::make_unique<TensorTrain>(po.x, st);
    return out;
}

double dmrg_energy(Mpo& op, TensorTrain& state, size_t center, double real_scalar_tol)
{
    if (!std::isfinite(real_scalar_tol) || real_scalar_tol < 0.0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid DMRG option real_scalar_tol: must be finite and non-negative");
    dmrg_validate_shapes(op.dims4(), dims3_of(state.cores), center, 1);
    ProjectedOperator po(op, state, nullptr);
    Engine& e = po.engine();
    {
        QrSweep sw(e);
        sw.canonicalize(po.x, center);
    }
    Lanczos lz(e);
    const double v = rayleigh_quotient(po, lz, center, real_scalar_tol);
    e.sync();
    return v;
}

// ------------------------------------------------------------------------------------------------ test hooks
LanczosResult lanczos_dense(const double* H, size_t n, const double* v0, const LanczosOptions& o, double* v_out)
{
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dH, dx;
    dH.reserve(n * n);
    dx.reserve(n);
    T4A_HIP(hipMemcpyAsync(dH.get(), H, sizeof(double) * n * n, hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(dx.get(), v0, sizeof(double) * n, hipMemcpyHostToDevice, st));
    Lanczos lz(e);
    const LanczosResult r =
        lz.solve([&](const double* v, double* y) { gemm_launch(gemm_desc((int)n, 1, (int)n, dH.get(), (int)n, v, (int)n, y, (int)n), st); }, n, dx.get(), o);
    T4A_HIP(hipMemcpyAsync(v_out, dx.get(), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    e.sync();
    return r;
}

void krylov_combine_host(const double* basis, size_t len, size_t nb, const double* coef, double* out, double* norm2)
{
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dV, dc, dout, npart, sum;
    dV.reserve(len * nb);
    dc.reserve(nb);
    dout.reserve(len);
    npart.reserve(GS_MAX_WORKGROUPS);
    sum.reserve(1);
    T4A_HIP(hipMemcpyAsync(dV.get(), basis, sizeof(double) * len * nb, hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(dc.get(), coef, sizeof(double) * nb, hipMemcpyHostToDevice, st));
    krylov_combine_launch(dV.get(), len, (int)nb, dc.get(), dout.get(), len, npart.get(), st);
    krylov_finish_launch(npart.get(), gs_workgroups(len), 1, sum.get(), st);
    T4A_HIP(hipGetLastError());
    T4A_HIP(hipMemcpyAsync(out, dout.get(), sizeof(double) * len, hipMemcpyDeviceToHost, st));
    T4A_HIP(hipMemcpyAsync(norm2, sum.get(), sizeof(double), hipMemcpyDeviceToHost, st));
    e.sync();
}

void eig_residual_host(const double* v, const double* hv, size_t len, double lambda, double* r, double sums[3])
{
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dv, dhv, dr, part, sum;
    dv.reserve(len);
    dhv.reserve(len);
    if (r) dr.reserve(len);
    part.reserve(3 * GS_MAX_WORKGROUPS);
    sum.reserve(3);
    T4A_HIP(hipMemcpyAsync(dv.get(), v, sizeof(double) * len, hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(dhv.get(), hv, sizeof(double) * len, hipMemcpyHostToDevice, st));
    eig_residual_launch(dv.get(), dhv.get(), lambda, r ? dr.get() : nullptr, len, part.get(), st);
    krylov_finish_launch(part.get(), gs_workgroups(len), 3, sum.get(), st);
    T4A_HIP(hipGetLastError());
    if (r) {
        T4A_HIP(hipMemcpyAsync(r, dr.get(), sizeof(double) * len, hipMemcpyDeviceToHost, st));
    }
    T4A_HIP(hipMemcpyAsync(sums, sum.get(), sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    e.sync();
}

void lanczos_time_finalise(size_t len, size_t nb, size_t reps, double ms[3])
{
    if (len == 0 || nb == 0 || nb > LINSOLVE_RESTART_DIM_MAX || reps == 0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "time_finalise: len, nb and reps must be positive, nb at most " + std::to_string(LINSOLVE_RESTART_DIM_MAX));
    if ((unsigned long long)len * (nb + 1) > (unsigned long long)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, "time_finalise: the basis holds more than INT_MAX elements");
    require_device();
    Engine e;
    Lanczos lz(e);
    lz.time_finalise(len, nb, reps, ms);
}

} // namespace t4a
