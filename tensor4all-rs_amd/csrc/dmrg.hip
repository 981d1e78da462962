// dmrg.hip — two-site DMRG on the device (see dmrg.hpp).  Shape bookkeeping and the lowest eigenpair of the small projected matrix
// of Lanczos (a cyclic Jacobi) are host work; every other floating-point operation runs in gfx950 kernels: the projected apply of
// linsolve.hpp, the Arnoldi step of krylov.hpp, the Ritz combination, the eigen-residual and the finishing sums of kernels_dmrg.hip, the
// QR and the SVD behind QrSweep and tensor_svd.
#include "dmrg.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

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
    if (has_svd_policy) validate_svd_policy(svd_policy, "DmrgOptions::svd_policy");
}

void dmrg_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter)
{
    const size_t n = state.size();
    validate_chain_operands("dmrg", op, nullptr, state, "two-site DMRG requires at least one state edge");
    if (center >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "dmrg: center " + std::to_string(center) + " is not a state node (" + std::to_string(n) + " sites)");
    for (size_t i = 0; i + 1 < n; ++i) check_bond_step_dims("dmrg", i, state[i][0], state[i][1], state[i + 1][1], state[i + 1][2], op[i][3], max_iter);
}

// ------------------------------------------------------------------------------------------------ Lanczos
void Lanczos::reserve(size_t len, size_t max_iter)
{
    ar_.reserve(len, max_iter);
    grow(eng_, ax_, len);
}

void Lanczos::residual_sums(const GmresApply& apply, size_t len, const double* d_v, double lambda, double sums[3])
{
    hipStream_t st = eng_.stream();
    KrylovOrth& gs = ar_.orth();
    grow(eng_, ax_, len);
    gs.reserve(1);
    apply(d_v, ax_.get());
    eig_residual_launch(d_v, ax_.get(), lambda, nullptr, len, gs.npart(), st);
    krylov_finish_launch(gs.npart(), gs_workgroups(len), 3, gs.scalars() + 1, st);
    T4A_HIP(hipGetLastError());
    T4A_HIP(hipMemcpyAsync(sums, gs.scalars() + 1, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    eng_.sync();
}

LanczosResult Lanczos::solve(const GmresApply& apply, size_t len, double* d_x, const LanczosOptions& o)
{
    LanczosResult res;
    hipStream_t st = eng_.stream();
    const size_t m = o.max_iter;
    reserve(len, m);
    const double n0 = ar_.start(d_x, len); // v_0 = theta_0 / |theta_0|
    if (!(n0 > o.breakdown_tol)) throw Error(T4A_GPU_INVALID_ARGUMENT, "hermitian_lanczos_lowest_eigenpair: the initial vector is numerically zero");

    std::vector<double> coef;
    // the Ritz vector sum_i c_i v_i into d_x and its true residual
    auto finalise = [&](size_t dim, double lambda, const std::vector<double>& c) {
        T4A_HIP(hipMemcpyAsync(ar_.coef(), c.data(), sizeof(double) * dim, hipMemcpyHostToDevice, st));
        // (the shares of |x|^2 that the combine leaves in npart are not read here: eig_residual below overwrites them with its own three
        // sums, and <v, v> comes from there)
        krylov_combine_launch(ar_.basis(), len, (int)dim, ar_.coef(), d_x, len, ar_.orth().npart(), st);
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
        const double beta = ar_.step(apply, j, o.hermitian_tol, "hermitian_lanczos_lowest_eigenpair");
        ++res.apply_calls;
        const size_t dim = j + 1;
        const double lambda = jacobi_lowest_eigenpair(ar_.projected(), dim, coef);
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
    KrylovOrth& gs = ar_.orth();
    fill_launch(ar_.basis(), len * (nb + 1), 1.0 / std::sqrt((double)len), st);
    fill_launch(ar_.coef(), nb, 1.0 / std::sqrt((double)nb), st);
    fill_launch(ax_.get(), len, 1.0, st);
    const int G = gs_workgroups(len);
    const std::function<void()> pieces[3] = {
        [&] { krylov_combine_launch(ar_.basis(), len, (int)nb, ar_.coef(), x.get(), len, gs.npart(), st); },
        [&] { eig_residual_launch(x.get(), ax_.get(), 0.5, nullptr, len, gs.npart(), st); },
        [&] { krylov_finish_launch(gs.npart(), G, 3, gs.scalars() + 1, st); },
    };
    time_pieces(st, pieces, 3, reps, ms);
    eng_.sync();
}

// ------------------------------------------------------------------------------------------------ the sweeps
namespace {

// the Rayleigh quotient at the region of `center` (rayleigh_region: the centre and a neighbour)
double rayleigh_quotient(ProjectedOperator& po, Lanczos& lz, size_t center, double real_scalar_tol)
{
    const size_t n = po.len();
    const size_t i = center + 1 < n ? center : center - 1;
    po.check_step(i, 1, "dmrg");
    DevBuf<double> theta;
    const size_t len = po.two_site_vector(i, theta);
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
    po.canonicalize(center);
    Lanczos lz(e);
    DevBuf<double> theta;
    const SvdOptions so = sweep_svd_options(o.has_svd_policy, o.svd_policy, o.has_max_bond_dim, o.max_bond_dim);
    double last_energy = 0.0;

    auto bond_step = [&](size_t i, bool move_right) {
        po.check_step(i, o.lanczos.max_iter, "dmrg");
        const size_t len = po.two_site_vector(i, theta); // theta_0 = x_i x_{i+1}
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
        for_each_bond_from(center, n, bond_step);
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
    require_tol(real_scalar_tol, "invalid DMRG option real_scalar_tol: must be finite and non-negative");
    dmrg_validate_shapes(op.dims4(), dims3_of(state.cores), center, 1);
    ProjectedOperator po(op, state, nullptr);
    Engine& e = po.engine();
    po.canonicalize(center);
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
    DevBuf<double> dH = upload_vector(st, H, n * n), dx = upload_vector(st, v0, n);
    Lanczos lz(e);
    const LanczosResult r = lz.solve(dense_apply(dH.get(), n, st), n, dx.get(), o);
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
