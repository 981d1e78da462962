// tdvp.hip — two-site TDVP on the device (see tdvp.hpp).  Shape bookkeeping, the region plan and the exponential of the small projected
// matrix of the Krylov solver (a cyclic Jacobi) are host work; every other floating-point operation runs in gfx950 kernels: the
// projected applies of linsolve.hpp, the Arnoldi step of krylov.hpp (with the projections of kernels_tdvp.hip), the combination of
// kernels_dmrg.hip, the QR and the SVD behind QrSweep and tensor_svd.
#include "tdvp.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

// ------------------------------------------------------------------------------------------------ options and shapes
void KrylovExpmOptions::validate() const
{
    const std::string who = "hermitian_krylov_expm_multiply: ";
    if (max_iter == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, who + "max_iter must be greater than zero");
    if (max_iter > LINSOLVE_RESTART_DIM_MAX)
        throw Error(T4A_GPU_INVALID_ARGUMENT, who + "max_iter above " + std::to_string(LINSOLVE_RESTART_DIM_MAX) + " is not supported");
    if (max_time_splits == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, who + "max_time_splits must be greater than zero");
    require_tol(tol, who + "tol must be finite and non-negative");
    require_tol(breakdown_tol, who + "breakdown_tol must be finite and non-negative");
    require_tol(hermitian_tol, who + "hermitian_tol must be finite and non-negative");
}

void TdvpOptions::validate() const
{
    if (nsite != 1 && nsite != 2)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "TDVP supports nsite=1 or nsite=2 in this version, got nsite=" + std::to_string(nsite));
    if (nsweeps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option nsweeps: must be greater than zero");
    if (order != 1 && order != 2 && order != 4)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "TDVP applyexp order " + std::to_string(order) + " is not supported; supported orders are 1, 2, and 4");
    if (!std::isfinite(exponent_step_re) || !std::isfinite(exponent_step_im))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option exponent_step: real and imaginary parts must be finite");
    if (has_max_bond_dim && max_bond_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option max_bond_dim: must be greater than zero when set");
    // this project's own restrictions
    if (nsite == 1)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp: one-site TDVP (nsite=1) is not implemented here: it needs the bond-centre apply; use nsite=2");
    if (exponent_step_im != 0.0)
        throw Error(T4A_GPU_INVALID_ARGUMENT,
                    "tdvp: exponent_step must be real here: real-time evolution (a non-zero imaginary part) needs complex tensor trains, which this project does not have");
    krylov.validate();
    if (has_svd_policy) validate_svd_policy(svd_policy, "TdvpOptions::svd_policy");
}

namespace {
void require_end_center(size_t n, size_t center)
{
    if (center >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp: TDVP center " + std::to_string(center) + " is not a state node (" + std::to_string(n) + " sites)");
    if (center != 0 && center != n - 1)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp: center " + std::to_string(center) + " is an inner node of the chain: the two-site region plan from an inner root applies the site "
                                              "correction at a leaf instead of the root, which is not a projector splitting; start from 0 or " + std::to_string(n - 1));
}
} // namespace

void tdvp_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter)
{
    const size_t n = state.size();
    validate_chain_operands("tdvp", op, nullptr, state, "two-site TDVP requires at least one state edge");
    require_end_center(n, center);
    for (size_t i = 0; i + 1 < n; ++i) check_bond_step_dims("tdvp", i, state[i][0], state[i][1], state[i + 1][1], state[i + 1][2], op[i][3], max_iter);
    for (size_t c = 1; c + 1 < n; ++c) check_site_step_dims("tdvp", c, state[c][0], state[c][1], state[c][2], op[c][3], max_iter);
}

// ------------------------------------------------------------------------------------------------ the plan
std::vector<double> tdvp_sub_steps(size_t order)
{
    if (order == 1) return {1.0};
    if (order == 2) return {0.5, 0.5};
    if (order == 4) {
        const double s = 1.0 / (2.0 - std::pow(2.0, 1.0 / 3.0));
        return {s / 2.0, s / 2.0, 0.5 - s, 0.5 - s, s / 2.0, s / 2.0};
    }
    throw Error(T4A_GPU_INVALID_ARGUMENT, "TDVP applyexp order " + std::to_string(order) + " is not supported; supported orders are 1, 2, and 4");
}

std::vector<TdvpStep> tdvp_plan(size_t n, size_t center, size_t order, double tau)
{
    const std::vector<double> weights = tdvp_sub_steps(order);
    if (!std::isfinite(tau)) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option exponent_step: real and imaginary parts must be finite");
    if (n < 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp: two-site TDVP requires at least one state edge");
    require_end_center(n, center);
    auto node = [&](size_t j) { return center == 0 ? j : n - 1 - j; }; // the chain as the walk from the root sees it
    std::vector<TdvpStep> base;
    for (size_t j = 0; j + 1 < n; ++j) {
        const size_t a = node(j), b = node(j + 1);
        base.push_back({TdvpStepKind::TwoSite, {a, b}, b, tau});
        if (j + 2 < n) base.push_back({TdvpStepKind::SiteCorrection, {b, b}, b, -tau});
    }
    std::vector<TdvpStep> steps;
    for (size_t k = 0; k < weights.size(); ++k) {
        std::vector<TdvpStep> part = base;
        for (TdvpStep& s : part) s.exponent = s.exponent * weights[k];
        if ((k + 1) % 2 == 0) {
            std::reverse(part.begin(), part.end());
            for (TdvpStep& s : part) {
                std::swap(s.nodes[0], s.nodes[1]);
                s.new_center = s.nodes[1];
            }
        }
        steps.insert(steps.end(), part.begin(), part.end());
    }
    return steps;
}

// ------------------------------------------------------------------------------------------------ the Krylov exponential
void KrylovExpm::reserve(size_t len, size_t max_iter)
{
    ar_.reserve(len, max_iter);
    grow(eng_, start_, len);
}

// hermitian_krylov_expm_multiply_once (krylov.rs:790-906)
KrylovExpmResult KrylovExpm::once(const GmresApply& apply, size_t len, double* d_x, double tau, const KrylovExpmOptions& o)
{
    KrylovExpmResult res;
    hipStream_t st = eng_.stream();
    const size_t m = o.max_iter;
    const double n0 = ar_.start(d_x, len); // v_0 = theta / |theta|
    if (n0 <= o.breakdown_tol) {
        res.converged = true;
        return res;
    }
    const double threshold = o.tol * std::max(n0, 1.0);
    std::vector<double> lams, q, coef, scaled;
    // out = |theta| sum_i c_i v_i into d_x: the coefficients scaled on the host, one copy
    auto finalise = [&](size_t dim) {
        scaled.resize(dim);
        for (size_t i = 0; i < dim; ++i) scaled[i] = n0 * coef[i];
        T4A_HIP(hipMemcpyAsync(ar_.coef(), scaled.data(), sizeof(double) * dim, hipMemcpyHostToDevice, st));
        krylov_combine_launch(ar_.basis(), len, (int)dim, ar_.coef(), d_x, len, ar_.orth().npart(), st);
        T4A_HIP(hipGetLastError());
        eng_.sync();
        res.iterations = res.apply_calls = dim;
    };
    for (size_t j = 0; j < m; ++j) {
        const double beta = ar_.step(apply, j, o.hermitian_tol, "hermitian_krylov_expm_multiply");
        const size_t dim = j + 1;
        // c = Q exp(tau Lambda) Q^T e_1
        jacobi_eigh(ar_.projected(), dim, lams, q);
        coef.assign(dim, 0.0);
        for (size_t k = 0; k < dim; ++k) {
            const double f = std::exp(tau * lams[k]) * q[dim * k];
            for (size_t r = 0; r < dim; ++r) coef[r] = coef[r] + q[r + dim * k] * f;
        }
        const bool broke_down = beta <= o.breakdown_tol;
        const double estimate = broke_down ? 0.0 : n0 * beta * std::fabs(coef[dim - 1]);
        res.error_estimate = estimate;
        if (broke_down || estimate <= threshold) {
            finalise(dim);
            res.converged = true;
            return res;
        }
    }
    finalise(m);
    return res; // converged = false
}

KrylovExpmResult KrylovExpm::solve(const GmresApply& apply, size_t len, double* d_x, double tau, const KrylovExpmOptions& o)
{
    KrylovExpmResult out;
    out.converged = true;
    if (tau == 0.0) return out;
    hipStream_t st = eng_.stream();
    reserve(len, o.max_iter);
    if (ar_.orth().norm(d_x, len) <= o.breakdown_tol) return out;
    T4A_HIP(hipMemcpyAsync(start_.get(), d_x, sizeof(double) * len, hipMemcpyDeviceToDevice, st));
    size_t splits = 1;
    for (bool first = true;; first = false) {
        if (!first) T4A_HIP(hipMemcpyAsync(d_x, start_.get(), sizeof(double) * len, hipMemcpyDeviceToDevice, st));
        const double step = tau / (double)splits;
        KrylovExpmResult acc;
        acc.converged = true;
        for (size_t s = 0; s < splits; ++s) {
            const KrylovExpmResult r = once(apply, len, d_x, step, o);
            acc.iterations += r.iterations;
            acc.apply_calls += r.apply_calls;
            acc.error_estimate = std::max(acc.error_estimate, r.error_estimate);
            if (!r.converged) {
                acc.converged = false;
                break;
            }
        }
        out.apply_calls += acc.apply_calls;
        if (acc.converged) {
            out.iterations = acc.iterations;
            out.error_estimate = acc.error_estimate;
            out.time_splits = splits;
            return out;
        }
        if (splits >= o.max_time_splits)
            throw Error(T4A_GPU_INTERNAL_ERROR, "hermitian_krylov_expm_multiply did not converge within max_time_splits=" + std::to_string(o.max_time_splits) +
                                                    " and max_iter=" + std::to_string(o.max_iter));
        splits = splits > o.max_time_splits / 2 ? o.max_time_splits : 2 * splits; // min(2 splits, max_time_splits)
    }
}

// ------------------------------------------------------------------------------------------------ the sweeps
TdvpResult tdvp(Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& o)
{
    o.validate();
    tdvp_validate_shapes(op.dims4(), dims3_of(init.cores), center, o.krylov.max_iter);
    const std::vector<TdvpStep> plan = tdvp_plan(init.cores.size(), center, o.order, o.exponent_step_re);
    TdvpResult out;
    ProjectedOperator po(op, init, nullptr);
    Engine& e = po.engine();
    hipStream_t st = e.stream();
    QrSweep sw(e);
    sw.canonicalize(po.x, center);
    size_t cur = center;
    KrylovExpm kx(e);
    DevBuf<double> theta;
    const SvdOptions so = sweep_svd_options(o.has_svd_policy, o.svd_policy, o.has_max_bond_dim, o.max_bond_dim);

    auto book = [&](const KrylovExpmResult& r) {
        out.max_error_estimate = std::max(out.max_error_estimate, r.error_estimate);
        out.max_krylov_iterations = std::max(out.max_krylov_iterations, r.iterations);
        out.stats.krylov_steps += r.iterations;
        out.stats.apply_calls += r.apply_calls;
        out.stats.max_time_splits = std::max(out.stats.max_time_splits, r.time_splits);
        ++out.local_updates;
    };
    // move_center_to_region_full_rank: thin QR steps to the nearest node of the region
    auto move_center = [&](size_t target) {
        while (cur < target) {
            sw.left_step(po.x, cur);
            po.invalidate(cur);
            po.invalidate(cur + 1);
            ++cur;
        }
        while (cur > target) {
            sw.right_step(po.x, cur);
            po.invalidate(cur);
            po.invalidate(cur - 1);
            --cur;
        }
    };

    for (size_t sweep = 0; sweep < o.nsweeps; ++sweep) {
        for (const TdvpStep& s : plan) {
            if (cur != s.nodes[0] && cur != s.nodes[1]) {
                const size_t d0 = cur > s.nodes[0] ? cur - s.nodes[0] : s.nodes[0] - cur, d1 = cur > s.nodes[1] ? cur - s.nodes[1] : s.nodes[1] - cur;
                move_center(d0 <= d1 ? s.nodes[0] : s.nodes[1]);
            }
            if (s.kind == TdvpStepKind::TwoSite) {
                const size_t i = std::min(s.nodes[0], s.nodes[1]);
                po.check_step(i, o.krylov.max_iter, "tdvp");
                const size_t len = po.two_site_vector(i, theta); // theta_0 = x_i x_{i+1}
                po.prepare(i);
                book(kx.solve([&](const double* v, double* y) { po.apply_prepared(v, y); }, len, theta.get(), s.exponent, o.krylov));
                po.split_and_advance(i, theta.get(), so, s.new_center == i + 1, "tdvp"); // the singular values go to the new centre, no renormalisation
                ++out.stats.two_site_steps;
            } else {
                const size_t c = s.nodes[0];
                po.check_site_step(c, o.krylov.max_iter, "tdvp");
                po.prepare_one_site(c);
                book(kx.solve([&](const double* v, double* y) { po.apply_one_site_prepared(v, y); }, po.x[c].size(), po.x[c].buf.get(), s.exponent, o.krylov));
                po.invalidate(c);
                ++out.stats.corrections;
            }
            cur = s.new_center;
        }
        out.sweeps_completed = sweep + 1;
    }
    e.sync();
    out.state = std::make_unique<TensorTrain>(po.x, st);
    return out;
}

// ------------------------------------------------------------------------------------------------ test hook
KrylovExpmResult krylov_expm_dense(const double* H, size_t n, const double* v0, double tau, const KrylovExpmOptions& o, double* v_out)
{
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dH = upload_vector(st, H, n * n), dx = upload_vector(st, v0, n);
    KrylovExpm kx(e);
    const KrylovExpmResult r = kx.solve(dense_apply(dH.get(), n, st), n, dx.get(), tau, o);
    T4A_HIP(hipMemcpyAsync(v_out, dx.get(), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    e.sync();
    return r;
}

} // namespace t4a
