// tdvp.hip — two-site and one-site TDVP on the device (see tdvp.hpp).  Shape bookkeeping, the region plan and the exponential of the small projected
// matrix of the Krylov solver (a cyclic Jacobi) are host work; every other floating-point operation runs in gfx950 kernels: the
// projected applies of linsolve.hpp, the Arnoldi step of krylov.hpp (with the projections of kernels_tdvp.hip), the combination of
// kernels_dmrg.hip, the QR and the SVD behind QrSweep and tensor_svd.
#include "tdvp.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <limits>
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

// The rules both modes share, each with the message of the reference
namespace {
void require_sweeps_and_order(const TdvpOptions& o)
{
    if (o.nsweeps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option nsweeps: must be greater than zero");
    if (o.order != 1 && o.order != 2 && o.order != 4)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "TDVP applyexp order " + std::to_string(o.order) + " is not supported; supported orders are 1, 2, and 4");
}
void require_finite_exponent(const TdvpOptions& o)
{
    if (!std::isfinite(o.exponent_step_re) || !std::isfinite(o.exponent_step_im))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option exponent_step: real and imaginary parts must be finite");
}
void require_real_exponent(const TdvpOptions& o, const char* who) // this project's own restriction
{
    if (o.exponent_step_im != 0.0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": exponent_step must be real here: real-time evolution (a non-zero imaginary part) needs complex "
                                                                 "tensor trains, which this project does not have");
}
void require_positive_max_bond_dim(const TdvpOptions& o)
{
    if (o.has_max_bond_dim && o.max_bond_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option max_bond_dim: must be greater than zero when set");
}
} // namespace

void TdvpOptions::validate(TdvpMode mode) const
{
    if (mode == TdvpMode::TwoSite) {
        if (nsite != 1 && nsite != 2)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "TDVP supports nsite=1 or nsite=2 in this version, got nsite=" + std::to_string(nsite));
        require_sweeps_and_order(*this);
        require_finite_exponent(*this);
        require_positive_max_bond_dim(*this);
        if (nsite == 1) // this project's own restriction
            throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp: one-site TDVP (nsite=1) is not implemented here: it needs the bond-centre apply; use nsite=2");
        require_real_exponent(*this, "tdvp");
        krylov.validate();
        if (has_svd_policy) validate_svd_policy(svd_policy, "TdvpOptions::svd_policy");
    } else {
        if (nsite != 1)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_one_site: one-site TDVP requires nsite=1, got nsite=" + std::to_string(nsite) + "; nsite=2 is tdvp");
        require_sweeps_and_order(*this);
        require_finite_exponent(*this);
        require_real_exponent(*this, "tdvp_one_site");
        require_positive_max_bond_dim(*this);
        if (has_max_bond_dim) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option max_bond_dim: one-site TDVP has fixed ranks; use nsite=2 for truncation");
        if (has_svd_policy) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option svd_policy: one-site TDVP has fixed ranks; use nsite=2 for truncation");
        krylov.validate();
    }
}

namespace {
void require_state_node(const char* who, size_t n, size_t center)
{
    if (center >= n)
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": TDVP center " + std::to_string(center) + " is not a state node (" + std::to_string(n) + " sites)");
}
void require_end_center(size_t n, size_t center)
{
    require_state_node("tdvp", n, center);
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

void tdvp_one_site_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter)
{
    const size_t n = state.size();
    validate_chain_operands("tdvp_one_site", op, nullptr, state, "a single site has no bond to correct and the shared chain checks need two sites: one-site TDVP requires at least two sites");
    require_state_node("tdvp_one_site", n, center);
    for (size_t c = 0; c < n; ++c) check_site_step_dims("tdvp_one_site", c, state[c][0], state[c][1], state[c][2], op[c][3], max_iter);
    for (size_t i = 0; i + 1 < n; ++i) check_bond_center_dims("tdvp_one_site", i, state[i][2], state[i][2], op[i][3], max_iter);
}

void tdvp_validate_shapes(TdvpMode mode, const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter)
{
    mode == TdvpMode::TwoSite ? tdvp_validate_shapes(op, state, center, max_iter) : tdvp_one_site_validate_shapes(op, state, center, max_iter);
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

namespace {
// One sweep: the base list once per substep with its exponents scaled by the weight; every even substep (1-based) is the reversed list,
// and `reversed(step)` does to each of its steps what the mode's reversal does beyond the order.
template <class F> std::vector<TdvpStep> expand_sub_steps(const std::vector<TdvpStep>& base, const std::vector<double>& weights, F&& reversed)
{
    std::vector<TdvpStep> steps;
    for (size_t k = 0; k < weights.size(); ++k) {
        std::vector<TdvpStep> part = base;
        for (TdvpStep& s : part) s.exponent = s.exponent * weights[k];
        if ((k + 1) % 2 == 0) {
            std::reverse(part.begin(), part.end());
            for (TdvpStep& s : part) reversed(s);
        }
        steps.insert(steps.end(), part.begin(), part.end());
    }
    return steps;
}
void require_finite_tau(double tau)
{
    if (!std::isfinite(tau)) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid TDVP option exponent_step: real and imaginary parts must be finite");
}
} // namespace

std::vector<TdvpStep> tdvp_plan(size_t n, size_t center, size_t order, double tau)
{
    const std::vector<double> weights = tdvp_sub_steps(order);
    require_finite_tau(tau);
    if (n < 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp: two-site TDVP requires at least one state edge");
    require_end_center(n, center);
    auto node = [&](size_t j) { return center == 0 ? j : n - 1 - j; }; // the chain as the walk from the root sees it
    std::vector<TdvpStep> base;
    for (size_t j = 0; j + 1 < n; ++j) {
        const size_t a = node(j), b = node(j + 1);
        base.push_back({TdvpStepKind::TwoSite, {a, b}, b, tau});
        if (j + 2 < n) base.push_back({TdvpStepKind::SiteCorrection, {b, b}, b, -tau});
    }
    return expand_sub_steps(base, weights, [](TdvpStep& s) { // the nodes reversed, the last node the new centre
        std::swap(s.nodes[0], s.nodes[1]);
        s.new_center = s.nodes[1];
    });
}

std::vector<TdvpStep> tdvp_one_site_plan(size_t n, size_t center, size_t order, double tau)
{
    const std::vector<double> weights = tdvp_sub_steps(order);
    require_finite_tau(tau);
    if (n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_one_site: the plan of an empty chain");
    require_state_node("tdvp_one_site", n, center);
    std::vector<TdvpStep> base; // post order: the left arm leaf first, the right arm leaf first, the centre
    for (size_t j = 0; j < center; ++j) base.push_back({TdvpStepKind::OneSite, {j, j}, j, tau});
    for (size_t j = n - 1; j > center; --j) base.push_back({TdvpStepKind::OneSite, {j, j}, j, tau});
    base.push_back({TdvpStepKind::OneSite, {center, center}, center, tau});
    return expand_sub_steps(base, weights, [](TdvpStep&) {}); // a one-site step is its own mirror image
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

// ------------------------------------------------------------------------------------------------ the bond-centre apply
// Measured on an MI355X at k_a = k_b = k (tools/probe_tdvp_one_site.py): the fused launch takes 0.36 - 0.78 of the
// two GEMMs at k = 8, 16, 32 with W = 4 and at k = 8, 16 with W = 16, and 1.15 - 3.1 times as long at k = 64, 128 with W = 4 and k = 32 with
// W = 16.  A workgroup owns 16 rows whatever the shape and its wavefronts walk W k_b (k_a + k_b) / 4 chunks of the summed indices between
// them, while the GEMM tiles both output dimensions: W k_b (k_a + k_b) is 8192 at the largest measured wins and 32768 at the smallest
// measured losses.  The spread of a measurement (min - max of 7) is below 8 % of its median, every win and loss above 14 %.  Shapes up to
// the measured wins take the fused launch; everything above, the unmeasured shapes between the two included, takes the GEMMs.
namespace {
std::atomic<int> g_bond_route{-1};
}
void tdvp_set_bond_apply_route(int route) { g_bond_route.store(route < 0 || route > 1 ? -1 : route); }

BondApplyRoute tdvp_bond_apply_route(size_t ka, size_t kb, size_t W)
{
    return tdvp_bond_apply_fused_admits(ka, kb, W) && W * kb * (ka + kb) <= TDVP_BOND_FUSED_AUTO_WORK ? BondApplyRoute::Fused : BondApplyRoute::Gemm;
}

void tdvp_bond_apply_gemm(const double* La, const double* C, const double* Rb, double* T, double* Y, int ka, int kb, int W, hipStream_t stream)
{
    gemm_launch(gemm_desc(ka * W, kb, ka, La, ka * W, C, ka, T, ka * W), stream);
    GemmDesc g = gemm_desc(ka, kb, W * kb, T, ka, Rb, kb, Y, ka);
    g.transB = 1;
    gemm_launch(g, stream);
}

namespace {
// The route of an apply that `forced` asks a route of: Gemm is taken as it is, Fused where the envelope admits the shape; Auto, and Fused
// outside the envelope, are the rule.
BondApplyRoute resolve_bond_route(BondApplyRoute forced, size_t ka, size_t kb, size_t W)
{
    if (forced == BondApplyRoute::Gemm || (forced == BondApplyRoute::Fused && tdvp_bond_apply_fused_admits(ka, kb, W))) return forced;
    return tdvp_bond_apply_route(ka, kb, W);
}
} // namespace

void ProjectedOperator::apply_bond_center_prepared(const double* d_c, double* d_out)
{
    hipStream_t st = engine().stream();
    const int forced = g_bond_route.load();
    if (resolve_bond_route(forced < 0 ? BondApplyRoute::Auto : (BondApplyRoute)forced, bc_ka_, bc_kb_, bc_w_) == BondApplyRoute::Fused) {
        tdvp_bond_apply_launch(bc_la_, d_c, bc_rb_, d_out, (int)bc_ka_, (int)bc_kb_, (int)bc_w_, st);
        ++fused_applies;
    } else {
        tdvp_bond_apply_gemm(bc_la_, d_c, bc_rb_, t_.get(), d_out, (int)bc_ka_, (int)bc_kb_, (int)bc_w_, st);
        ++gemm_applies;
    }
}

// ------------------------------------------------------------------------------------------------ the sweeps
namespace {
// What a sweep of either mode runs on: the state inside the projected operator, canonicalised onto `cur`, and the steps of tdvp.hpp.
// `who` is the driver's name in the messages of the step checks.
struct TdvpSweep {
    const TdvpOptions& o;
    const char* who;
    ProjectedOperator po;
    Engine& e;
    hipStream_t st;
    QrSweep sw;
    KrylovExpm kx;
    size_t cur;
    DevBuf<double> theta, cm; // the two-site vector; the bond matrix where it is not the R of the QR sweep
    TdvpResult out;

    TdvpSweep(Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& options, const char* name)
        : o(options), who(name), po(op, init, nullptr), e(po.engine()), st(e.stream()), sw(e), kx(e), cur(center)
    {
        sw.canonicalize(po.x, center);
    }

    void book(const KrylovExpmResult& r)
    {
        out.max_error_estimate = std::max(out.max_error_estimate, r.error_estimate);
        out.max_krylov_iterations = std::max(out.max_krylov_iterations, r.iterations);
        out.stats.krylov_steps += r.iterations;
        out.stats.apply_calls += r.apply_calls;
        out.stats.max_time_splits = std::max(out.stats.max_time_splits, r.time_splits);
        ++out.local_updates;
    }

    // move_center_to_region_full_rank: thin QR steps, every cache that contains a changed site goes stale
    void move_center(size_t target)
    {
        while (cur != target) {
            const size_t next = cur < target ? cur + 1 : cur - 1;
            if (next > cur)
                sw.left_step(po.x, cur);
            else
                sw.right_step(po.x, cur);
            po.invalidate(cur);
            po.invalidate(next);
            cur = next;
            ++out.stats.qr_steps;
        }
    }

    // exp(exponent H_c) on x_c, the centre: the one-site step of the one-site mode, the site correction of the two-site mode
    void site_exponential(size_t c, double exponent)
    {
        po.check_site_step(c, o.krylov.max_iter, who);
        po.prepare_one_site(c);
        book(kx.solve([&](const double* v, double* y) { po.apply_one_site_prepared(v, y); }, po.x[c].size(), po.x[c].buf.get(), exponent, o.krylov));
        po.invalidate(c);
    }

    // exp(exponent H_{i,i+1}) on theta = x_i x_{i+1}, then the split: the singular values go to the new centre, no renormalisation
    void two_site_step(size_t i, double exponent, const SvdOptions& so, bool move_right)
    {
        po.check_step(i, o.krylov.max_iter, who);
        const size_t len = po.two_site_vector(i, theta); // theta_0 = x_i x_{i+1}
        po.prepare(i);
        book(kx.solve([&](const double* v, double* y) { po.apply_prepared(v, y); }, len, theta.get(), exponent, o.krylov));
        po.split_and_advance(i, theta.get(), so, move_right, who);
        cur = move_right ? i + 1 : i;
        ++out.stats.two_site_steps;
    }

    // apply_one_site_bond_correction (mod.rs:702-860) at the centre c towards its neighbour on that side, which becomes the centre
    void bond_correction(size_t c, bool right, double exponent)
    {
        const DevCore& X = po.x[c];
        DevCore q = right ? sw.factor_left(X) : sw.factor_right(X);
        size_t ka, kb; // the shape of C
        double* C;
        if (right) { // x_c as (l s) x r is Q C: C is the R of the sweep
            ka = q.r;
            kb = X.r;
            C = sw.rr.get();
        } else { // x_c as l x (s r) is C Q: the QR of its transpose, C = R^T, l x k
            ka = X.l;
            kb = q.l;
            grow(e, cm, ka * kb);
            transpose_launch(sw.rr.get(), (int)kb, (int)ka, (int)kb, cm.get(), (int)ka, st);
            C = cm.get();
        }
        T4A_HIP(hipGetLastError());
        e.sync(); // the old site is released below
        po.x[c] = std::move(q);
        po.invalidate(c);
        ++out.stats.qr_steps;
        po.prepare_bond_center(c, right);
        po.check_bond_center(o.krylov.max_iter, who);
        book(kx.solve([&](const double* v, double* y) { po.apply_bond_center_prepared(v, y); }, ka * kb, C, exponent, o.krylov));
        ++out.stats.bond_corrections;
        // the neighbour absorbs C'; the environment built with Q stays the valid cache entry
        const size_t nb = right ? c + 1 : c - 1;
        const DevCore& Nb = po.x[nb];
        DevCore nn;
        if (right) {
            nn = DevCore::make(ka, Nb.s, Nb.r);
            const int rest = (int)(Nb.s * Nb.r);
            gemm_launch(gemm_desc((int)ka, rest, (int)kb, C, (int)ka, Nb.buf.get(), (int)kb, nn.buf.get(), (int)ka), st);
        } else {
            nn = DevCore::make(Nb.l, Nb.s, kb);
            const int pm = (int)(Nb.l * Nb.s);
            gemm_launch(gemm_desc(pm, (int)kb, (int)ka, Nb.buf.get(), pm, C, (int)ka, nn.buf.get(), pm), st);
        }
        T4A_HIP(hipGetLastError());
        e.sync();
        po.x[nb] = std::move(nn);
        po.invalidate(nb); // keeps L_{c+1} (right) or R_c (left): they do not contain the neighbour
        cur = nb;
    }

    TdvpResult finish()
    {
        e.sync();
        out.stats.fused_applies = po.fused_applies;
        out.stats.gemm_applies = po.gemm_applies;
        out.state = std::make_unique<TensorTrain>(po.x, st);
        return std::move(out);
    }
};
} // namespace

TdvpResult tdvp(Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& o)
{
    o.validate(TdvpMode::TwoSite);
    tdvp_validate_shapes(op.dims4(), dims3_of(init.cores), center, o.krylov.max_iter);
    const std::vector<TdvpStep> plan = tdvp_plan(init.cores.size(), center, o.order, o.exponent_step_re);
    TdvpSweep s(op, init, center, o, "tdvp");
    const SvdOptions so = sweep_svd_options(o.has_svd_policy, o.svd_policy, o.has_max_bond_dim, o.max_bond_dim);
    for (size_t sweep = 0; sweep < o.nsweeps; ++sweep) {
        for (const TdvpStep& t : plan) {
            if (s.cur != t.nodes[0] && s.cur != t.nodes[1]) { // to the nearest node of the region
                const size_t d0 = s.cur > t.nodes[0] ? s.cur - t.nodes[0] : t.nodes[0] - s.cur, d1 = s.cur > t.nodes[1] ? s.cur - t.nodes[1] : t.nodes[1] - s.cur;
                s.move_center(d0 <= d1 ? t.nodes[0] : t.nodes[1]);
            }
            if (t.kind == TdvpStepKind::TwoSite) {
                const size_t i = std::min(t.nodes[0], t.nodes[1]);
                s.two_site_step(i, t.exponent, so, t.new_center == i + 1);
            } else {
                s.site_exponential(t.nodes[0], t.exponent);
                ++s.out.stats.corrections;
            }
        }
        s.out.sweeps_completed = sweep + 1;
    }
    return s.finish();
}

TdvpResult tdvp_one_site(Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& o)
{
    o.validate(TdvpMode::OneSite);
    tdvp_one_site_validate_shapes(op.dims4(), dims3_of(init.cores), center, o.krylov.max_iter);
    const size_t n = init.cores.size();
    const std::vector<TdvpStep> plan = tdvp_one_site_plan(n, center, o.order, o.exponent_step_re);
    TdvpSweep s(op, init, center, o, "tdvp_one_site");
    for (size_t sweep = 0; sweep < o.nsweeps; ++sweep) {
        for (size_t k = 0; k < plan.size(); ++k) {
            const size_t c = plan[k].nodes[0];
            s.move_center(c);
            s.site_exponential(c, plan[k].exponent);
            ++s.out.stats.one_site_steps;
            if (k + 1 < plan.size() && plan[k + 1].nodes[0] != c) {
                const size_t t = plan[k + 1].nodes[0];
                const bool right = t > c;
                if ((k / n) % 2 == 1) s.move_center(right ? t - 1 : t + 1); // a reversed substep corrects the last edge of the path (tdvp.hpp)
                s.bond_correction(s.cur, right, -plan[k].exponent);
            }
        }
        s.out.sweeps_completed = sweep + 1;
    }
    return s.finish();
}

TdvpResult tdvp(TdvpMode mode, Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& o)
{
    return mode == TdvpMode::TwoSite ? tdvp(op, init, center, o) : tdvp_one_site(op, init, center, o);
}

// ------------------------------------------------------------------------------------------------ test hooks
BondApplyRoute tdvp_bond_apply_host(const double* L, const double* R, const double* C, size_t ka, size_t kb, size_t W, BondApplyRoute route, double* out)
{
    if (route == BondApplyRoute::Fused && !tdvp_bond_apply_fused_admits(ka, kb, W))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_bond_apply: the fused launch holds 16 W k_b doubles in the LDS: W k_b must be at most " +
                                                  std::to_string(TDVP_BOND_FUSED_MAX_PANEL));
    route = resolve_bond_route(route, ka, kb, W);
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dL = upload_vector(st, L, ka * W * ka), dR = upload_vector(st, R, kb * W * kb), dC = upload_vector(st, C, ka * kb), dT, dY;
    dT.reserve(ka * W * kb);
    dY.reserve(ka * kb);
    if (route == BondApplyRoute::Fused)
        tdvp_bond_apply_launch(dL.get(), dC.get(), dR.get(), dY.get(), (int)ka, (int)kb, (int)W, st);
    else
        tdvp_bond_apply_gemm(dL.get(), dC.get(), dR.get(), dT.get(), dY.get(), (int)ka, (int)kb, (int)W, st);
    T4A_HIP(hipGetLastError());
    T4A_HIP(hipMemcpyAsync(out, dY.get(), sizeof(double) * ka * kb, hipMemcpyDeviceToHost, st));
    e.sync();
    return route;
}

void tdvp_bond_apply_time(size_t ka, size_t kb, size_t W, size_t reps, double ms[2])
{
    if (ka == 0 || kb == 0 || W == 0 || reps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_bond_apply_time: ka, kb, W and reps must be positive");
    check_bond_center_dims("tdvp_bond_apply_time", 0, ka, kb, W, 0);
    require_device();
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dL, dR, dC, dT, dY;
    dL.reserve(ka * W * ka);
    dR.reserve(kb * W * kb);
    dC.reserve(ka * kb);
    dT.reserve(ka * W * kb);
    dY.reserve(ka * kb);
    fill_launch(dL.get(), ka * W * ka, 1.0 / std::sqrt((double)(ka * W)), st);
    fill_launch(dR.get(), kb * W * kb, 1.0 / std::sqrt((double)(kb * W)), st);
    fill_launch(dC.get(), ka * kb, 1.0 / std::sqrt((double)(ka * kb)), st);
    const bool fused = tdvp_bond_apply_fused_admits(ka, kb, W);
    const std::function<void()> pieces[2] = {
        [&] { tdvp_bond_apply_launch(dL.get(), dC.get(), dR.get(), dY.get(), (int)ka, (int)kb, (int)W, st); },
        [&] { tdvp_bond_apply_gemm(dL.get(), dC.get(), dR.get(), dT.get(), dY.get(), (int)ka, (int)kb, (int)W, st); },
    };
    if (fused) {
        time_pieces(st, pieces, 2, reps, ms);
    } else {
        ms[0] = std::numeric_limits<double>::quiet_NaN();
        time_pieces(st, pieces + 1, 1, reps, ms + 1);
    }
    e.sync();
}

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
