// fit_sum.hip — see fit_sum.hpp.  Validation, the sweep plan, the rank rule and the norm of the centre are host work; the halves run in
// fit_sum_half_kernel (kernels_fit_sum.hip) or, on the gemm route, in gemm_launch per target; Theta, the environment updates, the QR
// canonicalisation and the SVD split are the GEMM, QrSweep and tensor_svd every chain solver uses.
#include "fit_sum.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace t4a {

namespace {

[[noreturn]] void invalid(const std::string& what) { throw Error(T4A_GPU_INVALID_ARGUMENT, what); }

bool over_int_max(size_t a, size_t b)
{
    if (a == 0 || b == 0) return false;
    return a > (size_t)INT_MAX / b;
}

const char* alg_name(int alg) { return alg == 1 ? "QR" : alg == 2 ? "LU" : "CI"; }

// One half for K targets: the job table (fused) or the products (gemm) on `st`.  cores[k] is T_k[a_k, S, b_k] on the device.
// right == false: env EL chi x A, out P (chi S) x B; right == true: env ER B x chi, out Q A x (S chi).
struct HalfArgs {
    bool right;
    const double* env;
    size_t chi, S;
    const double* const* cores;
    const size_t* a;
    const size_t* b;
    size_t K;
    double* out;
};

void half_totals(const HalfArgs& h, size_t& A, size_t& B)
{
    A = B = 0;
    for (size_t k = 0; k < h.K; ++k) A += h.a[k], B += h.b[k];
}

// -> the number of workgroups; INVALID_ARGUMENT beyond INT_MAX
int half_jobs(const HalfArgs& h, std::vector<FitSumJob>& jobs)
{
    size_t A, B;
    half_totals(h, A, B);
    jobs.assign(h.K, FitSumJob{});
    long long tile = 0;
    size_t offa = 0, offb = 0;
    for (size_t k = 0; k < h.K; ++k) {
        FitSumJob& j = jobs[k];
        const size_t a = h.a[k], b = h.b[k];
        if (!h.right) { // block k of P: EL[:, offa ..] (chi x a) times T_k as a x (S b)
            j.X = h.env + h.chi * offa, j.xrs = 1, j.xcs = (long long)h.chi;
            j.Y = h.cores[k], j.yrs = 1, j.ycs = (long long)a;
            j.m = (int)h.chi, j.k = (int)a, j.n = (int)(h.S * b);
            j.O = h.out + h.chi * h.S * offb, j.ors = 1, j.ors2 = 0, j.rdiv = j.m, j.ocs = (long long)h.chi;
        } else { // block k of Q: T_k as (a S) x b times ER[offb .., :] (b x chi); the row (a, s) lands at a + A s
            j.X = h.cores[k], j.xrs = 1, j.xcs = (long long)(a * h.S);
            j.Y = h.env + offb, j.yrs = 1, j.ycs = (long long)B;
            j.m = (int)(a * h.S), j.k = (int)b, j.n = (int)h.chi;
            j.O = h.out + offa, j.ors = 1, j.ors2 = (long long)A, j.rdiv = (int)a, j.ocs = (long long)(A * h.S);
        }
        j.mfma = fit_sum_job_mfma((size_t)j.m, (size_t)j.k, (size_t)j.n) ? 1 : 0;
        j.tile0 = (int)tile;
        tile += fit_sum_job_tiles((size_t)j.m, (size_t)j.n, j.mfma != 0);
        if (tile > (long long)INT_MAX) invalid("fit_sum: a half launch needs more than INT_MAX workgroups");
        offa += a;
        offb += b;
    }
    return (int)tile;
}

void half_gemm(const HalfArgs& h, hipStream_t st)
{
    size_t A, B;
    half_totals(h, A, B);
    size_t offa = 0, offb = 0;
    for (size_t k = 0; k < h.K; ++k) {
        const size_t a = h.a[k], b = h.b[k];
        if (!h.right) {
            gemm_launch(gemm_desc((int)h.chi, (int)(h.S * b), (int)a, h.env + h.chi * offa, (int)h.chi, h.cores[k], (int)a, h.out + h.chi * h.S * offb,
                                  (int)h.chi),
                        st);
        } else {
            for (size_t s = 0; s < h.S; ++s)
                gemm_launch(gemm_desc((int)a, (int)h.chi, (int)b, h.cores[k] + a * s, (int)(a * h.S), h.env + offb, (int)B, h.out + offa + A * s, (int)(A * h.S)),
                            st);
        }
        offa += a;
        offb += b;
    }
}

double frobenius(Engine& e, const DevCore& c)
{
    const std::vector<double> h = to_host(e, c.buf.get(), c.size());
    double nrm = 0.0;
    for (double v : h) nrm = std::hypot(nrm, v);
    return nrm;
}

class SumFit {
public:
    SumFit(Engine& e, const std::vector<const std::vector<DevCore>*>& targets, const double* w, FitSumRoute route)
        : e_(e), st_(e.stream()), K_(targets.size()), n_(targets[0]->size()), route_(route), t_(targets)
    {
        scaled_.resize(K_);
        core_.assign(n_, std::vector<const double*>(K_));
        l_.assign(n_ + 1, std::vector<size_t>(K_, 1));
        sum_.assign(n_ + 1, K_);
        for (size_t i = 0; i < n_; ++i) {
            sum_[i] = 0;
            for (size_t k = 0; k < K_; ++k) {
                const DevCore& c = (*t_[k])[i];
                core_[i][k] = c.buf.get();
                l_[i][k] = c.l;
                sum_[i] += c.l;
            }
        }
        if (w)
            for (size_t k = 0; k < K_; ++k) {
                if (w[k] == 1.0) continue;
                const DevCore& c = (*t_[k])[0];
                scaled_[k] = DevCore::make(c.l, c.s, c.r);
                linsolve_scale_launch(c.buf.get(), w[k], scaled_[k].buf.get(), c.size(), st_);
                core_[0][k] = scaled_[k].buf.get();
            }
        d_jobs_.reserve(K_);
        envL_.resize(n_);
        envR_.resize(n_ + 1);
        okL_.assign(n_, 0);
        okR_.assign(n_ + 1, 0);
        envL_[0].reserve(K_);
        envR_[n_].reserve(K_);
        fill_launch(envL_[0].get(), K_, 1.0, st_);
        fill_launch(envR_[n_].get(), K_, 1.0, st_);
        okL_[0] = okR_[n_] = 1;
    }

    std::vector<DevCore> psi;

    size_t S(size_t i) const { return (*t_[0])[i].s; }

    void half(bool right, size_t i, const double* env, size_t chi, DevBuf<double>& out)
    {
        const size_t A = sum_[i], B = sum_[i + 1];
        grow(e_, out, right ? A * S(i) * chi : chi * S(i) * B);
        const HalfArgs h{right, env, chi, S(i), core_[i].data(), l_[i].data(), l_[i + 1].data(), K_, out.get()};
        FitSumRoute r = route_;
        if (r == FitSumRoute::Auto) {
            size_t bond = 1;
            for (size_t k = 0; k < K_; ++k) bond = std::max(bond, std::max(l_[i][k], l_[i + 1][k]));
            r = fit_sum_route(K_, bond, chi, S(i));
        }
        if (r == FitSumRoute::Gemm) {
            half_gemm(h, st_);
            return;
        }
        staged_.emplace_back();
        const int tiles = half_jobs(h, staged_.back());
        T4A_HIP(hipMemcpyAsync(d_jobs_.get(), staged_.back().data(), K_ * sizeof(FitSumJob), hipMemcpyHostToDevice, st_));
        fit_sum_half_launch(d_jobs_.get(), (int)K_, tiles, st_);
    }

    // EL_{i+1} = psi_i^T P_i with psi_i read as (c S) x c'
    void left_from(size_t i, const DevBuf<double>& P)
    {
        const DevCore& x = psi[i];
        const size_t B = sum_[i + 1];
        grow(e_, envL_[i + 1], x.r * B);
        GemmDesc g = gemm_desc((int)x.r, (int)B, (int)(x.l * x.s), x.buf.get(), (int)(x.l * x.s), P.get(), (int)(x.l * x.s), envL_[i + 1].get(), (int)x.r);
        g.transA = 1;
        gemm_launch(g, st_);
        okL_[i + 1] = 1;
    }
    // ER_i = Q_i psi_i^T with psi_i read as c x (S c')
    void right_from(size_t i, const DevBuf<double>& Q)
    {
        const DevCore& x = psi[i];
        const size_t A = sum_[i];
        grow(e_, envR_[i], A * x.l);
        GemmDesc g = gemm_desc((int)A, (int)x.l, (int)(x.s * x.r), Q.get(), (int)A, x.buf.get(), (int)x.l, envR_[i].get(), (int)A);
        g.transB = 1;
        gemm_launch(g, st_);
        okR_[i] = 1;
    }
    const double* left_env(size_t i)
    {
        if (!okL_[i]) {
            const double* prev = left_env(i - 1);
            check(i - 1);
            half(false, i - 1, prev, psi[i - 1].l, p_);
            left_from(i - 1, p_);
        }
        return envL_[i].get();
    }
    const double* right_env(size_t i)
    {
        if (!okR_[i]) {
            const double* next = right_env(i + 1);
            check(i);
            half(true, i, next, psi[i].r, q_);
            right_from(i, q_);
        }
        return envR_[i].get();
    }
    // SumFitEnvironment::prepare on a chain: every environment that points towards the centre
    void prepare(size_t center)
    {
        for (size_t i = 1; i <= center; ++i) left_env(i);
        for (size_t i = n_ - 1; i > center; --i) right_env(i);
        settle();
    }
    void check(size_t i) const { fit_sum_check_step(i, psi[i].l, psi[i].s, psi[i].s, psi[i].r, sum_[i], sum_[i + 1], 1); }

    // one site: the elementwise sum, the half of the single site against the all-ones environment on the right
    DevCore one_site()
    {
        half(false, 0, envL_[0].get(), 1, p_);
        const size_t s = S(0);
        DevCore out = DevCore::make(1, s, 1);
        gemm_launch(gemm_desc((int)s, 1, (int)K_, p_.get(), (int)s, envR_[1].get(), (int)K_, out.buf.get(), (int)s), st_);
        settle();
        return out;
    }

    void bond_step(size_t i, bool move_right, const FitSumOptions& o)
    {
        const size_t c = psi[i].l, s1 = psi[i].s, s2 = psi[i + 1].s, cn = psi[i + 1].r, mid = sum_[i + 1];
        fit_sum_check_step(i, c, s1, s2, cn, sum_[i], mid, sum_[i + 2]);
        const double* el = left_env(i);
        const double* er = right_env(i + 2);
        half(false, i, el, c, p_);
        half(true, i + 1, er, cn, q_);
        const int M = (int)(c * s1), N = (int)(s2 * cn);
        grow(e_, theta_, (size_t)M * N);
        gemm_launch(gemm_desc(M, N, (int)mid, p_.get(), M, q_.get(), (int)mid, theta_.get(), M), st_);
        // the bond cap of fit_two_site_update (fit.rs:691-703)
        const bool open = o.has_svd_policy || o.has_qr_rtol;
        const SvdOptions so = sweep_svd_options(o.has_svd_policy, o.svd_policy, o.has_max_bond_dim || !open, o.has_max_bond_dim ? o.max_bond_dim : psi[i].r);
        const TensorView tv{theta_.get(), {(size_t)M, (size_t)N}, {0, 1}};
        const UnfoldPlan un = plan_unfold_split(tv, {0});
        require_factorizable(un, "fit_sum", "svd");
        const UnfoldedFactors f = tensor_svd(e_, tv, un, so);
        DevCore nl = DevCore::make(c, s1, f.keep), nr = DevCore::make(f.keep, s2, cn);
        // Canonical::Left: the first node is the isometry, the second takes S Vt — whichever way the tour moves, its second node being
        // the new centre: moving left the nodes of the step are (i + 1, i), so site i + 1 holds the isometry Vt and site i takes U S
        split_two_site(st_, f.d_left, M, f.d_s, f.d_right, (int)f.k, N, (int)f.keep, move_right, nl, nr);
        T4A_HIP(hipGetLastError());
        settle(); // the old sites are released below
        psi[i] = std::move(nl);
        psi[i + 1] = std::move(nr);
        // after_step: every environment that contains one of the two sites is stale; the side left behind is rebuilt from this step's half
        for (size_t j = i + 1; j < n_; ++j) okL_[j] = 0;
        for (size_t j = 1; j <= i + 1; ++j) okR_[j] = 0;
        if (move_right) left_from(i, p_);
        else right_from(i + 1, q_);
    }

    void settle()
    {
        T4A_HIP(hipGetLastError());
        e_.sync();
        staged_.clear();
    }

private:
    Engine& e_;
    hipStream_t st_;
    size_t K_, n_;
    FitSumRoute route_;
    std::vector<const std::vector<DevCore>*> t_;
    std::vector<DevCore> scaled_;
    std::vector<std::vector<const double*>> core_; // [site][target]
    std::vector<std::vector<size_t>> l_;           // [bond][target]: the left bond of site `bond`, 1 at the end
    std::vector<size_t> sum_;                      // the concatenated bond
    std::vector<DevBuf<double>> envL_, envR_;
    std::vector<char> okL_, okR_;
    DevBuf<double> p_, q_, theta_;
    DevBuf<FitSumJob> d_jobs_;
    std::vector<std::vector<FitSumJob>> staged_; // the host tables of the launches queued since the last synchronisation
};

} // namespace

// ------------------------------------------------------------------------------------------------ options and shapes
void FitSumOptions::validate() const
{
    if (has_convergence_tol) require_tol(convergence_tol, "fit_sum: invalid options: convergence tolerance must be finite and non-negative");
    if (has_qr_rtol) require_tol(qr_rtol, "fit_sum: invalid options: QR relative tolerance must be finite and non-negative");
    const std::string who = "fit_sum: invalid options: invalid fit factorization options: ";
    if (has_max_bond_dim && max_bond_dim == 0) invalid(who + "max_bond_dim must be at least 1");
    if (has_svd_policy) validate_svd_policy(svd_policy, "FitSumOptions::svd_policy");
    if (factorize_alg < 0 || factorize_alg > 3) invalid(who + "unknown factorize_alg");
    if (factorize_alg == 0) {
        if (has_qr_rtol) invalid(who + "SVD factorization does not accept qr_rtol");
    } else if (factorize_alg == 1) {
        if (has_svd_policy) invalid(who + "QR factorization does not accept svd_policy");
    } else {
        if (has_svd_policy) invalid(who + "LU/CI factorization does not accept svd_policy");
        if (has_qr_rtol) invalid(who + "LU/CI factorization does not accept qr_rtol");
    }
    if (factorize_alg != 0)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, std::string("fit_sum: the ") + alg_name(factorize_alg) + " factorization is not implemented (SVD only)");
}

void fit_sum_check_step(size_t i, size_t c, size_t S1, size_t S2, size_t cn, size_t A, size_t B, size_t C)
{
    const size_t M = c * S1, N = S2 * cn;
    if (over_int_max(c, S1) || over_int_max(S2, cn) || over_int_max(M, B) || over_int_max(B, N) || over_int_max(M, N) || over_int_max(c, A) ||
        over_int_max(B, c) || over_int_max(B, cn) || over_int_max(C, cn))
        invalid("fit_sum: a work matrix of the bond step (" + std::to_string(i) + ", " + std::to_string(i + 1) + ") holds more than INT_MAX elements");
}

void fit_sum_validate_shapes(const std::vector<std::vector<std::array<size_t, 3>>>& targets, const std::vector<std::array<size_t, 3>>* initial,
                             size_t center)
{
    if (targets.empty()) invalid("fit_sum: targets must not be empty");
    const std::vector<std::array<size_t, 3>>& init = initial ? *initial : targets[0];
    const size_t n = init.size();
    if (n == 0) invalid("fit_sum: initial TreeTN must not be empty");
    if (center >= n) invalid("fit_sum: center node is not in initial TreeTN");
    for (size_t k = 0; k < targets.size(); ++k) {
        if (targets[k].empty()) invalid("fit_sum: target " + std::to_string(k) + " TreeTN must not be empty");
        if (targets[k].size() != n) invalid("fit_sum: target " + std::to_string(k) + " has an incompatible named topology");
        for (size_t i = 0; i < n; ++i)
            if (targets[k][i][1] != init[i][1]) invalid("fit_sum: target " + std::to_string(k) + " site-space validation failed");
    }
    std::vector<size_t> sum(n + 1, 0);
    for (size_t i = 0; i <= n; ++i)
        for (size_t k = 0; k < targets.size(); ++k) {
            const size_t d = i < n ? targets[k][i][0] : 1;
            if (sum[i] > (size_t)INT_MAX || d > (size_t)INT_MAX) invalid("fit_sum: the concatenated bond " + std::to_string(i) + " of the targets exceeds INT_MAX");
            sum[i] += d;
        }
    for (size_t i = 0; i + 1 < n; ++i) fit_sum_check_step(i, init[i][0], init[i][1], init[i + 1][1], init[i + 1][2], sum[i], sum[i + 1], sum[i + 2]);
    if (n == 1) fit_sum_check_step(0, 1, init[0][1], 1, 1, sum[0], sum[1], 1);
}

// ------------------------------------------------------------------------------------------------ route and plan
FitSumRoute fit_sum_route(size_t n_targets, size_t target_bond, size_t result_bond, size_t site_dim)
{
    (void)result_bond;
    (void)site_dim;
    // DESIGN.md §8 "Variational sum", the table of the halves (result bond 32, S = 2, target bonds 8 .. 256, 1 .. 256 targets): the one
    // launch where its median was below the minimum of the GEMM composition — everywhere but a single target of bond 128 or more,
    // whose left half IS one tuned GEMM.  Bonds above the measured 256 go to gemm_launch (not measured: the launch loads single elements).
    if (target_bond > 256) return FitSumRoute::Gemm;
    if (n_targets == 1 && target_bond >= 128) return FitSumRoute::Gemm;
    return FitSumRoute::Fused;
}

FitSumPlan fit_sum_plan(size_t n_sites, size_t center, size_t n_targets, size_t site_dim, FitSumRoute route)
{
    if (n_sites == 0) invalid("fit_sum: initial TreeTN must not be empty");
    if (center >= n_sites) invalid("fit_sum: center node is not in initial TreeTN");
    if (n_targets == 0) invalid("fit_sum: targets must not be empty");
    if (route == FitSumRoute::Auto) invalid("fit_sum_plan: the route must be fused or gemm");
    FitSumPlan p;
    if (n_sites == 1) return p;
    const bool fused = route == FitSumRoute::Fused;
    p.bond_steps_per_sweep = 2 * (n_sites - 1);
    p.half_launches_per_step = fused ? 2 : 0;
    p.gemms_per_step = 2 + (fused ? 0 : n_targets + n_targets * site_dim);
    p.svds_per_step = 1;
    // towards the centre: `center` left environments (one left half each) and n - 1 - center right ones
    p.prepare_half_launches = fused ? n_sites - 1 : 0;
    p.prepare_gemms = (n_sites - 1) + (fused ? 0 : center * n_targets + (n_sites - 1 - center) * n_targets * site_dim);
    return p;
}

// ------------------------------------------------------------------------------------------------ the driver
FitSumResult fit_sum(const std::vector<const std::vector<DevCore>*>& targets, const std::vector<Engine*>& target_engines, const double* coefficients,
                     const std::vector<DevCore>* initial, Engine* initial_engine, size_t center, const FitSumOptions& o, FitSumRoute route)
{
    o.validate();
    std::vector<std::vector<std::array<size_t, 3>>> dims;
    for (const auto* t : targets) dims.push_back(dims3_of(*t));
    std::vector<std::array<size_t, 3>> idims;
    if (initial) idims = dims3_of(*initial);
    fit_sum_validate_shapes(dims, initial ? &idims : nullptr, center);
    if (coefficients)
        for (size_t k = 0; k < targets.size(); ++k)
            if (!std::isfinite(coefficients[k])) invalid("fit_sum: coefficient " + std::to_string(k) + " is not finite");
    require_device();
    for (Engine* te : target_engines)
        if (te) te->sync();
    if (initial_engine) initial_engine->sync();

    Engine e;
    hipStream_t st = e.stream();
    FitSumResult out;
    const std::vector<DevCore>& start = initial ? *initial : *targets[0];
    const size_t n = start.size();
    auto finish = [&](std::vector<DevCore>&& cores) {
        T4A_HIP(hipGetLastError());
        e.sync();
        out.cores = std::move(cores);
        for (size_t i = 1; i < out.cores.size(); ++i) out.link_dims.push_back(out.cores[i].l);
    };
    if (o.nfullsweeps == 0) {
        finish(clone_cores(start, st));
        return out;
    }
    SumFit fit(e, targets, coefficients, route);
    if (n == 1) {
        std::vector<DevCore> one;
        one.push_back(fit.one_site());
        finish(std::move(one));
        return out;
    }
    fit.psi = clone_cores(start, st);
    {
        QrSweep sw(e);
        sw.canonicalize(fit.psi, center);
    }
    fit.prepare(center);
    double before = o.has_convergence_tol ? frobenius(e, fit.psi[center]) : 0.0;
    for (size_t sweep = 0; sweep < o.nfullsweeps; ++sweep) {
        for_each_bond_from(center, n, [&](size_t i, bool move_right) {
            fit.bond_step(i, move_right, o);
            ++out.local_updates;
        });
        out.sweeps_completed = sweep + 1;
        const double after = frobenius(e, fit.psi[center]);
        out.norms.push_back(after);
        if (o.has_convergence_tol) {
            // a zero norm on either side: log 0 - log 0 is NaN and never below the tolerance
            const double change = std::fabs(std::exp(std::log(after) - std::log(before)) - 1.0);
            if (change < o.convergence_tol) {
                out.converged = true;
                break;
            }
            before = after;
        }
    }
    fit.settle();
    finish(std::move(fit.psi));
    return out;
}

// ------------------------------------------------------------------------------------------------ test hook and probe
namespace {
void require_half_dims(size_t chi, size_t S, const size_t* a, const size_t* b, size_t K, size_t& A, size_t& B, size_t& cores)
{
    if (K == 0) invalid("fit_sum_half: no target");
    if (chi == 0 || S == 0) invalid("fit_sum_half: a dimension of 0");
    A = B = cores = 0;
    for (size_t k = 0; k < K; ++k) {
        if (a[k] == 0 || b[k] == 0) invalid("fit_sum_half: a bond of 0");
        if (over_int_max(a[k], S) || over_int_max(a[k] * S, b[k])) invalid("fit_sum_half: a core holds more than INT_MAX elements");
        A += a[k], B += b[k], cores += a[k] * S * b[k];
        if (A > (size_t)INT_MAX || B > (size_t)INT_MAX || cores > (size_t)INT_MAX) invalid("fit_sum_half: the operands hold more than INT_MAX elements");
    }
    if (over_int_max(chi, S) || over_int_max(chi * S, A) || over_int_max(chi * S, B)) invalid("fit_sum_half: a work matrix holds more than INT_MAX elements");
}
} // namespace

std::vector<double> fit_sum_half(bool right, FitSumRoute route, const double* env, size_t chi, size_t S, const double* cores, const size_t* a, const size_t* b,
                                 size_t K, const double* fill)
{
    if (route != FitSumRoute::Fused && route != FitSumRoute::Gemm) invalid("fit_sum_half: the route must be fused or gemm");
    size_t A, B, nc;
    require_half_dims(chi, S, a, b, K, A, B, nc);
    require_device();
    Engine e;
    hipStream_t st = e.stream();
    const size_t n_env = right ? B * chi : chi * A, n_out = right ? A * S * chi : chi * S * B;
    DevBuf<double> d_env = upload_vector(st, env, n_env), d_cores = upload_vector(st, cores, nc), d_out;
    const size_t guard = fill ? FIT_SUM_HALF_GUARD : 0; // behind the output: what no job may touch
    d_out.reserve(n_out + guard);
    if (fill) fill_launch(d_out.get(), n_out + guard, *fill, st);
    std::vector<const double*> ptr(K);
    size_t off = 0;
    for (size_t k = 0; k < K; ++k) {
        ptr[k] = d_cores.get() + off;
        off += a[k] * S * b[k];
    }
    const HalfArgs h{right, d_env.get(), chi, S, ptr.data(), a, b, K, d_out.get()};
    std::vector<FitSumJob> jobs;
    DevBuf<FitSumJob> d_jobs;
    if (route == FitSumRoute::Gemm) {
        half_gemm(h, st);
    } else {
        const int tiles = half_jobs(h, jobs);
        d_jobs.reserve(K);
        T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), K * sizeof(FitSumJob), hipMemcpyHostToDevice, st));
        fit_sum_half_launch(d_jobs.get(), (int)K, tiles, st);
    }
    T4A_HIP(hipGetLastError());
    return to_host(e, d_out.get(), n_out + guard);
}

void fit_sum_time_half(bool right, size_t K, size_t bond, size_t S, size_t chi, size_t reps, double ms[2])
{
    if (reps == 0) invalid("fit_sum_time_half: reps must be positive");
    std::vector<size_t> a(K, bond), b(K, bond);
    size_t A, B, nc;
    require_half_dims(chi, S, a.data(), b.data(), K, A, B, nc);
    require_device();
    Engine e;
    hipStream_t st = e.stream();
    const size_t n_env = chi * A, n_out = chi * S * A;
    DevBuf<double> d_env, d_cores, d_out;
    d_env.reserve(n_env);
    d_cores.reserve(nc);
    d_out.reserve(n_out);
    fill_launch(d_env.get(), n_env, 0.5, st); // constant operands: the time does not depend on the values
    fill_launch(d_cores.get(), nc, 0.25, st);
    std::vector<const double*> ptr(K);
    for (size_t k = 0; k < K; ++k) ptr[k] = d_cores.get() + k * bond * S * bond;
    const HalfArgs h{right, d_env.get(), chi, S, ptr.data(), a.data(), b.data(), K, d_out.get()};
    std::vector<FitSumJob> jobs;
    const int tiles = half_jobs(h, jobs);
    DevBuf<FitSumJob> d_jobs;
    d_jobs.reserve(K);
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), K * sizeof(FitSumJob), hipMemcpyHostToDevice, st));
    const std::function<void()> pieces[2] = {
        [&] { fit_sum_half_launch(d_jobs.get(), (int)K, tiles, st); },
        [&] { half_gemm(h, st); },
    };
    time_pieces(st, pieces, 2, reps, ms);
    T4A_HIP(hipGetLastError());
    e.sync();
}

} // namespace t4a
