// linsolve.hip — the two-site linear solver (a0 + a1 A) x = b on the device (see linsolve.hpp).  Shape bookkeeping, the Givens
// rotations and the small triangular solve of GMRES are host work; every other floating-point operation runs in gfx950 kernels:
// the half-operator builders and the Gram–Schmidt launches (kernels_linsolve.hip), the f64-MFMA GEMM (kernels_dense.hip), the
// Householder QR and the Jacobi SVD behind tensor_svd (kernels_linalg.hip), the naive MPO product of the residual (kernels_mpo.hip).
// The state is re-gauged by QrSweep and split by split_two_site (tt_chain.hpp).
#include "linsolve.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

namespace {

bool above_int_max(std::initializer_list<size_t> factors)
{
    const unsigned long long lim = INT_MAX;
    unsigned long long n = 1;
    for (size_t x : factors) {
        if (x == 0) return false;
        if (x > lim || n * x > lim) return true;
        n *= x;
    }
    return false;
}

void check_step_dims(size_t i, size_t chi_l, size_t d1, size_t d2, size_t chi_r, size_t W, size_t restart_dim)
{
    check_bond_step_dims("square_linsolve", i, chi_l, d1, d2, chi_r, W, restart_dim);
}

double host_norm(Engine& eng, const DevCore& c)
{
    const std::vector<double> h = to_host(eng, c.buf.get(), c.size());
    double s = 0.0;
    for (double v : h) s = s + v * v;
    return std::sqrt(s);
}

// |t| from the QR right-canonical form of a copy of its cores
double canonical_norm(TensorTrain& t)
{
    if (t.len() == 0) return 0.0;
    std::vector<DevCore> cores = clone_cores(t.cores, t.eng.stream());
    QrSweep sw(t.eng);
    sw.canonicalize(cores, 0);
    return host_norm(t.eng, cores[0]);
}

} // namespace

// ------------------------------------------------------------------------------------------------ options and shapes
void check_bond_step_dims(const char* who, size_t i, size_t chi_l, size_t d1, size_t d2, size_t chi_r, size_t W, size_t basis_dim)
{
    const size_t M = chi_l * d1, N = d2 * chi_r;
    if (above_int_max({W, M, M}) || above_int_max({W, N, N}) || above_int_max({W, M, N}) || above_int_max({basis_dim + 1, M, N}))
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": a work buffer of the bond step (" + std::to_string(i) + ", " + std::to_string(i + 1) +
                                                  ") holds more than INT_MAX elements");
}

void check_site_step_dims(const char* who, size_t c, size_t chi_l, size_t d, size_t chi_r, size_t W, size_t basis_dim)
{
    const size_t M = chi_l * d;
    if (above_int_max({W, M, M}) || above_int_max({W, M, chi_r}) || above_int_max({chi_r, W, chi_r}) || above_int_max({basis_dim + 1, M, chi_r}))
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": a work buffer of the one-site step at site " + std::to_string(c) + " holds more than INT_MAX elements");
}

void check_bond_center_dims(const char* who, size_t i, size_t ka, size_t kb, size_t W, size_t basis_dim)
{
    if (above_int_max({ka, W, ka}) || above_int_max({kb, W, kb}) || above_int_max({ka, W, kb}) || above_int_max({basis_dim + 1, ka, kb}))
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": a work buffer of the bond-centre step at the bond (" + std::to_string(i) + ", " +
                                                  std::to_string(i + 1) + ") holds more than INT_MAX elements");
}

void LinsolveOptions::validate() const
{
    if (gmres_restart_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "LinsolveOptions::gmres_restart_dim must be greater than zero");
    if (gmres_restart_dim > LINSOLVE_RESTART_DIM_MAX)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "LinsolveOptions::gmres_restart_dim above " + std::to_string(LINSOLVE_RESTART_DIM_MAX) + " is not supported");
    if (gmres_max_restarts == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "LinsolveOptions::gmres_max_restarts must be greater than zero");
    require_tol(gmres_tol, "LinsolveOptions::gmres_tol must be finite and not negative");
    if (has_convergence_tol) require_tol(convergence_tol, "LinsolveOptions::convergence_tol must be finite and not negative");
    if (!std::isfinite(a0) || !std::isfinite(a1)) throw Error(T4A_GPU_INVALID_ARGUMENT, "LinsolveOptions::a0 and a1 must be finite");
    if (has_max_bond_dim && max_bond_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "LinsolveOptions::max_bond_dim must be positive when specified");
    if (has_svd_policy) validate_svd_policy(svd_policy, "LinsolveOptions::svd_policy");
}

std::vector<std::array<size_t, 3>> dims3_of(const std::vector<DevCore>& cores)
{
    std::vector<std::array<size_t, 3>> d;
    for (const DevCore& c : cores) d.push_back({c.l, c.s, c.r});
    return d;
}

void require_tol(double v, const std::string& what)
{
    if (!std::isfinite(v) || v < 0.0) throw Error(T4A_GPU_INVALID_ARGUMENT, what);
}

void validate_svd_policy(const SvdPolicy& p, const char* who)
{
    require_tol(p.threshold, "Invalid SVD truncation threshold: threshold must be finite and non-negative");
    if (p.scale < 0 || p.scale > 1 || p.measure < 0 || p.measure > 1 || p.rule < 0 || p.rule > 1)
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": unknown scale, measure or rule");
}

void validate_chain_operands(const char* who, const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>* rhs,
                             const std::vector<std::array<size_t, 3>>& state, const char* few_sites)
{
    const std::string w = std::string(who) + ": ";
    const size_t n = state.size();
    if (op.size() != n || (rhs && rhs->size() != n))
        throw Error(T4A_GPU_INVALID_ARGUMENT, w + "lengths differ: the operator has " + std::to_string(op.size()) + " sites, the state " + std::to_string(n) +
                                                  (rhs ? ", the rhs " + std::to_string(rhs->size()) : std::string()));
    if (n < 2) throw Error(T4A_GPU_INVALID_ARGUMENT, w + few_sites);
    for (size_t i = 0; i < n; ++i) {
        const size_t d = state[i][1];
        if (op[i][1] != op[i][2])
            throw Error(T4A_GPU_INVALID_ARGUMENT, w + "site " + std::to_string(i) + " of the operator is not square: (" + std::to_string(op[i][1]) + ", " +
                                                      std::to_string(op[i][2]) + ")");
        if (op[i][1] != d)
            throw Error(T4A_GPU_INVALID_ARGUMENT, w + "site " + std::to_string(i) + " of the operator has dimension " + std::to_string(op[i][1]) +
                                                      ", the state " + std::to_string(d));
        if (rhs && (*rhs)[i][1] != d)
            throw Error(T4A_GPU_INVALID_ARGUMENT, w + "site " + std::to_string(i) + " of the rhs has dimension " + std::to_string((*rhs)[i][1]) +
                                                      ", the state " + std::to_string(d));
    }
}

SvdOptions sweep_svd_options(bool has_policy, const SvdPolicy& policy, bool has_max_bond_dim, size_t max_bond_dim)
{
    SvdOptions so;
    so.truncate = true;
    if (has_policy) so.policy = policy;
    so.has_max_bond_dim = has_max_bond_dim;
    so.max_bond_dim = max_bond_dim;
    return so;
}

void linsolve_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>* rhs,
                              const std::vector<std::array<size_t, 3>>& state, size_t center, size_t restart_dim)
{
    const size_t n = state.size();
    validate_chain_operands("square_linsolve", op, rhs, state, "fewer than two sites: the one-site local solve is not implemented");
    if (center >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "square_linsolve: center " + std::to_string(center) + " is out of range (" + std::to_string(n) + " sites)");
    for (size_t i = 0; i + 1 < n; ++i) check_step_dims(i, state[i][0], state[i][1], state[i + 1][1], state[i + 1][2], op[i][3], restart_dim);
}

// ------------------------------------------------------------------------------------------------ GMRES
void Gmres::reserve(size_t len, size_t restart_dim)
{
    const size_t m = restart_dim;
    grow(eng_, basis_, len * (m + 1));
    grow(eng_, ax_, len);
    gs_.reserve(m + 1);
    grow(eng_, hcol_, m + 3); // the column of H (m + 2) and one norm
    grow(eng_, coef_, m + 1);
}

namespace {
// compute_givens_rotation / apply_givens_rotation / solve_upper_triangular (krylov.rs:2708-2772) for real scalars
void givens(double a, double b, double& c, double& s)
{
    const double aa = std::fabs(a), ba = std::fabs(b);
    const double r = std::sqrt(aa * aa + ba * ba);
    if (r < 1e-15) {
        c = 1.0;
        s = 0.0;
    } else if (aa < 1e-15) {
        c = 0.0;
        s = b / r;
    } else {
        const double phase = a / aa;
        c = aa / r;
        s = phase * b / r;
    }
}
void rotate(double c, double s, double& x, double& y)
{
    const double nx = c * x + s * y, ny = -(s * x) + c * y;
    x = nx;
    y = ny;
}
std::vector<double> solve_upper(const std::vector<std::vector<double>>& h, const std::vector<double>& g, size_t n)
{
    std::vector<double> y(n, 0.0);
    for (size_t i = n; i-- > 0;) {
        double sum = g[i];
        for (size_t j = i + 1; j < n; ++j) sum = sum - h[j][i] * y[j];
        if (std::fabs(h[i][i]) < 1e-15) throw Error(T4A_GPU_INVALID_ARGUMENT, "Near-singular upper triangular matrix in GMRES");
        y[i] = sum / h[i][i];
    }
    return y;
}
} // namespace

GmresResult Gmres::solve(const GmresApply& apply, size_t len, const double* d_b, double* d_x, double a0, double a1, double tol, GmresToleranceMode mode,
                         size_t restart_dim, size_t max_restarts)
{
    GmresResult res;
    hipStream_t st = eng_.stream();
    const size_t m = restart_dim;
    reserve(len, m);
    const bool relative = mode == GmresToleranceMode::Relative;
    const double b_norm = gs_.norm(d_b, len);
    auto value = [&](double r) { return relative ? r / b_norm : r; };
    auto is_converged = [&](double r) { return value(r) < tol; };
    if (b_norm < 1e-15) {
        res.converged = true;
        return res;
    }
    if (a0 == 0.0 && a1 == 0.0) throw Error(T4A_GPU_INVALID_ARGUMENT, "gmres: a0 and a1 are both zero");
    if (a1 == 0.0) {
        linsolve_scale_launch(d_b, 1.0 / a0, d_x, len, st);
        T4A_HIP(hipGetLastError());
        eng_.sync();
        res.converged = true;
        return res;
    }
    double* V = basis_.get();
    double* d_hcol = hcol_.get();
    double* d_norm = hcol_.get() + m + 2;
    double* npart = gs_.npart();
    // |b - (a0 x + a1 H x)|; the residual is left in column 0 of the basis, normalised
    auto residual_norm = [&]() {
        double v = 0.0;
        apply(d_x, ax_.get());
        ++res.apply_calls;
        linsolve_residual_launch(d_b, d_x, ax_.get(), a0, a1, V, len, npart, st);
        gs_normalize_launch(V, len, npart, V, d_norm, st);
        T4A_HIP(hipMemcpyAsync(&v, d_norm, sizeof(double), hipMemcpyDeviceToHost, st));
        eng_.sync();
        return v;
    };
    std::vector<double> neg;
    auto update_solution = [&](const std::vector<double>& y) { // x += sum_i y_i v_i
        neg.resize(y.size());
        for (size_t i = 0; i < y.size(); ++i) neg[i] = -y[i];
        T4A_HIP(hipMemcpyAsync(coef_.get(), neg.data(), sizeof(double) * neg.size(), hipMemcpyHostToDevice, st));
        gs_update_launch(V, len, (int)y.size(), d_x, len, coef_.get(), 1, nullptr, true, nullptr, npart, st);
        T4A_HIP(hipGetLastError());
        eng_.sync();
    };
    std::vector<double> ha(m + 2);
    for (size_t restart = 0; restart < max_restarts; ++restart) {
        const double r_norm = residual_norm();
        if (is_converged(r_norm)) {
            res.residual = value(r_norm);
            res.converged = true;
            return res;
        }
        std::vector<std::vector<double>> hm;
        std::vector<double> cs, sn, g{r_norm};
        bool solution_already_updated = false;
        for (size_t j = 0; j < m; ++j) {
            ++res.iterations;
            double* w = V + len * (j + 1);
            apply(V + len * j, w);
            ++res.apply_calls;
            gs_.orth(V, len, (int)(j + 1), w, len, d_hcol, nullptr);
            T4A_HIP(hipMemcpyAsync(ha.data(), d_hcol, sizeof(double) * (j + 2), hipMemcpyDeviceToHost, st));
            eng_.sync();
            const double h_next = ha[j + 1];
            std::vector<double> hc(j + 2);
            for (size_t i = 0; i < j; ++i) hc[i] = a1 * ha[i];
            hc[j] = a0 + a1 * ha[j];
            hc[j + 1] = a1 * ha[j + 1];
            for (size_t i = 0; i < j; ++i) rotate(cs[i], sn[i], hc[i], hc[i + 1]);
            double c, s;
            givens(hc[j], hc[j + 1], c, s);
            cs.push_back(c);
            sn.push_back(s);
            double dummy = hc[j + 1];
            rotate(c, s, hc[j], dummy);
            hc[j + 1] = 0.0;
            double gj = g[j], gn = 0.0;
            rotate(c, s, gj, gn);
            g[j] = gj;
            g.push_back(gn);
            const double res_norm = std::fabs(gn);
            hm.push_back(std::move(hc));
            if (is_converged(res_norm)) {
                update_solution(solve_upper(hm, g, j + 1));
                // check_true_residual (local_gmres_options sets it)
                const double true_res = residual_norm();
                if (is_converged(true_res)) {
                    res.residual = value(true_res);
                    res.converged = true;
                    return res;
                }
                solution_already_updated = true;
                break;
            }
            if (!(h_next > 1e-14)) { // lucky breakdown: v_{j+1} is discarded
                update_solution(solve_upper(hm, g, j + 1));
                const double final_res = residual_norm();
                res.residual = value(final_res);
                res.converged = is_converged(final_res);
                return res;
            }
        }
        if (!solution_already_updated) update_solution(solve_upper(hm, g, hm.size()));
    }
    const double final_res = residual_norm();
    res.residual = value(final_res);
    res.converged = is_converged(final_res);
    return res;
}

// ------------------------------------------------------------------------------------------------ the projected operator
ProjectedOperator::ProjectedOperator(Mpo& op, TensorTrain& state, TensorTrain* rhs)
{
    std::vector<std::array<size_t, 3>> rd;
    if (rhs) rd = dims3_of(rhs->cores);
    linsolve_validate_shapes(op.dims4(), rhs ? &rd : nullptr, dims3_of(state.cores), 0, 1);
    op_ = std::make_unique<Mpo>(op.tt.cores, op.tt.eng.stream(), op.sd);
    Engine& e = engine();
    state.eng.sync();
    x = clone_cores(state.cores, e.stream());
    if (rhs) {
        rhs->eng.sync();
        b = clone_cores(rhs->cores, e.stream());
    }
    const size_t n = x.size();
    envL_.resize(n + 1);
    envR_.resize(n + 1);
    envLb_.resize(n + 1);
    envRb_.resize(n + 1);
    okL_.assign(n + 1, 0);
    okR_.assign(n + 1, 0);
    for (DevBuf<double>* one : {&envL_[0], &envR_[n], &envLb_[0], &envRb_[n]}) {
        one->reserve(1);
        fill_launch(one->get(), 1, 1.0, e.stream());
    }
    okL_[0] = okR_[n] = 1;
    T4A_HIP(hipGetLastError());
    e.sync();
}

std::array<size_t, 4> ProjectedOperator::local_dims(size_t site) const
{
    if (site + 1 >= x.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: the region (" + std::to_string(site) + ", " + std::to_string(site + 1) + ") is out of range");
    return {x[site].l, x[site].s, x[site + 1].s, x[site + 1].r};
}

void ProjectedOperator::check_step(size_t site, size_t restart_dim, const char* who) const
{
    check_bond_step_dims(who, site, x[site].l, x[site].s, x[site + 1].s, x[site + 1].r, op_->tt.cores[site].r, restart_dim);
}

void ProjectedOperator::invalidate(size_t site)
{
    if (site >= x.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: site " + std::to_string(site) + " is out of range");
    for (size_t j = site + 1; j < okL_.size(); ++j) okL_[j] = 0;
    for (size_t j = 0; j <= site; ++j) okR_[j] = 0;
    prepared_ = (size_t)-1;
    prepared1_ = (size_t)-1;
    if (hl_site_ != (size_t)-1 && site < hl_site_) hl_site_ = (size_t)-1; // L_c A_c depends on the sites < c only
}

// L_{k+1} from L_k, A_k (as the HL in hl_) and x_k:  T1 = HL X_k, then L_{k+1}[:, w, :] = X_k^T T1_w for every w in one batched product
void ProjectedOperator::update_left_from_prepared(size_t k)
{
    Engine& e = engine();
    hipStream_t st = e.stream();
    const DevCore& X = x[k];
    const DevCore& A = op_->tt.cores[k];
    const int chi = (int)X.l, d = (int)X.s, cn = (int)X.r, W = (int)A.r, M = chi * d;
    grow(e, t1_, (size_t)W * M * cn);
    grow(e, envL_[k + 1], (size_t)cn * W * cn);
    gemm_launch(gemm_desc(W * M, cn, M, hl_.get(), W * M, X.buf.get(), M, t1_.get(), W * M), st);
    GemmDesc g = gemm_desc(cn, cn, M, X.buf.get(), M, t1_.get(), W * M, envL_[k + 1].get(), cn * W);
    g.transA = 1;
    g.strideA = 0;
    g.strideB = M;
    g.strideC = cn;
    g.batch = W;
    gemm_launch(g, st);
    if (!b.empty()) { // Lb_{k+1} = X_k^T (Lb_k B_k)
        const DevCore& B = b[k];
        const int bl = (int)B.l, br = (int)B.r;
        grow(e, p1_, (size_t)M * br);
        grow(e, envLb_[k + 1], (size_t)cn * br);
        gemm_launch(gemm_desc(chi, d * br, bl, envLb_[k].get(), chi, B.buf.get(), bl, p1_.get(), chi), st);
        GemmDesc h = gemm_desc(cn, br, M, X.buf.get(), M, p1_.get(), M, envLb_[k + 1].get(), cn);
        h.transA = 1;
        gemm_launch(h, st);
    }
    T4A_HIP(hipGetLastError());
    okL_[k + 1] = 1;
}

// R_k from R_{k+1}, A_k (as the HR in hr_) and x_k:  T2 = X_k HR^T (chi x W N), then R_k[:, w, :] = T2_w X_k^T
void ProjectedOperator::update_right_from_prepared(size_t site)
{
    const size_t k = site + 1;
    Engine& e = engine();
    hipStream_t st = e.stream();
    const DevCore& X = x[k];
    const DevCore& A = op_->tt.cores[k];
    const int chi = (int)X.l, d = (int)X.s, cr = (int)X.r, W = (int)A.l, N = d * cr;
    grow(e, t1_, (size_t)chi * W * N);
    grow(e, envR_[k], (size_t)chi * W * chi);
    GemmDesc g1 = gemm_desc(chi, W * N, N, X.buf.get(), chi, hr_.get(), W * N, t1_.get(), chi);
    g1.transB = 1;
    gemm_launch(g1, st);
    GemmDesc g = gemm_desc(chi, chi, N, t1_.get(), chi * W, X.buf.get(), chi, envR_[k].get(), chi * W);
    g.transB = 1;
    g.strideA = chi;
    g.strideB = 0;
    g.strideC = chi;
    g.batch = W;
    gemm_launch(g, st);
    if (!b.empty()) { // Rb_k = X_k (B_k Rb_{k+1}^T)^T
        const DevCore& B = b[k];
        const int bl = (int)B.l, br = (int)B.r;
        grow(e, p2_, (size_t)bl * N);
        grow(e, envRb_[k], (size_t)chi * bl);
        GemmDesc h1 = gemm_desc(bl * d, cr, br, B.buf.get(), bl * d, envRb_[k + 1].get(), cr, p2_.get(), bl * d);
        h1.transB = 1;
        gemm_launch(h1, st);
        GemmDesc h2 = gemm_desc(chi, bl, N, X.buf.get(), chi, p2_.get(), bl, envRb_[k].get(), chi);
        h2.transB = 1;
        gemm_launch(h2, st);
    }
    T4A_HIP(hipGetLastError());
    okR_[k] = 1;
}

const double* ProjectedOperator::left_env(size_t i)
{
    size_t j = i;
    while (!okL_[j]) --j; // okL_[0] always holds
    Engine& e = engine();
    for (size_t k = j; k < i; ++k) {
        const DevCore& X = x[k];
        const DevCore& A = op_->tt.cores[k];
        if (above_int_max({A.r, X.l * X.s, X.l * X.s}) || above_int_max({A.r, X.l * X.s, X.r}))
            throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: the left environment of site " + std::to_string(k + 1) + " needs more than INT_MAX elements");
        grow(e, hl_, A.r * X.l * X.s * X.l * X.s);
        prepared_ = (size_t)-1;
        prepared1_ = hl_site_ = (size_t)-1;
        linsolve_hl_launch(envL_[k].get(), A.buf.get(), hl_.get(), (int)X.l, (int)A.l, (int)X.s, (int)A.r, e.stream());
        update_left_from_prepared(k);
    }
    return envL_[i].get();
}

const double* ProjectedOperator::right_env(size_t i)
{
    size_t j = i;
    while (!okR_[j]) ++j; // okR_[n] always holds
    Engine& e = engine();
    for (size_t k = j; k-- > i;) {
        const DevCore& X = x[k];
        const DevCore& A = op_->tt.cores[k];
        if (above_int_max({A.l, X.s * X.r, X.s * X.r}) || above_int_max({A.l, X.s * X.r, X.l}))
            throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: the right environment of site " + std::to_string(k) + " needs more than INT_MAX elements");
        grow(e, hr_, A.l * X.s * X.r * X.s * X.r);
        prepared_ = (size_t)-1;
        linsolve_hr_launch(A.buf.get(), envR_[k + 1].get(), hr_.get(), (int)X.r, (int)A.l, (int)X.s, (int)A.r, e.stream());
        update_right_from_prepared(k - 1);
    }
    return envR_[i].get();
}

const double* ProjectedOperator::left_rhs_env(size_t i)
{
    left_env(i);
    return envLb_[i].get();
}
const double* ProjectedOperator::right_rhs_env(size_t i)
{
    right_env(i);
    return envRb_[i].get();
}

void ProjectedOperator::prepare(size_t site)
{
    const auto ld = local_dims(site);
    check_step(site, 0);
    Engine& e = engine();
    const double* L = left_env(site);
    const double* R = right_env(site + 2);
    const DevCore& A1 = op_->tt.cores[site];
    const DevCore& A2 = op_->tt.cores[site + 1];
    const size_t M = ld[0] * ld[1], N = ld[2] * ld[3], W = A1.r;
    grow(e, hl_, W * M * M);
    grow(e, hr_, W * N * N);
    grow(e, t_, W * M * N);
    linsolve_hl_launch(L, A1.buf.get(), hl_.get(), (int)ld[0], (int)A1.l, (int)ld[1], (int)W, e.stream());
    linsolve_hr_launch(A2.buf.get(), R, hr_.get(), (int)ld[3], (int)W, (int)ld[2], (int)A2.r, e.stream());
    T4A_HIP(hipGetLastError());
    prepared_ = hl_site_ = site;
    if (prepared1_ != site) prepared1_ = (size_t)-1;
}

void ProjectedOperator::check_site_step(size_t c, size_t basis_dim, const char* who) const
{
    check_site_step_dims(who, c, x[c].l, x[c].s, x[c].r, op_->tt.cores[c].r, basis_dim);
}

bool ProjectedOperator::prepare_one_site(size_t c)
{
    if (c >= x.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: site " + std::to_string(c) + " is out of range");
    check_site_step(c, 0, "projected operator");
    Engine& e = engine();
    const double* L = left_env(c);
    r1_ = right_env(c + 1);
    const DevCore& X = x[c];
    const DevCore& A = op_->tt.cores[c];
    const size_t M = X.l * X.s, W = A.r;
    const bool reuse = hl_site_ == c;
    if (!reuse) {
        grow(e, hl_, W * M * M);
        if (prepared_ != c) prepared_ = (size_t)-1;
        linsolve_hl_launch(L, A.buf.get(), hl_.get(), (int)X.l, (int)A.l, (int)X.s, (int)W, e.stream());
        hl_site_ = c;
    }
    grow(e, t_, W * M * X.r);
    T4A_HIP(hipGetLastError());
    prepared1_ = c;
    return reuse;
}

void ProjectedOperator::prepare_bond_center(size_t c, bool toward_right)
{
    if (c >= x.size() || (toward_right ? c + 1 >= x.size() : c == 0))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: site " + std::to_string(c) + " has no neighbour on that side");
    Engine& e = engine();
    const DevCore& X = x[c];
    const DevCore& A = op_->tt.cores[c];
    if (toward_right) {
        prepare_one_site(c); // L_c, R_{c+1} and HL = L_c A_c (hl_ reused when it still holds it)
        update_left_from_prepared(c); // L_{c+1}[:, w, :] = Q^T (HL_w Q)
        bc_la_ = envL_[c + 1].get();
        bc_rb_ = right_env(c + 1);
        bc_ka_ = X.r;
        bc_kb_ = x[c + 1].l;
        bc_w_ = A.r;
        bc_bond_ = c;
    } else {
        bc_la_ = left_env(c);
        const double* R = right_env(c + 1);
        if (above_int_max({A.l, X.s * X.r, X.s * X.r}) || above_int_max({A.l, X.s * X.r, X.l}))
            throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: the right environment of site " + std::to_string(c) + " needs more than INT_MAX elements");
        grow(e, hr_, A.l * X.s * X.r * X.s * X.r);
        prepared_ = (size_t)-1;
        linsolve_hr_launch(A.buf.get(), R, hr_.get(), (int)X.r, (int)A.l, (int)X.s, (int)A.r, e.stream());
        update_right_from_prepared(c - 1); // R_c[:, w, :] = (Q HR_w^T) Q^T
        bc_rb_ = envR_[c].get();
        bc_ka_ = x[c - 1].r;
        bc_kb_ = X.l;
        bc_w_ = A.l;
        bc_bond_ = c - 1;
    }
    check_bond_center(0, "projected operator");
    grow(e, t_, bc_ka_ * bc_w_ * bc_kb_);
    T4A_HIP(hipGetLastError());
    prepared1_ = (size_t)-1; // t_ may have been regrown
}

void ProjectedOperator::check_bond_center(size_t basis_dim, const char* who) const
{
    check_bond_center_dims(who, bc_bond_, bc_ka_, bc_kb_, bc_w_, basis_dim);
}

std::vector<double> ProjectedOperator::bond_center_environment(size_t c, bool toward_right, size_t dims[3])
{
    prepare_bond_center(c, toward_right);
    const size_t k = toward_right ? bc_ka_ : bc_kb_;
    dims[0] = k;
    dims[1] = bc_w_;
    dims[2] = k;
    return to_host(engine(), toward_right ? bc_la_ : bc_rb_, k * bc_w_ * k);
}

void ProjectedOperator::apply_one_site_prepared(const double* d_v, double* d_out)
{
    const DevCore& X = x[prepared1_];
    const int M = (int)(X.l * X.s), cr = (int)X.r, W = (int)op_->tt.cores[prepared1_].r;
    hipStream_t st = engine().stream();
    gemm_launch(gemm_desc(W * M, cr, M, hl_.get(), W * M, d_v, M, t_.get(), W * M), st);
    GemmDesc g = gemm_desc(M, cr, W * cr, t_.get(), M, r1_, cr, d_out, M);
    g.transB = 1;
    gemm_launch(g, st);
}

std::vector<double> ProjectedOperator::apply_one_site(size_t site, const double* v, bool* reused_hl)
{
    if (site >= x.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: site " + std::to_string(site) + " is out of range");
    const size_t len = x[site].size();
    Engine& e = engine();
    bool reused = false;
    if (prepared1_ != site) reused = prepare_one_site(site);
    if (reused_hl) *reused_hl = reused;
    DevBuf<double> d_v, d_y;
    d_v.reserve(len);
    d_y.reserve(len);
    T4A_HIP(hipMemcpyAsync(d_v.get(), v, sizeof(double) * len, hipMemcpyHostToDevice, e.stream()));
    apply_one_site_prepared(d_v.get(), d_y.get());
    T4A_HIP(hipGetLastError());
    return to_host(e, d_y.get(), len);
}

void ProjectedOperator::time_one_site(size_t c, size_t reps, double ms[3])
{
    if (c >= x.size() || reps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "time_one_site: the site must exist and reps be positive");
    Engine& e = engine();
    hipStream_t st = e.stream();
    prepare_one_site(c);
    const DevCore& X = x[c];
    const DevCore& A = op_->tt.cores[c];
    const double* L = left_env(c);
    const size_t len = X.size();
    const int M = (int)(X.l * X.s), cr = (int)X.r, W = (int)A.r;
    DevBuf<double> v, y;
    v.reserve(len);
    y.reserve(len);
    fill_launch(v.get(), len, 1.0 / std::sqrt((double)len), st);
    GemmDesc g2 = gemm_desc(M, cr, W * cr, t_.get(), M, r1_, cr, y.get(), M);
    g2.transB = 1;
    const std::function<void()> pieces[3] = {
        [&] { linsolve_hl_launch(L, A.buf.get(), hl_.get(), (int)X.l, (int)A.l, (int)X.s, W, st); },
        [&] { gemm_launch(gemm_desc(W * M, cr, M, hl_.get(), W * M, v.get(), M, t_.get(), W * M), st); },
        [&] { gemm_launch(g2, st); },
    };
    time_pieces(st, pieces, 3, reps, ms);
    e.sync();
}

void ProjectedOperator::product_left(const double* d_v) // T = HL V
{
    const auto ld = local_dims(prepared_);
    const int M = (int)(ld[0] * ld[1]), N = (int)(ld[2] * ld[3]), W = (int)op_->tt.cores[prepared_].r;
    gemm_launch(gemm_desc(W * M, N, M, hl_.get(), W * M, d_v, M, t_.get(), W * M), engine().stream());
}

void ProjectedOperator::product_right(double* d_out) // Y = T HR, T read as M x (W N)
{
    const auto ld = local_dims(prepared_);
    const int M = (int)(ld[0] * ld[1]), N = (int)(ld[2] * ld[3]), W = (int)op_->tt.cores[prepared_].r;
    gemm_launch(gemm_desc(M, N, W * N, t_.get(), M, hr_.get(), W * N, d_out, M), engine().stream());
}

void ProjectedOperator::apply_prepared(const double* d_v, double* d_out)
{
    product_left(d_v);
    product_right(d_out);
}

void ProjectedOperator::split_and_advance(size_t i, const double* d_theta, const SvdOptions& so, bool move_right, const char* who)
{
    Engine& e = engine();
    hipStream_t st = e.stream();
    const auto ld = local_dims(i);
    const int M = (int)(ld[0] * ld[1]), N = (int)(ld[2] * ld[3]);
    const TensorView tv{d_theta, {(size_t)M, (size_t)N}, {0, 1}};
    const UnfoldPlan un = plan_unfold_split(tv, {0});
    require_factorizable(un, who, "svd");
    const UnfoldedFactors f = tensor_svd(e, tv, un, so);
    DevCore nl = DevCore::make(ld[0], ld[1], f.keep), nr = DevCore::make(f.keep, ld[2], ld[3]);
    split_two_site(st, f.d_left, M, f.d_s, f.d_right, (int)f.k, N, (int)f.keep, move_right, nl, nr); // x_i = U | x_i = U S
    T4A_HIP(hipGetLastError());
    e.sync(); // the old sites are released below
    x[i] = std::move(nl);
    x[i + 1] = std::move(nr);
    // both sites changed: every cache that contains one of them is stale; the side left behind is rebuilt from this step's half operator
    // (HL and HR depend on the environments and the operator only, not on the two sites)
    invalidate(i);
    invalidate(i + 1);
    if (move_right) update_left_from_prepared(i);
    else update_right_from_prepared(i);
}

size_t ProjectedOperator::two_site_vector(size_t i, DevBuf<double>& theta)
{
    Engine& e = engine();
    const auto ld = local_dims(i);
    const int M = (int)(ld[0] * ld[1]), N = (int)(ld[2] * ld[3]), mid = (int)x[i].r;
    const size_t len = (size_t)M * N;
    grow(e, theta, len);
    gemm_launch(gemm_desc(M, N, mid, x[i].buf.get(), M, x[i + 1].buf.get(), mid, theta.get(), M), e.stream());
    return len;
}

void ProjectedOperator::canonicalize(size_t center)
{
    QrSweep sw(engine());
    sw.canonicalize(x, center);
}

void ProjectedOperator::time_step(size_t site, size_t nb, size_t reps, double ms[5])
{
    const auto ld = local_dims(site);
    check_step(site, nb);
    if (nb == 0 || nb > LINSOLVE_RESTART_DIM_MAX || reps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "time_step: nb and reps must be positive");
    const size_t len = ld[0] * ld[1] * ld[2] * ld[3];
    Engine& e = engine();
    hipStream_t st = e.stream();
    prepare(site);
    DevBuf<double> basis, part, npart, hcol;
    basis.reserve(len * (nb + 1));
    part.reserve(nb * GS_MAX_WORKGROUPS);
    npart.reserve(GS_MAX_WORKGROUPS);
    hcol.reserve(nb + 1);
    fill_launch(basis.get(), len * (nb + 1), 1.0 / std::sqrt((double)len), st);
    double* w = basis.get() + len * nb;
    const int G = gs_workgroups(len);
    const std::function<void()> pieces[5] = {
        [&] { product_left(basis.get()); },
        [&] { product_right(w); },
        [&] { gs_dots_launch(basis.get(), len, (int)nb, w, len, part.get(), st); },
        [&] { gs_update_launch(basis.get(), len, (int)nb, w, len, part.get(), G, hcol.get(), true, nullptr, npart.get(), st); },
        [&] { gs_normalize_launch(w, len, npart.get(), w, hcol.get() + nb, st); },
    };
    time_pieces(st, pieces, 5, reps, ms);
    e.sync();
}

void ProjectedOperator::local_rhs(size_t site, double* d_out)
{
    const auto ld = local_dims(site);
    Engine& e = engine();
    hipStream_t st = e.stream();
    const double* Lb = left_rhs_env(site);
    const double* Rb = right_rhs_env(site + 2);
    const DevCore& B1 = b[site];
    const DevCore& B2 = b[site + 1];
    const int chi_l = (int)ld[0], d1 = (int)ld[1], d2 = (int)ld[2], chi_r = (int)ld[3];
    const int bl = (int)B1.l, bm = (int)B1.r, br = (int)B2.r, M = chi_l * d1, N = d2 * chi_r;
    grow(e, p1_, (size_t)M * bm);
    grow(e, p2_, (size_t)bm * N);
    gemm_launch(gemm_desc(chi_l, d1 * bm, bl, Lb, chi_l, B1.buf.get(), bl, p1_.get(), chi_l), st); // (chi_l d1) x bm
    GemmDesc g = gemm_desc(bm * d2, chi_r, br, B2.buf.get(), bm * d2, Rb, chi_r, p2_.get(), bm * d2); // bm x (d2 chi_r)
    g.transB = 1;
    gemm_launch(g, st);
    gemm_launch(gemm_desc(M, N, bm, p1_.get(), M, p2_.get(), bm, d_out, M), st);
    T4A_HIP(hipGetLastError());
}

std::vector<double> ProjectedOperator::apply(size_t site, const double* v)
{
    const auto ld = local_dims(site);
    const size_t len = ld[0] * ld[1] * ld[2] * ld[3];
    Engine& e = engine();
    if (prepared_ != site) prepare(site);
    DevBuf<double> d_v, d_y;
    d_v.reserve(len);
    d_y.reserve(len);
    T4A_HIP(hipMemcpyAsync(d_v.get(), v, sizeof(double) * len, hipMemcpyHostToDevice, e.stream()));
    apply_prepared(d_v.get(), d_y.get());
    T4A_HIP(hipGetLastError());
    return to_host(e, d_y.get(), len);
}

std::vector<double> ProjectedOperator::environment(int side, size_t bond, size_t dims[3])
{
    const size_t n = x.size();
    if (bond > n) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: bond " + std::to_string(bond) + " is out of range");
    const size_t chi = bond == 0 ? 1 : (bond == n ? 1 : x[bond].l);
    const size_t W = bond == 0 ? 1 : (bond == n ? 1 : op_->tt.cores[bond].l);
    dims[0] = chi;
    dims[1] = W;
    dims[2] = chi;
    Engine& e = engine();
    const double* src = side == 0 ? left_env(bond) : right_env(bond);
    return to_host(e, src, chi * W * chi);
}

void ProjectedOperator::set_site_tensors(size_t site, const size_t d1[3], const double* t1, const size_t d2[3], const double* t2)
{
    const size_t n = x.size();
    if (site + 1 >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: the region (" + std::to_string(site) + ", " + std::to_string(site + 1) + ") is out of range");
    if (d1[0] != x[site].l || d1[1] != x[site].s || d2[1] != x[site + 1].s || d2[2] != x[site + 1].r || d1[2] != d2[0] || d1[2] == 0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: the new site tensors must keep the outer bonds and the site dimensions and share their bond");
    Engine& e = engine();
    e.sync();
    DevCore a = DevCore::make(d1[0], d1[1], d1[2]), c = DevCore::make(d2[0], d2[1], d2[2]);
    T4A_HIP(hipMemcpyAsync(a.buf.get(), t1, sizeof(double) * a.size(), hipMemcpyHostToDevice, e.stream()));
    T4A_HIP(hipMemcpyAsync(c.buf.get(), t2, sizeof(double) * c.size(), hipMemcpyHostToDevice, e.stream()));
    e.sync();
    x[site] = std::move(a);
    x[site + 1] = std::move(c);
    invalidate(site);
    invalidate(site + 1);
}

std::vector<double> projected_apply_env(const double* L, const double* R, size_t chi_l, size_t chi_r, Mpo& op, size_t site, const double* v,
                                        std::vector<double>* hl, std::vector<double>* hr)
{
    if (site + 1 >= op.len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_env: the region (" + std::to_string(site) + ", " + std::to_string(site + 1) + ") is out of range");
    if (chi_l == 0 || chi_r == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_env: an environment has a zero dimension");
    const DevCore& A1 = op.tt.cores[site];
    const DevCore& A2 = op.tt.cores[site + 1];
    if (op.sd[site][0] != op.sd[site][1] || op.sd[site + 1][0] != op.sd[site + 1][1])
        throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_env: the operator sites are not square");
    const size_t d1 = op.sd[site][0], d2 = op.sd[site + 1][0], W = A1.r;
    check_step_dims(site, chi_l, d1, d2, chi_r, W, 0);
    if (above_int_max({chi_l, A1.l, chi_l}) || above_int_max({chi_r, A2.r, chi_r}))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_env: an environment holds more than INT_MAX elements");
    const size_t M = chi_l * d1, N = d2 * chi_r, len = M * N;
    Engine& e = op.tt.eng;
    hipStream_t st = e.stream();
    DevBuf<double> dL, dR, dv, dy, dhl, dhr, dt;
    const size_t nl = chi_l * A1.l * chi_l, nr = chi_r * A2.r * chi_r;
    dL.reserve(nl);
    dR.reserve(nr);
    dv.reserve(len);
    dy.reserve(len);
    dhl.reserve(W * M * M);
    dhr.reserve(W * N * N);
    dt.reserve(W * M * N);
    T4A_HIP(hipMemcpyAsync(dL.get(), L, sizeof(double) * nl, hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(dR.get(), R, sizeof(double) * nr, hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(dv.get(), v, sizeof(double) * len, hipMemcpyHostToDevice, st));
    linsolve_hl_launch(dL.get(), A1.buf.get(), dhl.get(), (int)chi_l, (int)A1.l, (int)d1, (int)W, st);
    linsolve_hr_launch(A2.buf.get(), dR.get(), dhr.get(), (int)chi_r, (int)W, (int)d2, (int)A2.r, st);
    const int m = (int)M, n = (int)N, w = (int)W;
    gemm_launch(gemm_desc(w * m, n, m, dhl.get(), w * m, dv.get(), m, dt.get(), w * m), st);
    gemm_launch(gemm_desc(m, n, w * n, dt.get(), m, dhr.get(), w * n, dy.get(), m), st);
    T4A_HIP(hipGetLastError());
    std::vector<double> out(len);
    T4A_HIP(hipMemcpyAsync(out.data(), dy.get(), sizeof(double) * len, hipMemcpyDeviceToHost, st));
    if (hl) {
        hl->resize(W * M * M);
        T4A_HIP(hipMemcpyAsync(hl->data(), dhl.get(), sizeof(double) * hl->size(), hipMemcpyDeviceToHost, st));
    }
    if (hr) {
        hr->resize(W * N * N);
        T4A_HIP(hipMemcpyAsync(hr->data(), dhr.get(), sizeof(double) * hr->size(), hipMemcpyDeviceToHost, st));
    }
    e.sync();
    return out;
}

// ------------------------------------------------------------------------------------------------ the residual and the sweeps
double relative_linear_system_residual(Mpo& op, TensorTrain& x, TensorTrain& rhs, double a0, double a1)
{
    const auto rd = dims3_of(rhs.cores);
    linsolve_validate_shapes(op.dims4(), &rd, dims3_of(x.cores), 0, 0);
    x.eng.sync();
    std::vector<std::array<size_t, 2>> sd;
    for (const DevCore& c : x.cores) sd.push_back({c.s, 1});
    Mpo xm(x.cores, x.eng.stream(), sd);
    MpoContractionOptions co;
    std::unique_ptr<Mpo> ax = mpo_contract(op, xm, MpoAlgorithm::Naive, false, co); // the exact product, bonds W * chi
    ax->tt.scale(a1);
    xm.tt.scale(a0);
    std::unique_ptr<TensorTrain> lhs = xm.tt.add(ax->tt, false);
    std::unique_ptr<TensorTrain> r = lhs->add(rhs, true);
    const double rn = canonical_norm(*r);
    const double bn = canonical_norm(rhs);
    return bn > 1e-15 ? rn / bn : rn;
}

LinsolveResult square_linsolve(Mpo& op, TensorTrain& rhs, TensorTrain& init, size_t center, const LinsolveOptions& o)
{
    o.validate();
    const auto rd = dims3_of(rhs.cores);
    linsolve_validate_shapes(op.dims4(), &rd, dims3_of(init.cores), center, o.gmres_restart_dim);
    LinsolveResult out;
    const bool wants_residual = o.check_residual || o.has_convergence_tol;
    if (o.a1 == 0.0 || canonical_norm(op.tt) <= 1e-15) { // solve_identity_term_only (square/mod.rs:362-407)
        if (o.a0 == 0.0) throw Error(T4A_GPU_INVALID_ARGUMENT, "square_linsolve: a0 and effective operator term are both zero");
        rhs.eng.sync();
        out.solution = std::make_unique<TensorTrain>(rhs.cores, rhs.eng.stream());
        out.solution->scale(1.0 / o.a0);
        if (wants_residual) {
            out.has_residual = true;
            out.residual = relative_linear_system_residual(op, *out.solution, rhs, o.a0, o.a1);
        }
        out.converged = o.has_convergence_tol && out.has_residual && out.residual < o.convergence_tol;
        return out;
    }

    ProjectedOperator po(op, init, &rhs);
    Engine& e = po.engine();
    hipStream_t st = e.stream();
    const size_t n = po.len();
    po.canonicalize(center);
    Gmres gm(e);
    DevBuf<double> theta, bt;
    const SvdOptions so = sweep_svd_options(o.has_svd_policy, o.svd_policy, o.has_max_bond_dim, o.max_bond_dim);

    auto bond_step = [&](size_t i, bool move_right) {
        po.check_step(i, o.gmres_restart_dim);
        const auto ld = po.local_dims(i);
        const size_t len = ld[0] * ld[1] * ld[2] * ld[3];
        grow(e, theta, len); // both vectors of the step are sized (and the stream drained, if one grows) before anything is queued
        grow(e, bt, len);
        gm.reserve(len, o.gmres_restart_dim);
        po.local_rhs(i, bt.get());
        po.prepare(i);
        po.two_site_vector(i, theta); // theta_0 = x_i x_{i+1}
        const GmresResult gr = gm.solve([&](const double* v, double* y) { po.apply_prepared(v, y); }, len, bt.get(), theta.get(), o.a0, o.a1, o.gmres_tol,
                                        o.gmres_tolerance_mode, o.gmres_restart_dim, o.gmres_max_restarts);
        ++out.stats.local_solves;
        out.stats.arnoldi_steps += gr.iterations;
        out.stats.apply_calls += gr.apply_calls;
        po.split_and_advance(i, theta.get(), so, move_right, "square_linsolve");
    };

    for (size_t sweep = 0; sweep < o.nfullsweeps; ++sweep) {
        out.sweeps = sweep + 1;
        for_each_bond_from(center, n, bond_step);
        if (o.has_convergence_tol) {
            e.sync();
            TensorTrain xt(po.x, st);
            out.has_residual = true;
            out.residual = relative_linear_system_residual(op, xt, rhs, o.a0, o.a1);
            if (out.residual < o.convergence_tol) {
                out.converged = true;
                break;
            }
        }
    }
    e.sync();
    out.solution = std::make_unique<TensorTrain>(po.x, st);
    if (!out.has_residual && o.check_residual) {
        out.residual = relative_linear_system_residual(op, *out.solution, rhs, o.a0, o.a1);
        out.has_residual = true;
        out.converged = o.has_convergence_tol && out.residual < o.convergence_tol;
    }
    return out;
}

// ------------------------------------------------------------------------------------------------ test hooks
GmresResult gmres_dense(const double* H, size_t n, const double* b, const double* x0, double a0, double a1, double tol, GmresToleranceMode mode,
                        size_t restart_dim, size_t max_restarts, double* x_out)
{
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dH = upload_vector(st, H, n * n), db = upload_vector(st, b, n), dx = upload_vector(st, x0, n);
    Gmres gm(e);
    const GmresResult r = gm.solve(dense_apply(dH.get(), n, st), n, db.get(), dx.get(), a0, a1, tol, mode, restart_dim, max_restarts);
    T4A_HIP(hipMemcpyAsync(x_out, dx.get(), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    e.sync();
    return r;
}

void linsolve_orth(const double* basis, size_t len, size_t nb, double* w, double* h_out, double* norm_out)
{
    krylov_orth_host(basis, len, nb, w, KrylovDotsRoute::Serial, h_out, norm_out);
}

void krylov_orth_host(const double* basis, size_t len, size_t nb, double* w, KrylovDotsRoute route, double* h_out, double* norm_out)
{
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> dV = upload_vector(st, basis, len * nb), dw = upload_vector(st, w, len);
    DevBuf<double> dh;
    dh.reserve(3 * nb + 1);
    KrylovOrth gs(e);
    gs.reserve(nb);
    gs.set_dots_route(route);
    gs.orth(dV.get(), len, (int)nb, dw.get(), len, dh.get(), dh.get() + nb + 1);
    T4A_HIP(hipGetLastError());
    std::vector<double> hc(nb + 1);
    T4A_HIP(hipMemcpyAsync(hc.data(), dh.get(), sizeof(double) * (nb + 1), hipMemcpyDeviceToHost, st));
    T4A_HIP(hipMemcpyAsync(h_out, dh.get() + nb + 1, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost, st));
    T4A_HIP(hipMemcpyAsync(w, dw.get(), sizeof(double) * len, hipMemcpyDeviceToHost, st));
    e.sync();
    *norm_out = hc[nb];
}

void krylov_time_dots(size_t len, size_t nb, size_t reps, double ms[2])
{
    if (len == 0 || nb == 0 || nb > LINSOLVE_RESTART_DIM_MAX || reps == 0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "time_dots: len, nb and reps must be positive, nb at most " + std::to_string(LINSOLVE_RESTART_DIM_MAX));
    if (above_int_max({len, nb + 1})) throw Error(T4A_GPU_INVALID_ARGUMENT, "time_dots: the basis holds more than INT_MAX elements");
    require_device();
    Engine e;
    hipStream_t st = e.stream();
    DevBuf<double> basis, part;
    basis.reserve(len * (nb + 1));
    part.reserve(nb * GS_MAX_WORKGROUPS);
    fill_launch(basis.get(), len * (nb + 1), 1.0 / std::sqrt((double)len), st);
    const double* w = basis.get() + len * nb;
    const std::function<void()> pieces[2] = {
        [&] { gs_dots_launch(basis.get(), len, (int)nb, w, len, part.get(), st); },
        [&] { gs_dots_wide_launch(basis.get(), len, (int)nb, w, len, part.get(), st); },
    };
    time_pieces(st, pieces, 2, reps, ms);
    e.sync();
}

} // namespace t4a
