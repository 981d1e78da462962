// linsolve.hpp — (a0 + a1 A) x = b for an MPO A and tensor trains x, b on the device: the two-site sweeps with a local GMRES of
// tensor4all-treetn's square_linsolve (crates/tensor4all-treetn/src/linsolve/: square/mod.rs:233-351, square/updater.rs:374-498,
// :549-622, :848-863, common/projected_operator.rs:230-410, :495-631, square/projected_state.rs, treetn/localupdate.rs:103-160,
// :377-448; tensor4all-core/src/krylov.rs:1083-1490 gmres_affine_impl), restated for a chain, f64, V_in = V_out: every site of A has
// s1 == s2 == the site dimension of the state.  Index mappings, tree topologies, spectator nodes and complex scalars stay out.
//
// Layouts (column-major): environments L[beta, w, alpha], R[beta, w, alpha] (bra bond, operator bond, ket bond), operator sites
// A_i[w_l, s, t, w_r], two-site vector v[alpha_l, t1, t2, alpha_r] read as the M x N matrix V, M = chi_l d_i, N = d_{i+1} chi_r.
// Half operators of a bond step (W the middle operator bond), built once per step by kernels_linsolve.hip:
//   HL[(beta_l s1) + M w, (alpha_l t1)] = sum_{w_l} L[beta_l, w_l, alpha_l] A_i[w_l, s1, t1, w]          (W M) x M
//   HR[w + W (t2 alpha_r), (s2 beta_r)] = sum_{w_r} A_{i+1}[w, s2, t2, w_r] R[beta_r, w_r, alpha_r]      (W N) x N
// The projected apply y = sum_w HL_w V HR_w is two plain products on gemm_launch: T = HL V, (W M) x N, and Y = T HR with the same
// memory of T read as M x (W N) — index m + M w + M W n in both views, which is why w is the fast index of HR's rows.
// 2 W M N (M + N) flops per apply; HL and HR take W (M^2 + N^2) doubles, T another W M N, the Krylov basis (restart_dim + 1) M N.
// A step one of whose buffers would hold more than INT_MAX elements is refused (INVALID_ARGUMENT naming the bond).
// The environments come from the same operands: L_{i+1}[:, w, :] = X_i^T (HL_w X_i), R_{i+1}[:, w, :] = (X_{i+1} HR_w^T) X_{i+1}^T.
#pragma once

#include <array>
#include <functional>
#include <memory>
#include <vector>

#include "krylov.hpp"
#include "mpo.hpp"
#include "tensorops.hpp"

namespace t4a {

// ---- kernels_linsolve.hip (the vector kernels of the Krylov solvers are declared in krylov.hpp).  All pointers are device pointers;
// launchers enqueue on `stream` and do not synchronise.
// HL from L[chi, Wl, chi] and A[Wl, d, d, W]; HR from A[W, d, d, Wr] and R[chi, Wr, chi]
void linsolve_hl_launch(const double* L, const double* A, double* HL, int chi, int Wl, int d, int W, hipStream_t stream);
void linsolve_hr_launch(const double* A, const double* R, double* HR, int chi, int W, int d, int Wr, hipStream_t stream);
// r = b - (a0 x + a1 ax) with the shares of |r|^2 in npart
void linsolve_residual_launch(const double* b, const double* x, const double* ax, double a0, double a1, double* r, size_t len, double* npart,
                              hipStream_t stream);
void linsolve_scale_launch(const double* in, double alpha, double* out, size_t len, hipStream_t stream);

// ---- GMRES on (a0 + a1 H) x = b (krylov.rs:1083-1490).  The Arnoldi basis is built from the unshifted H, a0 and a1 enter the
// Hessenberg column; Givens rotations and the triangular solve run on the host, which reads j + 2 doubles per step and one norm per
// restart.  Deviation from the reference: both orthogonalisation passes are classical Gram–Schmidt (all coefficients of a pass from
// one launch) where the reference's are modified Gram–Schmidt; the column of H is still pass 1 plus pass 2.
enum class GmresToleranceMode : int { Relative = 0, Absolute = 1 };
struct GmresResult {
    size_t iterations = 0;
    double residual = 0.0;
    bool converged = false;
    size_t apply_calls = 0;
};
class Gmres {
public:
    explicit Gmres(Engine& e) : eng_(e), gs_(e) {}
    // x: the start on entry, the solution on exit (device, len doubles).  Non-convergence is a flag.  INVALID_ARGUMENT: a0 == a1 == 0.
    GmresResult solve(const GmresApply& apply, size_t len, const double* d_b, double* d_x, double a0, double a1, double tol, GmresToleranceMode mode,
                      size_t restart_dim, size_t max_restarts);
    void reserve(size_t len, size_t restart_dim);

private:
    Engine& eng_;
    KrylovOrth gs_;
    DevBuf<double> basis_, ax_, hcol_, coef_;
};

// ---- options and results of the solver (LinsolveOptions, SquareLinsolveResult of the reference)
struct LinsolveOptions {
    size_t nfullsweeps = 5;
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    bool has_svd_policy = false; // none: the default policy tensor_svd applies
    SvdPolicy svd_policy;
    double gmres_tol = 1e-10;
    GmresToleranceMode gmres_tolerance_mode = GmresToleranceMode::Relative;
    size_t gmres_max_restarts = 100;
    size_t gmres_restart_dim = 30;
    double a0 = 0.0, a1 = 1.0;
    bool has_convergence_tol = false;
    double convergence_tol = 0.0;
    bool check_residual = true;
    void validate() const; // INVALID_ARGUMENT (host only)
};
struct LinsolveStats {
    size_t local_solves = 0, arnoldi_steps = 0, apply_calls = 0;
};
struct LinsolveResult {
    std::unique_ptr<TensorTrain> solution;
    size_t sweeps = 0;
    bool has_residual = false;
    double residual = 0.0;
    bool converged = false;
    LinsolveStats stats;
};
constexpr size_t LINSOLVE_RESTART_DIM_MAX = 8191; // the coefficients of a pass sit in the LDS of gs_update

// The shape checks of the solver on the host, before the device is touched (INVALID_ARGUMENT with a message): fewer than two sites,
// lengths differ, a site of A that is not square or does not match the state's or the rhs's site dimension, center >= n, and a bond
// step whose work buffers (HL, HR, T, the Krylov basis of restart_dim + 1 columns) would hold more than INT_MAX elements at the
// bonds of `state` (the bonds the sweeps reach are checked again as they grow).  rhs may be null (the projected operator alone).
void linsolve_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>* rhs,
                              const std::vector<std::array<size_t, 3>>& state, size_t center, size_t restart_dim);

// The INT_MAX bound of the buffers of the bond step (i, i + 1): HL, HR, T and a Krylov basis of basis_dim + 1 columns, M = chi_l d1,
// N = d2 chi_r, W the operator bond between the two sites.  INVALID_ARGUMENT "<who>: a work buffer of the bond step (i, i+1) ...".
void check_bond_step_dims(const char* who, size_t i, size_t chi_l, size_t d1, size_t d2, size_t chi_r, size_t W, size_t basis_dim);
// The same bound for the one-site step at site c: HL (W M M), T (W M chi_r), the environment R_{c+1} (chi_r W chi_r) and a Krylov basis of
// basis_dim + 1 columns of M chi_r elements, M = chi_l d, W the operator bond to the right of the site.
// INVALID_ARGUMENT "<who>: a work buffer of the one-site step at site c ...".
void check_site_step_dims(const char* who, size_t c, size_t chi_l, size_t d, size_t chi_r, size_t W, size_t basis_dim);

// The same bound for the bond-centre step of one-site TDVP at the bond (i, i + 1): the environments La (ka W ka) and Rb (kb W kb), T
// (ka W kb) and a Krylov basis of basis_dim + 1 columns of ka kb elements.
// INVALID_ARGUMENT "<who>: a work buffer of the bond-centre step at the bond (i, i+1) ...".
void check_bond_center_dims(const char* who, size_t i, size_t ka, size_t kb, size_t W, size_t basis_dim);

// ---- what the sweeps of square_linsolve, dmrg, tdvp and gse share on the host
std::vector<std::array<size_t, 3>> dims3_of(const std::vector<DevCore>& cores);
void require_tol(double v, const std::string& what); // INVALID_ARGUMENT `what` unless v is finite and not negative
// INVALID_ARGUMENT: a threshold that is not finite or negative, "<who>: unknown scale, measure or rule"
void validate_svd_policy(const SvdPolicy& policy, const char* who);
// The checks every solver starts with, in this order: "<who>: lengths differ: ..", "<who>: <few_sites>" for fewer than two sites, then per
// site an operator site that is not square, one that does not match the state's dimension, a rhs site (rhs may be null) that does not.
void validate_chain_operands(const char* who, const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>* rhs,
                             const std::vector<std::array<size_t, 3>>& state, const char* few_sites);
// The options of the split of a bond step: truncating, `policy` and `max_bond_dim` where the solver's options carry them
SvdOptions sweep_svd_options(bool has_policy, const SvdPolicy& policy, bool has_max_bond_dim, size_t max_bond_dim);
// The Euler tour of the bonds from `center`, the second node of a step the new centre: f(i, move_right) for the bonds c .. n-2 to the
// right, n-2 .. 0 to the left, 0 .. c-1 to the right
template <class F> void for_each_bond_from(size_t center, size_t n, F&& f)
{
    for (size_t i = center; i + 1 < n; ++i) f(i, true);
    for (size_t i = n - 1; i-- > 0;) f(i, false);
    for (size_t i = 0; i < center; ++i) f(i, true);
}

// ||(a0 + a1 A) x - b|| / ||b||, the absolute norm when ||b|| <= 1e-15: the exact naive apply, add / sub, and the norm of the residual
// train from its QR right-canonical form (the transfer-matrix norm2 would lose half of the digits in the cancellation).
double relative_linear_system_residual(Mpo& op, TensorTrain& x, TensorTrain& rhs, double a0, double a1);

// The projected operator of <x|A|x> on a chain with lazily computed, cached environments; with a rhs also the projected state <x|b>.
// It owns device copies of the operator, the state and the rhs on an engine of its own.
class ProjectedOperator {
public:
    ProjectedOperator(Mpo& op, TensorTrain& state, TensorTrain* rhs);

    size_t len() const { return x.size(); }
    // (chi_l, d_i, d_{i+1}, chi_r) of the region (site, site + 1)
    std::array<size_t, 4> local_dims(size_t site) const;
    // y = H v for the region (site, site + 1), host arrays of chi_l d_i d_{i+1} chi_r doubles
    std::vector<double> apply(size_t site, const double* v);
    // y = H v for the one-site region `site`, host arrays of chi_l d chi_r doubles: y[b, s, b'] = sum L_c[b, w, a] A_c[w, s, t, w']
    // v[a, t, a'] R_{c+1}[b', w', a'].  *reused_hl (may be null): whether the HL of an earlier prepare of the bond (site, site + 1) served.
    std::vector<double> apply_one_site(size_t site, const double* v, bool* reused_hl = nullptr);
    // side 0: L_bond[chi, W, chi] of the sites < bond; side 1: R_bond[chi, W, chi] of the sites >= bond (bond <= n); dims receives the shape
    std::vector<double> environment(int side, size_t bond, size_t dims[3]);
    // the caches that contain `site` go stale: L_j for j > site, R_j for j <= site
    void invalidate(size_t site);
    void set_site_tensors(size_t site, const size_t d1[3], const double* t1, const size_t d2[3], const double* t2);

    // -- the pieces the sweeps use (device side, on the engine's stream)
    Engine& engine() { return op_->tt.eng; }
    const double* left_env(size_t i);   // L_i, valid on the stream
    const double* right_env(size_t i);  // R_i
    const double* left_rhs_env(size_t i);
    const double* right_rhs_env(size_t i);
    void prepare(size_t site);                               // environments and HL, HR of the bond (site, site + 1)
    void apply_prepared(const double* d_v, double* d_out);   // the two products
    // The one-site region c (the site correction of TDVP): environments L_c and R_{c+1} and HL = L_c A_c, (W M) x M with M = chi_l d and
    // W the bond to the right of A_c, by linsolve_hl_launch — unless hl_ still holds it from prepare(c), the bond step that moved left
    // onto c (HL depends on the sites < c and on the operator only); -> whether it was reused.
    bool prepare_one_site(size_t c);
    // T = HL V, (W M) x chi_r, then Y = T_view R_view^T: T read as M x (W chi_r) with ld M, R_{c+1}[b', w', a'] as chi_r x (W chi_r) with
    // ld chi_r — the column index is w' + W a' in both views.  2 W M chi_r (M + chi_r) flops.
    void apply_one_site_prepared(const double* d_v, double* d_out);
    void check_site_step(size_t c, size_t basis_dim, const char* who) const;  // check_site_step_dims at the present bonds
    // The bond-centre (zero-site) region of one-site TDVP next to site c, whose tensor x[c] holds the isometry Q of the full-rank thin QR
    // x_c = Q C (toward_right) or x_c = C Q: the operator on the bond matrix C (ka x kb) is
    //   Y[b, b'] = sum_w sum_a sum_a' La[b, w, a] C[a, a'] Rb[b', w, a'].
    // toward_right: Rb = R_{c+1} from the cache and La[:, w, :] = Q^T (HL_w Q) from HL = L_c A_c (prepare_one_site(c), reused when hl_
    // still holds it) — the arithmetic of update_left_from_prepared, whose result is also the cache entry L_{c+1}; ka = x[c].r, kb the bond
    // to the right.  Else the mirror image: La = L_c, HR = A_c R_{c+1} by linsolve_hr_launch and Rb[:, w, :] = (Q HR_w^T) Q^T as
    // update_right_from_prepared forms it, the cache entry R_c; ka the bond to the left, kb = x[c].l.  Built once per step.
    void prepare_bond_center(size_t c, bool toward_right);
    // y = the operator above on the device matrix d_c, by the route of tdvp_bond_apply_route (or the forced one)
    void apply_bond_center_prepared(const double* d_c, double* d_out);
    std::array<size_t, 3> bond_center_dims() const { return {bc_ka_, bc_kb_, bc_w_}; }
    // Test hook: prepare_bond_center(c, toward_right) with the present x[c] as Q -> the environment that contains it on the host,
    // La[k, W, k] (toward_right) or Rb[k, W, k]; dims receives (k, W, k)
    std::vector<double> bond_center_environment(size_t c, bool toward_right, size_t dims[3]);
    void check_bond_center(size_t basis_dim, const char* who) const;  // check_bond_center_dims at the prepared bond
    const double* bond_center_env(bool left) const { return left ? bc_la_ : bc_rb_; }
    size_t fused_applies = 0, gemm_applies = 0;                       // launches of apply_bond_center_prepared by route
    // Probe: device ms of the three launches of the one-site apply at site c (linsolve_hl, T = HL V, Y = T R^T), events around `reps`
    // launches behind a warm-up launch
    void time_one_site(size_t c, size_t reps, double ms[3]);
    // Probe: device time in ms (HIP events around `reps` launches behind one warm-up launch) of the five launches of an Arnoldi step
    // with nb basis vectors at the region (site, site + 1): T = HL V, Y = T HR, gs_dots, gs_update, gs_normalize
    void time_step(size_t site, size_t nb, size_t reps, double ms[5]);
    void local_rhs(size_t site, double* d_out);              // Lb_i b_i b_{i+1} Rb_{i+2} as M x N
    void update_left_from_prepared(size_t site);             // L_{site+1} (and Lb) from x[site] and the HL of prepare(site)
    void update_right_from_prepared(size_t site);            // R_{site+1} (and Rb) from x[site+1] and the HR of prepare(site)
    void check_step(size_t site, size_t restart_dim, const char* who = "square_linsolve") const;  // INT_MAX bound of the step's buffers
    // The back half of a bond step of the sweeps (square_linsolve, dmrg): theta (device, M x N of the region (site, site + 1)) is split by
    // tensor_svd with `so`, x[site] = U | U S and x[site + 1] = S Vt | Vt (move_right | left: the singular values go to the new centre), both
    // sites are invalidated and the environment of the side left behind is rebuilt from the half operators of prepare(site).
    void split_and_advance(size_t site, const double* d_theta, const SvdOptions& so, bool move_right, const char* who);
    size_t two_site_vector(size_t site, DevBuf<double>& theta); // theta = x_site x_{site+1} as M x N, grown as needed -> M N
    void canonicalize(size_t center);                            // x onto `center` by the thin QR steps of a QrSweep

    std::vector<DevCore> x, b;

private:
    void product_left(const double* d_v);
    void product_right(double* d_out);
    std::unique_ptr<Mpo> op_;
    std::vector<DevBuf<double>> envL_, envR_, envLb_, envRb_;
    std::vector<char> okL_, okR_;
    DevBuf<double> hl_, hr_, t_, t1_, p1_, p2_;
    size_t prepared_ = (size_t)-1;
    size_t prepared1_ = (size_t)-1;  // the site of prepare_one_site
    size_t hl_site_ = (size_t)-1;    // hl_ holds L_c A_c of this site c
    const double* r1_ = nullptr;     // R_{c+1} of prepare_one_site
    const double *bc_la_ = nullptr, *bc_rb_ = nullptr;  // the environments of prepare_bond_center
    size_t bc_ka_ = 0, bc_kb_ = 0, bc_w_ = 0, bc_bond_ = 0;
};

// The apply on caller-supplied environments (host arrays), launched exactly as the sweeps launch it: L[chi_l, W_l, chi_l],
// R[chi_r, W_r, chi_r] with the operator bonds of sites `site` and `site + 1`, v and the result chi_l d_i d_{i+1} chi_r doubles.
// hl / hr (may be null) receive the half operators, (W M) x M and (W N) x N.
std::vector<double> projected_apply_env(const double* L, const double* R, size_t chi_l, size_t chi_r, Mpo& op, size_t site, const double* v,
                                        std::vector<double>* hl, std::vector<double>* hr);

// square_linsolve (square/mod.rs:233-351).  `init` is canonicalised onto `center` by thin QR sweeps; the sweep plan is the Euler tour
// from `center`, two sites per step, the second node of a step the new centre: bonds c .. n-2 to the right, n-2 .. 0 to the left,
// 0 .. c-1 to the right.  a1 == 0 or ||A|| <= 1e-15: the solution is rhs / a0 and sweeps = 0.
LinsolveResult square_linsolve(Mpo& op, TensorTrain& rhs, TensorTrain& init, size_t center, const LinsolveOptions& options);

// Test hook: GMRES as the sweeps run it on a dense n x n matrix H (host, column-major) applied on the device.
GmresResult gmres_dense(const double* H, size_t n, const double* b, const double* x0, double a0, double a1, double tol, GmresToleranceMode mode,
                        size_t restart_dim, size_t max_restarts, double* x_out);
// Test hook: krylov_orth_host on the serial route, what Gmres launches: basis len x nb, w len (in/out), h_out 2 nb (pass 1, pass 2), *norm_out
void linsolve_orth(const double* basis, size_t len, size_t nb, double* w, double* h_out, double* norm_out);
// Test hook: KrylovOrth::orth with the given route on host arrays
void krylov_orth_host(const double* basis, size_t len, size_t nb, double* w, KrylovDotsRoute route, double* h_out, double* norm_out);
// Probe hook: device ms (events around `reps` launches behind a warm-up launch) of gs_dots_launch [0] and gs_dots_wide_launch [1] with nb
// basis vectors of length len, behind the argument checks (INVALID_ARGUMENT) and require_device
void krylov_time_dots(size_t len, size_t nb, size_t reps, double ms[2]);

} // namespace t4a
