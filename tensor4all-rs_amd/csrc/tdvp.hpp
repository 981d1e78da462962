// tdvp.hpp — two-site TDVP on the device: a tensor train evolved under an MPO H by sweeps of projected exponentials, tensor4all-treetn's
// tdvp / tdvp_with_treetn_operator (crates/tensor4all-treetn/src/tdvp/mod.rs:1107-1268, update_two_site :916-1042, the site correction
// :639-700, the full-rank centre move :1318-1390, the region plan tdvp/plan.rs:41-181) on the Hermitian Krylov exponential of
// tensor4all-core (krylov.rs:693-926), restated for what square_linsolve and dmrg cover: a chain, f64, one site index per node,
// V_in = V_out (every site of H has s1 == s2 == the state's site dimension; the dimensions may differ from site to site).  Trees, index
// mappings and verbose output stay out.
//
// Deviations from the reference, both refused on the host with INVALID_ARGUMENT before the device is touched:
//   * The exponent is REAL.  The reference's exponent_step is complex with the default -0.1i; this code base has no complex scalars, so
//     the options carry exponent_step_re (default -0.1) and exponent_step_im, and a non-zero imaginary part is refused: real-time
//     evolution needs complex trains.  u' = -H u (heat and diffusion flows, imaginary-time relaxation) is what a real exponent covers.
//   * `center` must be 0 or n - 1.  The reference's two-site plan walks root-edge-first DFS edges; from an inner root of a chain it runs
//     one arm to its leaf, applies the site correction at that leaf and jumps to the other arm, while the projector splitting needs that
//     correction at the root (DESIGN.md §8 has the measured errors).  From an end the plan is the standard 2TDVP sweep.
//   * nsite = 1 (the bond-centre apply and a QR per step) is not implemented.
//
// The projected operator, its cached environments, the half operators, the QR canonicalisation and the SVD split are those of
// linsolve.hpp.  A two-site step at bond (i, i+1): theta_0 = x_i x_{i+1}, prepare(i), KrylovExpm with the step's exponent, tensor_svd
// (no renormalisation), the singular values into the new centre.  A correction step at site c: prepare_one_site(c), KrylovExpm with
// minus the step's exponent on x_c, the result replaces x_c.  Both orthogonalisation passes of the Krylov basis are classical
// Gram–Schmidt (the deviation of Gmres and Lanczos); their projections come from gs_dots_wide where krylov_dots_route says so.
#pragma once

#include "dmrg.hpp"

namespace t4a {

// ---- hermitian_krylov_expm_multiply (krylov.rs:707-926) for a real exponent
struct KrylovExpmOptions { // HermitianKrylovExpmOptions::default()
    size_t max_iter = 30, max_time_splits = 100;
    double tol = 1e-12, breakdown_tol = 1e-14, hermitian_tol = 1e-10;
    void validate() const; // INVALID_ARGUMENT (host only); max_iter <= LINSOLVE_RESTART_DIM_MAX
};
struct KrylovExpmResult {
    size_t iterations = 0, apply_calls = 0; // over all accepted substeps
    double error_estimate = 0.0;            // the largest |theta| beta |c_j| of an accepted substep
    bool converged = false;
    size_t time_splits = 1;
};
class KrylovExpm {
public:
    explicit KrylovExpm(Engine& e) : eng_(e), ar_(e) { ar_.orth().set_dots_route(KrylovDotsRoute::Auto); }
    void reserve(size_t len, size_t max_iter); // the basis: (max_iter + 1) len doubles, and a copy of the start
    // d_x: the start on entry, exp(tau H) start on exit.  tau == 0 or |start| <= breakdown_tol: d_x is left as it is.  The host reads one
    // norm per substep and j + 2 doubles per Krylov step.  INVALID_ARGUMENT: a projected matrix that is not Hermitian; INTERNAL_ERROR:
    // "hermitian_krylov_expm_multiply did not converge within max_time_splits=.. and max_iter=..".
    KrylovExpmResult solve(const GmresApply& apply, size_t len, double* d_x, double tau, const KrylovExpmOptions& o);

private:
    KrylovExpmResult once(const GmresApply& apply, size_t len, double* d_x, double tau, const KrylovExpmOptions& o);
    Engine& eng_;
    HermitianArnoldi ar_;
    DevBuf<double> start_;
};

// ---- the region plan (plan.rs) of a chain rooted at an end
enum class TdvpStepKind : int { TwoSite = 0, SiteCorrection = 1 };
struct TdvpStep {
    TdvpStepKind kind;
    size_t nodes[2]; // TwoSite: (the other node, the new centre); SiteCorrection: nodes[0] == nodes[1] == the site
    size_t new_center;
    double exponent;
};
// applyexp_sub_steps(order): [1], [1/2, 1/2], [s/2, s/2, 1/2 - s, 1/2 - s, s/2, s/2] with s = 1 / (2 - 2^(1/3)).  INVALID_ARGUMENT:
// another order.
std::vector<double> tdvp_sub_steps(size_t order);
// The first-order sweep from 0 is Two(0,1)->1, Corr(1, -tau), Two(1,2)->2, .., Two(n-2,n-1)->n-1 (no correction after the last edge),
// from n - 1 its mirror image; every substep carries tau * weight, every even substep (1-based) is the reversed list with the nodes
// reversed and the last node the new centre.  Host only.  INVALID_ARGUMENT: n < 2, an inner or missing centre, an unknown order, a
// non-finite tau.
std::vector<TdvpStep> tdvp_plan(size_t n, size_t center, size_t order, double tau);

// ---- TdvpOptions, TdvpResult of the reference
struct TdvpOptions {
    size_t nsite = 2, nsweeps = 1, order = 2;
    double exponent_step_re = -0.1, exponent_step_im = 0.0;
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    bool has_svd_policy = false; // none: the default policy tensor_svd applies
    SvdPolicy svd_policy;
    KrylovExpmOptions krylov;
    void validate() const; // INVALID_ARGUMENT (host only)
};
struct TdvpStats {
    size_t two_site_steps = 0, corrections = 0, krylov_steps = 0, apply_calls = 0, max_time_splits = 0;
};
struct TdvpResult {
    std::unique_ptr<TensorTrain> state;
    size_t sweeps_completed = 0, local_updates = 0;
    double max_error_estimate = 0.0;
    size_t max_krylov_iterations = 0;
    TdvpStats stats;
};

// The shape checks on the host, before the device is touched (INVALID_ARGUMENT with a message): lengths differ, fewer than two sites
// (EmptyTwoSiteSweep), a site of the operator that is not square or does not match the state's site dimension, a centre that is not a
// state node or not an end of the chain, and a bond step or a one-site step whose work buffers (HL, HR, T, the basis of max_iter + 1
// columns) would hold more than INT_MAX elements.
void tdvp_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter);

TdvpResult tdvp(Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& options);

// Test hook on host arrays: the solver the sweeps run, on a dense n x n matrix (column-major) applied on the device.
KrylovExpmResult krylov_expm_dense(const double* H, size_t n, const double* v0, double tau, const KrylovExpmOptions& o, double* out);

} // namespace t4a
