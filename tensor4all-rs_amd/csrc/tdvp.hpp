// tdvp.hpp — TDVP on the device in two modes, two-site (tdvp) and one-site (tdvp_one_site): a tensor train evolved under an MPO H by sweeps
// of projected exponentials, tensor4all-treetn's tdvp / tdvp_with_treetn_operator (crates/tensor4all-treetn/src/tdvp/mod.rs:1107-1268,
// update_two_site :916-1042, the site correction :639-700, the one-site update and its bond correction :639-914, the full-rank centre move
// :1318-1390, the region plan tdvp/plan.rs:41-181) on the Hermitian Krylov exponential of tensor4all-core (krylov.rs:693-926), restated
// for what square_linsolve and dmrg cover: a chain, f64, one site index per node, V_in = V_out (every site of H has s1 == s2 == the
// state's site dimension; the dimensions may differ from site to site).  Trees, index mappings and verbose output stay out.
//
// The shared core.  Both modes are one driver with two thin loops (tdvp.hip): one validator of TdvpOptions that takes the mode the
// caller requires (TdvpMode), one expansion of a base sweep over tdvp_sub_steps, one TdvpResult, and one sweep context that owns the
// projected operator, the QR sweep, the Krylov exponential, the centre and the result and provides the steps — the centre move by
// full-rank thin QR steps, the site exponential (the two-site mode's site correction and the one-site mode's site step are this one
// function), the two-site step, the bond correction, the epilogue.  A mode is its base plan, its shape checks and its loop over the plan.
//
// Deviations from the reference that both modes share, refused on the host with INVALID_ARGUMENT before the device is touched:
//   * The exponent is REAL.  The reference's exponent_step is complex with the default -0.1i; this code base has no complex scalars, so
//     the options carry exponent_step_re (default -0.1) and exponent_step_im, and a non-zero imaginary part is refused: real-time
//     evolution needs complex trains.  u' = -H u (heat and diffusion flows, imaginary-time relaxation) is what a real exponent covers.
// Deviations of the two-site mode, refused in the same way:
//   * `center` must be 0 or n - 1.  The reference's two-site plan walks root-edge-first DFS edges; from an inner root of a chain it runs
//     one arm to its leaf, applies the site correction at that leaf and jumps to the other arm, while the projector splitting needs that
//     correction at the root (DESIGN.md §8 has the measured errors).  From an end the plan is the standard 2TDVP sweep.
//   * tdvp refuses nsite = 1: one-site TDVP has entry points of its own, tdvp_one_site_plan and tdvp_one_site below.
// The deviations of the one-site mode stand with tdvp_one_site below.
//
// The projected operator, its cached environments, the half operators, the QR canonicalisation and the SVD split are those of
// linsolve.hpp.  A two-site step at bond (i, i+1): theta_0 = x_i x_{i+1}, prepare(i), KrylovExpm with the step's exponent, tensor_svd
// (no renormalisation), the singular values into the new centre.  A site exponential at site c: prepare_one_site(c), KrylovExpm with
// the step's exponent on x_c (minus tau for the correction of the two-site mode), the result replaces x_c.  Both orthogonalisation
// passes of the Krylov basis are classical Gram–Schmidt (the deviation of Gmres and Lanczos); their projections come from gs_dots_wide
// where krylov_dots_route says so.
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
enum class TdvpStepKind : int { TwoSite = 0, SiteCorrection = 1, OneSite = 2 };
struct TdvpStep {
    TdvpStepKind kind;
    size_t nodes[2]; // TwoSite: (the other node, the new centre); SiteCorrection, OneSite: nodes[0] == nodes[1] == the site
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
// The one-site plan (first_order_sweep with nsite = 1, plan.rs:97-111): the nodes in post order from `center` — the left arm leaf first
// (0 .. c-1), then the right arm leaf first (n-1 .. c+1), then c; "left arm first" is this project's rule, as in the GSE edge walk.  Every
// step is OneSite with the region [node], new_center = node and the exponent tau * weight (the operation order of tdvp_plan); every even
// substep (1-based) is the reversed list.  Any centre 0 <= c < n.  Host only.  INVALID_ARGUMENT: n == 0, center >= n, an unknown order,
// a non-finite tau.
std::vector<TdvpStep> tdvp_one_site_plan(size_t n, size_t center, size_t order, double tau);

// ---- TdvpOptions, TdvpResult of the reference
enum class TdvpMode : int { OneSite = 1, TwoSite = 2 }; // the driver a caller is about to run; its value is the nsite it requires
struct TdvpOptions {
    size_t nsite = 2, nsweeps = 1, order = 2;
    double exponent_step_re = -0.1, exponent_step_im = 0.0;
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    bool has_svd_policy = false; // none: the default policy tensor_svd applies
    SvdPolicy svd_policy;
    KrylovExpmOptions krylov;
    // INVALID_ARGUMENT (host only), the first rule that is broken.  TwoSite, the rules of tdvp: nsite outside {1, 2}, nsweeps, order, the
    // exponent finite, max_bond_dim == 0 when set, nsite == 1 (refused: see tdvp_one_site), the exponent real, the Krylov options, the
    // SVD policy.  OneSite, the rules of tdvp_one_site in the order of the reference's validate_options (mod.rs:1270-1316): nsite != 1
    // (this project's message, naming tdvp for nsite = 2), nsweeps, order, the exponent finite and real, max_bond_dim == 0 when set, then
    // "invalid TDVP option max_bond_dim: one-site TDVP has fixed ranks; use nsite=2 for truncation" and the same for svd_policy, then the
    // Krylov options.
    void validate(TdvpMode mode) const;
};
// The counters of both modes: a mode leaves those of the other at zero (qr_steps, the centre moves, is counted in both).
struct TdvpStats {
    size_t two_site_steps = 0, corrections = 0, one_site_steps = 0, bond_corrections = 0, qr_steps = 0, krylov_steps = 0, apply_calls = 0, max_time_splits = 0,
           fused_applies = 0, gemm_applies = 0;
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

// ---- one-site TDVP (tdvp/mod.rs:639-914): fixed bond dimensions, no SVD.  `init` is canonicalised onto `center` (any site).  Per step of
// tdvp_one_site_plan: the centre moves to the node by full-rank thin QR steps, prepare_one_site, KrylovExpm with the step's exponent on
// x_c.  A bond correction follows iff the next step of the same sweep's plan exists and has another node t: x_c is factorised towards t
// by the full-rank thin QR of the centre moves (x_c = Q C to the right, C Q to the left), prepare_bond_center builds the environment that
// contains Q once, KrylovExpm with MINUS the step's exponent runs on the bond matrix C (tdvp_bond_apply), x_c = Q stays, C' is absorbed
// into the neighbour, and the environment built with Q is the valid cache entry the next step needs.  No renormalisation.
// local_updates counts site and bond solves: w (2n - 1) per sweep with w in {1, 2, 6} substeps.
// Deviations from the reference:
//   * The gauge: the reference stores Q C' and factorises it again on the next centre move; here Q stays and the neighbour absorbs C'.
//     The state is the same, the bond dimension is k = min(rows, columns) in both.
//   * The edge of the correction at a jump.  From an inner centre the plan jumps once per substep between the two arms.  The reference
//     corrects the FIRST edge of the path to the next node.  In a post-order substep that is the edge that leaves the finished arm, as the
//     projector splitting wants it.  In a reversed substep the jump runs from a leaf to the node next to the centre: the first edge was
//     corrected one step earlier, and the edge INTO the next node never is — at n = 5, c = 2 the reversed substep evolves the bond (3, 4)
//     twice and the bond (1, 2) not at all, and a second-order sweep is 5e-2 away from exp(tau H) psi at full bonds.
//     Here a reversed substep first moves the centre to the neighbour of the next node and corrects the LAST edge of the path: the exact
//     mirror image of the post-order substep, exact at full bonds from every centre.  Paths of one edge — every step from an end centre,
//     and every step but the jump from an inner one — are the reference's.
// The shape checks on the host (INVALID_ARGUMENT): the shared chain checks of validate_chain_operands (a single site is refused with a
// message of its own: they need two), center >= n, and a one-site step or a bond-centre step whose work buffers would hold more than
// INT_MAX elements (the message names the site or the bond).
void tdvp_one_site_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter);
TdvpResult tdvp_one_site(Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& options);

// For callers that carry the mode as a value (GSE-TDVP, the C ABI): the shape checks and the driver of that mode.
void tdvp_validate_shapes(TdvpMode mode, const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter);
TdvpResult tdvp(TdvpMode mode, Mpo& op, TensorTrain& init, size_t center, const TdvpOptions& options);

// ---- the bond-centre apply (kernels_tdvp.hip, tdvp.hip; its environments: ProjectedOperator::prepare_bond_center).  Fused: tdvp_bond_apply_kernel, one launch, inside its envelope
// W k_b <= TDVP_BOND_FUSED_MAX_PANEL (16 W k_b doubles of LDS).  Gemm: T = La_view C with La read as (k_a W) x k_a, then Y = T_view Rb_view^T
// with T read as k_a x (W k_b) and Rb as k_b x (W k_b) — the column index is w + W a' in both views.  tdvp_bond_apply_route is the rule of
// Auto, a function of the shape alone (DESIGN.md section 8 has the measurements behind it); it never returns Auto.
enum class BondApplyRoute : int { Fused = 0, Gemm = 1, Auto = 2 };
constexpr size_t TDVP_BOND_FUSED_MAX_PANEL = 512; // W k_b: 64 KiB of LDS
constexpr int TDVP_BOND_MFMA_MIN = 16;            // the matrix cores from this bond up
constexpr size_t TDVP_BOND_FUSED_AUTO_WORK = 8192; // Auto: the fused launch up to W k_b (k_a + k_b) = 8192, the work of one workgroup, where it was measured to win
bool tdvp_bond_apply_fused_admits(size_t ka, size_t kb, size_t W);
BondApplyRoute tdvp_bond_apply_route(size_t ka, size_t kb, size_t W);
// forces the route of every bond-centre apply of the drivers (0 fused where the envelope admits it, 1 GEMM; anything else: the rule): a test hook
void tdvp_set_bond_apply_route(int route);
void tdvp_bond_apply_launch(const double* La, const double* C, const double* Rb, double* Y, int ka, int kb, int W, hipStream_t stream);
void tdvp_bond_apply_gemm(const double* La, const double* C, const double* Rb, double* T, double* Y, int ka, int kb, int W, hipStream_t stream);
// Test hook on host arrays: L[ka, W, ka], R[kb, W, kb], C and out ka x kb; -> the route taken.  INVALID_ARGUMENT: Fused outside the envelope.
BondApplyRoute tdvp_bond_apply_host(const double* L, const double* R, const double* C, size_t ka, size_t kb, size_t W, BondApplyRoute route, double* out);
// Probe: device ms (events around `reps` launches behind a warm-up launch, the routes alternating) of the fused launch [0] (NaN outside
// its envelope) and the two GEMMs [1]
void tdvp_bond_apply_time(size_t ka, size_t kb, size_t W, size_t reps, double ms[2]);

// Test hook on host arrays: the solver the sweeps run, on a dense n x n matrix (column-major) applied on the device.
KrylovExpmResult krylov_expm_dense(const double* H, size_t n, const double* v0, double tau, const KrylovExpmOptions& o, double* out);

} // namespace t4a
