// linop.hpp — an operator (MPO) applied to a state (tensor train) when it acts on a subset of the state's sites: the chain form of
// tensor4all-treetn/src/operator/ (apply.rs: apply_linear_operator with ApplyOptions::{zipup, fit, naive}; identity.rs: the identity
// on gap nodes; compose.rs: the operator bond carried along the state's path between two operator nodes, are_exclusive_operators,
// compose_exclusive_linear_operators).  Node names are positions.
//
// The state has n sites X_i[b, x, b'], the operator k >= 1 sites O_j[a, y, x, a'] (leg 0 the output, leg 1 the input) at the state
// positions sites = (p_0 < ... < p_{k-1}).  A state site is
//   Op       i == p_j: the result site has dimension O_j.s1,
//   Bridge   p_0 < i < p_{k-1}, i not in sites: the bond m_i between O_j and O_{j+1} passes through unchanged (the delta bridge),
//   Outside  i < p_0 or i > p_{k-1}: the operator bond is 1 (the identity with a dummy link).
// Bonds are fused with the operator index slow and the state index fast, (a Lb + b), which is the order of
// mpo_site_contract_kernel with the operator as A.  No identity or bridge tensor is materialised on the fused route; the composed
// route builds them (extend_operator_to_full_space) and runs the kernels of the MPO-MPO contraction.
#pragma once

#include "mpo.hpp"

namespace t4a {

enum class ApplySiteKind : int { Op = 0, Bridge = 1, Outside = 2 };
enum class ApplyRoute : int { Auto = 0, Fused = 1, Composed = 2 };

struct ApplySitePlan {
    ApplySiteKind kind = ApplySiteKind::Outside;
    size_t op_site = 0;          // j for an Op site
    size_t m_left = 1, m_right = 1; // the operator bond to the left and right of the site (equal on a gap site: the pass-through bond)
    size_t d_in = 1, d_out = 1;  // the state's site dimension and the result's
    std::array<size_t, 3> result = {1, 1, 1}; // (m_left Lb, d_out, m_right Rb)
};

// Host only; every refusal happens here, before the device is touched (INVALID_ARGUMENT): one position per operator site, `sites` not
// strictly ascending, a site >= n ("Operator nodes [..] are not a subset of state nodes [..]", apply.rs:333), the operator's input
// dimension against the state's ("Shared shape mismatch at site ..."), a fused bond above 65535, a core or work matrix of more than
// INT_MAX elements.
std::vector<ApplySitePlan> apply_plan(const std::vector<std::array<size_t, 4>>& op_dims4, const std::vector<size_t>& sites,
                                      const std::vector<std::array<size_t, 3>>& state_dims3);

// The full-length operator: Op sites are device copies, Bridge sites delta_{aa'} delta_{yx} of shape [m, d, d, m], Outside sites
// [1, d, d, 1] identities, built exactly on the host and uploaded.
std::unique_ptr<Mpo> extend_operator_to_full_space(Mpo& op, const std::vector<size_t>& sites, const std::vector<size_t>& state_site_dims);

// compose.rs on a chain: the supports are vertex-disjoint, each is connected (contiguous), and none lies on the path between two
// sites of another (which contiguity already excludes).  Host only.
bool are_exclusive_operators(size_t n, const std::vector<std::vector<size_t>>& supports);
// The full-length operator of exclusive operators, gaps identities with bond 1.  INVALID_ARGUMENT "Operators are not exclusive: they
// may overlap or not form connected subtrees" (compose.rs:209).
std::unique_ptr<Mpo> compose_exclusive_linear_operators(const std::vector<size_t>& state_site_dims, const std::vector<Mpo*>& ops,
                                                        const std::vector<std::vector<size_t>>& supports);

struct ApplyOptions { // ApplyOptions (apply.rs) mapped onto MpoContractionOptions / MpoFitOptions
    MpoAlgorithm method = MpoAlgorithm::ZipUp;
    double tolerance = 1e-12;
    size_t max_bond_dim = 0;      // 0 == None
    size_t max_sweeps = 1;        // nfullsweeps
    bool has_convergence_tol = false; // false: every sweep runs
    double convergence_tol = 0.0;
};
// INVALID_ARGUMENT for a negative or non-finite tolerance / convergence_tol (host only)
void apply_validate_options(const ApplyOptions& opt);

// The route Auto takes, host only: Fused exactly where tools/probe_linop.py measured it faster by more than the spread (DESIGN.md
// section 8), Composed everywhere else, unmeasured sizes included.
ApplyRoute apply_route(MpoAlgorithm method, size_t n_sites, size_t n_gap_sites, size_t state_bond, size_t op_bond);

// Naive: every site in one launch of apply_site_kernel, no truncation (tolerance and cap are ignored, as in the reference's local
// exact apply).  ZipUp: the recursion of the partial contraction's zip-up, the site step at an Op site the half product of
// kernels_partial.hip on the matrix-product plan with T = 1, at a gap site apply_gap_half_kernel.  Fit: the sweeps of the MPO fit with
// the half products dispatching on the site kind, started from `initial` (same length and result site dims) or the zip-up above.
// Composed: extend_operator_to_full_space, then mpo_partial_contract / mpo_contract_fit on the state as an MPO with s2 = 1.
// The result is an MPO with site dims (d_out, 1): its cores are those of the result train.  `initial` likewise.
std::unique_ptr<Mpo> apply_linear_operator(Mpo& op, const std::vector<size_t>& sites, TensorTrain& state, const ApplyOptions& opt, ApplyRoute route,
                                           Mpo* initial, MpoFitInfo& info, ApplyRoute* taken = nullptr);
// The fused zip-up (fit == false) and fit (mpo.hip, beside the contraction they share their recursion and sweeps with): the operator and
// the state are read in place.
std::unique_ptr<Mpo> linop_fused_contract(Mpo& op, TensorTrain& state, const std::vector<ApplySitePlan>& plan, bool fit, const MpoFitOptions& opt,
                                          Mpo* initial, MpoFitInfo& info);

// Test hook: apply_gap_half_kernel on host buffers, exactly as the drivers launch it.  right == false: env is L[n_env, m, Lb], x is
// X[Lb, d, Rb], the result P[n_env, d, m, Rb]; right == true: env is R[m, Rb, n_env], the result Q[m, Lb, d, n_env].  With `fill` the
// output and `guard` doubles behind it hold *fill before the launch and come back too (padding and neighbours untouched).
std::vector<double> apply_gap_half(bool right, const double* env, size_t n_env, size_t m, const double* x, size_t lb, size_t d, size_t rb,
                                   const double* fill, size_t guard);

// Probe (tools/probe_linop.py): device ms per launch (events around `reps` launches behind a warm-up) of the left half of a bridge site:
// ms[0] apply_gap_half_kernel, ms[1] mpo_partial_half_kernel on the materialised bridge site [m, d, d, m] at the same shapes.
void linop_time_half(size_t n_env, size_t m, size_t lb, size_t d, size_t rb, size_t reps, double ms[2]);

// ---- kernels_apply.hip ----
// Site product, every site of the chain in one launch (job list as MpoSiteJob: ascending offsets, jobs[0].off == 0, every site of at
// most INT_MAX elements).  gap == 0:  Y[(a lb + b), y, (a' rb + b')] = sum_x O[a, y, x, a'] X[b, x, b'], x ascending, multiply and add
// rounded separately: the chain of operations of mpo_site_contract_kernel with t = 1.  gap != 0 (ml == mr, s1 == k):
// Y[(a lb + b), x, (a' rb + b')] = X[b, x, b'] for a == a', 0.0 otherwise; O is not read.
struct ApplySiteJob {
    const double* O; // [ml, s1, k, mr]
    const double* X; // [lb, k, rb]
    double* Y;       // [ml lb, s1, mr rb]
    unsigned long long off;
    int ml, s1, k, mr, lb, rb, gap, pad_;
};
void apply_site_launch(const ApplySiteJob* d_jobs, int n_jobs, unsigned long long total, hipStream_t stream);
// Half product of a gap site, both mirrors through strides (all in elements; every operand and the output of at most INT_MAX elements):
//   out[n on + x ox + a oa + c oc] = sum_{k < K} E[n en + a ea + k ek] X[k xk + x xx + c xc]      n < N, a < M, x < S, c < C
// Returns false, having launched nothing, when the grid would hold more than INT_MAX workgroups.
struct ApplyGapHalfDesc {
    const double* E;
    const double* X;
    double* out;
    int N, M, S, K, C;
    long long en, ea, ek;
    long long xk, xx, xc;
    long long on, ox, oa, oc;
};
bool apply_gap_half_launch(const ApplyGapHalfDesc& d, hipStream_t stream);

} // namespace t4a
