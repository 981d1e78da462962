// fit_sum.hpp — variational sum of many tensor trains or MPOs on the device: tensor4all-treetn's fit_sum
// (crates/tensor4all-treetn/src/treetn/fit.rs:1521-1644, SumFitUpdater :1140-1337, fit_two_site_update :648-771, run_fit_sweeps
// :1076-1113, validate_fit_sum_options :1451-1473), restated for a chain, f64, by position.  An MPO enters as its train over the fused
// site index s1 + S1 s2.  Trees, complex scalars and the QR, LU and CI factorisations stay out.
//
// The result C is swept two sites at a time against the private environments <C|T_k> of every target; the local optimum of the bond
// (i, i+1) is Theta = sum_k L_k T_k[i] T_k[i+1] R_k.  On a chain the environments of all K targets at one bond are ONE matrix, the
// targets' bond indices concatenated (c a bond of C, S the site dimension, a_k / b_k the bonds of target k left / right of a site,
// A = sum_k a_k, B = sum_k b_k, off_k the offsets):
//   EL_i (c_i x A_i), ER_i (A_i x c_i), EL_0 = ER_n = ones
//   P = [EL_k T_k[i]]_k       (c S) x B:  P[c + chi_c (s + S (off_k + b))] = sum_a EL[c, offL_k + a] T_k[a, s, b]
//   Q = [T_k[i+1] ER_k]_k     B x (S c'): Q[(off_k + a) + A (s + S c')]    = sum_b T_k[a, s, b] ER[offR_k + b, c']
//   Theta = P Q               one GEMM over the concatenated index: the sum over the targets
//   EL_{i+1} = U^T P  (moving right),  ER_{i+1} = Q Vt^T  (moving left): one GEMM for all targets
// A bond step is two half launches (kernels_fit_sum.hip), two GEMMs, the SVD and the split, whatever K is.  The `gemm` route forms the
// same halves from gemm_launch, K products for P and K S for Q.
#pragma once

#include <array>
#include <memory>
#include <string>
#include <vector>

#include "linsolve.hpp"

namespace t4a {

// ---- kernels_fit_sum.hip.  One job of a half launch: O[r, c] = sum_kk X[r, kk] Y[kk, c] for r < m, c < n, kk < k ascending; the operands
// by row and column strides, the output row r at (r % rdiv) ors + (r / rdiv) ors2 (the right half writes the rows (a, s) of a target
// at a + A s of Q).  mfma: 16 x 16 output tiles on v_mfma_f64_16x16x4_f64 (a workgroup owns 16 rows x 64 columns); else one element per
// thread, 256 per workgroup.  tile0: the job's first workgroup; the table is sorted by it and lives in device memory.
struct FitSumJob {
    const double* X;
    const double* Y;
    double* O;
    long long xrs, xcs, yrs, ycs, ors, ors2, ocs;
    int m, k, n, rdiv;
    int tile0, mfma;
};
constexpr int FIT_SUM_MFMA_MIN = 16; // the summed and both output dimensions from here up: the matrix cores
inline bool fit_sum_job_mfma(size_t m, size_t k, size_t n) { return m >= FIT_SUM_MFMA_MIN && k >= FIT_SUM_MFMA_MIN && n >= FIT_SUM_MFMA_MIN; }
// workgroups of a job (m n <= INT_MAX)
inline long long fit_sum_job_tiles(size_t m, size_t n, bool mfma)
{
    return mfma ? (long long)((m + 15) / 16) * (long long)((n + 63) / 64) : (long long)((m * n + 255) / 256);
}
void fit_sum_half_launch(const FitSumJob* d_jobs, int n_jobs, int n_tiles, hipStream_t stream);

// ---- options and result (FitContractionOptions as fit_sum reads it)
enum class FitSumRoute : int { Auto = 0, Fused = 1, Gemm = 2 };
struct FitSumOptions { // FitOptions::new(1)
    size_t nfullsweeps = 1;
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    bool has_svd_policy = false; // none: the default policy tensor_svd applies
    SvdPolicy svd_policy;
    bool has_qr_rtol = false;
    double qr_rtol = 0.0;
    int factorize_alg = 0; // 0 SVD, 1 QR, 2 LU, 3 CI
    bool has_convergence_tol = false;
    double convergence_tol = 0.0;
    // validate_fit_sum_options, host only.  INVALID_ARGUMENT in the reference's order: the convergence tolerance, the QR tolerance, then
    // FactorizeOptions::validate (max_bond_dim == 0, the policy's threshold, "SVD factorization does not accept qr_rtol", "QR / LU/CI
    // factorization does not accept svd_policy / qr_rtol"); a valid QR, LU or CI request is NOT_IMPLEMENTED naming the algorithm.
    void validate() const;
};
struct FitSumResult {
    std::vector<DevCore> cores; // the fitted chain, its producing stream synchronised
    size_t sweeps_completed = 0, local_updates = 0;
    bool converged = false;
    std::vector<size_t> link_dims;
    std::vector<double> norms; // |psi| after each completed sweep
};
struct FitSumPlan {
    size_t bond_steps_per_sweep = 0; // 2 (n - 1): the Euler tour
    size_t half_launches_per_step = 0, gemms_per_step = 0, svds_per_step = 0;
    size_t prepare_half_launches = 0, prepare_gemms = 0;
};

// The checks on plain dimension lists, host only, in the reference's order: "fit_sum: targets must not be empty", an empty initial,
// "fit_sum: center node is not in initial TreeTN", per target "fit_sum: target i has an incompatible named topology" (another length)
// and "fit_sum: target i site-space validation failed" (another site dimension), then the INT_MAX bound of the work matrices (P, Q,
// Theta, the environments) of every bond step at the bonds of `initial`.  initial == nullptr: the first target (this project's).
void fit_sum_validate_shapes(const std::vector<std::vector<std::array<size_t, 3>>>& targets, const std::vector<std::array<size_t, 3>>* initial,
                             size_t center);
// INVALID_ARGUMENT "fit_sum: a work matrix of the bond step (i, i+1) holds more than INT_MAX elements": P (c S1) x B, Q B x (S2 c'),
// Theta, and the environments c x A, B x c, C x c' of the step
void fit_sum_check_step(size_t i, size_t c, size_t S1, size_t S2, size_t cn, size_t A, size_t B, size_t C);

// What `auto` takes for a bond step with K targets: Fused or Gemm (host only).  The rule is set from the measured table of DESIGN.md §8.
FitSumRoute fit_sum_route(size_t n_targets, size_t target_bond, size_t result_bond, size_t site_dim);
FitSumPlan fit_sum_plan(size_t n_sites, size_t center, size_t n_targets, size_t site_dim, FitSumRoute route);

// fit_sum (fit.rs:1521-1644).  `targets` are read in place (their streams are synchronised first); `initial` (nullptr: a clone of
// targets[0]) is copied and canonicalised onto `center` by forced thin-QR sweeps.  coefficients (nullptr: all ones): one real per
// target, sum_k w_k T_k, applied once by cloning and scaling site 0 of a target whose weight is not 1 (this project's extension, as is
// the null initial).  nfullsweeps == 0 returns a clone of the initial, one site the elementwise sum.  The sweep is the Euler tour from
// `center`, the second node of a step the new centre; the split is Canonical::Left (the first node takes the orthonormal factor, the
// second S Vt), capped by max_bond_dim, else uncapped under a policy, else by the present dimension of the bond.  With a convergence
// tolerance the sweeps stop when |exp(log|psi|_after - log|psi|_before) - 1| < tol.
FitSumResult fit_sum(const std::vector<const std::vector<DevCore>*>& targets, const std::vector<Engine*>& target_engines, const double* coefficients,
                     const std::vector<DevCore>* initial, Engine* initial_engine, size_t center, const FitSumOptions& options, FitSumRoute route);

// Test hook: one half for K targets on raw column-major host operands.  right == false: env is EL (chi x A), cores T_k[a_k, S, b_k] one
// after the other, the result P (chi S) x B; right == true: env is ER (B x chi), the result Q A x (S chi).  route Fused or Gemm.
// fill (may be null): the output buffer and FIT_SUM_HALF_GUARD doubles behind it hold *fill before the launch, and the guard is returned
// behind the result.
constexpr size_t FIT_SUM_HALF_GUARD = 64;
std::vector<double> fit_sum_half(bool right, FitSumRoute route, const double* env, size_t chi, size_t S, const double* cores, const size_t* a, const size_t* b,
                                 size_t K, const double* fill);
// Probe: device ms (events around `reps` launches behind a warm-up) of one half for K targets of bond `bond`, site dimension S, result
// bond chi: ms[0] the fused launch, ms[1] the gemm composition
void fit_sum_time_half(bool right, size_t K, size_t bond, size_t S, size_t chi, size_t reps, double ms[2]);

} // namespace t4a
