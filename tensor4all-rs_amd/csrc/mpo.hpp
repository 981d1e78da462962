// mpo.hpp — device-resident mirror of tensor4all-simplett's MPO<f64> and of the contraction of two MPOs
// (crates/tensor4all-simplett/src/mpo/: mpo.rs:35-480, contract_naive.rs:41-172, contract_zipup.rs:45-167,
//  canonical.rs:35-89, factorize.rs:126-313, contraction.rs:17-42, dispatch.rs:8-92).
// A site tensor is column-major [left, s1, s2, right], which is the [left, s1*s2, right] block of a tensor train over the
// fused site index s1 + S1*s2: an MPO is held as a TensorTrain over the fused index plus the (s1, s2) pair of every site, and
// evaluate / sum / the handle lifetime are those of tt.hip.
#pragma once

#include "tt.hpp"

namespace t4a {

enum class MpoFactorizeMethod : int { SVD = 0, RSVD = 1, LU = 2, CI = 3 }; // factorize.rs:12-20
enum class MpoAlgorithm : int { Naive = 0, ZipUp = 1, Fit = 2 };          // dispatch.rs:8-16

struct MpoContractionOptions { // ContractionOptions::default() (contraction.rs:17-42)
    double tolerance = 1e-12;
    size_t max_bond_dim = 0; // 0 == None
    MpoFactorizeMethod method = MpoFactorizeMethod::SVD;
};

// MPO::new (mpo.rs:35-60) on the host, before any device call: equal neighbouring bonds, first left and last right bond 1.
// This backend also refuses a zero dimension, a site of more than INT_MAX elements (the kernels index with int) and a
// dimension (fused s1*s2 included) above the tensor train's 65535.  Throws INVALID_ARGUMENT.
void mpo_validate_dims(const std::vector<std::array<size_t, 4>>& dims4);

class Mpo {
public:
    // dims4: (left, s1, s2, right) per site; host_data: the site tensors concatenated, each column-major
    Mpo(const std::vector<std::array<size_t, 4>>& dims4, const double* host_data);
    // copy of device cores (fused site index) with their (s1, s2) pairs
    Mpo(const std::vector<DevCore>& cores, hipStream_t src_stream, const std::vector<std::array<size_t, 2>>& site_dims);
    // adopt device cores whose producing stream has been synchronised (no copy)
    Mpo(std::vector<DevCore>&& cores, const std::vector<std::array<size_t, 2>>& site_dims);

    size_t len() const { return tt.len(); }
    std::vector<std::array<size_t, 4>> dims4() const;
    // evaluate (mpo.rs:245-340) for a batch: idx is 2 n_sites x n_pts column-major, [i1, j1, i2, j2, ...] per point
    std::vector<double> evaluate(const uint32_t* idx, size_t n_pts);
    double sum() { return tt.sum(); } // mpo.rs:341-392 (the empty MPO sums to 0)
    // s1 <-> s2 of every site (LinearOperator::transpose of the quantics operators): one axis permutation per site on this
    // MPO's stream
    std::unique_ptr<Mpo> transpose();
    // read the fused site index s1 + S1 * s2 of every site as another (s1, s2) pair of the same product; the cores stay
    void relabel_site_dims(const std::vector<std::array<size_t, 2>>& site_dims);

    TensorTrain tt;
    std::vector<std::array<size_t, 2>> sd; // (s1, s2) per site
};

// contract(a, b, algorithm, options) (dispatch.rs:67-92).  Naive with compress == false is contract_naive(a, b, None);
// Fit answers NOT_IMPLEMENTED after the shape checks, RSVD where the reference's factorize is reached.
std::unique_ptr<Mpo> mpo_contract(Mpo& a, Mpo& b, MpoAlgorithm alg, bool compress, const MpoContractionOptions& opt);
// The compress stage of contract_naive (compress_mpo, contract_naive.rs:100-172) on site tensors that exist already: right-canonicalise
// by QR, then the left-to-right SVD sweep with the rank rule of `opt`.  Every launch goes to the stream of `eng`, which the caller has
// made the owner of `cores`; ends synced.  The partitioned MPO (pmpo.hip) feeds it the output of its one product launch.
void mpo_compress_cores(Engine& eng, std::vector<DevCore>& cores, const MpoContractionOptions& opt);

// ---- variational (fit) contraction C ~ A·B.  This project's: the reference reserves FitOptions (contract_fit.rs:19-46) and answers
// Unsupported; mpo_contract(.., Fit, ..) keeps doing that.  The algorithm is the two-site fit of tensor4all-treetn (treetn/fit.rs)
// on a chain: C is an MPO with an orthogonality centre, the environments of A·B against C are cached, each bond step forms
// Theta = P_i Q_{i+1} from two half products (kernels_mpo_fit.hip), factorises it with the SVD rank rule of factorize and moves the
// centre.  One sweep is bonds 0 .. n-2 to the right, then n-2 .. 0 to the left; sweep k ends with norm_k = |S kept at its last step|,
// and the sweeps stop when |norm_k / norm_{k-1} - 1| < convergence_tol or k == max_sweeps (norm_0: the start, centred on site 0).
struct MpoFitOptions { // FitOptions::default()
    double tolerance = 1e-12;
    size_t max_bond_dim = 100; // 0 == None
    size_t max_sweeps = 10;
    double convergence_tol = 1e-10;
    MpoFactorizeMethod method = MpoFactorizeMethod::SVD;
};
struct MpoFitInfo {
    size_t n_sweeps = 0;
    std::vector<double> norms; // norm_0 .. norm_{n_sweeps}; empty when no sweep ran
};
// INVALID_ARGUMENT for a negative or non-finite tolerance / convergence_tol (host only)
void mpo_fit_validate_options(const MpoFitOptions& opt);
// The start is `initial` (same length and site dims (s1_a, s2_b), any bonds) or, for nullptr, the zip-up product with the same
// tolerance, cap and method.  max_sweeps == 0 returns the start as it is, one site the exact product, no site the empty MPO.
std::unique_ptr<Mpo> mpo_contract_fit(Mpo& a, Mpo& b, const MpoFitOptions& opt, Mpo* initial, MpoFitInfo& info);
// Test hook: the half product of one site exactly as the sweeps launch it.  right == false: env is L[n_env, la, lb] and the result
// P[n_env, s1, s2, ra, rb]; right == true: env is R[ra, rb, n_env] and the result Q[la, lb, s1, s2, n_env] (all column-major, host).
std::vector<double> mpo_fit_half(const double* env, size_t n_env, bool right, Mpo& a, Mpo& b, size_t site);

// ---- partial contraction of two MPOs: per leg contract, diagonal or keep (tensor4all-treetn/src/treetn/partial_contraction.rs,
// partial_contract with PartialContractionSpec, on a chain and by position).  A leg is (site, leg) with leg 0 or 1 of the site tensor
// [left, leg 0, leg 1, right].  A contract pair sums the two legs away; a diagonal pair identifies them and keeps A's ("the left-hand
// site index remains").  At a site the legs fall into three groups, each fused with its first leg fastest, an empty one of dimension 1:
//   S: the legs of A in no contract pair, in leg order;  K: the contract pairs, ordered by A's leg;  T: the legs of B in no pair,
//   C_i[(a, b), s, t, (a', b')] = sum_{kappa in K} A_i[a, x(s, kappa), a'] * B_i[b, y(s, kappa, t), b']
// with the bonds fused as the naive product fuses them; the result is an MPO with site dims (|S|, |T|).  The matrix product is
// {contract (i, 1)-(i, 0) for all i}, the Hadamard product of operators {diagonal (i, 0)-(i, 0), diagonal (i, 1)-(i, 1)}.
// Pairs across two sites and output_order are NOT_IMPLEMENTED (the reference moves indices with swap_site_indices; this project's,
// swap.hpp, is not wired in here yet); trees, mismatched topologies and complex scalars are outside this backend.
struct PartialPair {
    size_t site_a, leg_a, site_b, leg_b;
};
struct PartialSpec {
    std::vector<PartialPair> contract_pairs, diagonal_pairs;
    bool has_output_order = false;
};
struct PartialSitePlan {
    size_t S = 1, K = 1, T = 1;    // the fused groups
    size_t s0 = 1, k0 = 1, t0 = 1; // the dimension of the first leg of each group (the group's dimension below two legs)
    // offsets into the fused site index x0 + X0 x1 of A and y0 + Y0 y1 of B per step of the (first, second) leg of a group
    size_t as[2] = {0, 0}, ak[2] = {0, 0};
    size_t bs[2] = {0, 0}, bk[2] = {0, 0}, bt[2] = {0, 0};
    size_t leg_dims[4] = {0, 0, 0, 0}; // the dims of the legs of S (two slots), then of T (two slots); 0 = no such leg
};
// Host only.  a_sd / b_sd: (leg 0, leg 1) per site.  INVALID_ARGUMENT with the reference's messages (a leg out of range is "not found in
// first / second MPO external indices", then "index shape mismatch", then "appears in multiple pairs"; contract pairs before diagonal
// ones), lengths that differ, |S| * |T| above 65535; NOT_IMPLEMENTED for a pair across two sites and for output_order.
std::vector<PartialSitePlan> mpo_partial_plan(const std::vector<std::array<size_t, 2>>& a_sd, const std::vector<std::array<size_t, 2>>& b_sd,
                                              const PartialSpec& spec);
// Naive (one launch of the site product of kernels_partial.hip for the chain, then the compress stage of mpo_contract when `compress`)
// or ZipUp (the recursion of mpo_contract with the site step done by one launch of the half product of kernels_partial.hip, whose
// output is the matrix the SVD reads).  Fit and RSVD answer NOT_IMPLEMENTED as in mpo_contract.
std::unique_ptr<Mpo> mpo_partial_contract(Mpo& a, Mpo& b, const PartialSpec& spec, MpoAlgorithm alg, bool compress,
                                          const MpoContractionOptions& opt);
// mpo_contract_fit for a spec: same sweeps, environments and convergence rule, the half products taking the site plan.
std::unique_ptr<Mpo> mpo_partial_contract_fit(Mpo& a, Mpo& b, const PartialSpec& spec, const MpoFitOptions& opt, Mpo* initial, MpoFitInfo& info);
// Test hook, the counterpart of mpo_fit_half: env L[n_env, la, lb] -> P[n_env, s, t, ra, rb], or R[ra, rb, n_env] -> Q[la, lb, s, t, n_env].
std::vector<double> mpo_partial_half(const double* env, size_t n_env, bool right, Mpo& a, Mpo& b, const PartialSpec& spec, size_t site);

} // namespace t4a
