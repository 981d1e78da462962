// dmrg.hpp — two-site DMRG on the device: the lowest eigenpair of an MPO H over tensor trains, tensor4all-treetn's dmrg /
// dmrg_with_treetn_operator (crates/tensor4all-treetn/src/dmrg/mod.rs) on the Hermitian Lanczos of tensor4all-core
// (krylov.rs:517-634, helpers :2500-2675), restated for what square_linsolve covers: a chain, f64, one site index per node,
// V_in = V_out (every site of H has s1 == s2 == the state's site dimension; the dimensions may differ from site to site).  Trees,
// index mappings, complex scalars and nsite != 2 stay out.
//
// The projected operator, its cached environments, the half operators of a bond step, the sweep plan, the QR canonicalisation and
// the SVD split are those of linsolve.hpp; the local solver is Lanczos instead of GMRES.  One step at bond (i, i+1): theta_0 =
// x_i x_{i+1}, prepare(i), Lanczos from theta_0, tensor_svd of the unit-norm Ritz vector (no renormalisation after truncation),
// the singular values into the new centre, the environment of the side left behind from this step's half operator.
// Memory of a bond step: W (M^2 + N^2 + M N) + (max_iter + 2) M N doubles.
#pragma once

#include "linsolve.hpp"

namespace t4a {

// ---- hermitian_lanczos_lowest_eigenpair (krylov.rs:530-634)
struct LanczosOptions { // HermitianLanczosOptions::default()
    size_t max_iter = 64;
    double rtol = 1e-10, atol = 0.0, breakdown_tol = 1e-14, hermitian_tol = 1e-10;
    void validate() const; // INVALID_ARGUMENT (host only); max_iter <= LINSOLVE_RESTART_DIM_MAX
    double threshold(double eigenvalue) const;
};
struct LanczosResult {
    double eigenvalue = 0.0;
    size_t iterations = 0;
    double residual_norm = 0.0; // the true residual |H v - lambda v|
    bool converged = false;
    size_t apply_calls = 0;
};
class Lanczos {
public:
    explicit Lanczos(Engine& e) : eng_(e), ar_(e) {}
    void reserve(size_t len, size_t max_iter); // the basis: (max_iter + 1) len doubles
    // d_x: the start on entry, the unit-norm Ritz vector on exit.  The host reads one norm per solve, j + 2 doubles per step and three
    // per finalise.  INVALID_ARGUMENT: |start| <= breakdown_tol (ZeroInitialVector), a projected matrix that is not Hermitian.
    LanczosResult solve(const GmresApply& apply, size_t len, double* d_x, const LanczosOptions& o);
    // (|hv - lambda v|^2, <v, hv>, <v, v>) with hv = H v: one apply, eig_residual, the finishing launch, three doubles read
    void residual_sums(const GmresApply& apply, size_t len, const double* d_v, double lambda, double sums[3]);
    // Probe: device ms (events around `reps` launches behind a warm-up launch) of the three launches a finalise adds to its apply, with
    // nb basis vectors of length len: krylov_combine, eig_residual, krylov_finish (arguments checked by lanczos_time_finalise)
    void time_finalise(size_t len, size_t nb, size_t reps, double ms[3]);

private:
    Engine& eng_;
    HermitianArnoldi ar_;
    DevBuf<double> ax_;
};

// ---- DmrgOptions, DmrgResult of the reference
struct DmrgOptions {
    size_t nsite = 2;
    size_t nsweeps = 5;
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    bool has_svd_policy = false; // none: the default policy tensor_svd applies
    SvdPolicy svd_policy;
    LanczosOptions lanczos;
    bool has_energy_tol = false;
    double energy_tol = 0.0;
    double real_scalar_tol = 1e-10;
    void validate() const; // INVALID_ARGUMENT (host only)
};
struct DmrgStats {
    size_t local_solves = 0, lanczos_steps = 0, apply_calls = 0;
};
struct DmrgResult {
    std::unique_ptr<TensorTrain> state;
    double energy = 0.0;
    size_t sweeps_completed = 0, local_updates = 0;
    bool converged = false;
    double max_residual_norm = 0.0;
    DmrgStats stats;
};

// The shape checks on the host, before the device is touched (INVALID_ARGUMENT with a message): lengths differ, fewer than two sites
// (EmptyTwoSiteSweep), a site of the operator that is not square or does not match the state's site dimension, center >= n, and a
// bond step whose work buffers (HL, HR, T, the basis of max_iter + 1 columns) would hold more than INT_MAX elements.
void dmrg_validate_shapes(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center, size_t max_iter);

DmrgResult dmrg(Mpo& op, TensorTrain& init, size_t center, const DmrgOptions& options);
// <theta|H theta> / <theta|theta> at the region (center, center + 1), or (center - 1, center) when center == n - 1, of a copy of `state`
// canonicalised onto `center`, through the projected operator.  INVALID_ARGUMENT: a denominator <= real_scalar_tol (ZeroNormState).
double dmrg_energy(Mpo& op, TensorTrain& state, size_t center, double real_scalar_tol = 1e-10);

// Test hooks on host arrays.  lanczos_dense: the solver the sweeps run, on a dense n x n matrix (column-major) applied on the device.
LanczosResult lanczos_dense(const double* H, size_t n, const double* v0, const LanczosOptions& o, double* v_out);
void krylov_combine_host(const double* basis, size_t len, size_t nb, const double* coef, double* out, double* norm2);
void eig_residual_host(const double* v, const double* hv, size_t len, double lambda, double* r /* may be null */, double sums[3]);
// Probe hook: Lanczos::time_finalise on an engine of its own, behind the argument checks (INVALID_ARGUMENT) and require_device
void lanczos_time_finalise(size_t len, size_t nb, size_t reps, double ms[3]);

} // namespace t4a
