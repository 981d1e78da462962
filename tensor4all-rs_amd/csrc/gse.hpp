// gse.hpp — global subspace expansion (Yang & White) and GSE-TDVP on the device: tensor4all-treetn's global_subspace_expand,
// global_subspace_expand_with_references and gse_tdvp (crates/tensor4all-treetn/src/gse.rs:272-424, expand_edges :548-599,
// expand_one_edge :601-809, update_reference_edge :812-930, build_references :450-506; docs/design/gse-chain-mps-algorithm.md), restated
// for what tdvp covers: a chain, f64, one site index per node, V_in = V_out.  Trees, index mappings, complex scalars, the reference's AD
// preservation and a Julia-compatible absolute-tolerance mode stay out.
//
// The expansion widens every bond of psi by the directions of a few references that psi does not span yet, and does not change psi.
// The target and the references are canonicalised onto `center` (QrSweep), then the edges (child -> parent) are walked from the leaves
// to the centre: the left arm 0->1 .. c-1->c first, then the right arm n-1->n-2 .. c+1->c (the order of the arms changes the gauge
// only); before the first edge of an arm every train's centre is moved to that leaf by full-rank thin QR steps.  Per edge, with C the
// child core of the target as r x q (the bond to the parent as rows, q = site dimension times the far bond, which is 1 at a leaf and
// common to all trains after the previous edge):
//   1. old basis   B (k x q, k = min(r, q)): the right singular vectors of the thin SVD of C (Engine::svd);
//   2. project     N_j = R_j - (R_j B^T) B for the K reference children R_j (rho_j x q), stacked into one (sum rho_j) x q matrix, and
//                  the trace t = sum_j |R_j|_F^2 — one launch of kernels_gse.hip, ragged over j, reading the reference cores in place;
//   3. select      the thin SVD of the stack; the host reads its singular values and t (the only host read of the edge) and, if t > 0,
//                  keeps the right singular vectors with sigma^2 > density_weight_cutoff * t;
//   4. new child   B' = [B; kept rows], (k + m) x q.  t == 0 means m = 0, but B still replaces the child, as in the reference;
//   5. absorb      for the target and every reference tau: parent_tau <- parent_tau (C_tau B'^T) on the bond to the child — one launch,
//                  ragged over the K + 1 trains, both products chained; every child then becomes a copy of B'.
// The mirror orientation (child to the LEFT of its parent, the left arm) is the same kernels on the (l s) x r matricisation: every
// matrix above is held transposed.
//
// Deviations from the reference, none of which changes the expanded state beyond the gauge:
//   * Step 3 replaces the eigendecomposition of the Hermitianised P rho P / t (rho = sum_j R_j^T R_j, P = 1 - B^T B): the stack N has
//     N^T N = P rho P, so sigma^2 / t are the same eigenvalues and the right singular vectors span the same eigenspaces, without squaring
//     the condition number.  The kept rows are appended in descending order of sigma where the reference appends in its eigensolver's
//     order: a permutation of the gauge.  hermitian_tol is validated and has nothing else to check.
//   * The chained products of step 5 are associated as (parent_tau C_tau) B'^T, so that no workgroup waits for another one's G_tau.
//   * krylov_references applies the operator with this project's simplett zip-up, contract_zipup(op, MPO.from_tensor_train(cur)) with
//     max_bond_dim = reference_max_bond_dim, SVD factorisation and the tolerance of reference_svd_policy (1e-12 when unset), not with
//     treetn's apply_linear_operator.  The original state is not itself a reference.
//   * More than GSE_MAX_REFERENCES references are NOT_IMPLEMENTED (the ragged launches carry their operands as kernel arguments).
//
// Error wordings (INVALID_ARGUMENT unless said otherwise, all found on the host before the device is touched):
//   "invalid GSE option density_weight_cutoff: must be finite and non-negative", "invalid GSE option hermitian_tol: must be finite and
//   non-negative", "invalid GSE option reference_max_bond_dim: must be greater than zero when set", "GSE center <c> is not a state node",
//   "GSE requires target, references, and operator support to have the same tree topology" (lengths differ), "invalid GSE mapping at
//   node <i>: reference site dimension does not match target", "gse: more than 8 references are not implemented" (NOT_IMPLEMENTED);
//   gse_tdvp adds tdvp's own refusals unchanged (a real exponent, center in {0, n - 1}, nsite = 2); gse_tdvp_one_site adds those of
//   tdvp_one_site (nsite = 1, no max_bond_dim, no svd_policy; any centre).
#pragma once

#include "tdvp.hpp"

namespace t4a {

constexpr int GSE_MAX_REFERENCES = 8;
constexpr int GSE_MAX_JOBS = GSE_MAX_REFERENCES + 1; // the references and the target
constexpr int GSE_TILE = 16;                         // rows of a job per workgroup
constexpr int GSE_MFMA_MIN = 16;                     // the matrix cores from this bond up

// ---- kernels_gse.hip.  One workgroup forms a tile of GSE_TILE rows of the chained product of its job:
//   T = A_tile M1 (GSE_TILE x n1, kept in the job's scratch), O_tile = T M2, or A_tile - T M2 when `subtract`
// with A rows x k1, M1 k1 x n1, M2 n1 x n2, O rows x n2, every operand addressed by a row and a column stride (either orientation of a
// core is read in place).  mfma != 0: both products on v_mfma_f64_16x16x4_f64 (summed index in chunks of four, ascending, edges
// zero-padded); else one output element per thread, summed index ascending.  No floating-point atomics: the bits of a result depend on
// its operands and its shape alone.
struct GseJob {
    const double* A;
    long long ars, acs;
    int rows, k1;
    const double* M1;
    long long m1rs, m1cs;
    int n1;
    const double* M2;
    long long m2rs, m2cs;
    int n2;
    double* O;
    long long ors, ocs;
    double* T; // rows x n1 doubles, column-major
    int tile0; // the first workgroup of the job
    int mfma;
};
struct GseLaunch {
    GseJob job[GSE_MAX_JOBS];
    int n_jobs, n_tiles, subtract;
    // subtract only: the share of every workgroup in sum |A|^2, summed by the last workgroup to arrive in workgroup order
    double* trace_part;
    unsigned* ticket; // zero before the launch
    double* trace;
};
void gse_chain_launch(const GseLaunch& a, hipStream_t stream);

// The two steps on device operands.  orient 0: the bond to the parent is the FIRST leg of a child (the right arm): a matrix X over
// (bond row a, q index j) is column-major na x q, X[a + na j].  orient 1: the bond is the LAST leg (the left arm): X[j + q a].
// project: refs[j] rho[j] x q, B kb x q, stack (sum rho) x q (reference j at the rows off_j = rho_0 + .. + rho_{j-1}), *trace = t.
// scratch: (sum rho) kb doubles; trace_part: one double per workgroup (gse_tiles(rho, K)); ticket: one unsigned.
int gse_tiles(const int* rows, int n_jobs);
void gse_project_launch(int orient, int q, const double* const* refs, const int* rho, int K, const double* B, int kb, double* stack, double* scratch,
                        double* trace_part, unsigned* ticket, double* trace, hipStream_t stream);
// absorb: for train j, child[j] r[j] x q, parent[j] with its bond to the child (r[j]) as the last leg (orient 0: L[j] x r[j] column-major)
// or the first leg (orient 1: r[j] x L[j]); out[j] is the new parent with that bond kn: out_j = parent_j (child_j Bn^T), Bn kn x q.
// scratch: (sum L) q doubles (the GEMM composition: sum r kn).
void gse_absorb_launch(int orient, int q, const double* const* child, const int* r, const double* const* parent, const int* L, int n_trains,
                       const double* Bn, int kn, double* const* out, double* scratch, hipStream_t stream);
// The same results composed from gemm_launch (2 launches per job and the subtraction / no fusing): the route a shape takes when the
// probe finds the fused launch slower, and the yardstick of tools/probe_gse.py.
void gse_project_gemm(Engine& e, int orient, int q, const double* const* refs, const int* rho, int K, const double* B, int kb, double* stack, double* scratch,
                      double* trace_part, unsigned* ticket, double* trace);
void gse_absorb_gemm(Engine& e, int orient, int q, const double* const* child, const int* r, const double* const* parent, const int* L, int n_trains,
                     const double* Bn, int kn, double* const* out, double* scratch);
// Which route the driver takes at an edge with q columns and target bond `bond` — a function of the shape alone: the fused launches up to
// q * bond = GSE_FUSED_MAX_WORK, the GEMM composition above (DESIGN.md §8 has the measurements behind it).  gse_set_route forces one
// route for every edge (0 fused, 1 GEMM; anything else: back to the rule): a test hook, so that both routes of the driver run on small trains.
constexpr long long GSE_FUSED_MAX_WORK = 128 * 64;
bool gse_use_fused(int q, int bond);
void gse_set_route(int route);

// ---- options and results (GseOptions, GseResult, GseTdvpOptions, GseTdvpResult of the reference)
struct GseOptions {
    size_t krylov_dim = 0;
    bool has_reference_max_bond_dim = false; // none: max(link_dims(init)) + 1
    size_t reference_max_bond_dim = 0;
    bool has_reference_svd_policy = false; // none: threshold 1e-12
    SvdPolicy reference_svd_policy;
    double density_weight_cutoff = 1e-12, hermitian_tol = 1e-12;
    bool normalize_references = true, expand_before_first_sweep = true;
    void validate() const; // INVALID_ARGUMENT (host only)
};
struct GseResult {
    std::unique_ptr<TensorTrain> state;
    size_t references_built = 0, edges_processed = 0, bonds_expanded = 0, max_added_basis = 0;
};
struct GseTdvpOptions {
    GseOptions gse;
    TdvpOptions tdvp;
};
struct GseTdvpResult {
    std::unique_ptr<TensorTrain> state;
    size_t sweeps_completed = 0, local_updates = 0, gse_expansions = 0;
    double max_error_estimate = 0.0;
    size_t max_krylov_iterations = 0;
};

// The shape checks on the host (messages above): center, the number of references, their lengths and site dimensions.  refs: the dims3
// of every reference.  The bonds grow along the walk, so the INT_MAX bound of an edge's matrices is checked at the edge (INVALID_ARGUMENT
// "gse: .. of the edge at child i would hold more than INT_MAX elements", before that edge launches anything).
void gse_validate_shapes(const std::vector<std::array<size_t, 3>>& state, const std::vector<std::vector<std::array<size_t, 3>>>& refs, size_t center);

// build_references: H psi, H^2 psi, .. (krylov_dim of them), each the zip-up product capped at reference_max_bond_dim, divided by its
// norm when normalize_references is set and the norm is positive.
std::vector<std::unique_ptr<TensorTrain>> gse_krylov_references(Mpo& op, TensorTrain& init, const GseOptions& o);
GseResult global_subspace_expand_with_references(TensorTrain& init, const std::vector<TensorTrain*>& references, size_t center, const GseOptions& o);
GseResult global_subspace_expand(Mpo& op, TensorTrain& init, size_t center, const GseOptions& o);
// gse_tdvp (TwoSite) and gse_tdvp_one_site (OneSite): one loop, the one-sweep evolution after each expansion is the driver of `mode`,
// whose rules for o.tdvp and the shapes apply.  One-site: the expansion grows the bonds globally, the fixed-rank integrator evolves
// inside them; any centre, since both parts allow it.
GseTdvpResult gse_tdvp(TdvpMode mode, Mpo& op, TensorTrain& init, size_t center, const GseTdvpOptions& o);

// Test hooks on host arrays (column-major, layouts of gse_project_launch / gse_absorb_launch); route 0: the fused launch, 1: the GEMM
// composition.  project: refs concatenated, stack (sum rho) x q (orient 1: q x sum rho).  absorb: children, parents and results concatenated.
void gse_project_host(int orient, int q, const double* refs, const int* rho, int K, const double* B, int kb, int route, double* stack, double* trace);
void gse_absorb_host(int orient, int q, const double* children, const int* r, const double* parents, const int* L, int n_trains, const double* Bn, int kn,
                     int route, double* out);
// Probe: device ms (events around `reps` launches behind a warm-up launch) of project [0] fused [1] GEMMs, absorb [2] fused [3] GEMMs at
// bond chi, site dimension d (q = d chi, L = d chi), K references of bond chi + 1.
void gse_time_routes(size_t chi, size_t d, size_t K, size_t reps, double ms[4]);

} // namespace t4a
