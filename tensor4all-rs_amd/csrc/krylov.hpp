// krylov.hpp — what the Krylov solvers of the MPO sweeps share (Gmres of linsolve.hpp, Lanczos of dmrg.hpp, KrylovExpm of tdvp.hpp): the
// launchers of the vector kernels, the two-pass orthogonalisation step (KrylovOrth), the Hermitian Arnoldi step of Lanczos and KrylovExpm
// (HermitianArnoldi), the cyclic Jacobi of the small projected matrix, and the helpers of the dense test hooks and the probes.
#pragma once

#include <functional>
#include <vector>

#include "tt_chain.hpp"

namespace t4a {

// ---- kernels_linsolve.hip.  All pointers are device pointers; launchers enqueue on `stream` and do not synchronise.
constexpr int GS_MAX_WORKGROUPS = 128;
// workgroups of every vector kernel below for a vector of `len` elements (a function of len alone: the fixed partition)
int gs_workgroups(size_t len);
// part[i + nb g] = <V[:, i], w> over the elements of workgroup g, i < nb; V is len x nb with leading dimension ld
void gs_dots_launch(const double* V, size_t ld, int nb, const double* w, size_t len, double* part, hipStream_t stream);
// c[i] = sum_g part[i + nb g], g < n_part ascending (n_part = gs_workgroups(len) behind gs_dots_launch; 1: part holds the coefficients);
// w -= sum_i c[i] V[:, i] (i ascending, every term rounded); npart[g] = the share of workgroup g in |w|^2.
// hcol (may be null): hcol[i] = c[i] when first_pass, else hcol[i] += c[i]; hpass (may be null): hpass[i] = c[i].
void gs_update_launch(const double* V, size_t ld, int nb, double* w, size_t len, const double* part, int n_part, double* hcol, bool first_pass,
                      double* hpass, double* npart, hipStream_t stream);
void gs_norm2_launch(const double* w, size_t len, double* npart, hipStream_t stream);
// nrm = sqrt(sum_g npart[g]); out = w * (1 / nrm) (out may be w, or null: the norm only); *norm_out = nrm (may be null)
void gs_normalize_launch(const double* w, size_t len, const double* npart, double* out, double* norm_out, hipStream_t stream);
// ---- kernels_tdvp.hip.  gs_dots with a second grid dimension over the basis vectors: workgroup (g, y) forms part[i + nb g] for the
// GS_WIDE vectors i = GS_WIDE y .. of element group g, with the element partition, the summation order and the reduction tree of
// gs_dots_launch: every part[i + nb g] has the same bits, and gs_update_launch runs unchanged behind it.
constexpr int GS_WIDE = 8;
void gs_dots_wide_launch(const double* V, size_t ld, int nb, const double* w, size_t len, double* part, hipStream_t stream);
// ---- kernels_dmrg.hip.  The partition is gs_workgroups(len).
// out = sum_i c[i] V[:, i] (i ascending from c[0] V[:, 0], every term rounded); npart[g] = the share of workgroup g in |out|^2.
// nb <= LINSOLVE_RESTART_DIM_MAX: the coefficients sit in LDS.  Lanczos::solve does not read npart: eig_residual runs behind the combine on
// the same buffer and supplies <v, v>; the reduction serves t4a_gpu_krylov_combine.  The launchers throw INVALID_ARGUMENT on an empty vector,
// nb <= 0 or nq outside 1 .. 64 instead of leaving an output untouched.
void krylov_combine_launch(const double* V, size_t ld, int nb, const double* c, double* out, size_t len, double* npart, hipStream_t stream);
// r = hv - lambda v (r may be null); part3[3 g + (0, 1, 2)] = the shares of workgroup g in |r|^2, <v, hv>, <v, v>
void eig_residual_launch(const double* v, const double* hv, double lambda, double* r, size_t len, double* part3, hipStream_t stream);
// out[q] = sum_g part[q + nq g], g < n_part ascending, q < nq <= 64
void krylov_finish_launch(const double* part, int n_part, int nq, double* out, hipStream_t stream);

// Which launch forms the projections of an orthogonalisation pass.  Serial: gs_dots_launch, what Gmres and Lanczos run.  Wide:
// gs_dots_wide_launch.  Auto: krylov_dots_route(len, nb) decides per pass (KrylovExpm of tdvp.hpp).
enum class KrylovDotsRoute : int { Serial = 0, Wide = 1, Auto = 2 };
// The rule of Auto, a function of the shape alone: Wide when the serial kernel would walk more than GS_WIDE vectors per workgroup.
KrylovDotsRoute krylov_dots_route(size_t len, int nb);

using GmresApply = std::function<void(const double* d_v, double* d_out)>; // enqueues out = H v on the engine's stream
// What the Krylov solvers launch around their apply: the two-pass orthogonalisation step, the norm read by the host, and the buffers of
// the partial sums.
class KrylovOrth {
public:
    explicit KrylovOrth(Engine& e) : eng_(e) {}
    void reserve(size_t nb_max); // at most nb_max basis vectors per pass
    void set_dots_route(KrylovDotsRoute r) { route_ = r; } // Serial unless a solver asks otherwise; the results have the same bits
    // One two-pass orthogonalisation step: w against the nb columns of V (leading dimension ld), then normalised in place.
    // d_hcol: nb + 1 doubles (the column of H, h_{nb} = the norm); d_hpass (may be null): 2 nb doubles, the coefficients of pass 1 and of pass 2.
    void orth(const double* d_V, size_t ld, int nb, double* d_w, size_t len, double* d_hcol, double* d_hpass);
    // host value of |w| (one read); out (may be null, may be w) receives w / |w|
    double norm(const double* d_w, size_t len, double* d_out = nullptr);
    double* npart() { return npart_.get(); }   // 3 GS_MAX_WORKGROUPS doubles: the shares of |w|^2, or the three sums of eig_residual
    double* scalars() { return scal_.get(); }  // 4 doubles: [0] the landing place of norm(), [1..3] free for the caller
    Engine& engine() { return eng_; }

private:
    void dots(const double* d_V, size_t ld, int nb, const double* d_w, size_t len);
    Engine& eng_;
    DevBuf<double> part_, npart_, scal_;
    KrylovDotsRoute route_ = KrylovDotsRoute::Serial;
};

// All eigenpairs of a symmetric n x n matrix (column-major, only read) by cyclic Jacobi on the host: a = evecs diag(evals) evecs^T,
// evecs column-major with orthonormal columns, in the order the diagonal is left in (not sorted).
void jacobi_eigh(const std::vector<double>& a, size_t n, std::vector<double>& evals, std::vector<double>& evecs);
// The lowest eigenpair of jacobi_eigh (the first of equal lowest diagonal entries) -> eigenvalue; vec: its column divided by its norm.
double jacobi_lowest_eigenpair(const std::vector<double>& a, size_t n, std::vector<double>& vec);

// The Arnoldi step Lanczos and KrylovExpm share: v_{j+1} from H v_j by KrylovOrth, the column of H read by the host (j + 2 doubles and
// one sync per step), the projected matrix rebuilt from the columns, checked against hermitian_tol and symmetrised.  The stopping rule
// and what is done with the basis stay with the solver.
class HermitianArnoldi {
public:
    explicit HermitianArnoldi(Engine& e) : eng_(e), gs_(e) {}
    void reserve(size_t len, size_t max_iter); // the basis: (max_iter + 1) len doubles
    double start(const double* d_x, size_t len); // v_0 = x / |x| -> |x|; the columns of an earlier start are dropped
    // -> beta = h_{j+1,j}; projected() is then the symmetrised (j + 1) x (j + 1) matrix.  INVALID_ARGUMENT "<who>: projected operator is not
    // Hermitian: ..".
    double step(const GmresApply& apply, size_t j, double hermitian_tol, const char* who);
    const std::vector<double>& projected() const { return a_; }
    double* basis() { return basis_.get(); }
    double* coef() { return coef_.get(); } // max_iter + 1 doubles for the coefficients of a combination
    KrylovOrth& orth() { return gs_; }

private:
    Engine& eng_;
    KrylovOrth gs_;
    DevBuf<double> basis_, hcol_, coef_;
    size_t len_ = 0;
    std::vector<std::vector<double>> hcols_;
    std::vector<double> a_;
};

// Probes: ms[k] = device ms per launch of pieces[k], k < n: HIP events around `reps` launches behind one warm-up launch.
void time_pieces(hipStream_t stream, const std::function<void()>* pieces, int n, size_t reps, double* ms);
// Dense test hooks: `count` host doubles in a fresh device buffer (one copy queued on `stream`), and y = H v for a dense n x n matrix
// (column-major, on the device) as the apply of a solver.
DevBuf<double> upload_vector(hipStream_t stream, const double* h, size_t count);
GmresApply dense_apply(const double* dH, size_t n, hipStream_t stream);

} // namespace t4a
