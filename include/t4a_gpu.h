/*
 * t4a_gpu.h — C ABI of the MI355X (gfx950) backend for the tensor4all-rs TCI2 sweep hot path.
 *
 * This is the drop-in boundary.  The reference has NO existing FFI seam for this path
 * (tensor4all-capi deliberately excludes SimpleTT/TCI: crates/tensor4all-capi/src/lib.rs:13-14), so the
 * seam sits where the reference already crosses crates: the `Matrix<f64>`-level function surface of
 * tensor4all-core / tensor4all-tensorbackend and the `TensorCI2` driver of tensor4all-tensorci.  Each
 * entry point cites the Rust item it replaces.  Conventions are copied from tensor4all-capi:
 *   - status codes (crates/tensor4all-capi/src/lib.rs:49-68), thread-local last-error string fetched on
 *     the same OS thread (lib.rs:79-83, docs/CAPI_DESIGN.md:75-80);
 *   - opaque handles `*_new(..., out)` / `*_release` (docs/CAPI_DESIGN.md:24-52);
 *   - query-then-fill for variable-length outputs (docs/CAPI_DESIGN.md:108-123);
 *   - column-major dense buffers, `m[[r,c]] <-> data[r + nrows*c]`
 *     (crates/tensor4all-tensorbackend/src/matrix.rs:31-53);
 *   - no exception crosses the boundary (lib.rs:139-162).
 * All matrix pointers are HOST pointers unless a name ends in `_device`.  One in-flight call per
 * handle (the reference serialises backend calls behind one mutex, tensorbackend/src/context.rs:96).
 * Only f64 is in scope.
 */
#ifndef T4A_GPU_H
#define T4A_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- status codes: values 0..-7 identical to tensor4all-capi's t4a_status_code ---- */
typedef int32_t t4a_gpu_status;
#define T4A_GPU_SUCCESS 0
#define T4A_GPU_NULL_POINTER (-1)
#define T4A_GPU_INVALID_ARGUMENT (-2)
#define T4A_GPU_BUFFER_TOO_SMALL (-5)
#define T4A_GPU_INTERNAL_ERROR (-6)
#define T4A_GPU_NOT_IMPLEMENTED (-7)
/* extensions: MatrixCIError::{NaNEncountered, SingularMatrix} (core/src/matrixlu.rs:653-662,904,980) */
#define T4A_GPU_NAN_ENCOUNTERED (-8)
#define T4A_GPU_SINGULAR_MATRIX (-9)
/* no usable HIP device / HIP runtime failure: the product path never falls back to the CPU */
#define T4A_GPU_NO_DEVICE (-10)
/* a bounded in-kernel spin gave up (persistent rrLU hand-off) */
#define T4A_GPU_KERNEL_TIMEOUT (-11)
/* the user callback returned a wrong number of values (tensorci2.rs:1872-1874) */
#define T4A_GPU_CALLBACK_ERROR (-12)

/* Copies the calling thread's last error message (NUL terminated). `required_len` (may be NULL)
   receives the length including the terminator.  Mirrors t4a_last_error_message (capi/src/lib.rs:273). */
t4a_gpu_status t4a_gpu_last_error_message(char* buf, size_t buf_len, size_t* required_len);

/* Number of visible HIP devices (0 on a CPU-only host; never an error). */
t4a_gpu_status t4a_gpu_device_count(int32_t* out_count);
/* Select the device used by subsequent calls of this process (one process per GPU). */
t4a_gpu_status t4a_gpu_set_device(int32_t device);
/* Library version string. */
const char* t4a_gpu_version(void);
/* Always 0: the library has no experiment switches.  Kept so that existing binders keep linking. */
int32_t t4a_gpu_diag_switches_enabled(void);

/* The random stream of the reference's seeded searches: `rand 0.9` `StdRng::seed_from_u64(seed)` followed by
 * `rng.random_range(0..dims[i])` for i = 0 .. n-1 (tensorci2.rs:1653-1657 + globalpivot.rs:174-180,
 * adaptive_interpolation.rs:164,472-480, treetci/src/globalpivot.rs:118-122, aci/src/global_guard.rs:71-74).  Host-only (no device
 * needed): this is what every seeded search of this library draws its starting points from (csrc/stdrng.hpp). */
t4a_gpu_status t4a_gpu_stdrng_sample(uint64_t seed, const size_t* dims, size_t n, size_t* out /* n */);
/* One 64-byte ChaCha key-stream block (key: 8 little-endian words, 64-bit block counter, 64-bit stream id, `rounds` = 8 / 12 / 20):
 * the known-answer hook for the published vectors (RFC 8439 2.3.2; zero-key ChaCha20 / ChaCha12).  `StdRng` is the 12-round stream
 * with counter 0, stream 0. */
t4a_gpu_status t4a_gpu_chacha_block(const uint32_t* key8, uint64_t counter, uint64_t stream, int32_t rounds, uint32_t* out16);
/* The reference's two other seeded streams, restated from their published algorithms (csrc/smallrng.hpp), host only:
 *   - TreeTCI proposers (tensor4all-treetci/src/proposer.rs:344-409): std `DefaultHasher` = SipHash-1-3 with the zero key over
 *     (seed, tag, edge, history length, pivot counts) -> rand 0.9 `SmallRng::seed_from_u64` (xoshiro256++) -> `random_range` /
 *     `shuffle`;
 *   - ACI initial guess (tensor4all-aci/src/random_tt.rs:31,143-150): `ChaCha8Rng::seed_from_u64` + rand_distr `StandardNormal`.
 * These entry points exist for the known-answer tests (tests/test_cpu_stdrng.py: SipHash paper vector, CPython's zero-key SipHash-2-4,
 * the xoshiro256++ reference outputs, rand's seed_from_u64(0) vector, the ChaCha8 zero-key key stream). */
t4a_gpu_status t4a_gpu_siphash(const uint8_t* msg, size_t len, uint64_t k0, uint64_t k1, int32_t c_rounds, int32_t d_rounds, uint64_t* out);
/* state4 != NULL: the four state words given directly (published vectors); otherwise seed_from_u64(seed) */
t4a_gpu_status t4a_gpu_smallrng_words(uint64_t seed, const uint64_t* state4, size_t n, uint64_t* out /* n */);
t4a_gpu_status t4a_gpu_smallrng_sample(uint64_t seed, const size_t* dims, size_t n, size_t* out /* n */);
/* the permutation `(0..n).collect::<Vec<_>>().shuffle(&mut SmallRng::seed_from_u64(seed))` leaves behind */
t4a_gpu_status t4a_gpu_smallrng_shuffle(uint64_t seed, size_t n, size_t* out /* n */);
/* rng_for_edge's hash (proposer.rs:360-387): the u64 the proposer's SmallRng is seeded with */
t4a_gpu_status t4a_gpu_tree_edge_seed(uint64_t seed, const char* tag, size_t u, size_t v, size_t history_len, size_t n_pivots_i, size_t n_pivots_j,
                                      uint64_t* out);
/* n standard normals and / or n_words key-stream words of ChaCha8Rng::seed_from_u64(seed) (each from a fresh generator) */
t4a_gpu_status t4a_gpu_chacha8_standard_normal(uint64_t seed, size_t n, double* out, size_t n_words, uint32_t* out_words);


/* =====================================================================================
 * Dense kernels (host buffers in, host buffers out; each call is synchronous)
 * ===================================================================================== */

/* rrlu_mut(&mut Matrix<f64>, Option<RrLUOptions>) -> RrLU   (core/src/matrixlu.rs:735-819)
 * In-place full-pivot rank-revealing LU.  On return `a_inout` holds the factored matrix in the
 * physically permuted order of the reference's buffer (L below / U on+above the diagonal; read L,U
 * per extract_lu_from_factorized, matrixlu.rs:614-668).  `max_bond_dim == 0` means usize::MAX.
 * row_perm[m], col_perm[n]: RrLU::row_permutation / col_permutation.  Pivot selection is bit-exact.
 * Returns T4A_GPU_NAN_ENCOUNTERED exactly when the reference returns MatrixCIError::NaNEncountered. */
t4a_gpu_status t4a_gpu_rrlu_f64(double* a_inout, size_t m, size_t n, size_t max_bond_dim, double rel_tol,
                                double abs_tol, int32_t left_orthogonal, size_t* row_perm, size_t* col_perm,
                                size_t* npivots, double* last_error);

/* matrix_luci_factors_from_matrix(&Matrix<f64>, Option<RrLUOptions>) -> MatrixLuciFactors
 * (core/src/matrix_luci.rs:366-374; factors :256-279).
 * Caller-owned buffers sized for rank = min(m,n): rows/cols [min(m,n)], pivot_errors [min(m,n)+1],
 * left [m*min(m,n)], right [min(m,n)*n].  On return left is m x rank and right is rank x n, both
 * column-major and densely packed for the returned rank. */
t4a_gpu_status t4a_gpu_luci_f64(const double* a, size_t m, size_t n, size_t max_bond_dim, double rel_tol,
                                double abs_tol, int32_t left_orthogonal, size_t* rank, size_t* rows, size_t* cols,
                                double* pivot_errors, double* left, double* right);

/* matrix_luci_factors_from_blocks(nrows, ncols, fill_block, RrLUOptions) (core/src/matrix_luci.rs:440-456): the lazy
 * block-rook kernel behind PivotSearchStrategy::Rook (matrixluci/block_rook.rs:71-190, factors.rs:43-113).
 * fill_block(ctx, rows, nrows, cols, ncols, out) must write out[i + nrows*j] = A[rows[i], cols[j]]
 * (matrixluci/source.rs:15-24); this backend only ever asks for one full column or one full row per call and
 * never for the whole matrix.  Output buffers as for t4a_gpu_luci_f64. */
typedef void (*t4a_gpu_fill_block_fn)(void* ctx, const size_t* rows, size_t nrows, const size_t* cols, size_t ncols,
                                      double* out);
t4a_gpu_status t4a_gpu_luci_blocks_f64(size_t m, size_t n, t4a_gpu_fill_block_fn fill_block, void* ctx,
                                       size_t max_bond_dim, double rel_tol, double abs_tol, int32_t left_orthogonal,
                                       size_t* rank, size_t* rows, size_t* cols, double* pivot_errors, double* left,
                                       double* right);
/* Same kernel on a dense column-major matrix that is already in memory (LazyBlockRookKernel on a dense source,
 * matrixluci/block_rook/tests.rs:36-52). */
t4a_gpu_status t4a_gpu_luci_rook_f64(const double* a, size_t m, size_t n, size_t max_bond_dim, double rel_tol,
                                     double abs_tol, int32_t left_orthogonal, size_t* rank, size_t* rows, size_t* cols,
                                     double* pivot_errors, double* left, double* right);

/* mat_mul(&a,&b) (tensorbackend/src/matrix.rs:1488): c[m x n] = a[m x k] * b[k x n] */
t4a_gpu_status t4a_gpu_gemm_f64(const double* a, const double* b, size_t m, size_t k, size_t n, double* c);

/* batched_mat_mul_same_shape(batch,m,k,n,&a,&b) (matrix.rs:1538-1612): operands are column-major
 * [m,k,batch] and [k,n,batch] (batch slowest), result [m,n,batch]. */
t4a_gpu_status t4a_gpu_gemm_batched_f64(size_t batch, size_t m, size_t k, size_t n, const double* a,
                                        const double* b, double* c);

/* The route the GEMM launcher takes for `batch` products of shape m x n x k (host only; m, n, batch positive, k may be 0, all within
 * int): *bn = 32 (narrow 64 x 32 block tiles) or 64 (wide 64 x 64), *ksplit = slices of a split-K product (1: none), the grid of
 * *grid_m x *grid_n tiles per problem and slice, *remapped = 1 when (grid_m * grid_n) % 8 == 0: the XCD-aware tile order.  The launcher
 * launches what this reports. */
t4a_gpu_status t4a_gpu_gemm_route(size_t m, size_t n, size_t k, size_t batch, int32_t* bn, int32_t* ksplit, int32_t* grid_m,
                                  int32_t* grid_n, int32_t* remapped);
/* Test hook: the GEMM exactly as every layer launches it, one whole descriptor per product on flat host buffers.  Product p is
 *   C_j = alpha op(A_j) op(B_j) + beta C_j,  j < batch,   op(A) m x k, op(B) k x n, C m x n, all column-major,
 * with A_j at a[off_a + j stride_a] (stored m x k with leading dimension lda, or k x m when trans_a != 0), B_j at
 * b[off_b + j stride_b] likewise and C_j at c[off_c + j stride_c] (ldc); strides and offsets count elements, stride_a / stride_b may
 * be 0 (one operand shared by the batch).  a (na elements), b (nb) and c (nc) are uploaded, the n_descs products are queued in order
 * on one stream with no synchronisation between them, and c is downloaded after one synchronisation.  beta == 0: C is not read.
 * k == 0 goes to the kernel as it stands (C = beta C).  Refused with INVALID_ARGUMENT before the device is touched: a negative size or
 * one beyond int (m, n, k: beyond INT_MAX - 63), trans_a / trans_b other than 0 or 1, a leading dimension below the rows of the stored operand (or below 1), an
 * operand or result that runs past its buffer, results of two problems of one product that overlap (stride_c = 0 with batch > 1
 * included), more problems times split-K slices than the 65535 a launch takes.  No product code calls this. */
typedef struct t4a_gpu_gemm_desc {
    int64_t m, n, k;
    int64_t lda, ldb, ldc;
    int32_t trans_a, trans_b;
    double alpha, beta;
    int64_t batch;
    int64_t stride_a, stride_b, stride_c;
    int64_t off_a, off_b, off_c;
} t4a_gpu_gemm_desc;
t4a_gpu_status t4a_gpu_gemm_desc_f64(const t4a_gpu_gemm_desc* descs, size_t n_descs, const double* a, size_t na, const double* b,
                                     size_t nb, double* c, size_t nc);

/* triangular_solve_matrix(A,B,left_side,lower,transpose_a,unit_diagonal) (tensorbackend/src/backend.rs:924):
 * solves op(A) X = B (left_side) or X op(A) = B.  A is na x na, B and X are bm x bn. */
t4a_gpu_status t4a_gpu_trsm_f64(const double* a, size_t na, const double* b, size_t bm, size_t bn,
                                int32_t left_side, int32_t lower, int32_t transpose_a, int32_t unit_diagonal,
                                double* x);

/* solve_matrix(&A,&B) (backend.rs:865): A n x n, B n x nrhs, X n x nrhs.  Partial-pivot LU.
 * Returns T4A_GPU_SINGULAR_MATRIX for an exactly singular A. */
t4a_gpu_status t4a_gpu_solve_f64(const double* a, size_t n, const double* b, size_t nrhs, double* x);

/* svd_backend(&a) (tensorbackend/src/backend.rs:709-731): thin SVD, k = min(m,n); u is m x k, s has k entries in
 * non-increasing order, vt is k x n ("backend convention", simplett/src/compression.rs:254-287).  One-sided Jacobi
 * (from 64 columns on: on the transposed triangular factor of a Householder QR); a column pair rotates while the cosine of its
 * angle exceeds sqrt(rows) * eps (LAPACK dgesvj's rule): reconstruction and singular values to ~1e-14 relative to the largest.
 * Returns T4A_GPU_INVALID_ARGUMENT for an empty or non-finite matrix. */
t4a_gpu_status t4a_gpu_svd_f64(const double* a, size_t m, size_t n, double* u, double* s, double* vt);

/* qr_backend(&a) (backend.rs:742-760): thin QR, q is m x k, r is k x n upper trapezoidal.  Householder. */
t4a_gpu_status t4a_gpu_qr_f64(const double* a, size_t m, size_t n, double* q, double* r);

/* Randomized rank-k SVD (north_star: "one-sided Jacobi / randomized SVD"; Halko, Martinsson, Tropp 2011, algorithms 4.4 + 5.1 — the
 * reference itself only has the dense svd_backend above, so this is an ADDITION for truncated factorisations, not a replacement):
 * Y = A Omega with Omega n x (k + oversample) standard normal (drawn from the library's StdRng stream seeded with `seed`), power_iters
 * rounds of Y <- A (A^T Q(Y)) with a QR in between, Q = qr(Y), B = Q^T A, thin SVD of the small B by the one-sided Jacobi, U = Q U_B.
 * Everything between the upload of A and the download of the factors runs on the device (f64-MFMA GEMMs, Householder QR, Jacobi).
 * u is m x k, s has k entries (non-increasing), vt is k x n.  For a matrix of rank <= k the result is the thin SVD to rounding; for a
 * decaying spectrum the error is bounded by the usual (1 + 9 sqrt(k + p) sqrt(min(m, n))) sigma_{k+1} of the randomized range finder.
 * INVALID_ARGUMENT for k == 0, k + oversample > min(m, n) is clamped to min(m, n). */
t4a_gpu_status t4a_gpu_rsvd_f64(const double* a, size_t m, size_t n, size_t k, size_t oversample, size_t power_iters, uint64_t seed,
                                double* u, double* s, double* vt);

/* full_piv_lu_matrix(&a) (backend.rs:1022-1037) for a square n x n matrix: P A Q^T = L U with n x n factors;
 * row k of P (Q) carries its 1 in the column of the k-th pivot row (column), which is how
 * core/src/matrixluci/dense.rs:120-139 reads them.  Elimination order = rrlu_mut with zero tolerances. */
t4a_gpu_status t4a_gpu_full_piv_lu_f64(const double* a, size_t n, double* p, double* l, double* u, double* q);

/* =====================================================================================
 * TCI2 sweep driver (opaque handle; state resident on the device between calls)
 * ===================================================================================== */
typedef struct t4a_gpu_tci2 t4a_gpu_tci2;

/* TCI2Options (tensorci/src/tensorci2.rs:73-170).  max_bond_dim == 0 <=> None. */
typedef struct t4a_gpu_tci2_options {
    double tolerance;                 /* 1e-8 */
    size_t max_iter;                  /* 20 */
    size_t max_bond_dim;              /* 0 = None */
    int32_t pivot_search;             /* 0 = Full, 1 = Rook (lazy block-rook search, tensorci2.rs:286-296) */
    int32_t normalize_error;          /* 1 */
    size_t verbosity;                 /* 0 */
    size_t max_nglobal_pivot;         /* 5 */
    size_t nsearch;                   /* 5 */
    int32_t sweep_strategy;           /* 0 Forward, 1 Backward, 2 BackAndForth (default) */
    int32_t strictly_nested;          /* 0 */
    size_t ncheck_history;            /* 3 */
    double tol_margin_global_search;  /* 10.0 */
    int32_t has_seed;                 /* 0 = None */
    int32_t reserved_;
    uint64_t seed;
} t4a_gpu_tci2_options;

/* Fills `opts` with TCI2Options::default() (tensorci2.rs:152-170). */
t4a_gpu_status t4a_gpu_tci2_options_default(t4a_gpu_tci2_options* opts);

/* TCI2Termination (tensorci2.rs:197-205) */
#define T4A_GPU_TCI2_CONVERGED 0
#define T4A_GPU_TCI2_MAX_BOND_DIMENSION 1
#define T4A_GPU_TCI2_MAX_ITERATIONS 2

/* TensorCI2::new(local_dims) (tensorci2.rs:380-404) */
t4a_gpu_status t4a_gpu_tci2_new(const size_t* local_dims, size_t n_sites, t4a_gpu_tci2** out);
void t4a_gpu_tci2_release(t4a_gpu_tci2* h);

/* The user function `f` of crossinterpolate2 (tensorci2.rs:1513-1524), given either as
 *  (a) a built-in device functor: function id + parameters + integer weight table
 *      (include/t4a_testfunctions.h; weights has n_acc * sum(local_dims) entries), evaluated on the GPU; or
 *  (b) a host batch callback, the `batched_f` contract of the reference: one value per requested index.
 *      idx is n_sites x n_pts column-major (same shape as treetci's GlobalIndexBatch,
 *      treetci/src/update.rs:213-232); returns the number of values written (must equal n_pts),
 *      or a negative value to abort. */
t4a_gpu_status t4a_gpu_tci2_set_builtin_function(t4a_gpu_tci2* h, int32_t fid, int32_t n_acc,
                                                 const double* params /* [T4A_FN_MAX_PARAMS] */,
                                                 const uint64_t* weights);
typedef int64_t (*t4a_gpu_batch_eval_fn)(void* ctx, const uint32_t* idx, size_t n_sites, size_t n_pts, double* out);
t4a_gpu_status t4a_gpu_tci2_set_callback(t4a_gpu_tci2* h, t4a_gpu_batch_eval_fn cb, void* ctx);

/* TensorCI2::add_global_pivots (tensorci2.rs:668-711). pivots: n_sites x n_pivots column-major. */
t4a_gpu_status t4a_gpu_tci2_add_global_pivots(t4a_gpu_tci2* h, const size_t* pivots, size_t n_pivots);

/* crossinterpolate2(f, batched_f, local_dims, initial_pivots, options) (tensorci2.rs:1513-1563) on a fresh
 * handle: add initial pivots (n_pivots == 0 -> the all-zeros index), initialise max_sample_value, run
 * optimize_with_finder (tensorci2.rs:1626-1802) including the final sweep1site. */
t4a_gpu_status t4a_gpu_tci2_crossinterpolate2(t4a_gpu_tci2* h, const size_t* initial_pivots, size_t n_pivots,
                                              const t4a_gpu_tci2_options* options);

/* optimize_with_finder on the current state (tensorci2.rs:1626).  `final_sweep1site == 0` skips the final
 * cleanup sweep (tensorci2.rs:1787) so that callers (bench) can time individual half-sweeps. */
t4a_gpu_status t4a_gpu_tci2_optimize(t4a_gpu_tci2* h, const t4a_gpu_tci2_options* options, int32_t final_sweep1site);

/* TensorCI2::sweep2site(&f,&batched_f,forward,&options) (tensorci2.rs:746-798) */
t4a_gpu_status t4a_gpu_tci2_sweep2site(t4a_gpu_tci2* h, int32_t forward, const t4a_gpu_tci2_options* options);
/* TensorCI2::sweep1site(&f,forward,rel_tol,abs_tol,max_bond_dim,update_tensors) (tensorci2.rs:865-915) */
t4a_gpu_status t4a_gpu_tci2_sweep1site(t4a_gpu_tci2* h, int32_t forward, double rel_tol, double abs_tol,
                                       size_t max_bond_dim /* 0 = usize::MAX */, int32_t update_tensors);
/* TensorCI2::fill_site_tensors(&f) (tensorci2.rs:1065-1186) */
t4a_gpu_status t4a_gpu_tci2_fill_site_tensors(t4a_gpu_tci2* h);
/* TensorCI2::make_canonical (tensorci2.rs:1201-1221) */
t4a_gpu_status t4a_gpu_tci2_make_canonical(t4a_gpu_tci2* h, double rel_tol, double abs_tol, size_t max_bond_dim);

/* accessors (tensorci2.rs:585-649, 713-721) */
t4a_gpu_status t4a_gpu_tci2_len(const t4a_gpu_tci2* h, size_t* out);
t4a_gpu_status t4a_gpu_tci2_rank(const t4a_gpu_tci2* h, size_t* out);
t4a_gpu_status t4a_gpu_tci2_link_dims(const t4a_gpu_tci2* h, size_t* out /* n_sites-1 */);
t4a_gpu_status t4a_gpu_tci2_max_sample_value(const t4a_gpu_tci2* h, double* out);
t4a_gpu_status t4a_gpu_tci2_max_bond_error(const t4a_gpu_tci2* h, double* out);
t4a_gpu_status t4a_gpu_tci2_bond_errors(const t4a_gpu_tci2* h, double* out /* n_sites-1 */);
/* query-then-fill: out == NULL returns the count only */
t4a_gpu_status t4a_gpu_tci2_pivot_errors(const t4a_gpu_tci2* h, size_t* count, double* out);
/* which: 0 = i_set(site), 1 = j_set(site); entries are `width` digits each, returned as
 * width x count column-major (one multi-index per column). out == NULL queries count/width. */
t4a_gpu_status t4a_gpu_tci2_index_set(const t4a_gpu_tci2* h, int32_t which, size_t site, size_t* count,
                                      size_t* width, size_t* out);
/* TensorCI2::from_index_sets resume format (tensorci2.rs:551-582): overwrite one I/J set. */
t4a_gpu_status t4a_gpu_tci2_set_index_set(t4a_gpu_tci2* h, int32_t which, size_t site, size_t count,
                                          const size_t* data);
t4a_gpu_status t4a_gpu_tci2_set_max_sample_value(t4a_gpu_tci2* h, double value);
t4a_gpu_status t4a_gpu_tci2_clear_history(t4a_gpu_tci2* h);
/* site_tensor(p): dims3 = (left, site, right); column-major [left, site, right] like simplett Tensor3
 * (simplett/src/tensor.rs:13-18). out == NULL queries the dims only. */
t4a_gpu_status t4a_gpu_tci2_site_tensor(const t4a_gpu_tci2* h, size_t site, size_t* dims3, double* out);
/* Same tensor copied device-to-device into caller-provided device memory (used for the RCCL all-gather
 * of cores; `out_device` must hold left*site*right doubles). */
t4a_gpu_status t4a_gpu_tci2_site_tensor_device(const t4a_gpu_tci2* h, size_t site, void* out_device);
/* Overwrite a site tensor from device memory (receiving side of the core all-gather). */
t4a_gpu_status t4a_gpu_tci2_set_site_tensor_device(t4a_gpu_tci2* h, size_t site, const size_t* dims3,
                                                   const void* in_device);

/* results of the last optimize / crossinterpolate2 call (TCI2OptimizationResult, tensorci2.rs:236-245) */
t4a_gpu_status t4a_gpu_tci2_n_iterations(const t4a_gpu_tci2* h, size_t* out);
t4a_gpu_status t4a_gpu_tci2_history(const t4a_gpu_tci2* h, size_t* ranks, double* errors);
t4a_gpu_status t4a_gpu_tci2_termination(const t4a_gpu_tci2* h, int32_t* out);

/* to_tensor_train().evaluate(idx) for a batch of points (simplett/src/traits.rs:146-212), evaluated on
 * the device.  idx: n_sites x n_pts column-major. */
t4a_gpu_status t4a_gpu_tci2_evaluate(t4a_gpu_tci2* h, const size_t* idx, size_t n_pts, double* out);
/* to_tensor_train().sum() (traits.rs:231-275) */
t4a_gpu_status t4a_gpu_tci2_sum(t4a_gpu_tci2* h, double* out);

/* Restrict fill_site_tensors to the sites s with s % world == rank (site-sharded multi-GPU mode,
 * SURVEY.md §8e).  world == 1 restores the default.  Cores of foreign sites are left untouched and are
 * expected to arrive through t4a_gpu_tci2_set_site_tensor_device. */
t4a_gpu_status t4a_gpu_tci2_set_site_shard(t4a_gpu_tci2* h, size_t rank, size_t world);

/* Column-block shard of the candidate matrix for HOST-CALLBACK functions (entries of one candidate matrix are
 * independent, tensorci2.rs:1859-1893).  After set_pi_shard(rank, world, gather, ctx) every matrix this handle evaluates through its
 * batch callback (update_pivots, sweep1site, fill_site_tensors) is split into `world` blocks of ceil(N / world) columns: this rank's
 * callback sees only the points of its block (row index outer, column index inner: the order of tensorci2.rs:1862-1869 restricted to
 * the block), `gather` — an all-gather over the process group on HOST buffers: `count` doubles in from every rank, world * count out,
 * rank-major; 0 = success — assembles the whole matrix on every rank, and the rank-revealing LU runs replicated (deterministic: the same
 * pivots everywhere, nothing is broadcast).  Every rank must drive its handle through the same calls.  world == 1 switches it off. */
typedef int32_t (*t4a_gpu_allgather_fn)(void* ctx, const double* send, size_t count, double* recv);
t4a_gpu_status t4a_gpu_tci2_set_pi_shard(t4a_gpu_tci2* h, size_t rank, size_t world, t4a_gpu_allgather_fn gather, void* ctx);
/* [n_gathers, bytes_sent_by_this_rank] since the shard was set. */
t4a_gpu_status t4a_gpu_tci2_pi_shard_stats(t4a_gpu_tci2* h, size_t* out2);
/* The host part of the shard alone (no device, no handle): evaluates the na x nb matrix of the row halves `a` (na x wa digits, placed at
 * site a0) and the column halves `b` (nb x wb digits at site b0; wa + wb = n_sites) through `cb` + `gather` exactly as a sharded handle
 * does; out: na x nb row-major.  world == 1: one plain callback over all points.  (CPU-only test hook, tests/test_cpu_parallel.py.) */
t4a_gpu_status t4a_gpu_pi_shard_eval(size_t rank, size_t world, t4a_gpu_batch_eval_fn cb, void* cb_ctx, t4a_gpu_allgather_fn gather,
                                     void* gather_ctx, size_t n_sites, const uint32_t* a, size_t wa, size_t a0, size_t na,
                                     const uint32_t* b, size_t wb, size_t b0, size_t nb, double* out);

/* add_global_pivots invalidates the site tensors even when the pivot list is empty (tensorci2.rs:707-708), so
 * after optimize_with_finder without a final sweep1site the cores of the last fill_site_tensors are gone.  With
 * keep != 0 an EMPTY pivot list leaves them in place (the index sets did not change, so they are still the cores
 * of the current sets).  Default 0 = reference behaviour. */
t4a_gpu_status t4a_gpu_tci2_set_keep_site_tensors(t4a_gpu_tci2* h, int32_t keep);

/* Multi-GPU core gather without a host stall: copies every site tensor to dst_device + site * stride (stride in
 * doubles, >= the largest site tensor) on the stream of the fill_site_tensors that may still be in flight, and makes
 * `consumer_stream` (a hipStream_t, e.g. the stream an RCCL all-gather is issued from) wait for the copies.  With
 * keep != 0 (above) optimize() leaves its last fill_site_tensors in flight, so the next sweep's bond updates overlap
 * with it; errors of that fill are reported by the next call that reads a site tensor. */
t4a_gpu_status t4a_gpu_tci2_export_site_tensors_async(t4a_gpu_tci2* h, void* dst_device, size_t stride,
                                                      void* consumer_stream);
/* Site-sharded fill_site_tensors (BASELINE.json configs[3]; tensorci2.rs:1065-1186: sites are independent given the I/J
 * sets) without host staging.  After t4a_gpu_tci2_set_site_shard(rank, world):
 *   export: the local sites s = rank + world * k go to dst_device + k * stride (doubles), ordered after the fill that may
 *           still be in flight; `consumer_stream` (the stream the RCCL all-gather is issued from) waits for the copies;
 *   import: the gathered buffer is [world][per_rank][stride]; every remote site is copied into this handle (shapes follow
 *           from the replicated index sets) on the handle's stream, after what `producer_stream` has enqueued so far. */
t4a_gpu_status t4a_gpu_tci2_export_site_shard_async(t4a_gpu_tci2* h, void* dst_device, size_t stride, void* consumer_stream);
t4a_gpu_status t4a_gpu_tci2_import_site_shard_async(t4a_gpu_tci2* h, const void* src_device, size_t stride, size_t per_rank,
                                                    void* producer_stream);

/* =====================================================================================
 * SimpleTensorTrain<f64> (opaque handle; site tensors resident on the device)
 * tensor4all-simplett: tensortrain.rs:97, traits.rs:75-355, compression.rs:375-507, cache.rs:558-744
 * ===================================================================================== */
typedef struct t4a_gpu_tt t4a_gpu_tt;

/* SimpleTensorTrain::new(tensors) (tensortrain.rs:97-124).  dims3 is 3 x n_sites (left, site, right per site),
 * cores the site tensors concatenated, each column-major [left, site, right].  Same validation as the reference:
 * first left == 1, last right == 1, neighbouring bonds equal. */
t4a_gpu_status t4a_gpu_tt_new(const size_t* dims3, size_t n_sites, const double* cores, t4a_gpu_tt** out);
void t4a_gpu_tt_release(t4a_gpu_tt* h);
t4a_gpu_status t4a_gpu_tt_clone(const t4a_gpu_tt* h, t4a_gpu_tt** out);
t4a_gpu_status t4a_gpu_tt_len(const t4a_gpu_tt* h, size_t* out);
t4a_gpu_status t4a_gpu_tt_dims(const t4a_gpu_tt* h, size_t* dims3 /* 3 x n_sites */);
t4a_gpu_status t4a_gpu_tt_site_tensor(const t4a_gpu_tt* h, size_t site, double* out);
/* AbstractTensorTrain::evaluate (traits.rs:146-212) for a batch: idx is n_sites x n_pts column-major. */
t4a_gpu_status t4a_gpu_tt_evaluate(t4a_gpu_tt* h, const size_t* idx, size_t n_pts, double* out);
/* sum (traits.rs:231-275), norm2 = <tt|tt> (traits.rs:289-354) */
t4a_gpu_status t4a_gpu_tt_sum(t4a_gpu_tt* h, double* out);
t4a_gpu_status t4a_gpu_tt_norm2(t4a_gpu_tt* h, double* out);
/* SimpleTensorTrain::compress(&CompressionOptions) (compression.rs:375-507).
 * method: 0 LU, 1 CI, 2 SVD (compression.rs:40-52); max_bond_dim == 0 <=> None. */
#define T4A_GPU_COMPRESS_LU 0
#define T4A_GPU_COMPRESS_CI 1
#define T4A_GPU_COMPRESS_SVD 2
t4a_gpu_status t4a_gpu_tt_compress(t4a_gpu_tt* h, int32_t method, double tolerance, size_t max_bond_dim,
                                   int32_t normalize_error);
/* TTCache::evaluate_many(indices, split) (cache.rs:558-688): split == 0 <=> None (find_split_heuristic,
 * cache.rs:690-744); *used_split (may be NULL) reports the split position that was used. */
t4a_gpu_status t4a_gpu_tt_evaluate_many(t4a_gpu_tt* h, const size_t* idx, size_t n_pts, size_t split, double* out,
                                        size_t* used_split);

/* floating_zone(tt, f, local_dims, init_p, early_stop_tol) (tensorci/src/globalsearch.rs:163-243, walk:
 * tensor4all-core/src/floating_zone.rs:46-103): local search for the multi-index with the largest |f - tt|.  The tensor
 * train is evaluated on the device (TTCache::evaluate_many per site scan), f is the batch callback.  init_p == NULL: random
 * starting point (reference: thread rng of rand 0.9, "parity unpinned"; here splitmix64(seed)). */
t4a_gpu_status t4a_gpu_tt_floating_zone(t4a_gpu_tt* tt, t4a_gpu_batch_eval_fn f, void* ctx, const size_t* local_dims, size_t n_sites,
                                        const size_t* init_p, uint64_t seed, double early_stop_tol, size_t* pivot_out /* n_sites */,
                                        double* error_out);
/* estimate_true_error(tt, f, nsearch, initial_points, rng) (globalsearch.rs:70-118): floating_zone from every starting point,
 * results sorted by descending error, consecutive duplicates removed.  initial_points: n_sites x n_initial column-major or
 * NULL (then nsearch random points from StdRng::seed_from_u64(seed), csrc/stdrng.hpp).  Query-then-fill: *n_out is always set; BUFFER_TOO_SMALL when
 * capacity < *n_out (at most nsearch resp. n_initial results). */
t4a_gpu_status t4a_gpu_tt_estimate_true_error(t4a_gpu_tt* tt, t4a_gpu_batch_eval_fn f, void* ctx, size_t nsearch, const size_t* initial_points,
                                              size_t n_initial, uint64_t seed, size_t* pivots_out /* n_sites x capacity */,
                                              double* errors_out /* capacity */, size_t capacity, size_t* n_out);
/* opt_first_pivot(f, local_dims, first_pivot, max_sweep) (tensorci/src/optfirstpivot.rs:40-74): greedy coordinate search for
 * a large |f|; host logic over the batch callback (one batch per site scan), no device work. */
t4a_gpu_status t4a_gpu_opt_first_pivot(t4a_gpu_batch_eval_fn f, void* ctx, const size_t* local_dims, size_t n_sites, const size_t* first_pivot,
                                       size_t max_sweep, size_t* pivot_out /* n_sites */);

/* TensorCI2::to_tensor_train (tensorci2.rs:640-660): a device-to-device copy of the current site tensors. */
t4a_gpu_status t4a_gpu_tci2_to_tensor_train(t4a_gpu_tci2* h, t4a_gpu_tt** out);
/* TensorCI2::from_tensor_train(tt, TensorCI2FromTensorTrainOptions{tolerance, max_bond_dim, max_iter})
 * (tensorci/src/conversion.rs:66-121).  max_bond_dim == 0 <=> None; defaults 1e-12 / None / 3. */
t4a_gpu_status t4a_gpu_tci2_from_tensor_train(const t4a_gpu_tt* tt, double tolerance, size_t max_bond_dim,
                                              size_t max_iter, t4a_gpu_tci2** out);

/* =====================================================================================
 * Adaptive patching driver (BASELINE config 5): partitionedtt::adaptiveinterpolate
 * crates/tensor4all-partitionedtt/src/adaptive_interpolation.rs:58-262
 * ===================================================================================== */
typedef struct t4a_gpu_ptt t4a_gpu_ptt;

/* adaptiveinterpolate(f, batched_f, site_indices, initial_pivots, AdaptiveInterpolateOptions{tci_options, patch_order,
 * n_initial_pivots, recycle_pivots}).  Sites are identified by their position; `patch_order` is a permutation of
 * 0..n_sites-1 or NULL for the natural order (adaptive_interpolation.rs:336-354).  initial_pivots is n_sites x n_pivots
 * column-major.  One crossinterpolate2 runs on the device per patch; a patch is accepted when it terminated Converged
 * with final error <= tolerance (:357-359), otherwise it is split along the next unprojected site of patch_order.
 * The built-in variant restricts the integer weight tables of the device functor to the active sites of every patch. */
t4a_gpu_status t4a_gpu_adaptive_interpolate_builtin(const size_t* local_dims, size_t n_sites, int32_t fid, int32_t n_acc,
                                                    const double* params, const uint64_t* weights,
                                                    const size_t* initial_pivots, size_t n_pivots,
                                                    const t4a_gpu_tci2_options* tci_options, const size_t* patch_order,
                                                    size_t n_initial_pivots, int32_t recycle_pivots, t4a_gpu_ptt** out);
t4a_gpu_status t4a_gpu_adaptive_interpolate_callback(const size_t* local_dims, size_t n_sites, t4a_gpu_batch_eval_fn cb,
                                                     void* ctx, const size_t* initial_pivots, size_t n_pivots,
                                                     const t4a_gpu_tci2_options* tci_options, const size_t* patch_order,
                                                     size_t n_initial_pivots, int32_t recycle_pivots, t4a_gpu_ptt** out);
void t4a_gpu_ptt_release(t4a_gpu_ptt* h);
/* PartitionedTT::len: number of accepted patches (FIFO acceptance order). */
t4a_gpu_status t4a_gpu_ptt_len(const t4a_gpu_ptt* h, size_t* out);
/* Projector of patch k: `count` projected sites, positions ascending; positions / values may be NULL to query. */
t4a_gpu_status t4a_gpu_ptt_projector(const t4a_gpu_ptt* h, size_t k, size_t* count, size_t* positions, size_t* values);
/* SubDomainTT of patch k as a tensor train over ALL sites (projected sites carry copy-selector tensors,
 * adaptive_interpolation.rs:514-660); the new handle owns a device copy. */
t4a_gpu_status t4a_gpu_ptt_patch_tt(const t4a_gpu_ptt* h, size_t k, t4a_gpu_tt** out);
/* Sum over the patches at a batch of full multi-indices (idx: n_sites x n_pts column-major). */
t4a_gpu_status t4a_gpu_ptt_evaluate(t4a_gpu_ptt* h, const size_t* idx, size_t n_pts, double* out);

/* =====================================================================================
 * Tree tensor cross interpolation: tensor4all-treetci
 * crates/tensor4all-treetci/src/{graph,state,proposer,update,optimize,materialize,globalpivot,api}.rs
 * The batch evaluator of that crate, Fn(GlobalIndexBatch) with a column-major (n_sites, n_points) index buffer
 * (batch.rs:13-66, update.rs:213-232), IS t4a_gpu_batch_eval_fn.
 * ===================================================================================== */
typedef struct t4a_gpu_treetci t4a_gpu_treetci;

/* TreeTciOptions (optimize.rs:13-76).  max_bond_dim == 0 <=> None, has_seed == 0 <=> seed None. */
typedef struct t4a_gpu_treetci_options {
    double tolerance;                 /* 1e-8 */
    size_t max_iter;                  /* 20 */
    size_t max_bond_dim;              /* 0 */
    int32_t normalize_error;          /* 1 */
    int32_t enable_global_pivots;     /* 1 */
    size_t nsearch;                   /* 5 */
    size_t max_nglobal_pivot;         /* 5 */
    double tol_margin_global_search;  /* 10.0 */
    int32_t has_seed;                 /* 0 */
    uint64_t seed;
} t4a_gpu_treetci_options;
t4a_gpu_status t4a_gpu_treetci_options_default(t4a_gpu_treetci_options* opts);

/* TreeTciGraph::new(n_sites, edges) + TreeTCI2::new(local_dims, graph) (graph.rs:51-106, state.rs:66-103).
 * edges: 2 * n_edges site numbers (u0, v0, u1, v1, ...); the graph must be a tree. */
t4a_gpu_status t4a_gpu_treetci_new(const size_t* local_dims, size_t n_sites, const size_t* edges, size_t n_edges,
                                   t4a_gpu_treetci** out);
void t4a_gpu_treetci_release(t4a_gpu_treetci* h);
/* function source: as t4a_gpu_tci2_set_builtin_function / _set_callback */
t4a_gpu_status t4a_gpu_treetci_set_builtin_function(t4a_gpu_treetci* h, int32_t fid, int32_t n_acc, const double* params,
                                                    const uint64_t* weights);
t4a_gpu_status t4a_gpu_treetci_set_callback(t4a_gpu_treetci* h, t4a_gpu_batch_eval_fn cb, void* ctx);
/* TreeTCI2::add_global_pivots (state.rs:110-165): pivots is n_sites x n_pivots column-major. */
t4a_gpu_status t4a_gpu_treetci_add_global_pivots(t4a_gpu_treetci* h, const size_t* pivots, size_t n_pivots);
/* graph.rs:150-156 subregion_vertices(edge): the sorted site lists on the u side and on the v side (query with NULL). */
t4a_gpu_status t4a_gpu_treetci_subregion_vertices(const t4a_gpu_treetci* h, size_t u, size_t v, size_t* n_left,
                                                  size_t* left, size_t* n_right, size_t* right);
/* Proposer used by _candidates / _update_edge / _optimize / _crossinterpolate2 (proposer.rs:43-249): 0 DefaultProposer
 * (neighbour product), 1 SimpleProposer::seeded(seed) (d*chi random candidates per side), 2
 * TruncatedDefaultProposer::seeded(seed) (ordered sample of d*chi default candidates per side — keeps the matrices of
 * branching vertices at d*chi x d*chi).  The reference draws from rand SmallRng seeded through std DefaultHasher; the
 * stream here is splitmix64 ("parity unpinned"). */
t4a_gpu_status t4a_gpu_treetci_set_proposer(t4a_gpu_treetci* h, int32_t kind, uint64_t seed);
/* PivotCandidateProposer::candidates of the selected proposer (default: proposer.rs:57-88): left is (|left key| x n_left), right (|right key| x n_right),
 * both column-major; pass NULL buffers to query the counts. */
t4a_gpu_status t4a_gpu_treetci_candidates(const t4a_gpu_treetci* h, size_t u, size_t v, size_t* n_left, size_t* left,
                                          size_t* n_right, size_t* right);
/* update_edge with the default proposer (update.rs:22-115): candidate matrix on the device -> full-pivot rrLU ->
 * new pivot tables of both sides, bond error, pivot errors, max_sample_value.  rows / cols (>= min(n_left, n_right)
 * entries) receive the selected candidate numbers, pivot_errors rank + 1 values; all three may be NULL. */
t4a_gpu_status t4a_gpu_treetci_update_edge(t4a_gpu_treetci* h, size_t u, size_t v, size_t max_bond_dim, double rel_tol,
                                           double abs_tol, size_t* rank, size_t* rows, size_t* cols, double* pivot_errors);
/* optimize_default (optimize.rs:80-220) / crossinterpolate2 with the default proposer (api.rs:21-96; the tree network
 * is obtained afterwards with _materialize).  ranks / errors need max_iter entries; n_iter receives the sweep count. */
t4a_gpu_status t4a_gpu_treetci_optimize(t4a_gpu_treetci* h, const t4a_gpu_treetci_options* options, size_t* n_iter,
                                        size_t* ranks, double* errors);
t4a_gpu_status t4a_gpu_treetci_crossinterpolate2(t4a_gpu_treetci* h, const size_t* initial_pivots, size_t n_pivots,
                                                 const t4a_gpu_treetci_options* options, size_t* n_iter, size_t* ranks,
                                                 double* errors);
/* find_global_pivots (globalpivot.rs:24-172): out is n_sites x count column-major, at most max_nglobal_pivot columns. */
t4a_gpu_status t4a_gpu_treetci_find_global_pivots(t4a_gpu_treetci* h, size_t nsearch, size_t max_nglobal_pivot,
                                                  double tol_margin, double abs_tol, uint64_t seed, size_t* count,
                                                  size_t* out);
/* state accessors (state.rs:41-58, :168-199).  key: sorted site list of a subtree; out is |key| x count column-major. */
t4a_gpu_status t4a_gpu_treetci_pivots(const t4a_gpu_treetci* h, const size_t* key, size_t key_len, size_t* count,
                                      size_t* out);
t4a_gpu_status t4a_gpu_treetci_bond_errors(const t4a_gpu_treetci* h, double* out /* per edge, sorted edge order */);
t4a_gpu_status t4a_gpu_treetci_pivot_errors(const t4a_gpu_treetci* h, size_t* count, double* out);
t4a_gpu_status t4a_gpu_treetci_flush_pivot_errors(t4a_gpu_treetci* h);
t4a_gpu_status t4a_gpu_treetci_max_sample_value(const t4a_gpu_treetci* h, double* out);
t4a_gpu_status t4a_gpu_treetci_set_max_sample_value(t4a_gpu_treetci* h, double value);
t4a_gpu_status t4a_gpu_treetci_max_bond_error(const t4a_gpu_treetci* h, double* out);
t4a_gpu_status t4a_gpu_treetci_max_bond_dim(const t4a_gpu_treetci* h, size_t* out);
/* to_treetn(state, evaluate, center_site) (materialize.rs:17-166): builds one dense tensor per site on the device,
 * index order [site, incoming bonds (sorted neighbours except the parent), bond to the parent]; non-root sites solve
 * T * P = Pi1 by full-pivot LU, a numerically zero P gives a zero tensor. */
t4a_gpu_status t4a_gpu_treetci_materialize(t4a_gpu_treetci* h, size_t center_site);
/* ndims / dims (<= n_sites + 1 entries) / column-major data of one materialised site tensor; out may be NULL. */
t4a_gpu_status t4a_gpu_treetci_site_tensor(t4a_gpu_treetci* h, size_t site, size_t* ndims, size_t* dims, double* out);
/* TreeTN::evaluate of the materialised network at full multi-indices (idx: n_sites x n_pts column-major). */
t4a_gpu_status t4a_gpu_treetci_evaluate(t4a_gpu_treetci* h, const size_t* idx, size_t n_pts, double* out);

/* =====================================================================================
 * Quantics front end: tensor4all-quanticstci
 * crates/tensor4all-quanticstci/src/{options.rs,quantics_tci.rs}
 * Grid conventions (crate quanticsgrids @ 8214b72, un-vendored; restated from its published algorithm): R_d bits per
 * variable, most significant bit first, 0-based grid indices; unfolding 0 = Interleaved (one binary site per bit level
 * and variable), 1 = Fused (one site per bit level, value = sum_d bit_d * 2^d, first variable least significant).
 * ===================================================================================== */
typedef struct t4a_gpu_qtci t4a_gpu_qtci;
/* f: Fn(&[f64]) -> f64 evaluated for a batch: coords is n_vars x n_pts column-major; returns the number of values written */
typedef int64_t (*t4a_gpu_coord_eval_fn)(void* ctx, const double* coords, size_t n_vars, size_t n_pts, double* out);
/* f: Fn(&[usize]) -> f64 on 0-based grid indices, same batch layout */
typedef int64_t (*t4a_gpu_grididx_eval_fn)(void* ctx, const size_t* grididx, size_t n_vars, size_t n_pts, double* out);

/* QtciOptions (options.rs:9-45).  max_bond_dim == 0 <=> None.  The random initial pivots use rand::rng() in the
 * reference; here a fixed stream unless has_seed is set. */
typedef struct t4a_gpu_qtci_options {
    double tolerance;              /* 1e-8 */
    size_t max_bond_dim;           /* 0 */
    size_t max_iter;               /* 200 */
    size_t n_random_init_pivot;    /* 5 */
    int32_t unfolding_scheme;      /* 0 Interleaved */
    int32_t normalize_error;       /* 1 */
    int32_t has_seed;              /* 0 */
    uint64_t seed;
} t4a_gpu_qtci_options;
t4a_gpu_status t4a_gpu_qtci_options_default(t4a_gpu_qtci_options* opts);

/* quanticscrossinterpolate(&DiscretizedGrid, f, initial_pivots, options) (quantics_tci.rs:175-307).  The grid is given by
 * its builder arguments: bits per variable, bounds (NULL = 0 / 1), include_endpoint and the grid's own unfolding scheme.
 * initial_pivots: n_vars x n_pivots grid indices, column-major; has_pivots == 0 <=> None (first grid point).
 * Every distinct quantics point is evaluated once (cachedata); all misses of one candidate matrix reach `f` in one call. */
t4a_gpu_status t4a_gpu_quanticscrossinterpolate(const size_t* rs, size_t n_vars, const double* lower, const double* upper,
                                                int32_t include_endpoint, int32_t grid_unfolding, t4a_gpu_coord_eval_fn f,
                                                void* ctx, int32_t has_pivots, const size_t* initial_pivots, size_t n_pivots,
                                                const t4a_gpu_qtci_options* options, t4a_gpu_qtci** out);
/* quanticscrossinterpolate_discrete(size, f, initial_pivots, options) (:434-560): power-of-two sizes, equal in every
 * direction; unfolding from the options. */
t4a_gpu_status t4a_gpu_quanticscrossinterpolate_discrete(const size_t* sizes, size_t n_vars, t4a_gpu_grididx_eval_fn f,
                                                         void* ctx, int32_t has_pivots, const size_t* initial_pivots,
                                                         size_t n_pivots, const t4a_gpu_qtci_options* options,
                                                         t4a_gpu_qtci** out);
/* quanticscrossinterpolate_from_arrays(xvals, f, ..) (:309-432): xvals concatenated, sizes[d] values per variable;
 * uniform coordinates -> discretized grid with the end point included, otherwise coordinate lookup on an inherent grid. */
t4a_gpu_status t4a_gpu_quanticscrossinterpolate_from_arrays(const double* xvals, const size_t* sizes, size_t n_vars,
                                                            t4a_gpu_coord_eval_fn f, void* ctx, int32_t has_pivots,
                                                            const size_t* initial_pivots, size_t n_pivots,
                                                            const t4a_gpu_qtci_options* options, t4a_gpu_qtci** out);
void t4a_gpu_qtci_release(t4a_gpu_qtci* h);
/* QuanticsTensorCI2 accessors (:53-173) */
t4a_gpu_status t4a_gpu_qtci_evaluate(t4a_gpu_qtci* h, const size_t* grididx, size_t n_pts, double* out);
t4a_gpu_status t4a_gpu_qtci_sum(t4a_gpu_qtci* h, double* out);
t4a_gpu_status t4a_gpu_qtci_integral(t4a_gpu_qtci* h, double* out);
t4a_gpu_status t4a_gpu_qtci_n_sites(const t4a_gpu_qtci* h, size_t* n_sites, size_t* n_vars, int32_t* is_discretized);
t4a_gpu_status t4a_gpu_qtci_link_dims(const t4a_gpu_qtci* h, size_t* out /* n_sites - 1 */);
t4a_gpu_status t4a_gpu_qtci_history(const t4a_gpu_qtci* h, size_t* n_iter, size_t* ranks, double* errors);
/* tensor_train(): a new handle owning a device copy of the cores */
t4a_gpu_status t4a_gpu_qtci_tensor_train(t4a_gpu_qtci* h, t4a_gpu_tt** out);
/* tci(): pivot table of the underlying TreeTCI2 for a subtree key */
t4a_gpu_status t4a_gpu_qtci_tree_pivots(const t4a_gpu_qtci* h, const size_t* key, size_t key_len, size_t* count, size_t* out);
/* cachedata(): count entries; quantics is n_sites x count column-major (NULL to query); user_calls / user_points (may
 * be NULL) report how often and for how many points the user function was called */
t4a_gpu_status t4a_gpu_qtci_cachedata(const t4a_gpu_qtci* h, size_t* count, size_t* quantics, double* values,
                                      size_t* user_calls, size_t* user_points);
/* grid conversions: which = 0 grididx -> quantics, 1 quantics -> grididx, 2 quantics -> origcoord (out_d),
 * 3 local_dimensions, 4 grid_step (out_d) */
t4a_gpu_status t4a_gpu_qtci_grid(const t4a_gpu_qtci* h, int32_t which, const size_t* in, size_t* out_u, double* out_d);

/* quanticscrossinterpolate_batched (quanticstci/src/batched/mod.rs:50-191): vector / tensor valued f.  The callback
 * writes out[c + n_components * p] for every point p and returns n_components * n_pts; every coordinate reaches it once
 * for all components.  The result is a tensor train with one extra (component selector) site of dimension
 * prod(output_dims) (combine_component_tts, :193-318); ranks / errors (max_iter entries) are the element-wise maxima over
 * the per-component runs. */
typedef int64_t (*t4a_gpu_coord_eval_vec_fn)(void* ctx, const double* coords, size_t n_vars, size_t n_pts,
                                             size_t n_components, double* out);
t4a_gpu_status t4a_gpu_quanticscrossinterpolate_batched(const size_t* rs, size_t n_vars, const double* lower,
                                                        const double* upper, int32_t include_endpoint, int32_t grid_unfolding,
                                                        t4a_gpu_coord_eval_vec_fn f, void* ctx, const size_t* output_dims,
                                                        size_t n_output_dims, int32_t has_pivots, const size_t* initial_pivots,
                                                        size_t n_pivots, const t4a_gpu_qtci_options* options,
                                                        t4a_gpu_tt** out_tt, size_t* n_iter, size_t* ranks, double* errors,
                                                        size_t* user_points);

/* =====================================================================================
 * Dense labelled tensors: the einsum / linalg seam of tensor4all-core's dynamic-index layer
 * crates/tensor4all-core/src/defaults/{contract.rs:334-343, svd.rs:150-395, qr.rs:74-328, idx_tensor.rs:5278-5345},
 * index_ops.rs:660-696.  Tensors are column-major with one int64 label per axis (the caller's DynIndex ids); rank <= 16.
 * ===================================================================================== */
/* SvdTruncationPolicy (truncation.rs:137-147).  NULL = the default policy: relative, per value, 1e-12 (svd.rs:80-87). */
typedef struct t4a_gpu_svd_policy {
    double threshold;
    int32_t scale;    /* 0 Relative, 1 Absolute */
    int32_t measure;  /* 0 Value, 1 SquaredValue */
    int32_t rule;     /* 0 PerValue, 1 DiscardedTailSum */
} t4a_gpu_svd_policy;
/* compute_retained_rank (svd.rs:150-211) and compute_retained_rank_qr_from_dense (qr.rs:74-117; r is k x n column-major):
 * pure host functions, usable without a device. */
t4a_gpu_status t4a_gpu_svd_retained_rank(const double* s, size_t n, const t4a_gpu_svd_policy* policy, size_t* out);
t4a_gpu_status t4a_gpu_qr_retained_rank(const double* r, size_t k, size_t n, double rtol, size_t* out);
/* contract_pair(lhs, rhs): every common label is contracted; the result carries lhs's free axes then rhs's free axes, each in
 * operand order (no common label = outer product).  out may be NULL to query out_rank / out_dims / out_labels. */
t4a_gpu_status t4a_gpu_tensor_contract_f64(const double* a, const size_t* a_dims, const int64_t* a_labels, size_t a_rank,
                                           const double* b, const size_t* b_dims, const int64_t* b_labels, size_t b_rank,
                                           double* out, size_t* out_dims, int64_t* out_labels, size_t* out_rank);
/* svd_with(t, left_inds, options): unfold with the left labels first (in the given order) and the remaining axes in tensor
 * order, thin SVD, rank r = min(retained rank, max_bond_dim) >= 1 (truncate == 0: r = min(m, n)).
 * u: [left dims.., r], s: r values, v: [right dims.., r] (= V, not V^H).  Capacities: m*min(m,n), min(m,n), n*min(m,n).
 * has_max_bond_dim != 0 with max_bond_dim == 0 is an error (svd.rs:281-292). */
t4a_gpu_status t4a_gpu_tensor_svd_f64(const double* t, const size_t* dims, const int64_t* labels, size_t rank,
                                      const int64_t* left_labels, size_t n_left, int32_t truncate,
                                      const t4a_gpu_svd_policy* policy, int32_t has_max_bond_dim, size_t max_bond_dim,
                                      size_t* r, double* u, double* s, double* v);
/* qr_with(t, left_inds, options): q: [left dims.., r], r_factor: [r, right dims..]; truncate != 0 keeps the leading r rows
 * with r = number of rows of R whose norm is >= rtol * (largest row norm) (has_rtol == 0: default 1e-15). */
t4a_gpu_status t4a_gpu_tensor_qr_f64(const double* t, const size_t* dims, const int64_t* labels, size_t rank,
                                     const int64_t* left_labels, size_t n_left, int32_t truncate, int32_t has_rtol, double rtol,
                                     size_t* r, double* q, double* r_factor);

/* Device-resident labelled tensors: the same three operations without a host round trip per call (environment /
 * zip-up style chains keep their intermediates in HBM).  A handle owns its column-major payload, dims and labels. */
typedef struct t4a_gpu_tensor t4a_gpu_tensor;
t4a_gpu_status t4a_gpu_tensor_new(const double* data, const size_t* dims, const int64_t* labels, size_t rank,
                                  t4a_gpu_tensor** out);
void t4a_gpu_tensor_release(t4a_gpu_tensor* h);
t4a_gpu_status t4a_gpu_tensor_rank(const t4a_gpu_tensor* h, size_t* rank);
t4a_gpu_status t4a_gpu_tensor_dims(const t4a_gpu_tensor* h, size_t* dims, int64_t* labels);
t4a_gpu_status t4a_gpu_tensor_to_host(const t4a_gpu_tensor* h, double* out);
/* permute_indices: new axis k is the axis carrying labels[k] */
t4a_gpu_status t4a_gpu_tensor_permute(const t4a_gpu_tensor* h, const int64_t* labels, t4a_gpu_tensor** out);
/* replace label `from` by `to` (DynIndex replacement / priming on the caller's side) */
t4a_gpu_status t4a_gpu_tensor_relabel(t4a_gpu_tensor* h, int64_t from, int64_t to);
t4a_gpu_status t4a_gpu_tensor_contract(const t4a_gpu_tensor* a, const t4a_gpu_tensor* b, t4a_gpu_tensor** out);
/* N-ary contraction of ONE connected tensor network (tensor4all-core/src/defaults/contract.rs:283-298 contract /
 * contract_with_options; plan :885-941, connectivity :1167-1230): labels that occur in more than one operand are summed unless they
 * are listed in retain_labels (ContractionOptions::retain_indices: a retained shared label stays as a batch index and connects its
 * holders); the result carries the labels that occur once or are retained, in order of first appearance.  INVALID_ARGUMENT for no
 * operands, a retained label nobody has, a disconnected network ("Disconnected tensor network: k components found") or a label with
 * two dimensions.  One operand: a copy.  The network is reduced pair by pair (smallest intermediate first), every step a batched GEMM. */
t4a_gpu_status t4a_gpu_tensor_contract_many(const t4a_gpu_tensor* const* tensors, size_t n_tensors, const int64_t* retain_labels,
                                            size_t n_retain, t4a_gpu_tensor** out);
/* outer_product (contract.rs:440-447): the explicit product of operands WITHOUT a common label (INVALID_ARGUMENT otherwise) */
t4a_gpu_status t4a_gpu_tensor_outer_product(const t4a_gpu_tensor* a, const t4a_gpu_tensor* b, t4a_gpu_tensor** out);
/* tensordot (contract.rs:420-428, idx_tensor.rs:3596-3638): contraction along explicitly paired axes (labels_a[p] of a with
 * labels_b[p] of b; the labels may differ); result [free axes of a.., free axes of b..].  Errors as the reference's: no pairs, an
 * index that is not there, an axis named twice, unequal dimensions (INVALID_ARGUMENT); a common label that is not paired
 * (NOT_IMPLEMENTED: "Batch contraction is not yet implemented"). */
t4a_gpu_status t4a_gpu_tensor_tensordot(const t4a_gpu_tensor* a, const t4a_gpu_tensor* b, const int64_t* labels_a, const int64_t* labels_b,
                                        size_t n_pairs, t4a_gpu_tensor** out);
/* svd_with: u carries [left.., bond_label], s is a rank-1 tensor [bond_label] of singular values, v carries
 * [right.., bond_label_v]; qr_with: q [left.., bond_label], r [bond_label, right..] */
t4a_gpu_status t4a_gpu_tensor_svd(const t4a_gpu_tensor* t, const int64_t* left_labels, size_t n_left, int32_t truncate,
                                  const t4a_gpu_svd_policy* policy, int32_t has_max_bond_dim, size_t max_bond_dim,
                                  int64_t bond_label, int64_t bond_label_v, t4a_gpu_tensor** u, t4a_gpu_tensor** s,
                                  t4a_gpu_tensor** v);
t4a_gpu_status t4a_gpu_tensor_qr(const t4a_gpu_tensor* t, const int64_t* left_labels, size_t n_left, int32_t truncate,
                                 int32_t has_rtol, double rtol, int64_t bond_label, t4a_gpu_tensor** q, t4a_gpu_tensor** r);

/* factorize(t, left_inds, FactorizeOptions{alg, canonical, max_bond_dim, svd_policy, qr_rtol}) / factorize_full_rank
 * (defaults/factorize.rs:86-118, :399-425): left carries [left.., bond_label], right [bond_label, right..] and
 * left * right == t.  alg: 0 SVD (canonical 0 Left: left = U, right = S V^H; 1 Right: left = U S, right = V^H),
 * 1 QR (left = Q, right = R), 2 LU (rrLU with rel_tol 1e-14, permuted L and U, left-orthogonal for Left), 3 CI
 * (MatrixLUCI factors).  full_rank != 0: no truncation (rel_tol 0 for LU / CI).  singular_values (capacity min(m, n),
 * may be NULL) is written for SVD only; rank receives the bond dimension. */
t4a_gpu_status t4a_gpu_tensor_factorize(const t4a_gpu_tensor* t, const int64_t* left_labels, size_t n_left, int32_t alg,
                                        int32_t canonical, int32_t full_rank, const t4a_gpu_svd_policy* policy,
                                        int32_t has_max_bond_dim, size_t max_bond_dim, int32_t has_qr_rtol, double qr_rtol,
                                        int64_t bond_label, t4a_gpu_tensor** left, t4a_gpu_tensor** right, size_t* rank,
                                        double* singular_values);

/* SimpleTensorTrain arithmetic on the device (tensor4all-simplett/src/arithmetic.rs:34-180, tensortrain.rs:264-345,
 * :449-583).  add / sub: direct sum of the cores ([A | B], block diagonal, [A; B]; sub negates the last core of b first);
 * scale = scale_mut (the last core carries the factor); reverse swaps site order and the bond legs; partial_sum(dims) sums
 * the listed sites out (all sites summed: a one-site train of dimension 1 holding the scalar). */
t4a_gpu_status t4a_gpu_tt_add(const t4a_gpu_tt* a, const t4a_gpu_tt* b, t4a_gpu_tt** out);
t4a_gpu_status t4a_gpu_tt_sub(const t4a_gpu_tt* a, const t4a_gpu_tt* b, t4a_gpu_tt** out);
t4a_gpu_status t4a_gpu_tt_scale(t4a_gpu_tt* h, double factor);
/* inner_product (simplett/src/contraction.rs:82-186): sum over all indices of a * b, two MFMA GEMMs per site */
t4a_gpu_status t4a_gpu_tt_inner_product(const t4a_gpu_tt* a, const t4a_gpu_tt* b, double* out);
t4a_gpu_status t4a_gpu_tt_reverse(const t4a_gpu_tt* h, t4a_gpu_tt** out);
t4a_gpu_status t4a_gpu_tt_partial_sum(const t4a_gpu_tt* h, const size_t* dims, size_t n_dims, t4a_gpu_tt** out);

/* =====================================================================================
 * Gauge forms of a tensor train (opaque handles; tensors and bond vectors resident on the device)
 * tensor4all-simplett: canonical.rs:102-393 (SiteTensorTrain), :439-544 (center_canonicalize), vidal.rs:199-493
 * (VidalTensorTrain), :535-767 (InverseTensorTrain).  The MPO-side forms (SiteMPO::move_center_*, VidalMPO::from_mpo,
 * InverseMPO::from_mpo) are stubs in the reference and have no counterpart here.
 *
 * The reference's `qr_decomp` (canonical.rs:17-29, vidal.rs:22-33) is rrlu(matrix, {max_bond_dim: min(m, n), rel_tol: 0,
 * abs_tol: 0, left_orthogonal: true}) with lu.left(true) / lu.right(true): the gauged cores are unit-lower-trapezoidal LU
 * factors, not isometries, and the Vidal "singular values" are those of the LU-gauged bond matrices, NOT the Schmidt values of
 * the tensor.  These functions restate that.  A bond shrinks below min(m, n) only at an exactly zero pivot.
 *
 * Every form hands out its stored tensors as a plain train (`_tensors_tt`, a device-to-device copy): evaluate, sum and norm2
 * of AbstractTensorTrain on a form are t4a_gpu_tt_evaluate / _sum / _norm2 on that train.  Site tensors are column-major
 * [left, site, right]; dims3 is (left, site, right).  Argument errors are T4A_GPU_INVALID_ARGUMENT with the reference's
 * message, checked before the device is touched.
 * ===================================================================================== */
typedef struct t4a_gpu_site_tt t4a_gpu_site_tt;
typedef struct t4a_gpu_vidal_tt t4a_gpu_vidal_tt;
typedef struct t4a_gpu_inverse_tt t4a_gpu_inverse_tt;

/* SiteTensorTrain::from_tensor_train(tt, center) (canonical.rs:118-154): left sweep 0..center, right sweep n-1..center+1.
 * Errors: "Tensor train is empty", "Center {c} is out of range for {n} tensors". */
t4a_gpu_status t4a_gpu_site_tt_from_tt(const t4a_gpu_tt* tt, size_t center, t4a_gpu_site_tt** out);
void t4a_gpu_site_tt_release(t4a_gpu_site_tt* h);
t4a_gpu_status t4a_gpu_site_tt_len(const t4a_gpu_site_tt* h, size_t* out);
t4a_gpu_status t4a_gpu_site_tt_dims(const t4a_gpu_site_tt* h, size_t* dims3 /* 3 x n_sites */);
t4a_gpu_status t4a_gpu_site_tt_site_tensor(const t4a_gpu_site_tt* h, size_t site, double* out);
t4a_gpu_status t4a_gpu_site_tt_center(const t4a_gpu_site_tt* h, size_t* out);
/* move_center_left / move_center_right / set_center (canonical.rs:299-353): one gauge step per site moved.
 * Errors: "Cannot move center left: already at leftmost position", "... right: already at rightmost position",
 * "New center {c} is out of range for {n} tensors". */
t4a_gpu_status t4a_gpu_site_tt_move_center_left(t4a_gpu_site_tt* h);
t4a_gpu_status t4a_gpu_site_tt_move_center_right(t4a_gpu_site_tt* h);
t4a_gpu_status t4a_gpu_site_tt_set_center(t4a_gpu_site_tt* h, size_t center);
/* set_site_tensor / set_two_site_tensors (canonical.rs:363-392): plain replacement, nothing is re-gauged and the neighbouring
 * bonds are not checked (as in the reference).  Errors: site >= len; "Cannot set two-site tensors at site {i} (max {n-2})"
 * for site >= len - 1; a dimension above 65535 is NOT_IMPLEMENTED. */
t4a_gpu_status t4a_gpu_site_tt_set_site_tensor(t4a_gpu_site_tt* h, size_t site, const size_t* dims3, const double* data);
t4a_gpu_status t4a_gpu_site_tt_set_two_site_tensors(t4a_gpu_site_tt* h, size_t site, const size_t* dims3_1, const double* data1,
                                                    const size_t* dims3_2, const double* data2);
/* to_tensor_train (canonical.rs:356-358) and the stored tensors as a plain train: the same copy for this form.  A train whose
 * bonds no longer chain after a replacement is refused here (INVALID_ARGUMENT), not when it is stored. */
t4a_gpu_status t4a_gpu_site_tt_to_tt(const t4a_gpu_site_tt* h, t4a_gpu_tt** out);
t4a_gpu_status t4a_gpu_site_tt_tensors_tt(const t4a_gpu_site_tt* h, t4a_gpu_tt** out);
/* center_canonicalize(tensors, center) (canonical.rs:439-544) in place on a plain train; a silent no-op for n <= 1 or
 * center >= n, as there. */
t4a_gpu_status t4a_gpu_tt_center_canonicalize(t4a_gpu_tt* tt, size_t center);

/* VidalTensorTrain::from_tensor_train_with_partition(tt, start..end) (vidal.rs:229-395); from_tensor_train is 0..len.
 * Left sweep over start..end-1 (the LU-for-QR step), right sweep over end-1..start+1 by SVD without truncation
 * (singular_values[i-1] = all min(L, S R) values, core i = V^T, core i-1 = prev * (U diag(s))), then every element of the cores
 * start..end-2 is divided by sv[r] if sv[r] > 1e-15, else by 1.0.  An empty train gives the empty object.
 * Errors: "Partition end {e} exceeds tensor train length {n}", "Cannot compute Vidal singular values for an empty bond matrix". */
t4a_gpu_status t4a_gpu_vidal_tt_from_tt(const t4a_gpu_tt* tt, size_t start, size_t end, t4a_gpu_vidal_tt** out);
/* VidalTensorTrain::new(tensors, singular_values) (vidal.rs:403-428) from host data: cores concatenated as in t4a_gpu_tt_new,
 * svs the n_svs vectors concatenated with lengths sv_lens.  Only the number of vectors is checked, as in the reference
 * ("Expected {n-1} singular value vectors, got {n_svs}"); a vector shorter than its bond leaves the remaining indices unscaled,
 * a longer one is ignored beyond the bond (vidal.rs:476-480).  n_sites == 0 is the empty object (no device needed). */
t4a_gpu_status t4a_gpu_vidal_tt_new(const size_t* dims3, size_t n_sites, const double* cores, const size_t* sv_lens, size_t n_svs,
                                    const double* svs, t4a_gpu_vidal_tt** out);
void t4a_gpu_vidal_tt_release(t4a_gpu_vidal_tt* h);
t4a_gpu_status t4a_gpu_vidal_tt_len(const t4a_gpu_vidal_tt* h, size_t* out);
t4a_gpu_status t4a_gpu_vidal_tt_dims(const t4a_gpu_vidal_tt* h, size_t* dims3 /* 3 x n_sites */);
t4a_gpu_status t4a_gpu_vidal_tt_site_tensor(const t4a_gpu_vidal_tt* h, size_t site, double* out);
t4a_gpu_status t4a_gpu_vidal_tt_set_site_tensor(t4a_gpu_vidal_tt* h, size_t site, const size_t* dims3, const double* data);
t4a_gpu_status t4a_gpu_vidal_tt_partition(const t4a_gpu_vidal_tt* h, size_t* start, size_t* end);
/* singular_values(bond) (vidal.rs:431-433): *len receives the length; the values are written when out != NULL and
 * capacity >= *len (BUFFER_TOO_SMALL otherwise): query with out == NULL first.  The values live on the device and are read back
 * here.  set_singular_values replaces the vector (singular_values_mut, vidal.rs:451-453), any length. */
t4a_gpu_status t4a_gpu_vidal_tt_singular_values(const t4a_gpu_vidal_tt* h, size_t bond, double* out, size_t capacity, size_t* len);
t4a_gpu_status t4a_gpu_vidal_tt_set_singular_values(t4a_gpu_vidal_tt* h, size_t bond, const double* values, size_t len);
/* to_tensor_train (vidal.rs:456-492): every core but the last times sv[r] on its right bond, one launch for the train. */
t4a_gpu_status t4a_gpu_vidal_tt_to_tt(const t4a_gpu_vidal_tt* h, t4a_gpu_tt** out);
t4a_gpu_status t4a_gpu_vidal_tt_tensors_tt(const t4a_gpu_vidal_tt* h, t4a_gpu_tt** out);

/* InverseTensorTrain::from_vidal (vidal.rs:551-663): element (l, s, r) of a middle core is (val * sv[i-1][l]) * sv[i][r] in that
 * order, the first core gets only the right factor, the last only the left one; the stored inverse values are 1 / v if
 * |v| > 1e-15, else 0.  from_tt = from_vidal(VidalTensorTrain::from_tensor_train(tt)) (vidal.rs:671-678). */
t4a_gpu_status t4a_gpu_inverse_tt_from_vidal(const t4a_gpu_vidal_tt* vidal, t4a_gpu_inverse_tt** out);
t4a_gpu_status t4a_gpu_inverse_tt_from_tt(const t4a_gpu_tt* tt, t4a_gpu_inverse_tt** out);
void t4a_gpu_inverse_tt_release(t4a_gpu_inverse_tt* h);
t4a_gpu_status t4a_gpu_inverse_tt_len(const t4a_gpu_inverse_tt* h, size_t* out);
t4a_gpu_status t4a_gpu_inverse_tt_dims(const t4a_gpu_inverse_tt* h, size_t* dims3 /* 3 x n_sites */);
t4a_gpu_status t4a_gpu_inverse_tt_site_tensor(const t4a_gpu_inverse_tt* h, size_t site, double* out);
t4a_gpu_status t4a_gpu_inverse_tt_partition(const t4a_gpu_inverse_tt* h, size_t* start, size_t* end);
t4a_gpu_status t4a_gpu_inverse_tt_inverse_singular_values(const t4a_gpu_inverse_tt* h, size_t bond, double* out, size_t capacity,
                                                          size_t* len);
/* set_two_site_tensors(i, t1, inv_sv, t2) (vidal.rs:706-727); "Cannot set two-site tensors at site {i} (max {n-2})". */
t4a_gpu_status t4a_gpu_inverse_tt_set_two_site_tensors(t4a_gpu_inverse_tt* h, size_t site, const size_t* dims3_1, const double* data1,
                                                       const double* inv_sv, size_t inv_len, const size_t* dims3_2, const double* data2);
/* to_tensor_train (vidal.rs:730-766): every core but the last times the stored inverse values on its right bond. */
t4a_gpu_status t4a_gpu_inverse_tt_to_tt(const t4a_gpu_inverse_tt* h, t4a_gpu_tt** out);
t4a_gpu_status t4a_gpu_inverse_tt_tensors_tt(const t4a_gpu_inverse_tt* h, t4a_gpu_tt** out);

/* =====================================================================================
 * MPO<f64> (opaque handle; site tensors resident on the device) and the contraction of two MPOs
 * tensor4all-simplett/src/mpo/: mpo.rs:35-480, contract_naive.rs:41-172, contract_zipup.rs:45-167, canonical.rs:35-89,
 * factorize.rs:126-313, contraction.rs:17-42, dispatch.rs:8-92
 * A site tensor is column-major [left, s1, s2, right]; a state is an MPO whose s2 is 1 (t4a_gpu_mpo_from_tt).
 * ===================================================================================== */
typedef struct t4a_gpu_mpo t4a_gpu_mpo;

/* MPO::new(tensors) (mpo.rs:35-60).  dims4 is 4 x n_sites (left, s1, s2, right per site), cores the site tensors
 * concatenated.  INVALID_ARGUMENT, checked before the device is touched: neighbouring bonds differ, first left or last right
 * bond != 1, a zero dimension, a site of more than INT_MAX elements or a dimension (s1 * s2 included) above 65535.
 * n_sites == 0 is the empty MPO. */
t4a_gpu_status t4a_gpu_mpo_new(const size_t* dims4, size_t n_sites, const double* cores, t4a_gpu_mpo** out);
void t4a_gpu_mpo_release(t4a_gpu_mpo* h);
t4a_gpu_status t4a_gpu_mpo_clone(const t4a_gpu_mpo* h, t4a_gpu_mpo** out);
t4a_gpu_status t4a_gpu_mpo_len(const t4a_gpu_mpo* h, size_t* out);
t4a_gpu_status t4a_gpu_mpo_dims(const t4a_gpu_mpo* h, size_t* dims4 /* 4 x n_sites */);
t4a_gpu_status t4a_gpu_mpo_site_tensor(const t4a_gpu_mpo* h, size_t site, double* out);
/* MPO::evaluate (mpo.rs:245-340) for a batch: idx is 2 n_sites x n_pts column-major, [i1, j1, i2, j2, ...] per point; an index
 * out of range or an empty MPO is INVALID_ARGUMENT.  sum (mpo.rs:341-392): the empty MPO sums to 0. */
t4a_gpu_status t4a_gpu_mpo_evaluate(t4a_gpu_mpo* h, const size_t* idx, size_t n_pts, double* out);
t4a_gpu_status t4a_gpu_mpo_sum(t4a_gpu_mpo* h, double* out);
/* contract(a, b, algorithm, ContractionOptions{tolerance, max_bond_dim, factorize_method}) (dispatch.rs:67-92).
 * algorithm: 0 Naive, 1 ZipUp, 2 Fit.  compress (Naive only): 0 = contract_naive(a, b, None), the exact product with bonds
 * la * lb; != 0 = contract_naive(a, b, Some(options)), i.e. right-canonicalisation by QR (canonical.rs:35-89) and a left-to-right
 * SVD sweep (contract_naive.rs:100-172).  ZipUp (contract_zipup.rs:45-167) always truncates.  method: 0 SVD, 1 RSVD, 2 LU, 3 CI
 * (LU and CI fall back to SVD, factorize.rs:133-137).  max_bond_dim == 0 <=> None.  Truncation keeps singular values
 * s >= tolerance * s_max, at most max_bond_dim of them, at least one (a zero matrix gives a bond of 1, not an error).
 * INVALID_ARGUMENT: lengths differ, a.s2 != b.s1 at a site (the message names the site and both dimensions), a non-finite value
 * reaching the SVD, a result site above INT_MAX elements.  NOT_IMPLEMENTED: Fit (contract_fit.rs:65-96) and RSVD (:305-313). */
#define T4A_GPU_MPO_NAIVE 0
#define T4A_GPU_MPO_ZIPUP 1
#define T4A_GPU_MPO_FIT 2
#define T4A_GPU_FACTORIZE_SVD 0
#define T4A_GPU_FACTORIZE_RSVD 1
#define T4A_GPU_FACTORIZE_LU 2
#define T4A_GPU_FACTORIZE_CI 3
t4a_gpu_status t4a_gpu_mpo_contract(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, int32_t algorithm, int32_t compress, int32_t method,
                                    double tolerance, size_t max_bond_dim, t4a_gpu_mpo** out);
/* Bridges to t4a_gpu_tt (this project's; no simplett counterpart).  Both are device-to-device copies of the cores:
 * _from_tt gives site dims (d, 1) (a state as an MPO), _to_tt fuses (s1, s2) into one site index s1 + S1 * s2. */
t4a_gpu_status t4a_gpu_mpo_from_tt(const t4a_gpu_tt* tt, t4a_gpu_mpo** out);
t4a_gpu_status t4a_gpu_mpo_to_tt(const t4a_gpu_mpo* mpo, t4a_gpu_tt** out);
/* LinearOperator::transpose: s1 <-> s2 of every site, one axis permutation per site on the MPO's stream. */
t4a_gpu_status t4a_gpu_mpo_transpose(const t4a_gpu_mpo* mpo, t4a_gpu_mpo** out);

/* Variational (fit) contraction C ~ A·B with a bond cap.  This project's, as t4a_gpu_mpo_contract_tci is: the reference reserves
 * FitOptions (contract_fit.rs:19-46) and answers Unsupported, and t4a_gpu_mpo_contract(.., T4A_GPU_MPO_FIT, ..) keeps answering
 * NOT_IMPLEMENTED as dispatch.rs does.  The algorithm is the two-site fit of tensor4all-treetn (treetn/fit.rs) on a chain: C is kept
 * with an orthogonality centre, the environments of A·B against C are cached, every bond step factorises
 * Theta = (L_i A_i B_i) (A_{i+1} B_{i+1} R_{i+2}) with the rank rule of t4a_gpu_mpo_contract (s >= tolerance * s_max, at most
 * max_bond_dim values, at least one; LU and CI fall back to SVD, RSVD is NOT_IMPLEMENTED) and moves the centre.  One sweep visits
 * bonds 0 .. n-2 to the right, then n-2 .. 0 to the left.  norms[0] is the Frobenius norm of the start, norms[k] the norm of the
 * singular values kept at the last step of sweep k; the sweeps stop after sweep k when |norms[k] / norms[k-1] - 1| < convergence_tol
 * or k == max_sweeps.
 * initial: the start, or NULL for the zip-up product with the same tolerance, cap and method.  It must have the length of a and the
 * site dims (s1 of a, s2 of b); its bonds are free.  max_sweeps == 0 returns the start as it is, one site gives the exact product,
 * no site the empty MPO; none of the three runs a sweep (*n_sweeps = 0, norms untouched).
 * n_sweeps (may be NULL): the sweeps run.  norms (may be NULL): max_sweeps + 1 entries, the first *n_sweeps + 1 are written.
 * INVALID_ARGUMENT: the shape errors of t4a_gpu_mpo_contract (same messages), an initial of another length or other site dims, a
 * negative or non-finite tolerance or convergence_tol, an unknown factorize_method. */
typedef struct {
    double tolerance;
    int32_t has_max_bond_dim; /* 0 <=> None */
    size_t max_bond_dim;
    size_t max_sweeps;
    double convergence_tol;
    int32_t factorize_method; /* T4A_GPU_FACTORIZE_* */
} t4a_gpu_mpo_fit_options;
/* FitOptions::default(): 1e-12, Some(100), 10, 1e-10, SVD */
t4a_gpu_status t4a_gpu_mpo_fit_options_default(t4a_gpu_mpo_fit_options* out);
t4a_gpu_status t4a_gpu_mpo_contract_fit(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const t4a_gpu_mpo_fit_options* options,
                                        const t4a_gpu_mpo* initial /* may be NULL */, t4a_gpu_mpo** out, size_t* n_sweeps,
                                        double* norms /* max_sweeps + 1 entries, may be NULL */);
/* Test hook: one half product of the fit at `site`, launched exactly as the sweeps launch it (csrc/kernels_mpo_fit.hip), with host
 * arrays in and out, all column-major.  side 0: env is L[n_env, la, lb], out is P[n_env, s1, s2, ra, rb] = L A_site B_site;
 * side 1: env is R[ra, rb, n_env], out is Q[la, lb, s1, s2, n_env] = A_site B_site R  (la, ra: the bonds of a's site, lb, rb of b's,
 * s1 of a, s2 of b).  INVALID_ARGUMENT: the shape errors of t4a_gpu_mpo_contract, site out of range, n_env == 0, side not 0 or 1. */
t4a_gpu_status t4a_gpu_mpo_fit_half(const double* env, size_t n_env, int32_t side, const t4a_gpu_mpo* a, const t4a_gpu_mpo* b,
                                    size_t site, double* out);

/* Partial contraction of two MPOs: every leg is contracted, identified (diagonal) or kept (tensor4all-treetn/src/treetn/
 * partial_contraction.rs: partial_contract with PartialContractionSpec { contract_pairs, diagonal_pairs, output_order }), on a chain
 * and by position.  A pair is four numbers (site_a, leg_a, site_b, leg_b), leg 0 or 1 of the site tensor [left, leg 0, leg 1, right];
 * every leg is in at most one pair and the two dimensions of a pair are equal.  At a site the legs form three groups, each fused with
 * its first leg fastest and of dimension 1 when empty: S, the legs of a in no contract pair, in leg order (a diagonal pair keeps a's
 * leg); K, the contract pairs ordered by a's leg; T, the legs of b in no pair, in leg order.  The result is the MPO
 *   C_i[(a, b), s, t, (a', b')] = sum_{kappa in K} A_i[a, x(s, kappa), a'] * B_i[b, y(s, kappa, t), b']
 * with site dims (|S|, |T|) and the bonds fused as t4a_gpu_mpo_contract fuses them; a leg of b that is diagonally paired takes its
 * value from s.  {contract (i, 1, i, 0) for all i} is the matrix product, {diagonal (i, 0, i, 0), (i, 1, i, 1)} the Hadamard product
 * of two operators (site dims (s1 * s2, 1)), no pair at all the outer product.  The site product and the half product are HIP
 * kernels of their own (csrc/kernels_partial.hip); no copy tensor is multiplied into an operand.
 * INVALID_ARGUMENT (the reference's messages, contract pairs checked before diagonal ones): lengths differ; a site or leg out of range,
 * "partial_contract: (site i, leg l) from contract_pairs not found in first MPO external indices" (second for b); "partial_contract:
 * contract_pairs index shape mismatch: 2 != 3"; "partial_contract: first MPO index (site i, leg l) appears in multiple pairs"; |S| * |T|
 * above 65535.  NOT_IMPLEMENTED: a pair whose legs sit on two sites and output_order (n_output_order != 0) — the reference moves site
 * indices with swap_site_indices, which this backend does not have.  Trees, mismatched topologies and complex scalars are outside it. */
/* Host only: validates the spec against the (leg 0, leg 1) tables of both operands (2 x n each) and writes the result's site dims
 * (2 x n_a: |S|, |T|) and per-leg dims (4 x n_a: the legs of S, two slots, then those of T, two slots; 0 = no such leg).  Either
 * output may be NULL. */
t4a_gpu_status t4a_gpu_mpo_partial_plan(const size_t* a_site_dims, size_t n_a, const size_t* b_site_dims, size_t n_b,
                                        const size_t* contract_pairs, size_t n_contract, const size_t* diagonal_pairs, size_t n_diagonal,
                                        size_t n_output_order, size_t* out_site_dims, size_t* out_leg_dims);
/* algorithm: T4A_GPU_MPO_NAIVE (all site products in one launch; compress != 0 adds the compress stage of t4a_gpu_mpo_contract) or
 * T4A_GPU_MPO_ZIPUP (the recursion of t4a_gpu_mpo_contract, each site step one launch of the half product, no permutation).  method,
 * tolerance, max_bond_dim and the rank rule are those of t4a_gpu_mpo_contract; T4A_GPU_MPO_FIT and RSVD answer NOT_IMPLEMENTED with
 * its messages (the fit is t4a_gpu_mpo_partial_contract_fit). */
t4a_gpu_status t4a_gpu_mpo_partial_contract(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const size_t* contract_pairs, size_t n_contract,
                                            const size_t* diagonal_pairs, size_t n_diagonal, size_t n_output_order, int32_t algorithm,
                                            int32_t compress, int32_t method, double tolerance, size_t max_bond_dim, t4a_gpu_mpo** out);
/* t4a_gpu_mpo_contract_fit for a spec: options, initial (site dims (|S|, |T|)), n_sweeps and norms as there. */
t4a_gpu_status t4a_gpu_mpo_partial_contract_fit(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const size_t* contract_pairs, size_t n_contract,
                                                const size_t* diagonal_pairs, size_t n_diagonal, size_t n_output_order,
                                                const t4a_gpu_mpo_fit_options* options, const t4a_gpu_mpo* initial /* may be NULL */,
                                                t4a_gpu_mpo** out, size_t* n_sweeps, double* norms /* max_sweeps + 1 entries, may be NULL */);
/* Test hook, the counterpart of t4a_gpu_mpo_fit_half for a spec: side 0, env L[n_env, la, lb] -> P[n_env, s, t, ra, rb]; side 1, env
 * R[ra, rb, n_env] -> Q[la, lb, s, t, n_env], launched as zip-up and the fit launch it. */
t4a_gpu_status t4a_gpu_mpo_partial_half(const double* env, size_t n_env, int32_t side, const t4a_gpu_mpo* a, const t4a_gpu_mpo* b,
                                        const size_t* contract_pairs, size_t n_contract, const size_t* diagonal_pairs, size_t n_diagonal,
                                        size_t site, double* out);
/* Reads the fused site index s1 + S1 * s2 of every site as another (s1, s2) pair of the same product, in place; the cores stay
 * (Mpo::relabel_site_dims).  The Hadamard product of two operators comes out with site dims (s1 * s2, 1) and is relabelled to
 * (s1, s2) with it.  INVALID_ARGUMENT: n_sites is not the length, or a product differs. */
t4a_gpu_status t4a_gpu_mpo_relabel_site_dims(t4a_gpu_mpo* mpo, const size_t* site_dims /* 2 x n_sites */, size_t n_sites);

/* =====================================================================================
 * Contraction<f64>: the lazy product A·B of two MPOs (opaque handle; both operands resident on the device)
 * tensor4all-simplett/src/mpo/contraction.rs:60-383
 * Single elements and left / right environments of A·B without forming the product with bonds la * lb.  An index tuple is
 * [i_0, j_0, i_1, j_1, ...]: i_k indexes s1 of A, j_k indexes s2 of B, as in t4a_gpu_mpo_evaluate; idx is 2 n_sites x n_pts
 * column-major in every call.  Calls on one handle are serialised by a mutex inside it and may come from several threads.
 * The reference memoises environments across calls; this handle keeps nothing between calls (a batch computes every unique
 * half of its own points once), so _clear_cache is a no-op kept for parity — results are identical either way.
 * Contraction::with_transform (contraction.rs:118-125) has no entry here: a transform is applied to the returned values by the
 * caller (the Python binding does so on the host); a C function pointer per element would be the slowest part of a batch.
 * ===================================================================================== */
typedef struct t4a_gpu_contraction t4a_gpu_contraction;

/* Contraction::new (contraction.rs:69-110).  INVALID_ARGUMENT, checked before any device work: lengths differ
 * ("MPO length mismatch"), a.s2 != b.s1 at a site ("Shared shape mismatch at site", naming the site and both dimensions).  The
 * handle keeps device copies of both operands: a and b may be released at once. */
t4a_gpu_status t4a_gpu_contraction_new(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, t4a_gpu_contraction** out);
void t4a_gpu_contraction_release(t4a_gpu_contraction* h);
t4a_gpu_status t4a_gpu_contraction_len(const t4a_gpu_contraction* h, size_t* out);
/* result_site_dims (contraction.rs:142-147): (s1_a, s2_b) per site, 2 x n_sites */
t4a_gpu_status t4a_gpu_contraction_result_site_dims(const t4a_gpu_contraction* h, size_t* dims2);
/* evaluate (contraction.rs:187-252) for a batch.  INVALID_ARGUMENT: the empty contraction ("MPO is empty"), an index out of range
 * ("Index out of bounds: index .. at site .. (max: ..)", contraction.rs:158-175). */
t4a_gpu_status t4a_gpu_contraction_evaluate(t4a_gpu_contraction* h, const size_t* idx /* 2 n x n_pts */, size_t n_pts, double* out);
/* evaluate_left(n, .) / evaluate_right(n, .) (contraction.rs:262-383) for a batch: the environment of sites 0 .. n-1 (ra x rb) /
 * of sites n .. len-1 (la x lb); out receives n_pts column-major matrices one after the other, dims2 their (rows, cols).
 * n == 0 / n == len give [[1]].  Only the sites an environment covers are range-checked.  INVALID_ARGUMENT: n > len
 * ("Site n is out of range [0, len]"), an index out of range. */
t4a_gpu_status t4a_gpu_contraction_evaluate_left(t4a_gpu_contraction* h, size_t n, const size_t* idx, size_t n_pts, double* out,
                                                 size_t* dims2);
t4a_gpu_status t4a_gpu_contraction_evaluate_right(t4a_gpu_contraction* h, size_t n, const size_t* idx, size_t n_pts, double* out,
                                                  size_t* dims2);
/* The batch evaluation in the manner of TTCache::evaluate_many (cache.rs:558-744): unique left halves of `split` sites and unique
 * right halves are found on the host, their environments computed once each and paired on the device.  split == 0 applies
 * find_split_heuristic (cache.rs:690-744); used_split (may be NULL) receives the split that was used.  Environments whose working
 * set 2 * max(la*lb) + K * lb * ra exceeds 8192 doubles (64 KiB of LDS) are walked through global scratch, above 2 GiB per
 * workgroup the call is INVALID_ARGUMENT. */
t4a_gpu_status t4a_gpu_contraction_evaluate_many(t4a_gpu_contraction* h, const size_t* idx, size_t n_pts, size_t split, double* out,
                                                 size_t* used_split);
t4a_gpu_status t4a_gpu_contraction_clear_cache(t4a_gpu_contraction* h);
/* Points evaluated so far through _evaluate, _evaluate_many, _evaluate_matrix and _batch_eval (this project's: the function evaluations a cross
 * interpolation spent on the handle). */
t4a_gpu_status t4a_gpu_contraction_n_evaluated(const t4a_gpu_contraction* h, size_t* out);
/* A t4a_gpu_batch_eval_fn whose ctx is a t4a_gpu_contraction*: idx carries the fused site index f = i + S1_a * j of the product (the
 * fusion of t4a_gpu_mpo_to_tt), n_sites x n_pts column-major.  Decodes, evaluates as _evaluate_many with split == 0, returns n_pts;
 * a negative status code after recording the message otherwise.  Hand it to t4a_gpu_tci2_set_callback, t4a_gpu_treetci_*,
 * t4a_gpu_tt_estimate_true_error, t4a_gpu_tt_floating_zone or t4a_gpu_opt_first_pivot for a device-evaluated operator product. */
int64_t t4a_gpu_contraction_batch_eval(void* ctx, const uint32_t* idx, size_t n_sites, size_t n_pts, double* out);
/* The product A·B as an MPO by cross interpolation (this project's; no simplett counterpart — the model is the `algorithm = :TCI`
 * contraction of TensorCrossInterpolation.jl; t4a_gpu_mpo_contract keeps its three algorithms): a contraction of a and b, a
 * TensorCI2 over the fused local dims S1_a * S2_b with the callback above, crossinterpolate2 with `options`, to_tensor_train, and
 * the site dims relabelled to (s1_a, s2_b).  n_pivots == 0: the first pivot is found by opt_first_pivot (optfirstpivot.rs) from
 * the all-zero index through the same evaluator; what crossinterpolate2 answers for a pivot that is still zero is passed through.
 * initial_pivots: n_sites x n_pivots column-major fused indices.  info: [termination code, rank, function evaluations, last
 * error estimate]. */
t4a_gpu_status t4a_gpu_mpo_contract_tci(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const t4a_gpu_tci2_options* options,
                                        const size_t* initial_pivots, size_t n_pivots, t4a_gpu_mpo** out_mpo, double* info /* [4] */);

/* ---- candidate matrices of A·B filled on the device (this project's) ----
 * The four entries below answer INVALID_ARGUMENT, not NULL_POINTER, for a NULL handle or buffer ("... is null"), before a device is
 * touched.
 *
 * _evaluate_matrix: out[r + n_rows * c] = (A·B)(rows[r] + cols[c]) in host memory.  rows: 2 cut x n_rows column-major, the [i, j]
 * pairs of sites 0 .. cut-1 per row half; cols: 2 (len - cut) x n_cols, the pairs of sites cut .. len-1.  cut == 0 / cut == len:
 * that side's environment is [[1]] and its buffer is not read.  One environment launch per side (one workgroup per half, as in
 * _evaluate_many, with its LDS / global-scratch limit), one pairing launch over la * lb at the cut on the f64 matrix cores, one
 * download.  No unique map: the halves of a candidate matrix are distinct, equal ones would be walked twice.  The bits of an entry depend on its row half and its column half
 * only — not on n_rows, n_cols, the position of the entry or the other halves of the request: la * lb is summed in chunks of four in
 * ascending order for every entry alike.  INVALID_ARGUMENT: the empty contraction ("MPO is empty"), cut > len ("Invalid split
 * position"), an index out of range ("Index out of bounds: ..."), more than INT_MAX rows or 65535 * 64 columns.  n_rows == 0 or
 * n_cols == 0: nothing is written.  Counts n_rows * n_cols evaluations in _n_evaluated. */
t4a_gpu_status t4a_gpu_contraction_evaluate_matrix(t4a_gpu_contraction* h, size_t cut, const size_t* rows, size_t n_rows,
                                                   const size_t* cols, size_t n_cols, double* out);
/* The contraction as the DEVICE MATRIX SOURCE of a TensorCI2 over the fused site index f = i + S1_a * j: every candidate matrix the
 * driver builds whole (the two-site matrix of a bond under full pivot search, the matrices of fill_site_tensors, the last tensor of a
 * one-site sweep) is filled in device memory as _evaluate_matrix does, ordered against the handle's stream by events — no index
 * buffer, no unique map, no transfer of values.  t4a_gpu_contraction_batch_eval over the same contraction is installed as the host
 * callback beside it and serves everything that is not a whole matrix: global pivot search, pivot values, error estimates, a
 * candidate matrix sharded by t4a_gpu_tci2_set_pi_shard, and the single rows and columns of a rook search (pivot_search == 1 goes
 * through the host evaluator).  The driver otherwise treats the handle as one with a callback.  Replaces a callback or built-in
 * function set before, and is replaced by setting one.  INVALID_ARGUMENT before any device work: a NULL handle, different lengths,
 * a local dimension of the TensorCI2 that is not S1_a * S2_b of the site.  The values of the two routes agree to rounding, not
 * bit for bit (the pairing sums la * lb in another order).
 * LIFETIME: the TensorCI2 keeps the bare pointer, as it keeps the ctx of _set_callback: `contraction` must outlive `tci2`, or the
 * next _set_callback / _set_builtin_function / _set_contraction_source on it. */
t4a_gpu_status t4a_gpu_tci2_set_contraction_source(t4a_gpu_tci2* tci2, t4a_gpu_contraction* contraction);
/* out[0] candidate matrices filled by a device source, out[1] their entries, out[2] entries this handle asked of its host callback
 * (matrices of the callback route, rook rows and columns, global pivot search, pivot values; a sharded matrix counts in full).
 * With a contraction source, out[1] + out[2] is what the TensorCI2 added to t4a_gpu_contraction_n_evaluated. */
t4a_gpu_status t4a_gpu_tci2_source_stats(const t4a_gpu_tci2* tci2, uint64_t* out /* [3] */);
/* t4a_gpu_mpo_contract_tci with the contraction set as the device matrix source instead of the host callback; the first pivot search
 * and `info` are the same (function evaluations count both routes).  t4a_gpu_mpo_contract_tci itself keeps the host route. */
t4a_gpu_status t4a_gpu_mpo_contract_tci_device(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const t4a_gpu_tci2_options* options,
                                               const size_t* initial_pivots, size_t n_pivots, t4a_gpu_mpo** out_mpo,
                                               double* info /* [4] */);

/* =====================================================================================
 * Quantics transform operators as MPOs — the real-valued part of tensor4all-quanticstransform
 * shift.rs:49-291, flip.rs:44-249, cumsum.rs:76-346, common.rs:549-654, affine.rs:497-553, :673-711, :1386-1834,
 * difference_kernel.rs:29-107.  The complex-valued operators (quantics_fourier_operator, phase_rotation_operator*) are not
 * part of this f64 library.
 * An operator acts on a function held as a quantics tensor train with site 0 the most significant bit; its site tensors are
 * column-major [left, s1 = out, s2 = in, right], the layout of t4a_gpu_mpo.  Building one is exact integer bookkeeping on the
 * host: the builders and the _len / _dims / _site_tensor readers need no device and work with none visible.
 * t4a_gpu_qt_op_to_mpo is the one upload; the result is applied with t4a_gpu_mpo_contract.
 * ===================================================================================== */
typedef struct t4a_gpu_qt_op t4a_gpu_qt_op;
#define T4A_GPU_QT_PERIODIC 0
#define T4A_GPU_QT_ANTIPERIODIC 1
#define T4A_GPU_QT_OPEN 2
#define T4A_GPU_QT_LOWER 0
#define T4A_GPU_QT_UPPER 1
/* shift_operator: (M g)[x] = g[x - offset]; a wrap-around is weighted 1 / -1 / 0.  Any offset (negative, |offset| >= 2^r).
 * INVALID_ARGUMENT: r == 0, r > 63.  _multivar (nvariables >= 2, target_var < nvariables): the operator on one variable of a
 * fused train (site index var0 + 2 var1 + ...), identity on the others. */
t4a_gpu_status t4a_gpu_qt_shift_operator(size_t r, int64_t offset, int32_t bc, t4a_gpu_qt_op** out);
t4a_gpu_status t4a_gpu_qt_shift_operator_multivar(size_t r, int64_t offset, int32_t bc, size_t nvariables, size_t target_var,
                                                  t4a_gpu_qt_op** out);
/* flip_operator: x -> 2^r - x; x = 0 maps to itself with weight 1 / -1 / 0.  r >= 2. */
t4a_gpu_status t4a_gpu_qt_flip_operator(size_t r, int32_t bc, t4a_gpu_qt_op** out);
t4a_gpu_status t4a_gpu_qt_flip_operator_multivar(size_t r, int32_t bc, size_t nvariables, size_t target_var, t4a_gpu_qt_op** out);
/* triangle_operator: M[i, j] = [i > j] (LOWER) or [i < j] (UPPER); cumsum_operator is LOWER.  r >= 2. */
t4a_gpu_status t4a_gpu_qt_triangle_operator(size_t r, int32_t triangle, t4a_gpu_qt_op** out);
t4a_gpu_status t4a_gpu_qt_cumsum_operator(size_t r, t4a_gpu_qt_op** out);
/* affine_operator: |x> -> |y> with scale * y = a x + b, n input and m output variables (site dims 2^m x 2^n, m + n <= 15).
 * a (a_len = m * n, column-major a[i + m * j]), b (b_len = m) and scale > 0 are the rational matrix, vector and their common
 * denominator (AffineParams::to_integer_scaled); bc has n_bc = m entries.  The carries of a site are ordered ascending, so bond
 * indices are reproducible.  INVALID_ARGUMENT: wrong lengths, r == 0, m + n > 15, scale <= 0, a carry that leaves int64. */
t4a_gpu_status t4a_gpu_qt_affine_operator(size_t r, const int64_t* a, size_t a_len, const int64_t* b, size_t b_len, int64_t scale,
                                          size_t m, size_t n, const int32_t* bc, size_t n_bc, t4a_gpu_qt_op** out);
void t4a_gpu_qt_op_release(t4a_gpu_qt_op* h);
t4a_gpu_status t4a_gpu_qt_op_len(const t4a_gpu_qt_op* h, size_t* out);
t4a_gpu_status t4a_gpu_qt_op_dims(const t4a_gpu_qt_op* h, size_t* dims4 /* 4 x n_sites */);
t4a_gpu_status t4a_gpu_qt_op_site_tensor(const t4a_gpu_qt_op* h, size_t site, double* out);
/* the upload: NO_DEVICE without a GPU */
t4a_gpu_status t4a_gpu_qt_op_to_mpo(const t4a_gpu_qt_op* h, t4a_gpu_mpo** out);
/* difference_kernel_mpo: A[x, x'] = f((x - x') mod 2^r), times -1 for x < x' when ANTIPERIODIC, from a train f with binary
 * sites that stays on the device.  Bonds are 2 * f's (left = dl * f_left + fl); all sites are formed in one launch of the naive
 * MPO site contraction.  INVALID_ARGUMENT: OPEN, an empty train, a non-binary site. */
t4a_gpu_status t4a_gpu_qt_difference_kernel(const t4a_gpu_tt* f, int32_t bc, t4a_gpu_mpo** out);

/* Bridge between the tensor-train handles and the labelled tensors (tensor4all-treetn/src/simplett_bridge.rs).
 * _tt_to_tensors = tensor_train_to_treetn_with_names_and_site_indices (:118, :706-794) on a chain: out[s] carries the legs
 * [bond_labels[s-1], site_labels[s], bond_labels[s]], the two boundary legs of dimension 1 dropped (a single site gives
 * [site_labels[0]]); bond_labels has n_sites - 1 entries, out n_sites handles (all released again on failure).
 * _tensors_to_tt = treetn_to_tensor_train (:172-277): tensors[s] must have exactly one leg that is not shared with a chain
 * neighbour (its site index); the bond of tensors[s] and tensors[s+1] is the one label they share; legs are permuted to
 * (left bond, site, right bond) whatever their order. */
t4a_gpu_status t4a_gpu_tt_to_tensors(const t4a_gpu_tt* tt, const int64_t* site_labels, const int64_t* bond_labels,
                                     t4a_gpu_tensor** out);
t4a_gpu_status t4a_gpu_tensors_to_tt(const t4a_gpu_tensor* const* tensors, size_t n_sites, t4a_gpu_tt** out);

/* ---- tensor4all-aci: Alternating Cross Interpolation of an elementwise operator over tensor trains ----
 * (crates/tensor4all-aci/src: elementwise.rs:107-218, state.rs:24-925, local.rs:299-394, global_guard.rs:49-181).
 * Inputs are device-resident trains (t4a_gpu_tt handles); the local candidate matrices are built, pivoted (rrLU) and
 * factorised on the device. */
typedef struct t4a_gpu_aci_options { /* AciOptions (options.rs:37-168) */
    size_t max_iters;                 /* 20 */
    size_t min_iters;                 /* 2 */
    int32_t has_max_bond_dim;         /* 0 <=> None */
    size_t max_bond_dim;
    double tolerance;                 /* 1e-12 */
    int32_t scale_tolerance;          /* 1 */
    uint64_t rng_seed;                /* 0 */
    int32_t enable_global_guard;      /* 1 */
    size_t nsearch_global_pivots;     /* 5 */
    size_t max_nglobal_pivot;         /* 5 */
    size_t nsweeps_global_search;     /* 100 */
    double tol_margin_global_search;  /* 10.0 */
} t4a_gpu_aci_options;
t4a_gpu_status t4a_gpu_aci_options_default(t4a_gpu_aci_options* opts);
/* elementwise_batched's operator (batch.rs:33-217): values[input + n_inputs * point] -> out[point]; non-zero return stops
 * the sweep with T4A_GPU_CALLBACK_ERROR. */
typedef int32_t (*t4a_gpu_aci_op_fn)(void* user, const double* values, size_t n_inputs, size_t n_points, double* out);
/* op_kind: 0 callback `op`, 1 product of the inputs, 2 sum of the inputs (both fused into the candidate-matrix kernel) */
#define T4A_GPU_ACI_OP_CALLBACK 0
#define T4A_GPU_ACI_OP_PRODUCT 1
#define T4A_GPU_ACI_OP_SUM 2
/* elementwise_batched (elementwise.rs:107): initial_guess == NULL -> AciOptions::initial_guess None (random guess: the
 * reference draws ChaCha8 normals, this library a splitmix64 stream — pass the guess for a reproducible match).  ranks /
 * errors / nglobal_pivots need max_iters entries (NULL allowed); termination: 0 Converged, 1 RankLimited, 2 MaxIterations. */
t4a_gpu_status t4a_gpu_aci_elementwise(const t4a_gpu_tt* const* inputs, size_t n_inputs, int32_t op_kind, t4a_gpu_aci_op_fn op,
                                       void* user, const t4a_gpu_aci_options* options, const t4a_gpu_tt* initial_guess,
                                       t4a_gpu_tt** result, size_t* n_iters, size_t* ranks, double* errors,
                                       size_t* nglobal_pivots, int32_t* termination);
/* ElementwiseProblem (state.rs:24-109) stepped bond by bond; the inputs must outlive the problem. */
typedef struct t4a_gpu_aci_problem t4a_gpu_aci_problem;
t4a_gpu_status t4a_gpu_aci_problem_new(const t4a_gpu_tt* const* inputs, size_t n_inputs, int32_t op_kind, t4a_gpu_aci_op_fn op,
                                       void* user, const t4a_gpu_aci_options* options, const t4a_gpu_tt* initial_guess,
                                       t4a_gpu_aci_problem** out);
void t4a_gpu_aci_problem_release(t4a_gpu_aci_problem* h);
/* local_update (state.rs:729-860) */
t4a_gpu_status t4a_gpu_aci_problem_local_update(t4a_gpu_aci_problem* h, size_t bond, int32_t left_orthogonal);
/* add_global_pivots (state.rs:551-652): pivots is n_sites x n_pivots column-major; added = injected pivot count */
t4a_gpu_status t4a_gpu_aci_problem_add_global_pivots(t4a_gpu_aci_problem* h, const size_t* pivots, size_t n_pivots,
                                                     size_t* added);
/* find_global_pivots (global_guard.rs:49): out is n_sites x count column-major, capacity max_nglobal_pivot columns */
t4a_gpu_status t4a_gpu_aci_problem_find_global_pivots(t4a_gpu_aci_problem* h, uint64_t seed, size_t* count, size_t* out);
t4a_gpu_status t4a_gpu_aci_problem_solution(t4a_gpu_aci_problem* h, t4a_gpu_tt** out);
/* left (right == 0) / right frame of `input` at `site` (0..n_sites): shape (0, 0) when absent; out may be NULL */
t4a_gpu_status t4a_gpu_aci_problem_frame(t4a_gpu_aci_problem* h, int32_t right, size_t input, size_t site, size_t* rows,
                                         size_t* cols, double* out);
/* per bond: last pivot error and largest sampled operator magnitude (n_sites - 1 entries each) */
t4a_gpu_status t4a_gpu_aci_problem_errors(const t4a_gpu_aci_problem* h, double* pivot_errors, double* pivot_scales);

/* ---- tensor4all-treeaci: the edge-local step of TreeACI (crates/tensor4all-treeaci/src/local_update.rs:35-262
 * materialize_and_factor_edge; operator contract elementwise.rs:66,197 / batch.rs) from the candidate frames on: for every input k
 * row_frames[k] is bond_dims[k] x row_count and col_frames[k] is bond_dims[k] x col_count, column-major (one contiguous frame vector
 * per candidate, as InputFrameStore::candidate_frames_for_edge returns them).  value_k(row, col) = row_frame . col_frame; the operator
 * (op_kind / op / user as for t4a_gpu_aci_elementwise; callback batch layout values[input + n_inputs * (row + row_count * col)])
 * yields the local matrix; MatrixLUCI with max_bond_dim (0 = None), rel_tol = tolerance when scale_tolerance else abs_tol = tolerance.
 * A zero matrix comes back as the rank-one zero update (rank 1, indices 0, zero factors).  Capacities: row_indices / col_indices
 * min(row_count, col_count), pivot_errors min(row_count, col_count) + 1 (n_pivot_errors = entries written), left row_count x that,
 * right that x col_count (column-major, leading dimensions = row_count resp. *rank); local_values row_count x col_count (may be NULL). */
t4a_gpu_status t4a_gpu_treeaci_local_update_f64(size_t n_inputs, const size_t* bond_dims, const double* const* row_frames,
                                                const double* const* col_frames, size_t row_count, size_t col_count, int32_t op_kind,
                                                t4a_gpu_aci_op_fn op, void* user, size_t max_bond_dim, double tolerance,
                                                int32_t scale_tolerance, int32_t left_orthogonal, size_t* rank, size_t* row_indices,
                                                size_t* col_indices, double* pivot_errors, size_t* n_pivot_errors, double* left,
                                                double* right, double* sampled_scale, double* local_values);

/* ---- measurement hooks (bench.py) ---- */
/* (M, N, rank) of every bond update of the most recent 2-site half-sweep: out is 3 x (n_sites-1). */
t4a_gpu_status t4a_gpu_tci2_last_sweep_shapes(const t4a_gpu_tci2* h, size_t* out);
/* HIP-event profile accumulated since the last reset.  Slots (all in milliseconds / counts):
 *  [0] rrlu kernel ms  [1] rrlu launches  [2] pi-eval kernel ms  [3] pi launches
 *  [4] fill_site_tensors device ms  [5] fill calls  [6] factor (trsm+gemm) ms  [7] factor calls
 *  [8] total pivot steps executed by the rrlu kernel  [9] algorithmic rrlu bytes (BASELINE.md §2 model)
 *  [10] algorithmic flops (rrlu + factors + fill)  [11] function evaluations
 *  [12..15] the rrLU kernel instantiation with the largest total time: ms, launches, algorithmic bytes,
 *           code = RPT*1000 + CPT*10 + 4*row_major_ties + 2*single_workgroup + wave_uniform_columns (negative: LDS / HBM
 *           kernels; >= 100000: single-XCD kernel, see t4a_gpu_tci2_profile_variants) */
#define T4A_GPU_PROFILE_SLOTS 16
t4a_gpu_status t4a_gpu_tci2_profile_enable(t4a_gpu_tci2* h, int32_t enable);
t4a_gpu_status t4a_gpu_tci2_profile_reset(t4a_gpu_tci2* h);
t4a_gpu_status t4a_gpu_tci2_profile_get(const t4a_gpu_tci2* h, double* out /* [T4A_GPU_PROFILE_SLOTS] */);
/* One row {code, ms, launches, algorithmic bytes, pivot steps} per rrLU kernel instantiation used since the last reset
 * (query-then-fill: out == NULL returns the row count).  code >= 100000: single-XCD kernel,
 * 100000 + RPT*100 + CPT*10 + 4*row_major_ties; otherwise as slot 15 of t4a_gpu_tci2_profile_get.  Rows with
 * code >= 10000000 are SUB-aggregates of row code - 10000000: the launches of a bond chain that ran all max_bond_dim pivot
 * steps (the saturated bonds of a sweep); they are already contained in their parent row. */
t4a_gpu_status t4a_gpu_tci2_profile_variants(const t4a_gpu_tci2* h, double* out /* [cap_rows][5] */, size_t cap_rows, size_t* n_rows);

/* Device-side bond chain (the host-free half-sweep of update_pivots, tensorci2.rs:1695-1725 + :1821-2007 for built-in
 * functors): out[0] half-sweeps enqueued as one chain, out[1] bond updates inside such chains, out[2] chains that fell back to
 * the per-bond path part-way (a launch gave up), out[3] half-sweeps that were not eligible (host callback, rook search, shapes
 * beyond the device-dimension kernels) and ran bond by bond, out[4] chained half-sweeps that ran as part of a GROUP chain (one
 * launch per kernel and bond for all handles of a t4a_gpu_tci2_optimize_group call; counted in out[0] as well). */
t4a_gpu_status t4a_gpu_tci2_chain_stats(const t4a_gpu_tci2* h, uint64_t* out /* [5] */);
/* More of the same: out[0] chained sweeps (2-site half-sweeps counted in chain_stats out[0], and 1-site sweeps) that ran as ONE
 * persistent workgroup walking all bonds — every matrix of the sweep at most 64 x 32: small-rank problems and the first iterations
 * of every run (one launch per sweep instead of three per bond); out[1] 1-site sweeps (t4a_gpu_tci2_sweep1site, make_canonical,
 * the final sweep of optimize: tensorci2.rs:865-1050) that ran as a device-side chain — the independent side of every bond is the
 * index table itself, the site tensors come from the factored matrices the chain leaves behind; out[2] 1-site sweeps that were
 * not eligible and ran bond by bond; out[3] chained 1-site sweeps that fell back to the per-bond path part-way. */
t4a_gpu_status t4a_gpu_tci2_chain_stats_ext(const t4a_gpu_tci2* h, uint64_t* out /* [4] */);
/* Segments of launched chains.  A half-sweep whose middle bonds outgrow 64 x 32 is launched bond by bond, but every maximal run of
 * consecutive bonds that do fit (the two ends of such a chain) runs as ONE persistent workgroup between the launches of its
 * neighbours: out[0] such walked segments since the handle was created, out[1] the bonds in them.  A half-sweep that is one walk
 * as a whole counts in chain_stats_ext out[0] and not here; 1-site sweeps, group chains, chains with event timing and T4A_NO_WALK=1
 * have no segments.  Diagnostics only: a segment computes what the launches it replaces compute, bit for bit. */
t4a_gpu_status t4a_gpu_tci2_chain_segments(const t4a_gpu_tci2* h, uint64_t* out /* [2] */);
/* The split behind it (host only, no device is touched): bond b of n_bonds has the upper bounds dep_ub[b] rows of the dependent and
 * ind_ub[b] of the independent side, order[k] is the bond at position k of the half-sweep.  Segment s covers positions first[s] ..
 * first[s] + count[s] - 1 and is walked (walked[s] = 1) when every bond in it has dep_ub <= 64 and ind_ub <= 32; segments are maximal,
 * in sweep order, and cover every position once.  *n_segments is always written; with the three arrays NULL that is all, else
 * `capacity` must hold it (BUFFER_TOO_SMALL). */
t4a_gpu_status t4a_gpu_tci2_chain_plan_segments(const size_t* dep_ub, const size_t* ind_ub, const size_t* order, size_t n_bonds, size_t capacity,
                                                size_t* first, size_t* count, int32_t* walked, size_t* n_segments);
/* out[0] asynchronous fill_site_tensors issued by the optimisation loop, out[1] of them replayed from the captured HIP graph, out[2]
 * graph captures (a capture happens the second time a fill with the same signature — device addresses, shapes, staging buffers —
 * is issued; handles whose cores were exported / imported through stream 0 never replay: csrc/tci2_fill.hip issue_fill_ops). */
t4a_gpu_status t4a_gpu_tci2_fill_stats(const t4a_gpu_tci2* h, uint64_t* out /* [3] */);
/* PivotSearchStrategy::Rook on this handle: out[0] searches that ran device-resident (one launch, one host synchronisation per bond:
 * built-in functors), out[1] rows / columns they visited, out[2] searches driven from the host (callback functions: one round trip per
 * visited row / column), out[3] host synchronisations of all searches. */
t4a_gpu_status t4a_gpu_tci2_rook_stats(const t4a_gpu_tci2* h, uint64_t* out /* [4] */);
/* optimize_with_finder (tensorci2.rs:1626-1802) on up to EIGHT handles at once, driven in lock-step by the calling thread: every
 * iteration enqueues the half-sweeps of all handles — as ONE chain of launches when they line up (same number of sites, built-in
 * functors: every kernel serves all handles, handle i's rrLU runs on XCD i), otherwise one chain per handle — then completes them
 * one after the other.  This is the
 * per-GPU form of the patch farm (BASELINE.json configs[4]: eight patches per GPU; adaptive_interpolation.rs:171-330 runs the
 * patches one after the other): results on every handle are exactly those of t4a_gpu_tci2_optimize. */
t4a_gpu_status t4a_gpu_tci2_optimize_group(t4a_gpu_tci2* const* handles, size_t n_handles, const t4a_gpu_tci2_options* options,
                                           int32_t final_sweep1site);
/* fill_site_tensors (tensorci2.rs:1065-1186) on several handles at once: the fills of all handles are issued first — each on its
 * handle's own fill stream, so their kernels share the chip — and completed afterwards, instead of issue + wait handle by handle.
 * Results on every handle are exactly those of t4a_gpu_tci2_fill_site_tensors; a deferred solve error (singular pivot matrix) of
 * any handle is reported after all fills have completed. */
t4a_gpu_status t4a_gpu_tci2_fill_site_tensors_group(t4a_gpu_tci2* const* handles, size_t n_handles);
/* enable == 0: this handle runs every half-sweep bond by bond (A/B measurements, tests).  verify bit 0: after every chain the
 * device-side index tables are read back and compared with the host's I / J sets (T4A_GPU_INTERNAL_ERROR on a difference);
 * bit 1: while profiling, the rrLU launches of a chain are timed with HIP events around each launch instead of the kernels' own
 * time stamps (two more packets per bond on the stream: for calibration runs);
 * bit 2: the small-problem engine (below) is switched off for this handle; bit 3: its launch stamps its phases (diagnostic);
 * bit 4: opt-in to the relaxed guard of the captured fill_site_tensors graph — replay also on a handle whose site tensors are exported /
 * imported asynchronously, unless the legacy default stream or a blocking stream took part (default: never on such a handle);
 * bit 5: the small-problem engine keeps candidate matrices up to 32 x 32 (default 16 x 16: measured, the larger tile is slower than the
 * general path, so growing runs are handed over early). */
t4a_gpu_status t4a_gpu_tci2_set_chain(t4a_gpu_tci2* h, int32_t enable, int32_t verify);
/* Opt-in (default 1): the points of ONE candidate matrix (tensorci2.rs:1859-1893) are split into n_threads contiguous blocks and the host
 * callback is called for the blocks CONCURRENTLY from n_threads host threads (idx / out pointing into the block).  This is outside the
 * reference's contract — it calls `f` / `batched_f` sequentially from one thread on purpose (docs/design/adaptive-tci-interpolation.md:9-11)
 * — so only for callbacks that are thread safe; values, pivots and results are bitwise those of n_threads == 1.  Matrices below 16 384
 * points stay on the calling thread. */
t4a_gpu_status t4a_gpu_tci2_set_callback_threads(t4a_gpu_tci2* h, size_t n_threads);
/* The small-problem engine (round 6): optimize_with_finder (tensorci2.rs:1626-1802) of a small problem — iteration loop, the
 * update_pivots chain (:1821-2007), fill_site_tensors (:1065-1186), convergence_criterion (:1407-1437) and the final 1-site sweep
 * (:1781-1794) — as ONE launch, index sets in the LDS, every candidate matrix (up to 16 x 16; 32 x 32 on request) in the registers of one wavefront.
 * Offered every t4a_gpu_tci2_optimize / _crossinterpolate2 call on a built-in functor without global pivot search; when a set
 * outgrows 16 entries or a matrix its tile the launch hands the state at the start of that iteration back and the general path
 * continues.  Results are those of the general path (index sets, errors, ranks bit for bit).
 * out[0] calls the engine completed, [1] iterations it ran, [2] runs handed back, [3] calls that were not eligible,
 * [4..6] device time of the last launch in 100 MHz ticks (input, iterations, final sweep + results), [7] why the last launch handed back
 * (0 it did not, 1 list / matrix beyond the tile, 2 non-finite value, 3 rank beyond 16, 4 fill not representable / singular),
 * [8..15] shader cycles per phase of the last launch when the phase stamps are on (lists, evaluation, pivot steps, gather, factors,
 * fill, snapshots, convergence + rest). */
t4a_gpu_status t4a_gpu_tci2_small_stats(const t4a_gpu_tci2* h, uint64_t* out /* [16] */);

/* Evaluate a built-in function on the device for a batch of full multi-indices (parity check of the
 * workload definition itself).  idx: n_sites x n_pts column-major. */
t4a_gpu_status t4a_gpu_fn_eval(int32_t fid, int32_t n_acc, const double* params, const uint64_t* weights,
                               const size_t* local_dims, size_t n_sites, const size_t* idx, size_t n_pts,
                               double* out);

/* =====================================================================================
 * square_linsolve: (a0 + a1 A) x = b for an MPO A and tensor trains x, b resident on the device
 * tensor4all-treetn/src/linsolve/ (square/mod.rs:233-351, square/updater.rs, common/projected_operator.rs,
 * square/projected_state.rs), tensor4all-core/src/krylov.rs:1083-1490 (gmres_affine_impl), restated for a chain.
 * Scope: a chain, f64, V_in = V_out — every site of A has s1 == s2 == the state's site dimension.  Index mappings, tree
 * topologies, spectator nodes and complex scalars are not mirrored.
 * The algorithm is DMRG-style two-site sweeps with a local GMRES.  `init` is canonicalised onto `center` by thin QR sweeps.  The
 * sweep plan is the Euler tour from `center`, two sites per step, the second node of a step the new centre: bonds center .. n-2 to
 * the right, n-2 .. 0 to the left, 0 .. center-1 to the right (for center == 0 the order of t4a_gpu_mpo_contract_fit; the reference's
 * order at an inner centre follows petgraph's adjacency order and is not pinned).  One step at bond (i, i+1): theta_0 = x_i x_{i+1},
 * the local rhs Lb_i b_i b_{i+1} Rb_{i+2}, GMRES on (a0 + a1 H) theta = rhs from theta_0 with H the projected operator, an SVD of
 * theta as (chi_l d_i) x (d_{i+1} chi_r) with max_bond_dim and the policy of t4a_gpu_tensor_svd (none: its default), x_i = U and
 * x_{i+1} = S V^T moving right, x_i = U S and x_{i+1} = V^T moving left, then the environment of the side left behind.
 * GMRES builds the Arnoldi basis from the unshifted H; a0 and a1 enter the Hessenberg column; Givens rotations and the triangular
 * solve run on the host, which reads j + 2 doubles per Arnoldi step and one norm per restart.  ||rhs|| < 1e-15 returns the start,
 * lucky breakdown is at h_{j+1,j} <= 1e-14, the true residual is checked on convergence (local_gmres_options), non-convergence is
 * a flag, never an error.  Deviation: both orthogonalisation passes are classical Gram-Schmidt (all coefficients of a pass from one
 * launch), the reference's are modified Gram-Schmidt; the column of H is still pass 1 plus pass 2.
 * After each sweep with has_convergence_tol the residual ||(a0 + a1 A) x - b|| / ||b|| (the absolute norm when ||b|| <= 1e-15) is
 * computed from the exact naive apply, add / sub and the norm of the QR-canonical residual train, and the sweeps stop below the
 * tolerance; otherwise it is computed once at the end if check_residual.  converged is false when no convergence_tol was given.
 * a1 == 0 or ||A|| <= 1e-15: the solution is rhs / a0, *sweeps = 0 (a0 == 0 as well: INVALID_ARGUMENT).
 * Memory of a bond step: W (M^2 + N^2 + M N) + (gmres_restart_dim + 1) M N doubles, M = chi_l d_i, N = d_{i+1} chi_r, W the operator
 * bond between the two sites.
 * INVALID_ARGUMENT with a message, before the device is touched: fewer than two sites ("the one-site local solve is not
 * implemented"), lengths differ, a site of A that is not square or does not match the state's or the rhs's site dimension,
 * center >= n, gmres_restart_dim == 0 or gmres_max_restarts == 0, a negative or non-finite tolerance, a work buffer of a bond step
 * above INT_MAX elements (the message names the bond).
 * ===================================================================================== */
#define T4A_GPU_GMRES_RELATIVE 0
#define T4A_GPU_GMRES_ABSOLUTE 1
typedef struct {
    size_t nfullsweeps;
    int32_t has_max_bond_dim; /* 0 <=> None */
    size_t max_bond_dim;
    int32_t has_svd_policy;   /* 0 <=> None: the default policy of t4a_gpu_tensor_svd */
    t4a_gpu_svd_policy svd_policy;
    double gmres_tol;
    int32_t gmres_tolerance_mode; /* T4A_GPU_GMRES_* */
    size_t gmres_max_restarts;
    size_t gmres_restart_dim;
    double a0, a1;
    int32_t has_convergence_tol;
    double convergence_tol;
    int32_t check_residual;
} t4a_gpu_linsolve_options;
typedef struct {
    size_t local_solves;  /* bond steps */
    size_t arnoldi_steps; /* over all local solves */
    size_t apply_calls;   /* projected applies, the residual evaluations of GMRES included */
} t4a_gpu_linsolve_stats;
/* LinsolveOptions::default(): 5, None, None, 1e-10, relative, 100, 30, a0 = 0, a1 = 1, None, check_residual = 1 */
t4a_gpu_status t4a_gpu_linsolve_options_default(t4a_gpu_linsolve_options* out);
/* The shape checks of t4a_gpu_square_linsolve on plain dimension lists: op_dims4 (left, s1, s2, right) per site, rhs_dims3 (may be
 * NULL with n_rhs == 0: no rhs) and state_dims3 (left, site, right) per site.  A pure host function, usable without a device. */
t4a_gpu_status t4a_gpu_linsolve_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* rhs_dims3, size_t n_rhs,
                                             const size_t* state_dims3, size_t n_state, size_t center, size_t gmres_restart_dim);
t4a_gpu_status t4a_gpu_square_linsolve(const t4a_gpu_mpo* op, const t4a_gpu_tt* rhs, const t4a_gpu_tt* init, size_t center,
                                       const t4a_gpu_linsolve_options* options, t4a_gpu_tt** solution, size_t* sweeps,
                                       int32_t* has_residual, double* residual, int32_t* converged,
                                       t4a_gpu_linsolve_stats* stats /* may be NULL */);
/* relative_linear_system_residual (square/mod.rs:432-): ||(a0 + a1 A) x - b|| / ||b||, the absolute norm when ||b|| <= 1e-15 */
t4a_gpu_status t4a_gpu_relative_linear_system_residual(const t4a_gpu_mpo* op, const t4a_gpu_tt* solution, const t4a_gpu_tt* rhs, double a0,
                                                       double a1, double* out);

/* ProjectedOperator (common/projected_operator.rs:230-410, :495-631) of <x|A|x> on a chain: an opaque handle that keeps device copies
 * of the operator and the state.  Environments are column-major L[beta, w, alpha], R[beta, w, alpha] (bra bond, operator bond, ket
 * bond), computed lazily from the state and cached.
 * _local_dims: (chi_l, d_site, d_{site+1}, chi_r) of the region (site, site + 1).
 * _apply: out = H v for that region, v and out column-major [alpha_l, t1, t2, alpha_r] of chi_l d_site d_{site+1} chi_r doubles.
 * _environment: side 0 the left environment of the sites < bond, side 1 the right environment of the sites >= bond (bond <= n);
 *   dims receives (chi, W, chi); out may be NULL to query dims.
 * _invalidate: the caches that contain `site` go stale (left ones beyond it, right ones up to it).
 * _set_site_tensors: replaces sites (site, site + 1) by host tensors (outer bonds and site dimensions kept, the shared bond free)
 *   and invalidates both. */
typedef struct t4a_gpu_projected_operator t4a_gpu_projected_operator;
t4a_gpu_status t4a_gpu_projected_operator_new(const t4a_gpu_mpo* op, const t4a_gpu_tt* state, t4a_gpu_projected_operator** out);
void t4a_gpu_projected_operator_release(t4a_gpu_projected_operator* h);
t4a_gpu_status t4a_gpu_projected_operator_local_dims(const t4a_gpu_projected_operator* h, size_t site, size_t* dims4);
t4a_gpu_status t4a_gpu_projected_operator_apply(t4a_gpu_projected_operator* h, size_t site, const double* v, double* out);
t4a_gpu_status t4a_gpu_projected_operator_environment(t4a_gpu_projected_operator* h, int32_t side, size_t bond, size_t* dims3, double* out);
/* _apply_one_site: out = H v for the one-site region `site` (the site correction of t4a_gpu_tdvp), v and out column-major
 *   [alpha_l, t, alpha_r] of chi_l d_site chi_r doubles: out[b, s, b'] = sum L_site[b, w, a] A_site[w, s, t, w'] v[a, t, a']
 *   R_{site+1}[b', w', a'], launched as the sweeps launch it (the half operator HL = L A and two products).  *reused_hl (may be NULL)
 *   is 1 when the HL left behind by an earlier _apply of the bond (site, site + 1) served instead of a new one, else 0.
 * _time_one_site (tools/probe_tdvp.py): device milliseconds of its three launches, ms[0] HL = L A, ms[1] T = HL V, ms[2] Y = T R^T. */
t4a_gpu_status t4a_gpu_projected_operator_apply_one_site(t4a_gpu_projected_operator* h, size_t site, const double* v, double* out,
                                                         int32_t* reused_hl);
t4a_gpu_status t4a_gpu_projected_operator_time_one_site(t4a_gpu_projected_operator* h, size_t site, size_t reps, double* ms /* [3] */);
/* Test hook of one-site TDVP: the environment of the bond-centre step next to `site`, built with the PRESENT tensor of that site as the
 * isometry Q (ProjectedOperator::prepare_bond_center): toward_right 1: La[:, w, :] = Q^T (HL_w Q) with HL = L_site A_site, which is also
 * L_{site+1}; 0: Rb[:, w, :] = (Q HR_w^T) Q^T with HR = A_site R_{site+1}, which is also R_site.  dims3 receives (k, W, k); out may be NULL. */
t4a_gpu_status t4a_gpu_projected_operator_bond_center_env(t4a_gpu_projected_operator* h, size_t site, int32_t toward_right, size_t* dims3,
                                                          double* out);
t4a_gpu_status t4a_gpu_projected_operator_invalidate(t4a_gpu_projected_operator* h, size_t site);
t4a_gpu_status t4a_gpu_projected_operator_set_site_tensors(t4a_gpu_projected_operator* h, size_t site, const size_t* dims3_a, const double* t_a,
                                                           const size_t* dims3_b, const double* t_b);
/* Probe (tools/probe_linsolve.py): device time in milliseconds of the five launches of one Arnoldi step with nb basis vectors at the
 * region (site, site + 1), each measured with events around `reps` launches behind a warm-up launch: ms[0] T = HL V, ms[1] Y = T HR,
 * ms[2] gs_dots, ms[3] gs_update, ms[4] gs_normalize. */
t4a_gpu_status t4a_gpu_projected_operator_time_step(t4a_gpu_projected_operator* h, size_t site, size_t nb, size_t reps, double* ms /* [5] */);
/* The apply on caller-supplied environments, launched exactly as the sweeps launch it (the two half-operator builders of
 * csrc/kernels_linsolve.hip and two products); the counterpart of t4a_gpu_mpo_fit_half.  dims = (chi_l, chi_r); L is
 * [chi_l, W_l, chi_l], R is [chi_r, W_r, chi_r] with the outer operator bonds of sites `site`, `site + 1`; v and out hold
 * chi_l d_site d_{site+1} chi_r doubles.  hl / hr (may be NULL) receive the half operators: HL (W M) x M with
 * HL[(beta_l s1) + M w, (alpha_l t1)], HR (W N) x N with HR[w + W (t2 alpha_r), (s2 beta_r)], M = chi_l d_site, N = d_{site+1} chi_r. */
t4a_gpu_status t4a_gpu_projected_operator_apply_env(const double* L, const double* R, const size_t* dims, const t4a_gpu_mpo* op, size_t site,
                                                    const double* v, double* out, double* hl, double* hr);
/* Test hooks.  _orth: one two-pass orthogonalisation step of GMRES as the solver launches it: w (len, in / out) against the nb columns
 * of basis (len x nb), then normalised; h_out receives 2 nb doubles, the coefficients of pass 1 and of pass 2 (the column of H is
 * their sum), norm_out the norm of w before the normalisation.
 * _gmres_dense: the solver the sweeps run on (a0 + a1 H) x = b for a dense n x n matrix H (column-major) applied on the device. */
t4a_gpu_status t4a_gpu_linsolve_orth(const double* basis, size_t len, size_t nb, double* w_inout, double* h_out, double* norm_out);
t4a_gpu_status t4a_gpu_linsolve_gmres_dense(const double* H, size_t n, const double* b, const double* x0, double a0, double a1, double tol,
                                            int32_t mode, size_t restart_dim, size_t max_restarts, double* x, size_t* iterations,
                                            double* residual, int32_t* converged);
/* _krylov_orth: t4a_gpu_linsolve_orth with the launch of the projections chosen: route 0 the serial gs_dots (what GMRES and Lanczos
 *   run), 1 gs_dots_wide (a second grid dimension over the basis vectors, GS_WIDE = 8 per workgroup), 2 the rule the Krylov exponential
 *   of t4a_gpu_tdvp applies.  The three give the same bits.
 * _krylov_dots_route: that rule for a vector of len elements and nb basis vectors (host only) -> 0 or 1.
 * _krylov_time_dots (tools/probe_tdvp.py): device milliseconds of the serial [0] and the wide [1] launch. */
t4a_gpu_status t4a_gpu_krylov_orth(const double* basis, size_t len, size_t nb, double* w_inout, int32_t route, double* h_out, double* norm_out);
t4a_gpu_status t4a_gpu_krylov_dots_route(size_t len, size_t nb, int32_t* route);
t4a_gpu_status t4a_gpu_krylov_time_dots(size_t len, size_t nb, size_t reps, double* ms /* [2] */);

/* =====================================================================================
 * Two-site DMRG: the lowest eigenpair of an MPO H over tensor trains resident on the device
 * tensor4all-treetn/src/dmrg/mod.rs (dmrg, dmrg_with_treetn_operator, DmrgOptions, DmrgResult) on the Hermitian Lanczos of
 * tensor4all-core/src/krylov.rs:517-634 (hermitian_lanczos_lowest_eigenpair, helpers :2500-2675), restated for a chain.
 * Scope: that of t4a_gpu_square_linsolve — a chain, f64, one site index per node, V_in = V_out (every site of H has s1 == s2 == the
 * state's site dimension; the dimensions may differ from site to site).  Trees, index mappings, complex scalars and nsite != 2 are
 * not mirrored; nsite = 1 is refused as the reference refuses it.
 * `init` is canonicalised onto `center` and swept exactly as t4a_gpu_square_linsolve does it: bonds center .. n-2 to the right,
 * n-2 .. 0 to the left, 0 .. center-1 to the right, the second node of a step the new centre.  One step at bond (i, i+1): theta_0 =
 * x_i x_{i+1}, the half operators of the projected operator, Lanczos for its lowest eigenpair from theta_0, the SVD split of the
 * unit-norm Ritz vector with max_bond_dim and the policy of t4a_gpu_tensor_svd (none: its default), the singular values into the new
 * centre (no renormalisation after truncation), then the environment of the side left behind from this step's half operator.
 * Lanczos: v_0 = theta_0 / |theta_0| (|theta_0| <= breakdown_tol: INVALID_ARGUMENT); step j: w = H v_j, two orthogonalisation passes
 * against v_0 .. v_j, the column of the projected matrix is pass 1 plus pass 2, beta = |w|; the (j+1) x (j+1) projected matrix is the
 * full upper-Hessenberg data, checked entry pair by entry pair with scale max(1, |a_ij|, |a_ji|) against hermitian_tol
 * (INVALID_ARGUMENT "projected operator is not Hermitian"), symmetrised, and its lowest eigenpair taken on the host by a cyclic
 * Jacobi; estimate = beta |c_j|, threshold = max(atol, rtol max(1, |lambda|)); on estimate <= threshold or beta <= breakdown_tol the
 * Ritz vector sum_i c_i v_i and its true residual |H v - lambda v| are formed on the device and the solve returns if that residual
 * is below the threshold or on breakdown; after max_iter steps the last Ritz state is returned.  Non-convergence is a flag, never
 * an error.  The host reads one norm per solve, j + 2 doubles per step and three per finalise.  Deviation: both passes are classical
 * Gram-Schmidt (all coefficients of a pass from one launch), the reference's are modified Gram-Schmidt.
 * With has_energy_tol the sweeps stop when the last step's Ritz value moved by <= energy_tol against the sweep before (converged = 1;
 * the first sweep only records); converged is 0 otherwise.  *energy is the Rayleigh quotient <theta|H theta> / <theta|theta> at the
 * region (center, center + 1), or (center - 1, center) when center == n - 1, through the projected operator; a denominator <=
 * real_scalar_tol is INVALID_ARGUMENT ("DMRG Rayleigh quotient denominator is zero").  *max_residual_norm is the maximum of the
 * steps' true residuals, *local_updates the number of steps.
 * Memory of a bond step: W (M^2 + N^2 + M N) + (max_iter + 2) M N doubles, M = chi_l d_i, N = d_{i+1} chi_r.
 * INVALID_ARGUMENT with a message, before the device is touched: nsite != 2, nsweeps == 0, max_bond_dim == 0 when set, energy_tol or
 * real_scalar_tol negative or non-finite, lanczos.max_iter == 0 or above 8191, a negative or non-finite rtol, atol, breakdown_tol or
 * hermitian_tol, center >= n, lengths differ, a site of H that is not square or does not match the state, fewer than two sites
 * ("two-site DMRG requires at least one state edge"), a work buffer of a bond step above INT_MAX elements (the message names the bond).
 * ===================================================================================== */
typedef struct {
    size_t max_iter;
    double rtol, atol, breakdown_tol, hermitian_tol;
} t4a_gpu_lanczos_options;
typedef struct {
    size_t nsite;
    size_t nsweeps;
    int32_t has_max_bond_dim; /* 0 <=> None */
    size_t max_bond_dim;
    int32_t has_svd_policy;   /* 0 <=> None: the default policy of t4a_gpu_tensor_svd */
    t4a_gpu_svd_policy svd_policy;
    t4a_gpu_lanczos_options lanczos;
    int32_t has_energy_tol;
    double energy_tol;
    double real_scalar_tol;
} t4a_gpu_dmrg_options;
typedef struct {
    size_t local_solves;  /* bond steps */
    size_t lanczos_steps; /* over all local solves */
    size_t apply_calls;   /* projected applies, those of the true residuals included */
} t4a_gpu_dmrg_stats;
/* DmrgOptions::default(): 2, 5, None, None, (64, 1e-10, 0, 1e-14, 1e-10), None, 1e-10 */
t4a_gpu_status t4a_gpu_dmrg_options_default(t4a_gpu_dmrg_options* out);
/* The shape checks of t4a_gpu_dmrg on plain dimension lists: op_dims4 (left, s1, s2, right) and state_dims3 (left, site, right) per
 * site.  A pure host function, usable without a device. */
t4a_gpu_status t4a_gpu_dmrg_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* state_dims3, size_t n_state, size_t center,
                                         size_t max_iter);
t4a_gpu_status t4a_gpu_dmrg(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_dmrg_options* options,
                            t4a_gpu_tt** state, double* energy, size_t* sweeps_completed, size_t* local_updates, int32_t* converged,
                            double* max_residual_norm, t4a_gpu_dmrg_stats* stats /* may be NULL */);
/* The Rayleigh quotient of t4a_gpu_dmrg for any state: a copy is canonicalised onto `center` (real_scalar_tol = 1e-10) */
t4a_gpu_status t4a_gpu_dmrg_energy(const t4a_gpu_mpo* op, const t4a_gpu_tt* state, size_t center, double* out);
/* Test hooks.  _lanczos_dense: the solver the sweeps run, on a dense n x n matrix H (column-major) applied on the device, from v0;
 *   eigenvector receives n doubles.
 * _krylov_combine: out = sum_i coef[i] basis[:, i] (basis len x nb column-major, i ascending) and *norm2 = |out|^2, as a finalise
 *   launches it.
 * _eig_residual: r = hv - lambda v (r may be NULL) and sums3 = (|r|^2, <v, hv>, <v, v>) from the launch pair of a finalise.
 * Probe (tools/probe_dmrg.py): _lanczos_time_finalise: device milliseconds, events around `reps` launches behind a warm-up launch, of
 *   krylov_combine, eig_residual and the finishing launch with nb basis vectors of length len. */
t4a_gpu_status t4a_gpu_lanczos_dense(const double* H, size_t n, const double* v0, const t4a_gpu_lanczos_options* options, double* eigenvalue,
                                     double* eigenvector, size_t* iterations, double* residual_norm, int32_t* converged);
t4a_gpu_status t4a_gpu_krylov_combine(const double* basis, size_t len, size_t nb, const double* coef, double* out, double* norm2);
t4a_gpu_status t4a_gpu_eig_residual(const double* v, const double* hv, size_t len, double lambda, double* r /* may be NULL */,
                                    double* sums3);
t4a_gpu_status t4a_gpu_lanczos_time_finalise(size_t len, size_t nb, size_t reps, double* ms /* [3] */);

/* =====================================================================================
 * Two-site TDVP: a tensor train evolved under an MPO H, exp(tau H) per sweep, resident on the device
 * tensor4all-treetn/src/tdvp/mod.rs (tdvp, tdvp_with_treetn_operator, TdvpOptions, TdvpResult), tdvp/plan.rs (the region plan) on the
 * Hermitian Krylov exponential of tensor4all-core/src/krylov.rs:693-926 (hermitian_krylov_expm_multiply), restated for a chain.
 * Scope: that of t4a_gpu_square_linsolve and t4a_gpu_dmrg — a chain, f64, one site index per node, V_in = V_out.  Trees, index
 * mappings and verbose output are not mirrored.  Deviations from the reference, refused with INVALID_ARGUMENT on the host:
 *   - the exponent is real: exponent_step_re (default -0.1 where the reference has -0.1i) and exponent_step_im, which must be 0:
 *     real-time evolution needs complex trains, which this project does not have.  u' = -H u is what a real exponent covers;
 *   - `center` must be 0 or n - 1: the reference's two-site plan from an inner root of a chain applies a site correction at a leaf
 *     where the projector splitting needs it at the root (relative error 0.17 against exp(tau H) psi at n = 4 from centre 1, 1e-15
 *     from an end); from an end it is the standard 2TDVP sweep;
 *   - nsite = 1 is refused here with a message of its own (nsite outside {1, 2} gets the reference's): one-site TDVP has entry points
 *     of its own, t4a_gpu_tdvp_one_site_plan and t4a_gpu_tdvp_one_site below.
 * `init` is canonicalised onto `center`.  One sweep runs the plan of t4a_gpu_tdvp_plan: two-site steps (theta_0 = x_i x_{i+1}, the
 * Krylov exponential with the step's exponent, an SVD split with max_bond_dim / svd_policy, the singular values into the new centre,
 * no renormalisation) and, between two of them, the site correction with minus the exponent on the shared site.  Where the centre is
 * not in a step's region (the start of the second sweep when order = 1) it is moved there by full-rank thin QR steps.
 * The Krylov solver orthogonalises by two passes of classical Gram-Schmidt (the reference: modified), as GMRES and Lanczos here do.
 * Errors: INVALID_ARGUMENT with the reference's wording for nsweeps == 0, an order outside {1, 2, 4}, a non-finite exponent,
 * max_bond_dim == 0 when set, fewer than two sites, and the Krylov options (max_iter == 0 or above 8191, max_time_splits == 0, a
 * negative or non-finite tolerance); a projected operator that is not Hermitian; INTERNAL_ERROR "hermitian_krylov_expm_multiply did not
 * converge within max_time_splits=.. and max_iter=..". */
typedef struct {
    size_t max_iter;        /* 30 */
    size_t max_time_splits; /* 100 */
    double tol;             /* 1e-12, times max(|start|, 1) */
    double breakdown_tol;   /* 1e-14 */
    double hermitian_tol;   /* 1e-10 */
} t4a_gpu_krylov_expm_options;
typedef struct {
    size_t nsite;   /* 2 */
    size_t nsweeps; /* 1 */
    size_t order;   /* 2: the substeps [1], [1/2, 1/2] or the six of order 4 */
    double exponent_step_re; /* -0.1 */
    double exponent_step_im; /* 0, and nothing else */
    int32_t has_max_bond_dim;
    size_t max_bond_dim;
    int32_t has_svd_policy; /* 0: the default policy of t4a_gpu_tensor_svd */
    t4a_gpu_svd_policy svd_policy;
    t4a_gpu_krylov_expm_options krylov;
} t4a_gpu_tdvp_options;
typedef struct {
    size_t two_site_steps;
    size_t corrections;
    size_t krylov_steps;    /* over all accepted substeps of all local solves */
    size_t apply_calls;     /* projected applies, those of rejected time splits included */
    size_t max_time_splits; /* the largest number of time splits a local solve needed */
} t4a_gpu_tdvp_stats;

t4a_gpu_status t4a_gpu_tdvp_options_default(t4a_gpu_tdvp_options* out);
/* The shape checks of t4a_gpu_tdvp on plain dimension lists (see t4a_gpu_dmrg_check_shapes), the centre rule included; host only. */
t4a_gpu_status t4a_gpu_tdvp_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* state_dims3, size_t n_state, size_t center,
                                         size_t max_iter);
/* The region plan of one sweep (host only): kinds[k] 0 a two-site step, 1 a site correction; nodes[2 k], nodes[2 k + 1] the region
 * in the reference's order (the other node, then the new centre; twice the site for a correction); new_centers[k]; exponents[k].
 * *n_steps receives the number of steps; with the four arrays NULL that is all, else `capacity` must hold it (BUFFER_TOO_SMALL). */
t4a_gpu_status t4a_gpu_tdvp_plan(size_t n, size_t center, size_t order, double tau, size_t capacity, int32_t* kinds, size_t* nodes,
                                 size_t* new_centers, double* exponents, size_t* n_steps);
t4a_gpu_status t4a_gpu_tdvp(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_tdvp_options* options, t4a_gpu_tt** state,
                            size_t* sweeps_completed, size_t* local_updates, double* max_error_estimate, size_t* max_krylov_iterations,
                            t4a_gpu_tdvp_stats* stats /* may be NULL */);
/* Test hook: the solver the sweeps run, out = exp(tau H) v0 for a dense n x n matrix H (column-major) applied on the device. */
t4a_gpu_status t4a_gpu_krylov_expm_dense(const double* H, size_t n, const double* v0, double tau, const t4a_gpu_krylov_expm_options* options,
                                         double* out, size_t* iterations, double* error_estimate, int32_t* converged, size_t* time_splits);

/* ---- one-site TDVP (TdvpOptions::with_nsite(1), tdvp/mod.rs:639-914, tdvp/plan.rs:97-111): every bond dimension stays fixed, a step
 * needs no SVD.  Scope and the real exponent as t4a_gpu_tdvp; ANY centre 0 <= center < n.
 * The plan (t4a_gpu_tdvp_one_site_plan, host only, in the shape of t4a_gpu_tdvp_plan): the nodes in post order from `center` — the left
 * arm leaf first (0 .. c-1), then the right arm leaf first (n-1 .. c+1), then c —, every step of kind 2 (one site) with nodes (node, node),
 * new_center = node and the exponent tau * weight; every even substep (1-based) is the reversed list.
 * The driver: `init` is canonicalised onto `center`; per step the centre moves to the node by full-rank thin QR steps, then the Krylov
 * exponential with the step's exponent on the site tensor.  A bond correction follows iff the next step of the same sweep's plan exists and
 * has another node: the site is factorised towards it by the full-rank thin QR of the centre moves (x = Q C to the right, C Q to the left,
 * k = min(rows, columns)), the Krylov exponential with MINUS the exponent runs on the bond matrix C under
 *   Y[b, b'] = sum_w sum_a sum_a' La[b, w, a] C[a, a'] Rb[b', w, a']
 * (t4a_gpu_tdvp_bond_apply; the environment that contains Q is built once per step), Q stays in the site and C' is absorbed into the
 * neighbour.  No renormalisation.  *local_updates counts site and bond solves: w (2 n - 1) per sweep, w in {1, 2, 6} substeps.
 * Deviations from the reference: (1) the gauge — the reference stores Q C' and factorises it again on the next centre move; the state is
 * the same and the bond dimension is k in both.  (2) At the one jump of a REVERSED substep from an inner centre (from a leaf to the node
 * next to the centre) the reference corrects the first edge of the path, which it has corrected one step earlier, and never the edge into
 * the next node; that is not a projector splitting (a second-order sweep at n = 5 from centre 2 is 5e-2 away from exp(tau H) psi at full
 * bonds).  Here a reversed substep moves the centre to the neighbour of the next node first and corrects the LAST edge of the path, the
 * mirror image of the post-order substep: exact at full bonds from every centre.  Paths of one edge are the reference's.
 * Errors (INVALID_ARGUMENT on the host before an operand is looked at, in this order): nsite != 1 ("tdvp_one_site: one-site TDVP requires
 * nsite=1, got nsite=..; nsite=2 is tdvp"), nsweeps, order and the exponent as t4a_gpu_tdvp, max_bond_dim == 0 when set, "invalid TDVP
 * option max_bond_dim: one-site TDVP has fixed ranks; use nsite=2 for truncation", the same for svd_policy, the Krylov options; then the
 * shapes: lengths differ, a single site (a message of its own), operator sites that are not square or do not match, center >= n, a
 * one-site or bond-centre step with a work buffer above INT_MAX elements (the message names the site or the bond). */
typedef struct {
    size_t one_site_steps;
    size_t bond_corrections;
    size_t qr_steps;        /* full-rank thin QR steps: centre moves and the factorisations of the bond corrections */
    size_t krylov_steps;
    size_t apply_calls;
    size_t max_time_splits;
    size_t fused_applies;   /* bond-centre applies by the fused launch */
    size_t gemm_applies;    /* and by the two GEMMs */
} t4a_gpu_tdvp_one_site_stats;
/* t4a_gpu_tdvp_options_default with nsite = 1 */
t4a_gpu_status t4a_gpu_tdvp_one_site_options_default(t4a_gpu_tdvp_options* out);
t4a_gpu_status t4a_gpu_tdvp_one_site_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* state_dims3, size_t n_state, size_t center,
                                                  size_t max_iter);
t4a_gpu_status t4a_gpu_tdvp_one_site_plan(size_t n, size_t center, size_t order, double tau, size_t capacity, int32_t* kinds, size_t* nodes,
                                          size_t* new_centers, double* exponents, size_t* n_steps);
t4a_gpu_status t4a_gpu_tdvp_one_site(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_tdvp_options* options,
                                     t4a_gpu_tt** state, size_t* sweeps_completed, size_t* local_updates, double* max_error_estimate,
                                     size_t* max_krylov_iterations, t4a_gpu_tdvp_one_site_stats* stats /* may be NULL */);
/* The bond-centre apply on caller-supplied host arrays (column-major): L[ka, W, ka], R[kb, W, kb] (bra bond fastest), C and out ka x kb.
 * route 0: the fused launch (one kernel; a workgroup holds T = La C for 16 rows in the LDS, so W kb <= 512, else INVALID_ARGUMENT),
 * 1: two GEMMs (T = La_view C, Y = T_view Rb_view^T), 2: the rule of the driver.  *route_taken (may be NULL) receives 0 or 1.  The bits of
 * a result depend on the operands, the shape and the route alone.
 * _route: the rule, a function of the shape alone (host only).  _fused_admits: the envelope (host only).  _set_bond_apply_route forces the
 * route of every bond-centre apply of the drivers (0: fused where admitted, 1: GEMM, anything else: the rule).
 * _time (tools/probe_tdvp_one_site.py): device milliseconds, events around `reps` launches behind a warm-up launch, of the fused launch
 * ms[0] (NaN outside its envelope) and the two GEMMs ms[1]. */
t4a_gpu_status t4a_gpu_tdvp_bond_apply(const double* L, const double* R, const double* C, size_t ka, size_t kb, size_t W, int32_t route, double* out,
                                       int32_t* route_taken);
t4a_gpu_status t4a_gpu_tdvp_bond_apply_route(size_t ka, size_t kb, size_t W, int32_t* route);
t4a_gpu_status t4a_gpu_tdvp_bond_apply_fused_admits(size_t ka, size_t kb, size_t W, int32_t* admits);
t4a_gpu_status t4a_gpu_tdvp_set_bond_apply_route(int32_t route);
t4a_gpu_status t4a_gpu_tdvp_bond_apply_time(size_t ka, size_t kb, size_t W, size_t reps, double* ms /* [2] */);

/* ---- global subspace expansion (GSE) and GSE-TDVP: tensor4all-treetn's global_subspace_expand, .._with_references and gse_tdvp
 * (crates/tensor4all-treetn/src/gse.rs) for a chain, f64, one site index per node, V_in = V_out.  The expansion widens every bond of
 * `init` by the directions of the references that it does not span yet and does not change the state.  The target and the references
 * are canonicalised onto `center` (any site); the edges are walked from the leaves to the centre, the left arm first.  Per edge: the
 * old row basis B of the child (thin SVD), the references projected off it and stacked (t4a_gpu_gse_project), the thin SVD of the
 * stack — the host reads its singular values and the trace t = sum |R_j|_F^2 and keeps the right singular vectors with
 * sigma^2 > density_weight_cutoff * t —, and the parents of all trains absorbing the coefficients (t4a_gpu_gse_absorb).
 * Deviations: the SVD of the stack replaces the reference's eigendecomposition of the Hermitianised P rho P / t (the same eigenvalues
 * sigma^2 / t and eigenspaces; the kept rows come in descending order: a permutation of the gauge; hermitian_tol is validated and has
 * nothing else to check); the references of t4a_gpu_gse_krylov_references are built by this project's simplett zip-up
 * (t4a_gpu_mpo_contract, ZipUp, SVD, max_bond_dim = reference_max_bond_dim, the tolerance of reference_svd_policy or 1e-12), not by
 * treetn's apply_linear_operator; more than 8 references are NOT_IMPLEMENTED.
 * Errors (INVALID_ARGUMENT, on the host before the device is touched): "invalid GSE option density_weight_cutoff: must be finite and
 * non-negative", "invalid GSE option hermitian_tol: must be finite and non-negative", "invalid GSE option reference_max_bond_dim: must
 * be greater than zero when set", "GSE center <c> is not a state node", "GSE requires target, references, and operator support to have
 * the same tree topology" (lengths differ), "invalid GSE mapping at node <i>: reference site dimension does not match target";
 * t4a_gpu_gse_tdvp adds the refusals of t4a_gpu_tdvp unchanged (nsite = 1 included: that is t4a_gpu_gse_tdvp_one_site). */
typedef struct {
    size_t krylov_dim;                      /* 0 */
    int32_t has_reference_max_bond_dim;     /* 0: max(link_dims(init)) + 1 */
    size_t reference_max_bond_dim;
    int32_t has_reference_svd_policy;       /* 0: threshold 1e-12 */
    t4a_gpu_svd_policy reference_svd_policy;
    double density_weight_cutoff;           /* 1e-12 */
    double hermitian_tol;                   /* 1e-12 */
    int32_t normalize_references;           /* 1 */
    int32_t expand_before_first_sweep;      /* 1 */
} t4a_gpu_gse_options;
t4a_gpu_status t4a_gpu_gse_options_default(t4a_gpu_gse_options* out);
/* The option and shape checks of the expansion on plain dimension lists (host only): ref_dims3 holds the dims3 of the n_refs
 * references one after the other, ref_lens[j] the number of sites of reference j. */
t4a_gpu_status t4a_gpu_gse_check_shapes(const t4a_gpu_gse_options* options, const size_t* state_dims3, size_t n_state, const size_t* ref_dims3,
                                        const size_t* ref_lens, size_t n_refs, size_t center);
/* build_references: H psi, H^2 psi, .. (krylov_dim of them) into refs[0 .. krylov_dim), which the caller releases. */
t4a_gpu_status t4a_gpu_gse_krylov_references(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, const t4a_gpu_gse_options* options, size_t capacity,
                                             t4a_gpu_tt** refs, size_t* n_refs);
t4a_gpu_status t4a_gpu_gse_expand_with_references(const t4a_gpu_tt* init, const t4a_gpu_tt* const* references, size_t n_refs, size_t center,
                                                  const t4a_gpu_gse_options* options, t4a_gpu_tt** state, size_t* references_built,
                                                  size_t* edges_processed, size_t* bonds_expanded, size_t* max_added_basis);
t4a_gpu_status t4a_gpu_gse_expand(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_gse_options* options, t4a_gpu_tt** state,
                                  size_t* references_built, size_t* edges_processed, size_t* bonds_expanded, size_t* max_added_basis);
/* gse_tdvp: before sweep s an expansion when krylov_dim > 0 and (s > 0 or expand_before_first_sweep), then t4a_gpu_tdvp with nsweeps = 1. */
t4a_gpu_status t4a_gpu_gse_tdvp(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_gse_options* gse,
                                const t4a_gpu_tdvp_options* tdvp, t4a_gpu_tt** state, size_t* sweeps_completed, size_t* local_updates,
                                size_t* gse_expansions, double* max_error_estimate, size_t* max_krylov_iterations);
/* gse_tdvp with t4a_gpu_tdvp_one_site (tdvp->nsite == 1) for the one-sweep evolution after each expansion: the expansion grows the bonds,
 * the fixed-rank integrator evolves inside them.  Any centre.  The refusals of the expansion plus those of t4a_gpu_tdvp_one_site. */
t4a_gpu_status t4a_gpu_gse_tdvp_one_site(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_gse_options* gse,
                                         const t4a_gpu_tdvp_options* tdvp, t4a_gpu_tt** state, size_t* sweeps_completed, size_t* local_updates,
                                         size_t* gse_expansions, double* max_error_estimate, size_t* max_krylov_iterations);
/* Test hooks: the two launches of an edge on raw column-major operands.  orient 0: a matrix over (bond row a, q index j) is na x q,
 * X[a + na j] (the child's first leg is the bond to its parent); orient 1: X[j + q a] (its last leg is).  route 0: the fused launch,
 * 1: the same products composed from the GEMM.
 * _project: refs holds the K references R_j (rho[j] x q) one after the other, B is kb x q; stack receives N_j = R_j - (R_j B^T) B
 * stacked over j as (sum rho) x q in the same orientation, *trace = sum_j |R_j|_F^2.
 * _absorb: children C_j (r[j] x q) and parents one after the other — orient 0: parent j is L[j] x r[j], orient 1: r[j] x L[j], both
 * column-major; Bn is kn x q; out receives parent_j (C_j Bn^T) as L[j] x kn (orient 1: (Bn C_j^T) parent_j as kn x L[j]) one after
 * the other.  At most 8 references / 9 trains; every dimension positive and every matrix within INT_MAX elements. */
t4a_gpu_status t4a_gpu_gse_project(int32_t orient, size_t q, const double* refs, const size_t* rho, size_t K, const double* B, size_t kb,
                                   int32_t route, double* stack, double* trace);
t4a_gpu_status t4a_gpu_gse_absorb(int32_t orient, size_t q, const double* children, const size_t* r, const double* parents, const size_t* L,
                                  size_t n_trains, const double* Bn, size_t kn, int32_t route, double* out);
/* The route the driver takes at an edge with q columns and target bond `bond` (host only): *route = 0 the fused launches (q * bond <=
 * 8192), 1 the GEMM composition.  _set_route forces one route for every edge of every later call (0 or 1; -1: back to the rule): a test
 * hook, so that both routes of the driver run on small trains. */
t4a_gpu_status t4a_gpu_gse_route(size_t q, size_t bond, int32_t* route);
t4a_gpu_status t4a_gpu_gse_set_route(int32_t route);
/* Probe: device ms of project [0] fused [1] GEMMs and absorb [2] fused [3] GEMMs at bond chi, site dimension d, K references of bond chi + 1. */
t4a_gpu_status t4a_gpu_gse_time_routes(size_t chi, size_t d, size_t K, size_t reps, double* ms4);

/* =====================================================================================
 * Partitioned MPOs: the algebra of tensor4all-partitionedtt on device-resident MPOs
 * crates/tensor4all-partitionedtt/src/: projector.rs:39-268, subdomain_tt.rs:171-443 (project, contract), partitioned_tt.rs:104-480
 * (from_subdomains, insert, norm, contract, add, contraction_tasks, to_tensor_train), contract.rs:41-110, error.rs
 * This project's slice: f64 on a chain, sites identified by position, every site an MPO site [left, s1, s2, right] (a train is the
 * case s2 = 1).  The reference's index objects are legs here: a projector key is (site, leg), leg 0 = s1, leg 1 = s2; a projector
 * is `count` triples (site, leg, value) of size_t, and a list of projectors is their triples one after the other plus one count each.
 * In a contraction A·B the shared index is A.(i, 1) == B.(i, 0).  Deviations from the reference: the task order of a contraction is
 * fixed (a-major, insertion order: the reference iterates a hash map), patches keep their insertion order, _to_mpo sorts by
 * (site, leg) then value with a shorter prefix first.  partitionedtreetn, budget_squared and autodiff metadata are out of scope.
 * ===================================================================================== */
/* ---- projector.rs on the host: no device is touched.  Outputs are triples in ascending (site, leg) order; `out` may be NULL to
 * query *out_count (never more than count_a + count_b).  A key given twice keeps its last value (from_pairs :57-63); leg > 1 is
 * INVALID_ARGUMENT. ---- */
/* validate_invariants against the chain site_dims (2 x n_sites: s1, s2 per site).  INVALID_ARGUMENT: "projector index (site <i>, leg
 * <l>) is absent from the chain of <n> sites", "projector coordinate <v> is out of range for index (site <i>, leg <l>) with dimension <d>". */
t4a_gpu_status t4a_gpu_projector_validate(const size_t* site_dims, size_t n_sites, const size_t* p, size_t count);
t4a_gpu_status t4a_gpu_projector_is_compatible(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* out); /* :172 */
/* intersection (:130-145): *compatible = 0 on a conflict (nothing is written then) */
t4a_gpu_status t4a_gpu_projector_intersection(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* compatible,
                                              size_t* out, size_t* out_count);
t4a_gpu_status t4a_gpu_projector_common_restriction(const size_t* a, size_t count_a, const size_t* b, size_t count_b, size_t* out,
                                                    size_t* out_count); /* :157-167 */
t4a_gpu_status t4a_gpu_projector_is_subset_of(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* out); /* :183-194 */
t4a_gpu_status t4a_gpu_projector_are_disjoint(const size_t* entries, const size_t* counts, size_t n_projectors, int32_t* out); /* :199-208 */
/* filter_indices (:214-224): keys is 2 x n_keys (site, leg) */
t4a_gpu_status t4a_gpu_projector_filter(const size_t* p, size_t count, const size_t* keys, size_t n_keys, size_t* out, size_t* out_count);
/* the total order of _to_mpo: entries ascending by (site, leg), then value, compared in turn; a proper prefix comes first.  -1, 0, 1. */
t4a_gpu_status t4a_gpu_projector_compare(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* out);

/* contraction_tasks (partitioned_tt.rs:401-445) from two projector lists, host only: the analogue of t4a_gpu_tdvp_plan.  A pair
 * (i, j) is a task when A_i's leg-1 entries and B_j's leg-0 entries agree at every site that both project; tasks are listed a-major in
 * insertion order.  The result projector of a task is A_i's leg-0 entries plus B_j's leg-1 entries; equal result projectors share one
 * slot, slots are numbered by first appearance.  *n_tasks, *n_results and *n_result_entries are always written; the arrays are
 * written when task_capacity >= *n_tasks and entry_capacity >= *n_result_entries (else INVALID_ARGUMENT unless both capacities are 0:
 * the query).  task_a / task_b / task_result: task_capacity each; result_counts: task_capacity; result_entries: 3 x entry_capacity. */
t4a_gpu_status t4a_gpu_pmpo_contract_plan(const size_t* a_entries, const size_t* a_counts, size_t n_a, const size_t* b_entries,
                                          const size_t* b_counts, size_t n_b, size_t task_capacity, size_t entry_capacity, size_t* n_tasks,
                                          size_t* task_a, size_t* task_b, size_t* task_result, size_t* n_results, size_t* result_counts,
                                          size_t* result_entries, size_t* n_result_entries);
/* The host checks of t4a_gpu_pmpo_new on plain dimension lists: patch_site_dims holds (s1, s2) per site of every patch one after the
 * other, patch_lens[k] the number of sites of patch k. */
t4a_gpu_status t4a_gpu_pmpo_check(const size_t* site_dims, size_t n_sites, const size_t* patch_site_dims, const size_t* patch_lens,
                                  size_t n_patches, const size_t* entries, const size_t* counts);

typedef struct t4a_gpu_pmpo t4a_gpu_pmpo;
/* PartitionedTT::from_subdomains (partitioned_tt.rs:104-110, insert :196-210).  Device copies of the patches are taken, in the order
 * given; they are NOT masked (as in the reference).  site_dims (2 x n_sites) may be NULL when there is a patch: the first patch's.
 * INVALID_ARGUMENT, before the device is touched: "partitioned MPO: patch <k> has <m> sites, the chain has <n>", "partitioned MPO:
 * patch <k> has site dims (<a>, <b>) at site <i>, the chain has (<c>, <d>)", the two messages of _projector_validate, "Projectors
 * overlap: patches <i> and <j> are not disjoint". */
t4a_gpu_status t4a_gpu_pmpo_new(const t4a_gpu_mpo* const* patches, size_t n_patches, const size_t* entries, const size_t* counts,
                                const size_t* site_dims, size_t n_sites, t4a_gpu_pmpo** out);
/* From the result of adaptive_interpolate: cores copied device-to-device and read as (s1, s2) pairs (Mpo::relabel_site_dims);
 * site_dims is 2 x n_sites or NULL for (d, 1).  A projected fused value v becomes (v % S1, v / S1) on the two legs. */
t4a_gpu_status t4a_gpu_pmpo_from_ptt(const t4a_gpu_ptt* ptt, const size_t* site_dims, t4a_gpu_pmpo** out);
void t4a_gpu_pmpo_release(t4a_gpu_pmpo* h);
t4a_gpu_status t4a_gpu_pmpo_len(const t4a_gpu_pmpo* h, size_t* out);
t4a_gpu_status t4a_gpu_pmpo_n_sites(const t4a_gpu_pmpo* h, size_t* out);
t4a_gpu_status t4a_gpu_pmpo_site_dims(const t4a_gpu_pmpo* h, size_t* site_dims /* 2 x n_sites */);
/* projector of patch k as triples; `entries` may be NULL to query *count */
t4a_gpu_status t4a_gpu_pmpo_projector(const t4a_gpu_pmpo* h, size_t k, size_t* count, size_t* entries);
/* patch k as a new MPO handle (a device copy) */
t4a_gpu_status t4a_gpu_pmpo_patch(const t4a_gpu_pmpo* h, size_t k, t4a_gpu_mpo** out);
/* norm (:286-295): sqrt(sum_k norm2(patch k)), norm2 being the tensor train's squared Frobenius norm (t4a_gpu_tt_norm2) */
t4a_gpu_status t4a_gpu_pmpo_norm(t4a_gpu_pmpo* h, double* out);
/* a batch in the layout of t4a_gpu_mpo_evaluate, summed over the patches in their order on the host (no patch: zeros) */
t4a_gpu_status t4a_gpu_pmpo_evaluate(t4a_gpu_pmpo* h, const size_t* idx, size_t n_pts, double* out);
/* SubDomainTT::project (subdomain_tt.rs:171-260) patch by patch: patches whose projector conflicts with p are dropped, the others are
 * copied, carry the intersection and are masked — every site of every patch in ONE launch (pmpo_mask_kernel), which stores 0.0 outside
 * the subdomain and touches nothing inside, so a non-finite value outside disappears (mask_index). */
t4a_gpu_status t4a_gpu_pmpo_project(const t4a_gpu_pmpo* h, const size_t* p, size_t count, t4a_gpu_pmpo** out);
/* add (:356-398): the union of the projectors must be pairwise disjoint ("Incompatible projectors: Projectors must be pairwise disjoint
 * for patch-wise addition"); a patch present on both sides is added by direct sum and truncated by the compress stage of
 * t4a_gpu_mpo_contract (QR to the right, SVD sweep, s >= tolerance * s_max, at most max_bond_dim, at least one); the others are cloned,
 * a's first.  tolerance == 0 with max_bond_dim == 0 keeps every singular value: the sweep is skipped and the direct sum returned. */
t4a_gpu_status t4a_gpu_pmpo_add(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, double tolerance, size_t max_bond_dim, t4a_gpu_pmpo** out);
/* to_tensor_train (:460-480): the direct sum of the patches in the order of t4a_gpu_projector_compare (bonds: sums of the patch bonds).
 * Every site of the result is written by one launch (pmpo_direct_sum_kernel); one site is the plain sum of the values.
 * No patch: INVALID_ARGUMENT "Partitioned tensor train is empty". */
t4a_gpu_status t4a_gpu_pmpo_to_mpo(const t4a_gpu_pmpo* h, t4a_gpu_mpo** out);
/* Test and probe hook: _to_mpo by a given route.  1: the reference's chain of G - 1 pairwise train additions; 2: every site of the
 * result in one launch (pmpo_direct_sum_kernel); 0: what _to_mpo takes (route 2 from two sites and two patches up).  Same bits. */
t4a_gpu_status t4a_gpu_pmpo_to_mpo_route(const t4a_gpu_pmpo* h, int32_t route, t4a_gpu_mpo** out);
/* contract (:305-340).  Arguments, rank rule, NOT_IMPLEMENTED (Fit, RSVD) and shape errors of t4a_gpu_mpo_contract.  Every task of
 * t4a_gpu_pmpo_contract_plan is contracted with both operands projected onto their own projectors (apply_projection); the first result
 * of a slot is inserted, a later one is added to it by direct sum and truncated with the same tolerance and cap — except for Naive
 * with compress == 0 (and for tolerance == 0 without a cap), where the direct sum stays as it is.
 * Naive: the site products of ALL tasks and ALL sites are one launch (pmpo_pair_contract_kernel) with the projection folded in, then
 * the compress stage per task.  ZipUp: copies of the operands are masked in one launch, then the zip-up of t4a_gpu_mpo_contract per
 * task.  INVALID_ARGUMENT besides the shape errors: "Projectors overlap: results <i> and <j> of the contraction are not disjoint" (two
 * result projectors that overlap without being equal, the refusal of PartitionedTT::insert, before the device is touched), a result
 * site above INT_MAX elements with the task and site in the message. */
t4a_gpu_status t4a_gpu_pmpo_contract(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, int32_t algorithm, int32_t compress, int32_t method,
                                     double tolerance, size_t max_bond_dim, t4a_gpu_pmpo** out);
/* Test hook: the product launch exactly as _contract issues it, on host arrays.  dims is 7 x n_jobs (la, s1, k, ra, lb, t, rb), sel
 * 4 x n_jobs (k0, k1, s mask, t mask; a mask < 0 = none), A / B / C the sites [la, s1, k, ra] / [lb, k, t, rb] / [la*lb, s1, t, ra*rb]
 * one after the other.  _mask_sites: the mask launch; dims 4 x n_jobs (l, s1, s2, r), sel 2 x n_jobs (s1 value, s2 value; < 0 = none). */
t4a_gpu_status t4a_gpu_pmpo_pair_products(const size_t* dims, const int64_t* sel, size_t n_jobs, const double* A, const double* B, double* C);
t4a_gpu_status t4a_gpu_pmpo_mask_sites(const size_t* dims, const int64_t* sel, size_t n_jobs, double* X);
/* blocks of 256 threads either launch uses for `total` elements (host only) */
t4a_gpu_status t4a_gpu_pmpo_launch_blocks(size_t total, size_t* blocks);
/* Probe (tools/probe_pmpo.py): wall ms per repetition, each ending synced, of [0] the fused product launch of every task of a·b, [1]
 * the mask launch on copies plus one mpo_site_contract launch per task, [2] the compress stage of every task. */
t4a_gpu_status t4a_gpu_pmpo_time_contract(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, double tolerance, size_t max_bond_dim, size_t reps,
                                          double* ms3);

/* =====================================================================================
 * The compress stage as an operation of its own, and for many MPOs in lock step
 * This project's (the reference reaches compress_mpo, contract_naive.rs:100-172, only through contract_naive).
 * _mpo_compress: the stage of t4a_gpu_mpo_contract on a copy of one MPO: right-canonicalisation by thin QR, then the left-to-right SVD
 * sweep keeping s >= tolerance * s_max, at most max_bond_dim (0 = no cap), at least one; U[:, :rank] stays, diag(S) Vt goes into the
 * next site.  The operand is untouched; fewer than two sites give a copy.
 * _mpo_compress_many: the same result for `count` MPOs of the same number of sites (site dims and bonds may differ), out[k] for mpos[k].
 * An item is inside the ENVELOPE when, after the bound the shapes give (k_n = 1, k_i = min(l_i, s1_i s2_i k_{i+1}) from the right), every
 * bond is at most T4A_GPU_COMPRESS_MANY_BMAX = 64.  route BATCHED sends every item inside the envelope through the batched site-step
 * kernels: one workgroup per item, n - 1 right-step launches and n - 1 left-step launches for the whole call whatever `count` is, no
 * host synchronisation inside a sweep and ONE per call; every other item takes the serial stage of _mpo_compress in the same call.
 * SERIAL takes the serial stage for every item (the bits of _mpo_compress).  AUTO is BATCHED when no bond k_i of the items inside the
 * envelope is above 16 or when at least 16 items are inside it, else SERIAL (the measured rule).  Ranks, the dense
 * operator (to the tolerance) and the left-orthogonality of the sites 0 .. n-2 are those of the serial stage; the gauge (signs,
 * rotations inside degenerate subspaces) is not.  A zero matrix is forced to rank 1 with a unit column in U and a zero right factor.
 * Two calls give the same bits, and an item's bits do not depend on the other items of the call.
 * INVALID_ARGUMENT: count == 0 ("compress_many: the list is empty"), items of different length ("compress_many: item <k> has <a> sites,
 * item 0 has <b>"), an unknown route — all before the device is touched; a non-finite value: "compress_many: item <k>: SVD computation
 * failed: non-finite input" with the lowest such k, and every out[k] stays NULL.  NULL_POINTER: a null list or item.
 * _counted: as _compress_many; counts4 (may be NULL) receives what the driver counted for the batched part — kernel launches, stream
 * synchronisations — and the number of items on the batched and on the serial route.  Outside that count: the call synchronises every
 * operand's own stream before it reads it, and items on the serial stage synchronise as that stage does.
 * RSVD is NOT_IMPLEMENTED up front on every route here (t4a_gpu_pmpo_contract_routed passes a method), also for chains of fewer than
 * two sites, which the serial stage of t4a_gpu_mpo_contract copies without reaching its factorisation; on the BATCHED and AUTO routes
 * of t4a_gpu_pmpo_contract_routed an error of the compress stage reads "compress_many: item <task>: ..." .
 * _plan (host only, no device needed): item k has n_sites[k] sites, dims4 holds (l, s1, s2, r) of all sites of all items one after the
 * other.  batched[count]: 1 = the kernels, 0 = the serial stage; bonds / qr_bonds: n_sites[k] + 1 values per item, the bounds of the
 * result's bonds (k_i, the rank bound min(l s, r) and the cap, from the left) and the bonds after the right sweep (k_i, exact); counts3:
 * launches and synchronisations of the batched part (2 (n - 1) and 1; 0 and 0 when nothing is batched) and the number of batched items.
 * Any output may be NULL.  Refuses what _compress_many refuses, and shapes t4a_gpu_mpo_new refuses ("compress_many: item <k>: ...").
 * What stays serial: zip-up (its SVDs interleave with its products), the add_truncate of partitioned results that share a projector,
 * and items outside the envelope. */
#define T4A_GPU_COMPRESS_AUTO 0
#define T4A_GPU_COMPRESS_BATCHED 1
#define T4A_GPU_COMPRESS_SERIAL 2
#define T4A_GPU_COMPRESS_MANY_BMAX 64
t4a_gpu_status t4a_gpu_mpo_compress(const t4a_gpu_mpo* mpo, double tolerance, size_t max_bond_dim, t4a_gpu_mpo** out);
t4a_gpu_status t4a_gpu_mpo_compress_many(const t4a_gpu_mpo* const* mpos, size_t count, double tolerance, size_t max_bond_dim, int32_t route,
                                         t4a_gpu_mpo** out);
t4a_gpu_status t4a_gpu_mpo_compress_many_counted(const t4a_gpu_mpo* const* mpos, size_t count, double tolerance, size_t max_bond_dim,
                                                 int32_t route, t4a_gpu_mpo** out, size_t* counts4);
t4a_gpu_status t4a_gpu_mpo_compress_many_plan(const size_t* dims4, const size_t* n_sites, size_t count, double tolerance, size_t max_bond_dim,
                                              int32_t route, int32_t* batched, size_t* bonds, size_t* qr_bonds, size_t* counts3);
/* Probe (tools/probe_compress_many.py): wall ms per repetition, each ending synced, of the compress stage on copies of the same chains:
 * ms2[0] item by item on the serial stage, ms2[1] one call on the batched route; the two alternate, one warm-up round of each first. */
t4a_gpu_status t4a_gpu_mpo_time_compress_many(const t4a_gpu_mpo* const* mpos, size_t count, double tolerance, size_t max_bond_dim, size_t reps,
                                              double* ms2);
/* t4a_gpu_pmpo_contract with the route of its compress stage (Naive with compress != 0): SERIAL is t4a_gpu_pmpo_contract, bit for bit;
 * BATCHED and AUTO hand the products of ALL tasks to one _mpo_compress_many call.  ZipUp with BATCHED is INVALID_ARGUMENT.  The
 * add_truncate of results that share a projector is serial on every route.  _time_compress: _mpo_time_compress_many on the task
 * products of a·b. */
t4a_gpu_status t4a_gpu_pmpo_contract_routed(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, int32_t algorithm, int32_t compress, int32_t method,
                                            double tolerance, size_t max_bond_dim, int32_t route, t4a_gpu_pmpo** out);
t4a_gpu_status t4a_gpu_pmpo_time_compress(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, double tolerance, size_t max_bond_dim, size_t reps,
                                          double* ms2);

/* =====================================================================================
 * Budgeted truncation of many MPOs in lock step, and adaptive patching of partitioned MPOs
 * TensorTrain::truncate (itensorlike/src/tensortrain.rs:1180, treetn/truncate.rs:129-198) and
 * crates/tensor4all-partitionedtt/src/patching.rs ("Adaptive Patching for Tensor Train Computations", arXiv:2602.22372), for f64 on
 * a chain with legs (site, leg) in place of index objects.  Out of scope: partitionedtreetn, trees, complex scalars, autodiff
 * metadata.
 * _mpo_truncate_many: out[k] is mpos[k] truncated as TensorTrain::truncate does it — canonicalised onto the last site, then every bond
 * truncated twice, on the way from n - 1 down to 0 and on the way back — under policies[k] (all eight combinations of scale, measure
 * and rule; the rank is t4a_gpu_svd_retained_rank of the singular values, then max_bond_dims[k], 0 = none, then at least one).
 * The envelope, the routes and the determinism are those of _mpo_compress_many, with the shape bound taken from the left (k_0 = 1,
 * k_{i+1} = min(k_i s1_i s2_i, r_{i+1})): the batched part is n - 1 QR-step launches and 2 (n - 1) SVD-step launches whatever `count`
 * is, and ONE host synchronisation; the two directions of the SVD step are mirrored instantiations of one kernel.  Items outside the
 * envelope take a serial stage with the same policy in the same call.  bonds (may be NULL) receives n + 1 values per item.  With
 * ranks_only != 0 the same launches run and `out` (may be NULL) stays NULL: only the bonds come back.
 * INVALID_ARGUMENT as _mpo_compress_many with "truncate_many" in the messages, and for a negative or non-finite threshold or an unknown
 * policy field ("truncate_many: item <k>: ...").
 * _counted: counts4 as _mpo_compress_many_counted.  _plan (host only): as _mpo_compress_many_plan with a cap per item; counts3 =
 * launches (3 (n - 1)), synchronisations (1; 2 with rules_from_norms != 0, the call shape of the patching driver, which reads the norms
 * after the QR sweep to derive the budgets), batched items.
 * _trace (test hook): as _counted with ranks_only, and per item norm2 (the squared Frobenius norm the QR sweep found), ranks
 * (2 (n - 1) per item: the SVD steps in the order they run) and sv (64 values per step: the singular values the step computed,
 * non-increasing, zero-filled). */
t4a_gpu_status t4a_gpu_mpo_truncate_many(const t4a_gpu_mpo* const* mpos, size_t count, const t4a_gpu_svd_policy* policies,
                                         const size_t* max_bond_dims, int32_t route, int32_t ranks_only, t4a_gpu_mpo** out, size_t* bonds);
t4a_gpu_status t4a_gpu_mpo_truncate_many_counted(const t4a_gpu_mpo* const* mpos, size_t count, const t4a_gpu_svd_policy* policies,
                                                 const size_t* max_bond_dims, int32_t route, int32_t ranks_only, t4a_gpu_mpo** out,
                                                 size_t* bonds, size_t* counts4);
t4a_gpu_status t4a_gpu_mpo_truncate_many_plan(const size_t* dims4, const size_t* n_sites, size_t count, const size_t* max_bond_dims,
                                              int32_t route, int32_t rules_from_norms, int32_t* batched, size_t* bonds, size_t* qr_bonds,
                                              size_t* counts3);
t4a_gpu_status t4a_gpu_mpo_truncate_many_trace(const t4a_gpu_mpo* const* mpos, size_t count, const t4a_gpu_svd_policy* policies,
                                               const size_t* max_bond_dims, int32_t route, size_t* bonds, size_t* counts4, double* norm2,
                                               int32_t* ranks, double* sv);
/* PatchingOptions (patching.rs:68-107).  patch_order: n_patch_order pairs (site, leg).  Defaults: rtol 1e-12, max_bond_dim 100,
 * an empty order, EXACT_PARAMETER_GAIN. */
#define T4A_GPU_PATCH_SPLIT_SEQUENTIAL 0
#define T4A_GPU_PATCH_SPLIT_EXACT_PARAMETER_GAIN 1
typedef struct {
    double rtol;
    int32_t has_max_bond_dim;
    size_t max_bond_dim;
    const size_t* patch_order;
    size_t n_patch_order;
    int32_t split_strategy;
} t4a_gpu_patching_options;
/* Host only.  _validate: "rtol must be finite and non-negative", "max_bond_dim must be at least 1", a leg outside the chain,
 * "patch_order cannot contain zero-dimensional indices".  _patch_volume: the product of the dims of the unprojected legs ("subdomain
 * volume overflowed usize").  _patch_budgets: budgets[k] = rtol^2 sum(norm2) volumes[k] / sum(volumes), drop[k] = norm2[k] <=
 * budgets[k]; *empty = 1 (and nothing else written) for no patch or a zero total volume; "partition volume overflowed usize",
 * "partitioned norm is not finite", "rtol produced a non-finite truncation budget".  _split_candidates: the unprojected legs of
 * patch_order, or all legs in chain order when it is empty, duplicates removed; legs holds up to 2 n_sites pairs. */
t4a_gpu_status t4a_gpu_pmpo_validate_patching_options(const t4a_gpu_patching_options* options, const size_t* site_dims, size_t n_sites);
t4a_gpu_status t4a_gpu_pmpo_patch_volume(const size_t* entries, size_t count, const size_t* site_dims, size_t n_sites, size_t* out);
t4a_gpu_status t4a_gpu_pmpo_patch_budgets(const size_t* volumes, const double* norm2, size_t count, double rtol, double* budgets,
                                          int32_t* drop, int32_t* empty);
t4a_gpu_status t4a_gpu_pmpo_split_candidates(const size_t* entries, size_t count, const size_t* site_dims, size_t n_sites,
                                             const t4a_gpu_patching_options* options, size_t* legs, size_t* n_legs);
/* truncate_adaptive (:566-615): every patch masked by its own projector (one launch), budgets from the norms of ONE batched call's QR
 * sweep, patches at or below their budget dropped, the others truncated by the same call's SVD sweeps with Absolute / SquaredValue /
 * DiscardedTailSum at the budget and the cap.  The survivors keep their order and carry budget_squared (_pmpo_budget_squared: *has = 0
 * where unset).  add_with_patching (:154-198): the loop of the reference on the patches of `subdomains`; chosen (may be NULL,
 * 2 * chosen_capacity values) receives the legs of the splits in order, *n_chosen their number.  counts6 (may be NULL): rounds,
 * tensor calls, ranks-only calls, launches and synchronisations of their batched parts, splits. */
t4a_gpu_status t4a_gpu_pmpo_truncate_adaptive(const t4a_gpu_pmpo* p, double rtol, int32_t has_max_bond_dim, size_t max_bond_dim,
                                              int32_t route, t4a_gpu_pmpo** out, size_t* counts6);
/* Probe (tools/probe_patching.py): _pmpo_truncate_adaptive on the BATCHED route with the stream drained after every sweep; ms5 = wall ms
 * of the QR sweep, the first synchronisation with its read of the norms, the leftward sweep, the rightward sweep, the last
 * synchronisation with its read of the ranks.  The result is dropped. */
t4a_gpu_status t4a_gpu_pmpo_truncate_adaptive_timed(const t4a_gpu_pmpo* p, double rtol, int32_t has_max_bond_dim, size_t max_bond_dim,
                                                    double* ms5);
t4a_gpu_status t4a_gpu_pmpo_add_with_patching(const t4a_gpu_pmpo* subdomains, const t4a_gpu_patching_options* options, int32_t route,
                                              t4a_gpu_pmpo** out, size_t* counts6, size_t* chosen, size_t chosen_capacity,
                                              size_t* n_chosen);
/* contract_adaptive (:282-412): the pairwise products of the patches (both sides in the order of t4a_gpu_projector_compare, algorithm /
 * method / tolerance / max_bond_dim as _pmpo_contract with compress on) grouped by result projector; per group the contributions are
 * summed by direct sum and truncated after each addition with the same rank rule; when the sum or a contribution REACHES the cap of
 * `options` the group is split along a leg of the result — (i, 0) is a's s1 leg of site i, (i, 1) b's s2 leg — chosen as in
 * _pmpo_add_with_patching, the operand that has the leg is projected per value (once per projector and value) and truncated with
 * Relative / Value / PerValue at 64 eps, and the group recurses; a final _pmpo_truncate_adaptive runs over everything.  Refusals before
 * the device is touched: the messages of _pmpo_contract for the shapes, those of _pmpo_validate_patching_options on the result's site
 * dims.  counts6 as above (launches and synchronisations of the truncate_many calls; splits = groups split). */
t4a_gpu_status t4a_gpu_pmpo_contract_adaptive(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, int32_t algorithm, int32_t method, double tolerance,
                                              size_t max_bond_dim, const t4a_gpu_patching_options* options, int32_t route, t4a_gpu_pmpo** out,
                                              size_t* counts6);
t4a_gpu_status t4a_gpu_pmpo_budget_squared(const t4a_gpu_pmpo* p, size_t k, int32_t* has, double* value);

/* =====================================================================================
 * swap_site_indices on a chain: which site holds which site index
 * tensor4all-treetn/src/treetn/swap.rs (SwapOptions, ScheduledSwapStep, SwapSchedule::build), treetn/mod.rs (swap_on_edge,
 * swap_site_indices), for f64 and by position.
 * A leg train is a tensor train over fused site indices plus, per site, an ordered list of legs (key, dim): keys are unique across
 * the train and ordered as int64, the first leg of a site is the fastest in its fused index, a site may hold no leg or several.
 * Legs travel as leg_counts[n_sites] and the keys / dims of all sites one after the other.
 * LEG ORDER WRITTEN BY A STEP: on both sites of a step the legs are stored in ascending key order; sites that no step touches keep
 * their order (this project's rule; the reference has index objects and no positional order).
 * ===================================================================================== */
typedef struct t4a_gpu_swap_schedule t4a_gpu_swap_schedule;
#define T4A_GPU_SWAP_PASSES_DIAMETER ((size_t)-1)
#define T4A_GPU_SWAP_ROUTE_SCALAR 1 /* a tile of the step kernel summed per thread */
#define T4A_GPU_SWAP_ROUTE_MFMA 2   /* a tile on the f64 matrix cores */
/* SwapSchedule::build on a chain of n_sites; host only, usable with no device.  current / target: (key, site) pairs; the base sweep
 * starts at root (for root 0: the edges (i, i+1) rightwards, then (i+1, i) leftwards), at most max_passes passes
 * (T4A_GPU_SWAP_PASSES_DIAMETER: n_sites - 1, as the reference), a step only where a targeted leg crosses.  INVALID_ARGUMENT with the
 * reference's messages: "root .. not in topology", "target_assignment contains index .. which is not in the network", "target node ..
 * is not in the topology", "did not converge within {n} passes".
 * cur_dims (may be NULL; one per current leg) adds the plan checks, still before any device is touched: a step whose merged pair
 * holds more than 8 legs, a step either of whose sides exceeds the fused-dimension limit 65535 and, with link_dims (may be NULL;
 * n_sites - 1 bonds), a work matrix above INT_MAX elements (max_bond_dim: 0 = none). */
t4a_gpu_status t4a_gpu_swap_schedule_build(size_t n_sites, const int64_t* cur_keys, const size_t* cur_sites, const size_t* cur_dims,
                                           size_t n_current, const int64_t* target_keys, const size_t* target_sites, size_t n_target,
                                           size_t root, size_t max_passes, const size_t* link_dims, size_t max_bond_dim,
                                           t4a_gpu_swap_schedule** out);
void t4a_gpu_swap_schedule_release(t4a_gpu_swap_schedule* schedule);
t4a_gpu_status t4a_gpu_swap_schedule_len(const t4a_gpu_swap_schedule* schedule, size_t* n_steps);
/* sizes[3]: the lengths of transport_path, a_side and b_side of a step; _step reads it out (node_ab[2] = node_a, node_b; the sides in
 * ascending key order — they are sets). */
t4a_gpu_status t4a_gpu_swap_schedule_step_sizes(const t4a_gpu_swap_schedule* schedule, size_t step, size_t* sizes);
t4a_gpu_status t4a_gpu_swap_schedule_step(const t4a_gpu_swap_schedule* schedule, size_t step, size_t* transport_path, size_t* node_ab,
                                          int64_t* a_side, int64_t* b_side);
/* swap_site_indices: a new train with every targeted leg on its target site.  An empty target or an empty schedule: *out is a copy,
 * the legs as given, *moved = 0 and no canonicalisation (as in the reference).  Otherwise QR canonicalisation around site 0, then per
 * step the exact QR transport of the centre, the step kernel, the truncated SVD (threshold = rtol, or 0 for has_rtol == 0 — never a
 * global default —, Relative / Value / PerValue; max_bond_dim when has_max_bond_dim) and the split with node_a's site the isometry and
 * node_b's carrying S; *center = node_b of the last step.  out_keys / out_dims hold as many legs as came in.  ms3 (may be NULL): device
 * ms of the step kernel, the SVD with the split, and the QR steps (tools/probe_swap.py). */
t4a_gpu_status t4a_gpu_tt_swap_site_indices(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                            const int64_t* target_keys, const size_t* target_sites, size_t n_target,
                                            int32_t has_max_bond_dim, size_t max_bond_dim, int32_t has_rtol, double rtol, t4a_gpu_tt** out,
                                            size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, int32_t* moved, size_t* center,
                                            size_t* n_steps, double* ms3);
/* Test hook, the counterpart of t4a_gpu_mpo_partial_half: the step kernel exactly as a step launches it on the host cores
 * left[l, X, m] and right[m, Y, r] (chain order; X, Y the products of the leg dims).  to_left / to_right: the keys that end on the
 * left / the right site, stored there in ascending order.  out: Theta' with M = l |left'| rows and N = |right'| r columns,
 * column-major, row = l_idx + l xa', column = xb' + |right'| r_idx; mn[2] = (M, N); *route = the T4A_GPU_SWAP_ROUTE_* bits taken. */
t4a_gpu_status t4a_gpu_swap_theta(const double* left, size_t l, size_t m, const double* right, size_t r, const int64_t* left_keys,
                                  const size_t* left_dims, size_t n_left, const int64_t* right_keys, const size_t* right_dims,
                                  size_t n_right, const int64_t* to_left, size_t n_to_left, const int64_t* to_right, size_t n_to_right,
                                  double* out, size_t* mn, int32_t* route);
/* Probe (tools/probe_swap.py): device ms per launch over `reps` launches, binary legs exchanged at l = m = r = bond, of [0] the step
 * kernel and [1] the composition from existing pieces: GEMM, then one permutation launch. */
t4a_gpu_status t4a_gpu_swap_theta_time(size_t bond, size_t reps, double* ms2);
/* The legs of the named sites in another order, in place, one gather launch over all of them.  order_counts[n_named] keys per named
 * site, each a permutation of the site's keys; leg_counts / keys / dims describe the train and are rewritten. */
t4a_gpu_status t4a_gpu_legtrain_reorder(t4a_gpu_tt* tt, const size_t* leg_counts, int64_t* keys, size_t* dims, const size_t* sites,
                                        const size_t* order_counts, const int64_t* order_keys, size_t n_named);

/* ---- fuse_to, split_to and restructure_to on a chain (tensor4all-treetn: treetn/transform.rs, treetn/restructure/mod.rs,
 * options.rs: SplitOptions, RestructureOptions), f64, by position.  The train is described as for swap_site_indices (leg_counts / keys /
 * dims: per site its legs, first leg fastest).  The target is an ordered list of n_groups groups of keys (group_counts[n_groups],
 * group_keys): group j is site j of the result and the order of its keys the leg order of that site, first key fastest.  Refused
 * before the device is touched: an empty group, a key in two groups, a key set that differs from the train's. */
#define T4A_GPU_RESTRUCTURE_FUSE_ONLY 0
#define T4A_GPU_RESTRUCTURE_SWAP_THEN_FUSE 1
#define T4A_GPU_RESTRUCTURE_SPLIT_ONLY 2
#define T4A_GPU_RESTRUCTURE_SWAP_ONLY 3
#define T4A_GPU_RESTRUCTURE_SPLIT_THEN_FUSE 4
#define T4A_GPU_FUSE_MAX_LEGS 16
#define T4A_GPU_FUSE_ROUTE_SCALAR 1
#define T4A_GPU_FUSE_ROUTE_MFMA 2
/* The plan, host only (no device is needed).  op 0: restructure_to — *kind receives the T4A_GPU_RESTRUCTURE_* kind, chosen with the
 * precedence of build_plan; op 1: fuse_to and op 2: split_to with their own conditions and messages (*kind = FUSE_ONLY / SPLIT_ONLY).
 * link_dims (n_sites - 1 bonds, may be NULL) adds the check that no core of a fuse exceeds INT_MAX elements.  out_leg_counts (n_groups
 * entries) / out_keys / out_dims (as many legs as came in): the legs of the result.  counts4: [0] the rounds of the fuse phase
 * (k_max - 1), [1] its launches (the rounds plus one when a group of one site is reordered; for op 2 the reorder launch of the split),
 * [2] the QR factorisations of the split phase, [3] the entries of the swap target written to swap_keys / swap_sites (capacity: the
 * number of legs; may be NULL when not wanted). */
t4a_gpu_status t4a_gpu_restructure_plan(int32_t op, size_t n_sites, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                        const size_t* link_dims, size_t n_groups, const size_t* group_counts, const int64_t* group_keys,
                                        int32_t* kind, size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, size_t* counts4,
                                        int64_t* swap_keys, size_t* swap_sites);
/* fuse_to: a new train of n_groups sites, exact.  Every site's legs lie in one group, the sites of a group are contiguous, groups
 * ascend; sites without legs are absorbed as in the reference.  All groups are contracted in lock step, left to right: k_max - 1
 * launches of one kernel for a largest group of k_max sites, the last round of a group writing its legs in the target's order; a group
 * of one site in another order costs one reorder launch.  center: the train's centre or -1; *out_center the group that holds it or -1.
 * _counted also reports the launches. */
t4a_gpu_status t4a_gpu_tt_fuse_to(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims, int64_t center,
                                  size_t n_groups, const size_t* group_counts, const int64_t* group_keys, t4a_gpu_tt** out,
                                  size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, int64_t* out_center);
t4a_gpu_status t4a_gpu_tt_fuse_to_counted(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                          int64_t center, size_t n_groups, const size_t* group_counts, const int64_t* group_keys,
                                          t4a_gpu_tt** out, size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims,
                                          int64_t* out_center, size_t* launches);
/* split_to: every group's legs lie on one site, the groups of a site are consecutive and sites ascend.  Phase 1 (exact): one reorder
 * launch, then fragment after fragment peeled from the left by the thin QR with the rank rule of t4a_gpu_qr_retained_rank at rtol 0.
 * form: 0 unitary (1 LU, 2 CI: NOT_IMPLEMENTED).  final_sweep != 0: TensorTrain::truncate by the serial stage of
 * t4a_gpu_mpo_truncate_many with `policy` (NULL: the default policy) and max_bond_dim.  The result has no centre.  *n_qr (may be NULL):
 * the QR factorisations. */
t4a_gpu_status t4a_gpu_tt_split_to(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims, size_t n_groups,
                                   const size_t* group_counts, const int64_t* group_keys, int32_t form, const t4a_gpu_svd_policy* policy,
                                   int32_t has_max_bond_dim, size_t max_bond_dim, int32_t final_sweep, t4a_gpu_tt** out,
                                   size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, size_t* n_qr);
/* restructure_to: plan (t4a_gpu_restructure_plan, op 0), then the phases of the kind with the split options (as t4a_gpu_tt_split_to), the
 * swap options (as t4a_gpu_tt_swap_site_indices) and, when final_policy is not NULL, a final truncation as above with final_policy and
 * final_max_bond_dim (0: no cap).  counts3 (may be NULL): launches of the fuse and reorder kernels, QR factorisations, swap steps. */
t4a_gpu_status t4a_gpu_tt_restructure_to(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                         int64_t center, size_t n_groups, const size_t* group_counts, const int64_t* group_keys,
                                         int32_t split_form, const t4a_gpu_svd_policy* split_policy, int32_t split_has_max_bond_dim,
                                         size_t split_max_bond_dim, int32_t split_final_sweep, int32_t swap_has_max_bond_dim,
                                         size_t swap_max_bond_dim, int32_t swap_has_rtol, double swap_rtol,
                                         const t4a_gpu_svd_policy* final_policy, size_t final_max_bond_dim, t4a_gpu_tt** out,
                                         size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, int32_t* kind, int64_t* out_center,
                                         size_t* counts3);
/* Test hook, the counterpart of t4a_gpu_swap_theta: ONE launch of the fuse kernel over n_jobs jobs on host cores.  Job k: shapes5[5 k ..]
 * = (l, X, m, Y, r), A[l, X, m] and B[m, Y, r] concatenated in a / b; leg_counts[k] legs of the result site with their dims in chain
 * order (leg_dims) and, per leg of the result in its new order, its position in chain order (leg_order); leg_counts[k] == 0: chain
 * order.  out: the results [l, X Y, r] concatenated; routes[k]: the T4A_GPU_FUSE_ROUTE_* bits of job k. */
t4a_gpu_status t4a_gpu_fuse_round(size_t n_jobs, const double* a, const double* b, const size_t* shapes5, const size_t* leg_counts,
                                  const size_t* leg_dims, const size_t* leg_order, double* out, int32_t* routes);
/* Probe (tools/probe_restructure.py): device ms per repetition of fusing n_groups pairs of binary-leg sites with every bond equal to
 * `bond`: [0] the one lock-step launch, [1] one t4a_gpu_swap_theta kernel launch per pair, issued group by group. */
t4a_gpu_status t4a_gpu_fuse_time(size_t n_groups, size_t bond, size_t reps, double* ms2);

/* =====================================================================================
 * Variational sum of many tensor trains or MPOs resident on the device: fit_sum
 * tensor4all-treetn/src/treetn/fit.rs:1521-1644 (fit_sum, SumFitUpdater :1140-1337, fit_two_site_update :648-771, run_fit_sweeps
 * :1076-1113), restated for a chain, f64, by position; an MPO enters over its fused site index s1 + S1 s2.  Trees, complex scalars and
 * the QR, LU and CI factorisations are not mirrored (a valid request for one of the three: NOT_IMPLEMENTED naming it).
 * One result C is swept two sites at a time against the environments <C|T_k> of every target, the local optimum of a bond being
 * Theta = sum_k L_k T_k[i] T_k[i+1] R_k; the sum T_1 + .. + T_K with its bond sum_k chi_k is never formed.  The environments of all
 * targets at a bond are one matrix with the targets' bonds concatenated: a bond step is two half launches (one kernel launch each for
 * all targets), Theta = P Q as one GEMM over the concatenated index, the SVD split and one GEMM for the environment left behind.
 * `initial` (NULL: a clone of targets[0], this project's extension) gives the length, the site dimensions and the starting bonds; it is
 * canonicalised onto `center` by forced thin-QR sweeps, every environment towards the centre is built, and each full sweep is the Euler
 * tour bonds center .. n-2 to the right, n-2 .. 0 to the left, 0 .. center-1 to the right, the second node of a step the new centre.
 * The split is Canonical::Left: the first node of the step takes the orthonormal factor, the second S Vt, by the policy of
 * t4a_gpu_tensor_svd (none: its default).  The bond cap is max_bond_dim when given, else none when svd_policy or qr_rtol is given, else
 * THE PRESENT DIMENSION OF THAT BOND: with no option set the ranks never grow.  With has_convergence_tol the sweeps stop after a sweep
 * with |exp(log|psi|_after - log|psi|_before) - 1| < convergence_tol (*converged = 1); else exactly nfullsweeps sweeps run.
 * nfullsweeps == 0 returns a clone of the initial after validation; one site returns the elementwise sum of the targets' tensors.
 * coefficients (NULL: all ones; this project's extension): one finite real per target, sum_k w_k T_k, applied once by scaling a copy of
 * site 0 of a target whose weight is not 1.
 * route: T4A_GPU_FIT_SUM_AUTO, _FUSED (the one launch per half) or _GEMM (the same halves from one GEMM per target for P and one per
 * target and site index for Q).  On integer operands the routes give equal integers; on real operands not necessarily equal bits.
 * INVALID_ARGUMENT with a message, before an operand is looked at: "convergence tolerance must be finite and non-negative", "QR
 * relative tolerance must be finite and non-negative", max_bond_dim == 0 when set, an invalid svd_policy, "SVD factorization does not
 * accept qr_rtol" (FactorizeOptions::validate; QR with svd_policy, LU/CI with either likewise), an unknown route; then "fit_sum: targets
 * must not be empty", an empty initial, "fit_sum: center node is not in initial TreeTN", per target "fit_sum: target i has an
 * incompatible named topology" (another length) and "fit_sum: target i site-space validation failed" (another site dimension), a
 * coefficient that is not finite, and a work matrix of a bond step (P, Q, Theta, an environment) above INT_MAX elements.
 * ===================================================================================== */
#define T4A_GPU_FIT_SUM_AUTO 0
#define T4A_GPU_FIT_SUM_FUSED 1
#define T4A_GPU_FIT_SUM_GEMM 2
typedef struct {
    size_t nfullsweeps;
    int32_t has_max_bond_dim; /* 0 <=> None */
    size_t max_bond_dim;
    int32_t has_svd_policy;   /* 0 <=> None: the default policy of t4a_gpu_tensor_svd */
    t4a_gpu_svd_policy svd_policy;
    int32_t has_qr_rtol;      /* 0 <=> None */
    double qr_rtol;
    int32_t factorize_alg;    /* 0 SVD, 1 QR, 2 LU, 3 CI */
    int32_t has_convergence_tol;
    double convergence_tol;
} t4a_gpu_fit_sum_options;
/* FitOptions::new(1): 1, None, None, None, SVD, None */
t4a_gpu_status t4a_gpu_fit_sum_options_default(t4a_gpu_fit_sum_options* out);
/* The checks of t4a_gpu_tt_fit_sum on plain dimension lists, a pure host function: options (may be NULL: not checked), then the shapes.
 * target_dims3: (left, site, right) per site of every target, one target after the other; target_lens: sites per target.
 * has_initial == 0: the first target stands in for the initial. */
t4a_gpu_status t4a_gpu_fit_sum_check_shapes(const size_t* target_dims3, const size_t* target_lens, size_t n_targets, int32_t has_initial,
                                            const size_t* initial_dims3, size_t n_initial, size_t center,
                                            const t4a_gpu_fit_sum_options* options);
/* norms (may be NULL): room for nfullsweeps doubles, |psi| after each completed sweep */
t4a_gpu_status t4a_gpu_tt_fit_sum(const t4a_gpu_tt* const* targets, size_t n_targets, const double* coefficients /* may be NULL */,
                                  const t4a_gpu_tt* initial /* may be NULL */, size_t center, const t4a_gpu_fit_sum_options* options,
                                  int32_t route, t4a_gpu_tt** out, size_t* sweeps_completed, size_t* local_updates, int32_t* converged,
                                  double* norms);
/* the same for MPOs; every target must have the (s1, s2) pairs of the initial */
t4a_gpu_status t4a_gpu_mpo_fit_sum(const t4a_gpu_mpo* const* targets, size_t n_targets, const double* coefficients /* may be NULL */,
                                   const t4a_gpu_mpo* initial /* may be NULL */, size_t center, const t4a_gpu_fit_sum_options* options,
                                   int32_t route, t4a_gpu_mpo** out, size_t* sweeps_completed, size_t* local_updates, int32_t* converged,
                                   double* norms);
/* Test hook: one half for K targets on raw column-major host operands, route _FUSED or _GEMM.  cores: T_k[a_k, S, b_k] one after the
 * other; right == 0: env is EL (chi x sum a_k), out P (chi S) x (sum b_k), block k at column sum_{j<k} b_j:
 *   P[c + chi (s + S (off_k + b))] = sum_a EL[c, offL_k + a] T_k[a, s, b];
 * right != 0: env is ER (sum b_k x chi), out Q (sum a_k) x (S chi), block k at row sum_{j<k} a_j:
 *   Q[(off_k + a) + A (s + S c)] = sum_b T_k[a, s, b] ER[offR_k + b, c].
 * has_fill != 0: the output buffer and 64 guard doubles behind it hold `fill` before the launch, and `out` (room for 64 more doubles)
 * receives the guard behind the result. */
t4a_gpu_status t4a_gpu_fit_sum_half(int32_t right, int32_t route, const double* env, size_t chi, size_t S, const double* cores,
                                    const size_t* a, const size_t* b, size_t K, int32_t has_fill, double fill, double* out);
/* Host only: the route T4A_GPU_FIT_SUM_AUTO takes for a half with n_targets targets whose largest bond is target_bond. */
t4a_gpu_status t4a_gpu_fit_sum_route(size_t n_targets, size_t target_bond, size_t result_bond, size_t site_dim, int32_t* route);
/* Host only: out6 = bond steps per sweep, then per bond step half launches, GEMMs and SVDs, then half launches and GEMMs of the
 * preparation, for a chain of n_sites sites of dimension site_dim on route _FUSED or _GEMM. */
t4a_gpu_status t4a_gpu_fit_sum_plan(size_t n_sites, size_t center, size_t n_targets, size_t site_dim, int32_t route, size_t* out6);
/* Probe (tools/probe_fit_sum.py): device ms per repetition (events around `reps` launches behind a warm-up) of one half for K targets
 * of bond `bond`, site dimension S and result bond chi: [0] the fused launch, [1] the GEMM composition. */
t4a_gpu_status t4a_gpu_fit_sum_time_half(int32_t right, size_t K, size_t bond, size_t S, size_t chi, size_t reps, double* ms2);

/* ---- an operator applied on a subset of a state's sites (csrc/linop.hpp; tensor4all-treetn/src/operator/: apply.rs, compose.rs,
 * identity.rs, on a chain and by position).  The operator is an MPO of k >= 1 sites O_j[a, y, x, a'] (leg 0 the output, leg 1 the
 * input), `sites` its k strictly ascending state positions.  A state site is an operator site (kind 0), a bridge between two operator
 * sites that carries the operator bond through unchanged (kind 1), or outside the operator's span (kind 2).  Result bonds are fused
 * with the operator index slow and the state index fast.  Refusals (INVALID_ARGUMENT, all before the device is touched): `sites` not
 * strictly ascending, "Operator nodes [..] are not a subset of state nodes [..]", "Shared shape mismatch at site i: operator has input
 * dim p, the state has site dim q", a fused bond above 65535, a core of more than INT_MAX elements. */
#define T4A_GPU_LINOP_NAIVE 0
#define T4A_GPU_LINOP_ZIPUP 1
#define T4A_GPU_LINOP_FIT 2
#define T4A_GPU_LINOP_ROUTE_AUTO 0
#define T4A_GPU_LINOP_ROUTE_FUSED 1    /* the kernels of csrc/kernels_apply.hip: no identity is materialised */
#define T4A_GPU_LINOP_ROUTE_COMPOSED 2 /* t4a_gpu_linop_extend, then the MPO-MPO contraction */
typedef struct {
    int32_t method;           /* T4A_GPU_LINOP_NAIVE / _ZIPUP / _FIT; naive ignores everything below */
    double tolerance;         /* the SVD rank rule of the MPO contraction: values below tolerance * s_max are dropped */
    int32_t has_max_bond_dim; /* 0 <=> None */
    size_t max_bond_dim;
    size_t nfullsweeps;       /* fit */
    int32_t has_convergence_tol; /* fit; 0 <=> None: every sweep runs */
    double convergence_tol;
} t4a_gpu_linop_options;
/* ApplyOptions::default(): zip-up, 1e-12, None, 1, None */
t4a_gpu_status t4a_gpu_linop_options_default(t4a_gpu_linop_options* out);
/* Host only.  op_dims4: (left, s1, s2, right) per operator site; state_dims3: (left, site, right) per state site.  Outputs (each may be
 * NULL), one entry per state site: kinds; bonds: the operator bond (left, right) of the site; result_dims3. */
t4a_gpu_status t4a_gpu_linop_plan(const size_t* op_dims4, size_t n_op, const size_t* sites, size_t n_sites, const size_t* state_dims3,
                                  size_t n_state, int32_t* kinds, size_t* bonds, size_t* result_dims3);
/* initial (may be NULL): the start of the fit, a train with the result's site dims; NULL is the zip-up with the same tolerance and cap.
 * n_sweeps, norms (room for nfullsweeps + 1 doubles: the start, then one per sweep), route_taken may be NULL. */
t4a_gpu_status t4a_gpu_linop_apply(const t4a_gpu_mpo* op, const size_t* sites, size_t n_sites, const t4a_gpu_tt* state,
                                   const t4a_gpu_linop_options* options, int32_t route, const t4a_gpu_tt* initial, t4a_gpu_tt** out,
                                   size_t* n_sweeps, double* norms, int32_t* route_taken);
/* extend_operator_to_full_space: operator sites are device copies, bridge sites delta_{aa'} delta_{yx} of shape [m, d, d, m], outside
 * sites [1, d, d, 1] identities. */
t4a_gpu_status t4a_gpu_linop_extend(const t4a_gpu_mpo* op, const size_t* sites, size_t n_sites, const size_t* state_site_dims, size_t n_state,
                                    t4a_gpu_mpo** out);
/* are_exclusive_operators, host only.  sites: the positions of every operator one after the other; lens: positions per operator. */
t4a_gpu_status t4a_gpu_linop_exclusive(size_t n_state, const size_t* sites, const size_t* lens, size_t n_ops, int32_t* exclusive);
/* compose_exclusive_linear_operators: the full-length operator, gaps identities with bond 1.  INVALID_ARGUMENT "... Operators are not
 * exclusive: they may overlap or not form connected subtrees". */
t4a_gpu_status t4a_gpu_linop_compose(const size_t* state_site_dims, size_t n_state, const t4a_gpu_mpo* const* ops, const size_t* sites,
                                     const size_t* lens, size_t n_ops, t4a_gpu_mpo** out);
/* Test hook: the half product of a gap site on host buffers, launched exactly as the drivers launch it (column-major throughout).
 * right == 0: env is L[n_env, m, lb], x is X[lb, d, rb], out P[n_env, d, m, rb] = sum_b L[n, a, b] X[b, x, c];
 * right != 0: env is R[m, rb, n_env], out Q[m, lb, d, n_env] = sum_c X[b, x, c] R[a, c, n].
 * has_fill != 0: the output buffer and 64 guard doubles behind it hold `fill` before the launch and `out` has room for 64 more doubles,
 * which receive the guard. */
t4a_gpu_status t4a_gpu_linop_gap_half(int32_t right, const double* env, size_t n_env, size_t m, const double* x, size_t lb, size_t d,
                                      size_t rb, int32_t has_fill, double fill, double* out);
/* Host only: the route T4A_GPU_LINOP_ROUTE_AUTO takes. */
t4a_gpu_status t4a_gpu_linop_route(int32_t method, size_t n_state, size_t n_gap_sites, size_t state_bond, size_t op_bond, int32_t* route);
/* Probe (tools/probe_linop.py): device ms per repetition (events around `reps` launches behind a warm-up) of the left half of a bridge
 * site with operator bond m, site dim d, state bonds lb x rb and n_env environment rows: [0] apply_gap_half_kernel, [1] the half kernel
 * of the partial contraction on the materialised bridge site. */
t4a_gpu_status t4a_gpu_linop_time_half(size_t n_env, size_t m, size_t lb, size_t d, size_t rb, size_t reps, double* ms2);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* T4A_GPU_H */
