// dense.hpp — the dense routines behind the handle-less C-ABI entry points, on device memory: triangular solve, LU solve,
// randomised SVD, the square factors of the full-pivot LU and the two candidate-matrix sources of the rook LUCI.
// Every routine works on the engine's stream with column-major device matrices; locking, caller memory and status codes
// stay with the entry points (capi.hip).
#pragma once

#include "rook.hpp"

namespace t4a {

// op(A) X = B (left_side) or X op(A) = B with the triangular na x na matrix at dA and the bm x bn matrix at dB, X in place of B.
// dA and dB are the first halves of buffers of 2 na^2 + 1 and 2 bm bn + 1 doubles: the second halves take the transposes.
void trsm(Engine& e, double* dA, size_t na, double* dB, size_t bm, size_t bn, bool left_side, bool lower, bool transpose_a,
          bool unit_diagonal);

// A X = B by partial-pivot LU, X in place of B (n x nrhs); A (n x n) is overwritten by its factors.
// Throws SINGULAR_MATRIX for an exactly zero pivot.
void solve(Engine& e, double* dA, size_t n, double* dB, size_t nrhs);

// Randomised SVD at sketch width l: range finder with power iterations, then the SVD of the small projected matrix.  The caller
// reserves the buffers and fills A (m x n) and omega (n x l, rsvd_sketch); afterwards U is m x l, S holds l values and Vt is l x n.
struct RsvdBuffers {
    DevBuf<double> A, omega, Y, Q, R, Z, B, Ub, S, Vt, U;
    void reserve(size_t m, size_t n, size_t l);
};
std::vector<double> rsvd_sketch(size_t n, size_t l, uint64_t seed); // n x l standard normals by Box-Muller on the library's StdRng stream
void rsvd(Engine& e, RsvdBuffers& w, size_t m, size_t n, size_t l, size_t power_iters);

// The square factors of the full-pivot LU that luci(..., want_lu_copy = true) left in lu_buf(), of an n x n matrix:
// L = [lower trapezoid of the first rank columns | identity columns] at the returned pointer (in d_tmp), U = [first rank rows ; 0]
// n * n doubles behind it.
double* full_piv_lu_factors(Engine& e, const LuciResult& r, size_t n);

// Rook sources.  Device matrix: A (m x n) at d_a; its transpose (rows contiguous) is formed at d_at.  With T4A_ROOK_HOST set
// (read once per process) the source offers no `full` matrix, which keeps the search on the host-driven path.
RookSource rook_source_device(Engine& e, const double* d_a, double* d_at, size_t m, size_t n);
// Host callback: one full column or row per call, staged through pageable memory.
RookSource rook_source_blocks(Engine& e, size_t m, size_t n, t4a_gpu_fill_block_fn fill_block, void* ctx);

} // namespace t4a
