// quanticstransform.hpp — the real-valued operators of tensor4all-quanticstransform as MPOs
// (crates/tensor4all-quanticstransform/src/: shift.rs:49-291, flip.rs:44-249, cumsum.rs:76-346, common.rs:549-654,
//  affine.rs:497-553, :673-711, :1386-1834, difference_kernel.rs:29-107).
// Construction is integer bookkeeping (every entry is 0, +-1 or a small count) and runs on the host without a device: a
// QtOperator holds the site tensors in the layout of mpo.hpp, column-major [left, s1 = out, s2 = in, right], site 0 the most
// significant bit.  qt_upload is the one copy to the device; everything numerical after it is the MPO code of mpo.hip.
// Complex-valued operators of the crate (quantics_fourier_operator, phase_rotation_operator*) are outside this f64 backend.
#pragma once

#include <cstdint>

#include "mpo.hpp"

namespace t4a {

enum class BoundaryCondition : int { Periodic = 0, AntiPeriodic = 1, Open = 2 }; // common.rs BoundaryCondition
enum class TriangleType : int { Lower = 0, Upper = 1 };                          // cumsum.rs TriangleType

struct QtOperator {
    std::vector<std::array<size_t, 4>> dims; // (left, s1, s2, right) per site
    std::vector<std::vector<double>> sites;  // column-major site tensors
    size_t len() const { return dims.size(); }
};

// |x> -> |x + offset>: (M g)[x] = g[x - offset] (shift.rs:122-291).  1 <= r <= 63.
QtOperator qt_shift(size_t r, int64_t offset, BoundaryCondition bc);
// |x> -> |2^r - x>; x = 0 carries the boundary weight 1 / -1 / 0 (flip.rs:129-249).  r >= 2.
QtOperator qt_flip(size_t r, BoundaryCondition bc);
// M[i, j] = [i > j] (Lower, the cumulative sum) or [i < j] (Upper) (cumsum.rs:142-346).  r >= 2.
QtOperator qt_triangle(size_t r, TriangleType triangle);
// embed_single_var_mpo (common.rs:573-654): `op` on variable target_var, identity on the others; site index var0 + 2 var1 + ...
QtOperator qt_embed(const QtOperator& op, size_t nvariables, size_t target_var);
// affine_transform_tensors (affine.rs:1386-1629) of y = (a x + b) / scale: a is m x n column-major, all three cleared of
// denominators (to_integer_scaled, :497-523); bc has one entry per output variable.  int64 with checked arithmetic where the
// reference uses BigInt: an overflow is INVALID_ARGUMENT.  Bits of b at and above 2^r join the carry out of site 0 before the
// boundary weight is taken (for Open the reference's extension loop, :1445-1523; for AntiPeriodic what affine_transform_matrix
// says, :820-934).
QtOperator qt_affine(size_t r, const std::vector<int64_t>& a, const std::vector<int64_t>& b, int64_t scale, size_t m, size_t n,
                     const std::vector<BoundaryCondition>& bc);
// s1 <-> s2 of every site on the host (the device counterpart is Mpo::transpose)
QtOperator qt_transpose(const QtOperator& op);

// the one upload (needs a device)
std::unique_ptr<Mpo> qt_upload(const QtOperator& op);
// difference_kernel_mpo (difference_kernel.rs:29-107): A[x, x'] = f(x - x') from a binary train f that stays on the device;
// bonds delta_bond * f_bond with left = dl * f_left + fl.  One launch of the naive MPO site contraction.
std::unique_ptr<Mpo> qt_difference_kernel(TensorTrain& f, BoundaryCondition bc);

} // namespace t4a
