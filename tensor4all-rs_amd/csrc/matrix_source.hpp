// matrix_source.hpp — a function source of a TensorCI2 that fills candidate matrices in device memory itself (Tci2::set_source).
// The driver hands over the two index sets of a matrix as they are stored (one fused digit per site, host memory) and the place
// the matrix belongs; nothing of the matrix passes through the host.  Everything that is not a matrix (global pivot search, the
// first pivot, error estimates, a sharded candidate matrix, rook rows and columns) goes through eval_points.
// MpoContraction (contraction.hpp) is the first implementation.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

namespace t4a {

class MatrixSource {
public:
    virtual ~MatrixSource() = default;
    // the index space: one local dimension per site
    virtual std::vector<size_t> source_local_dims() const = 0;
    // rows: n_rows x cut digits of sites [0, cut), cols: n_cols x (len - cut) digits of sites [cut, len), both item-major in host
    // memory and free to be reused when the call returns.  d_out[r + ld * c] = f(rows[r] + cols[c]), with `transposed`
    // d_out[c + ld * r].  The result is ordered behind what `consumer` held when the call was made and in front of what is enqueued
    // on it afterwards; the call does not wait for the device beyond what handing over the digits needs.
    virtual void fill_matrix(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, double* d_out, size_t ld,
                             bool transposed, hipStream_t consumer) = 0;
    // idx: n_sites x n_pts column-major digits -> out[n_pts] in host memory (the contract of t4a_gpu_batch_eval_fn, errors thrown)
    virtual void eval_points(const uint32_t* idx, size_t n_sites, size_t n_pts, double* out) = 0;
};

} // namespace t4a
