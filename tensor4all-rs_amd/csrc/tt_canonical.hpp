// tt_canonical.hpp — the gauge forms of tensor4all-simplett on the device: SiteTensorTrain / center_canonicalize
// (crates/tensor4all-simplett/src/canonical.rs:118-393, :439-544), VidalTensorTrain (vidal.rs:215-493) and InverseTensorTrain
// (vidal.rs:551-767).  The MPO-side forms (SiteMPO::move_center_*, VidalMPO::from_mpo, InverseMPO::from_mpo) are stubs in the
// reference and are not mirrored.
//
// The reference's `qr_decomp` is NOT a QR: it is rrlu(matrix, {max_bond_dim: min(m, n), rel_tol: 0, abs_tol: 0, left_orthogonal:
// true}) followed by lu.left(true) / lu.right(true) (canonical.rs:17-29, vidal.rs:22-33).  The "orthogonal" cores of these forms are
// therefore unit-lower-trapezoidal LU factors, and the Vidal "singular values" are those of the LU-gauged bond matrices, not the
// Schmidt values of the tensor.  This file restates that algorithm; it does not repair it.
#pragma once

#include <memory>
#include <vector>

#include "tt.hpp"

namespace t4a {

// Work buffers of the gauge steps.  Buffers a step replaces are parked in `retired` until the stream has been synchronised.
struct GaugeScratch {
    DevBuf<double> mat, fac, u, vt;
    std::vector<DevBuf<double>> retired;
};

// make_left_orthogonal (canonical.rs:191-241): core i <- left(true) of the rrLU of its left matrix, core i + 1 <- right(true) * next.
void gauge_left_step(Engine& eng, std::vector<DevCore>& cores, size_t i, GaugeScratch& w);
// make_right_orthogonal (canonical.rs:244-291): lq_decomp literally — the rrLU runs on the TRANSPOSE of the right matrix (rows
// s * R + r), both factors are transposed back; core i - 1 <- prev * L.
void gauge_right_step(Engine& eng, std::vector<DevCore>& cores, size_t i, GaugeScratch& w);
// center_canonicalize(tensors, center) (canonical.rs:439-544), in place; a silent no-op for n <= 1 or center >= n as there.
void center_canonicalize(TensorTrain& tt, size_t center);

// replaces `dst` by the host tensor (l, s, r); the old buffer is parked in w.retired
void replace_core(Engine& eng, DevCore& dst, const size_t dims[3], const double* host, GaugeScratch& w);

class SiteTrain { // SiteTensorTrain<f64> (canonical.rs:102-393)
public:
    // SiteTensorTrain::new (canonical.rs:118-143): copies the cores, then canonicalises around `center`
    SiteTrain(const std::vector<DevCore>& src, hipStream_t src_stream, size_t center);
    static void check_new(size_t n, size_t center); // the argument errors of new(), before the device is touched

    size_t len() const { return cores.size(); }
    size_t center() const { return center_; }
    void move_center_right();
    void move_center_left();
    void set_center(size_t new_center);
    void set_site_tensor(size_t i, const size_t dims[3], const double* host);
    void set_two_site_tensors(size_t i, const size_t d1[3], const double* t1, const size_t d2[3], const double* t2);

    std::vector<DevCore> cores;
    Engine eng;

private:
    size_t center_ = 0;
    GaugeScratch w_;
};

class VidalTrain { // VidalTensorTrain<f64> (vidal.rs:199-493)
public:
    VidalTrain() = default; // the empty object (n == 0): holds no device resources
    // from_tensor_train_with_partition (vidal.rs:229-395)
    VidalTrain(const std::vector<DevCore>& src, hipStream_t src_stream, size_t start, size_t end);
    // new(tensors, singular_values) (vidal.rs:403-428) from host data
    VidalTrain(const std::vector<std::array<size_t, 3>>& dims3, const double* cores_host, const std::vector<size_t>& sv_lens,
               const double* svs_host);
    static void check_partition(size_t n, size_t end);
    static void check_new(size_t n, size_t n_svs);

    size_t len() const { return cores.size(); }
    std::vector<double> singular_values_host(size_t bond);
    void set_singular_values(size_t bond, const double* host, size_t len);
    void set_site_tensor(size_t i, const size_t dims[3], const double* host);
    std::vector<DevCore> to_tensor_train_cores(); // vidal.rs:456-492 (valid on the stream of `eng`)

    std::vector<DevCore> cores;
    std::vector<DevBuf<double>> sv; // n - 1 vectors on the device
    std::vector<size_t> sv_len;
    size_t part_start = 0, part_end = 0;
    std::unique_ptr<Engine> eng; // null for the empty object

private:
    GaugeScratch w_;
};

class InverseTrain { // InverseTensorTrain<f64> (vidal.rs:535-767)
public:
    explicit InverseTrain(VidalTrain& vidal); // from_vidal (vidal.rs:551-663)

    size_t len() const { return cores.size(); }
    std::vector<double> inverse_singular_values_host(size_t bond);
    void set_two_site_tensors(size_t i, const size_t d1[3], const double* t1, const double* inv_sv, size_t inv_len, const size_t d2[3],
                              const double* t2);
    std::vector<DevCore> to_tensor_train_cores(); // vidal.rs:730-766

    std::vector<DevCore> cores;
    std::vector<DevBuf<double>> inv; // n - 1 vectors on the device
    std::vector<size_t> inv_len;
    size_t part_start = 0, part_end = 0;
    std::unique_ptr<Engine> eng;

private:
    GaugeScratch w_;
};

} // namespace t4a
