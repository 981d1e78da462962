// contraction.hpp — device-resident mirror of tensor4all-simplett's Contraction<f64> (crates/tensor4all-simplett/src/mpo/
// contraction.rs:60-383): the lazy product of two MPOs.  Single elements and left / right environments of A·B are computed
// without ever forming the product with bonds la*lb.  The environment walks run in the kernels of kernels_contraction.hip, the
// pairing of a left with a right environment is tt_env_dot (kernels_tt.hip) over la*lb entries; unique halves and the split are
// host integer work shared with TensorTrain::evaluate_many (tt.hpp).  A whole candidate matrix (evaluate_matrix) skips that host
// work: packed halves up, two environment launches, contraction_pair_launch, the result left in device memory — which makes the
// object a MatrixSource (matrix_source.hpp) of a TensorCI2.
//
// Differences from the reference, none of them visible in a result:
//  * the reference memoises environments in hash maps across calls; here nothing is kept between calls — a batch call computes
//    every unique half of ITS points once.  clear_cache() exists for API parity and does nothing.
//  * the transform function of Contraction::with_transform (contraction.rs:118-125) is applied by the language binding on the
//    host to the returned values (a C function pointer per element would be the slowest part of a batch); it is not part of
//    this class.
#pragma once

#include <mutex>

#include "matrix_source.hpp"
#include "mpo.hpp"

namespace t4a {

class MpoContraction : public MatrixSource {
public:
    // Contraction::new (contraction.rs:69-110): lengths and the shared dimension a.s2 == b.s1 of every site are checked before
    // any device work, with the wording of mpo_contract.  The object keeps device copies of both operands (the reference takes
    // them by value): the caller's MPOs may be released afterwards.
    MpoContraction(Mpo& a, Mpo& b);
    ~MpoContraction() override;

    size_t len() const { return n_; }
    std::vector<std::array<size_t, 2>> result_site_dims() const; // (s1_a, s2_b) per site (contraction.rs:142-147)
    std::vector<size_t> fused_local_dims() const;                 // s1_a * s2_b per site: the index i + s1_a * j
    void clear_cache() {}                                         // contraction.rs:150-153: nothing is cached here

    // idx: 2 len x n_pts column-major, [i_0, j_0, i_1, j_1, ...] per point.
    // evaluate (contraction.rs:187-252): the left-to-right walk of every point.
    void evaluate(const uint32_t* idx, size_t n_pts, double* out);
    // evaluate_left(n, .) / evaluate_right(n, .) (contraction.rs:262-383): out holds n_pts column-major matrices of dims2 =
    // (rows, cols): ra x rb behind site n-1 / la x lb in front of site n; [[1]] for n == 0 / n == len.
    void evaluate_left(size_t n, const uint32_t* idx, size_t n_pts, double* out, size_t dims2[2]);
    void evaluate_right(size_t n, const uint32_t* idx, size_t n_pts, double* out, size_t dims2[2]);
    std::array<size_t, 2> left_dims(size_t n) const;
    std::array<size_t, 2> right_dims(size_t n) const;
    // The batch evaluation in the manner of TTCache::evaluate_many (cache.rs:558-744): unique left halves of `split` sites and
    // unique right halves, two environment launches, one pairing launch, one download.  split == 0: find_split_heuristic.
    // Returns the split that was used.
    size_t evaluate_many(const uint32_t* idx, size_t n_pts, size_t split, double* out);
    // the same for the fused site index f = i + s1_a * j (n_sites x n_pts column-major): the batch callback of a TensorCI2
    void evaluate_fused(const uint32_t* fidx, size_t n_sites, size_t n_pts, double* out);

    // A candidate matrix of a cross interpolation of A·B, left in device memory: rows are n_rows index halves over sites [0, cut)
    // (2 cut values each, [i, j] per site, item-major, host memory), cols n_cols halves over sites [cut, len);
    // d_out[r + ld * c] = (A·B)(rows[r] + cols[c]), with `transposed` d_out[c + ld * r].  cut may be 0 or len: that side's
    // environment is [[1]].  Two environment launches (launch_left / launch_right: one workgroup per half, LDS or global scratch as
    // in evaluate_many) and contraction_pair_launch over K = la * lb at the cut — no per-point index buffer, no unique map (the
    // halves of a candidate matrix are distinct by construction; equal halves are simply computed twice), nothing downloaded.  The
    // bits of an entry depend on its row half and its column half only, not on the request it is part of.
    // The work runs on this object's stream behind what `consumer` holds at the call, and `consumer` is made to wait for it (two
    // events; consumer == nullptr: this object's own stream, no events).  The host waits only for the previous call's upload of
    // index halves out of the pinned staging buffer it is about to overwrite.  The checks and messages are evaluate_many's; a cut
    // beyond len is "Invalid split position".  Counts n_rows * n_cols evaluations.
    void evaluate_matrix(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, double* d_out, size_t ld,
                         bool transposed, hipStream_t consumer);
    // the same into host memory, n_rows x n_cols column-major: evaluate_matrix and one download
    void evaluate_matrix_host(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, double* out);

    // MatrixSource: the function of a TensorCI2 over the fused site index f = i + s1_a * j.  fill_matrix decodes the digits on the
    // host (n_rows * cut + n_cols * (len - cut) integers) and is evaluate_matrix; eval_points is evaluate_fused.
    std::vector<size_t> source_local_dims() const override { return fused_local_dims(); }
    void fill_matrix(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, double* d_out, size_t ld,
                     bool transposed, hipStream_t consumer) override;
    void eval_points(const uint32_t* idx, size_t n_sites, size_t n_pts, double* out) override { evaluate_fused(idx, n_sites, n_pts, out); }

    // points evaluated by evaluate / evaluate_many / evaluate_fused / evaluate_matrix so far
    size_t n_evaluated()
    {
        std::lock_guard<std::mutex> lock(mu_);
        return n_evaluated_;
    }

private:
    struct Site {
        size_t la, s1, k, ra, lb, s2, rb;
    };
    void validate_indices(const uint32_t* idx, size_t n_pts, size_t first, size_t last) const; // contraction.rs:158-175
    void upload_descs();
    // environment kernels over sites [0, n) / [n, len): n_items packed index halves in device memory -> d_out (n_items x ld)
    void launch_left(size_t n, const uint32_t* d_idx, size_t n_items, double* d_out, size_t ld);
    void launch_right(size_t n, const uint32_t* d_idx, size_t n_items, double* d_out, size_t ld);
    double* working_set(size_t n_items, int& env_cap, int& t_cap, int& blocks, size_t first, size_t last, bool left);
    void environments(bool left, size_t n, const uint32_t* idx, size_t n_pts, double* out);
    // validate_indices for packed halves: n_items x 2 (last - first) values of sites [first, last)
    void validate_halves(const uint32_t* packed, size_t n_items, size_t first, size_t last) const;
    void matrix_locked(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, bool fused, double* d_out,
                       size_t ld, bool transposed, hipStream_t consumer);

    std::mutex mu_; // every entry point: the callback route may call from several host threads
    size_t n_ = 0;
    std::vector<Site> sites_;
    std::unique_ptr<Mpo> a_, b_;
    Engine* eng_ = nullptr; // a_'s engine: this object's own stream
    bool descs_uploaded_ = false;
    size_t n_evaluated_ = 0;
    DevBuf<ContractionSiteDesc> d_desc_;
    DevBuf<uint32_t> d_idx_, d_il_, d_ir_;
    DevBuf<double> d_vals_, d_envl_, d_envr_, d_scratch_l_, d_scratch_r_;
    // evaluate_matrix: pinned staging of the index halves, the event behind their upload, the two events that order a consumer
    PinBuf<uint32_t> h_halves_;
    PinBuf<double> h_vals_; // evaluate_matrix_host: the download lands here
    hipEvent_t ev_upload_ = nullptr, ev_consumer_ = nullptr, ev_done_ = nullptr;
    bool upload_pending_ = false;
};

// contract by cross interpolation (this project's; the model is TensorCrossInterpolation.jl's `algorithm = :TCI` contraction):
// a TensorCI2 over the fused local dims s1_a * s2_b whose function is MpoContraction::evaluate_fused, then to_tensor_train and an
// MPO with site dims (s1_a, s2_b).  info: [termination code, rank, function evaluations, last error estimate].
// device_source: the contraction is the TensorCI2's matrix source (Tci2::set_source) — candidate matrices are filled on the device by
// evaluate_matrix, everything else goes through evaluate_fused as before.
struct TCI2Options;
std::unique_ptr<Mpo> mpo_contract_tci(Mpo& a, Mpo& b, const TCI2Options& options, std::vector<std::vector<uint32_t>> initial_pivots,
                                      double info[4], bool device_source = false);

} // namespace t4a
