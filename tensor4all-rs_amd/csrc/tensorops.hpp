// tensorops.hpp — dense part of the dynamic-index tensor layer of tensor4all-core on the gfx950 engine:
// unfold_split (defaults/idx_tensor.rs:5278-5345), contract_pair for dense operands (defaults/contract.rs:334-343 with
// prepare_contraction, index_ops.rs:660-696), svd_with (defaults/svd.rs:255-395) and qr_with (defaults/qr.rs:206-328)
// with the reference's rank rules, factorize (defaults/factorize.rs:86-834) over SVD, QR, LU and CI.  Indices are integer
// labels; prime levels, tags, structured storage and AD stay with the caller.  Permutations run as one gather kernel,
// contractions on the f64-MFMA GEMM, factorisations on the Jacobi SVD / Householder QR of kernels_linalg.hip and the rrLU kernels.
#pragma once

#include "engine.hpp"
#include "tt_chain.hpp"

#include <algorithm>

namespace t4a {

constexpr int TENSOR_MAX_RANK = PERMUTE_MAX_RANK;

struct SvdPolicy { // truncation.rs:137-147; default relative / per value / 1e-12 (svd.rs:80-87)
    double threshold = 1e-12;
    int scale = 0;   // 0 Relative, 1 Absolute
    int measure = 0; // 0 Value, 1 SquaredValue
    int rule = 0;    // 0 PerValue, 1 DiscardedTailSum
};

// host-side rank rules (no device needed)
size_t svd_retained_rank(const double* s, size_t n, const SvdPolicy& policy);   // svd.rs:150-211
size_t qr_retained_rank(const double* r, size_t k, size_t n, double rtol);      // qr.rs:74-117, r is k x n column-major

struct TensorView {
    const double* d_data; // device, column-major
    std::vector<size_t> dims;
    std::vector<int64_t> labels;
    size_t size() const
    {
        size_t n = 1;
        for (size_t d : dims) n *= d;
        return n;
    }
};

// out index k takes input index perm[k]; d_out must hold t.size() doubles
void tensor_permute(Engine& e, const TensorView& t, const std::vector<size_t>& perm, double* d_out);

struct ContractPlan {
    std::vector<size_t> perm_a, perm_b;
    size_t M = 1, K = 1, N = 1;
    std::vector<size_t> out_dims;
    std::vector<int64_t> out_labels;
};
ContractPlan plan_contract_pair(const TensorView& a, const TensorView& b);
// d_out: M x N doubles = the result tensor [free a.., free b..]; uses e.d_tmp / e.d_tmp2 as permutation scratch
void tensor_contract_pair(Engine& e, const TensorView& a, const TensorView& b, const ContractPlan& plan, double* d_out);

// What the operations on one or two labelled tensors refuse (index_ops.rs, defaults/contract.rs).  Host only: their callers look before
// they take a device.
void require_distinct_labels(const TensorView& t);                            // "duplicate index in tensor"
std::vector<size_t> plan_permute(const TensorView& t, const int64_t* labels); // out axis k takes the axis labelled labels[k]
size_t plan_relabel(const TensorView& t, int64_t from, int64_t to);           // the axis that takes the new label
ContractPlan plan_outer_product(const TensorView& a, const TensorView& b);    // operands without a common label: M x 1 times 1 x N
// tensordot (prepare_contraction_pairs, index_ops.rs): pair p contracts the axis of `a` labelled labels_a[p] with the axis of `b` labelled
// labels_b[p]: every pair names one axis of each operand, no axis twice, equal dimensions; a label the operands have in common that is not
// paired would be a batch contraction (not implemented in the reference either).  The paired axes of `b` take the labels of their partners.
ContractPlan plan_tensordot(const TensorView& a, TensorView& b, const int64_t* labels_a, const int64_t* labels_b, size_t n_pairs);

// N-ary contraction of a connected tensor network (defaults/contract.rs:283-298 contract / contract_with_options, plan :885-941,
// connectivity :1167-1230): every label that occurs in more than one operand is summed unless it is retained; the result carries the
// labels that occur once, or are retained, in order of first appearance (operands in order, axes in order).  Errors like the
// reference's: no operands, a retained label that no operand has, operands that fall into several connected components (a retained
// label connects its holders), a label with two different dimensions.  The network is reduced pair by pair — at every step the
// connected pair with the smallest result — each step one (batched) GEMM on the f64 matrix cores: a shared label that another
// operand or the result still needs stays as a batch axis of that step (the reference hands the whole network to tenferro's einsum;
// summation order is the backend's there as here: values agree to rounding).
struct OwnedTensor {
    DevBuf<double> buf;
    std::vector<size_t> dims;
    std::vector<int64_t> labels;
    OwnedTensor() = default;
    OwnedTensor(const std::vector<size_t>& d, const std::vector<int64_t>& l) : dims(d), labels(l) { buf.reserve(std::max<size_t>(size(), 1)); }
    size_t size() const { return view().size(); }
    TensorView view() const { return TensorView{buf.get(), dims, labels}; }
};
struct NetworkPlan {
    std::vector<int64_t> out_labels;
    std::vector<size_t> out_dims;
};
NetworkPlan plan_contract_network(const std::vector<TensorView>& ts, const std::vector<int64_t>& retain); // validation + result indices (host only)
OwnedTensor tensor_contract_network(Engine& e, const std::vector<TensorView>& ts, const std::vector<int64_t>& retain);

// simplett_bridge.rs on a chain; in each direction a host-only check or plan, then the device step.
// To tensors (tensor_train_to_treetn, :706-794): n site labels and n - 1 bond labels, all distinct; one tensor per core with legs
// [bond s-1, site s, bond s], boundary legs dropped.  `src` is the engine the cores were written on.
void require_distinct_chain_labels(const int64_t* site_labels, const int64_t* bond_labels, size_t n);
std::vector<OwnedTensor> chain_to_tensors(Engine& e, Engine& src, const std::vector<DevCore>& cores, const int64_t* site_labels, const int64_t* bond_labels);
// Back (treetn_to_tensor_train, :172-277): neighbours share exactly one label, no other pair shares any, and every node has one more leg,
// its site index; legs in any order.  Per site the permutation into [l, s, r] and that shape.
struct ChainPlan {
    std::vector<std::vector<size_t>> perm;
    std::vector<std::array<size_t, 3>> dims;
};
ChainPlan plan_tensors_to_chain(const std::vector<TensorView>& tensors);
std::vector<DevCore> tensors_to_chain(Engine& e, const std::vector<TensorView>& tensors, const ChainPlan& plan);

struct UnfoldPlan {
    std::vector<size_t> perm;
    std::vector<size_t> left_dims, right_dims;
    std::vector<int64_t> left_labels, right_labels;
    size_t m = 1, n = 1;
};
UnfoldPlan plan_unfold_split(const TensorView& t, const std::vector<int64_t>& left);
// a factor of an unfolding, allocated: the legs of one side followed (bond_first: preceded) by a bond of dimension r
OwnedTensor bonded_tensor(std::vector<size_t> dims, std::vector<int64_t> labels, size_t r, int64_t bond, bool bond_first = false);

// What the factorisations below refuse needs no device to be found, and their callers look before they take one, in this order: the
// options' values (validate(): INVALID_ARGUMENT; svd/tests/mod.rs:120-160: before any linear algebra), then require_factorizable: an empty
// tensor (INVALID_ARGUMENT, "<empty_what> of an empty tensor") and an unfolding beyond Engine::FACTOR_DIM_MAX (NOT_IMPLEMENTED, "<op>: unfolded ...").
void require_factorizable(const UnfoldPlan& un, const char* op, const char* empty_what);
// They unfold into the second half of e.pi(2 * count), count = t.size(): the first half is free for a caller that has to bring the tensor
// to the device first, and a view into it stays valid through the call.
inline double* tensor_staging(Engine& e, size_t count) { return e.pi(2 * count); }

struct SvdOptions { // SvdOptions (svd.rs:80-87) with the truncating / full-rank choice of svd_with
    bool truncate = true;
    SvdPolicy policy;
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    void validate() const;
};
struct QrOptions {
    bool truncate = true;
    double rtol = 1e-15; // default_qr_rtol (qr.rs:62-66)
    void validate() const;
};
struct UnfoldedFactors { // of the m x n unfolding, k = min(m, n), the leading `keep` columns of left / rows of right retained; pointers into e.d_tmp
    size_t m, n, k, keep;
    const double* d_left;  // U or Q: m x k, leading dimension m
    const double* d_right; // V^T or R: k x n, leading dimension k
    const double* d_s;     // SVD only: k singular values ...
    std::vector<double> s; // ... and their host copy
};
UnfoldedFactors tensor_svd(Engine& e, const TensorView& t, const UnfoldPlan& un, const SvdOptions& o); // svd.rs:255-395
UnfoldedFactors tensor_qr(Engine& e, const TensorView& t, const UnfoldPlan& un, const QrOptions& o);   // qr.rs:206-328

struct FactorizeOptions {
    int alg = 0;       // 0 SVD, 1 QR, 2 LU, 3 CI
    int canonical = 0; // 0 Left: the left factor is the isometry and the right one takes S (SVD) / the pivot block; 1 Right
    SvdOptions svd;    // truncate and max_bond_dim also bound LU and CI
    QrOptions qr;
    void validate() const; // the chosen algorithm's values only
};
struct FactorizeResult {
    OwnedTensor left, right; // [left.., bond], [bond, right..]
    size_t rank = 0;
    std::vector<double> singular_values; // the retained ones; SVD only
};
FactorizeResult tensor_factorize(Engine& e, const TensorView& t, const UnfoldPlan& un, const FactorizeOptions& o, int64_t bond_label);

// out[i + ldo*j] = in[i + ldi*j] * (by_row ? s[i] : s[j])   (S absorbed into a factor, factorize.rs:519-557)
void diag_scale_launch(const double* in, int ldi, int rows, int cols, const double* s, bool by_row, double* out, int ldo,
                       hipStream_t stream);

} // namespace t4a
