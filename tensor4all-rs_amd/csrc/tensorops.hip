// tensorops.hip — see tensorops.hpp.
#include "tensorops.hpp"

#include <memory>

#include <algorithm>
#include <cmath>

namespace t4a {

size_t svd_retained_rank(const double* s, size_t n, const SvdPolicy& p)
{
    if (n == 0) return 1;
    std::vector<double> m(n);
    bool all_zero = true;
    for (size_t k = 0; k < n; ++k) {
        m[k] = p.measure == 0 ? s[k] : s[k] * s[k];
        if (m[k] != 0.0) all_zero = false;
    }
    if (all_zero) return 1;
    size_t keep = 0;
    if (p.rule == 0) {
        if (p.scale == 0) {
            double ref = 0.0;
            for (double v : m) ref = std::max(ref, v);
            while (keep < n && ref > 0.0 && m[keep] / ref > p.threshold) ++keep;
        } else {
            while (keep < n && m[keep] > p.threshold) ++keep;
        }
    } else {
        double total = 0.0;
        for (double v : m) total += v;
        if (p.scale == 0 && total == 0.0) return 1;
        double discarded = 0.0;
        keep = n;
        for (size_t i = n; i-- > 0;) {
            const bool ok = p.scale == 0 ? (discarded + m[i]) / total <= p.threshold : discarded + m[i] <= p.threshold;
            if (!ok) break;
            discarded += m[i];
            keep = i;
        }
    }
    return std::max<size_t>(keep, 1);
}

size_t qr_retained_rank(const double* r, size_t k, size_t n, double rtol)
{
    if (k == 0 || n == 0) return 1;
    const size_t md = std::min(k, n);
    std::vector<double> norms(md);
    double mx = 0.0;
    for (size_t i = 0; i < md; ++i) {
        double sq = 0.0;
        for (size_t j = i; j < n; ++j) {
            const double v = std::fabs(r[i + j * k]);
            sq += v * v;
        }
        norms[i] = std::sqrt(sq);
        mx = std::max(mx, norms[i]);
    }
    if (mx == 0.0) return 1;
    const double thr = rtol * mx;
    size_t cnt = 0;
    for (double v : norms)
        if (v >= thr) ++cnt;
    return std::max<size_t>(cnt, 1);
}

namespace {

__global__ void __launch_bounds__(256) diag_scale_kernel(const double* __restrict__ in, int ldi, int rows, int cols,
                                                         const double* __restrict__ s, int by_row, double* __restrict__ out, int ldo)
{
    const size_t total = (size_t)rows * cols;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e % (size_t)rows), j = (int)(e / (size_t)rows);
        out[i + (size_t)ldo * j] = in[i + (size_t)ldi * j] * (by_row ? s[i] : s[j]);
    }
}

void validate(const TensorView& t, const char* who)
{
    if (t.dims.size() != t.labels.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": dims / labels length mismatch");
    if (t.dims.size() > (size_t)TENSOR_MAX_RANK)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, std::string(who) + ": tensors of rank above " + std::to_string(TENSOR_MAX_RANK) + " are not supported");
    for (size_t a = 0; a < t.labels.size(); ++a)
        for (size_t b = a + 1; b < t.labels.size(); ++b)
            if (t.labels[a] == t.labels[b]) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": duplicate index in tensor");
}

} // namespace

void tensor_permute(Engine& e, const TensorView& t, const std::vector<size_t>& perm, double* d_out)
{
    const size_t r = t.dims.size();
    const size_t total = t.size();
    if (total == 0) return;
    bool identity = true;
    for (size_t k = 0; k < r; ++k) identity = identity && perm[k] == k;
    if (identity) {
        T4A_HIP(hipMemcpyAsync(d_out, t.d_data, total * sizeof(double), hipMemcpyDeviceToDevice, e.stream()));
        return;
    }
    permute_launch(t.d_data, t.dims.data(), perm.data(), (int)r, d_out, e.stream());
    T4A_HIP(hipGetLastError());
}

ContractPlan plan_contract_pair(const TensorView& a, const TensorView& b) // index_ops.rs:660-696
{
    validate(a, "contract_pair lhs");
    validate(b, "contract_pair rhs");
    std::vector<size_t> axes_a, axes_b;
    for (size_t i = 0; i < a.labels.size(); ++i)
        for (size_t j = 0; j < b.labels.size(); ++j)
            if (a.labels[i] == b.labels[j]) {
                if (a.dims[i] != b.dims[j])
                    throw Error(T4A_GPU_INVALID_ARGUMENT, "contraction dimension mismatch: lhs axis " + std::to_string(i) + " has " +
                                                              std::to_string(a.dims[i]) + ", rhs axis " + std::to_string(j) + " has " +
                                                              std::to_string(b.dims[j]));
                axes_a.push_back(i);
                axes_b.push_back(j);
            }
    ContractPlan p;
    for (size_t i = 0; i < a.labels.size(); ++i)
        if (std::find(axes_a.begin(), axes_a.end(), i) == axes_a.end()) {
            p.perm_a.push_back(i);
            p.M *= a.dims[i];
            p.out_dims.push_back(a.dims[i]);
            p.out_labels.push_back(a.labels[i]);
        }
    for (size_t i : axes_a) {
        p.perm_a.push_back(i);
        p.K *= a.dims[i];
    }
    for (size_t j : axes_b) p.perm_b.push_back(j);
    for (size_t j = 0; j < b.labels.size(); ++j)
        if (std::find(axes_b.begin(), axes_b.end(), j) == axes_b.end()) {
            p.perm_b.push_back(j);
            p.N *= b.dims[j];
            p.out_dims.push_back(b.dims[j]);
            p.out_labels.push_back(b.labels[j]);
        }
    if (p.out_dims.size() > (size_t)TENSOR_MAX_RANK) throw Error(T4A_GPU_NOT_IMPLEMENTED, "contract_pair: result rank too large");
    if (p.M > 0x7FFFFFFFull || p.N > 0x7FFFFFFFull || p.K > 0x7FFFFFFFull)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "contract_pair: fused dimension above 2^31");
    return p;
}

void tensor_contract_pair(Engine& e, const TensorView& a, const TensorView& b, const ContractPlan& p, double* d_out)
{
    if (p.M * p.N == 0) return;
    if (p.K == 0) {
        fill_launch(d_out, p.M * p.N, 0.0, e.stream());
        return;
    }
    e.d_tmp.reserve(std::max<size_t>(a.size(), 1));
    e.d_tmp2.reserve(std::max<size_t>(b.size(), 1));
    tensor_permute(e, a, p.perm_a, e.d_tmp.get());
    tensor_permute(e, b, p.perm_b, e.d_tmp2.get());
    gemm_launch(gemm_desc((int)p.M, (int)p.N, (int)p.K, e.d_tmp.get(), (int)p.M, e.d_tmp2.get(), (int)p.K, d_out, (int)p.M), e.stream());
    T4A_HIP(hipGetLastError());
}

void require_distinct_labels(const TensorView& t)
{
    for (size_t a = 0; a < t.labels.size(); ++a)
        for (size_t b = a + 1; b < t.labels.size(); ++b)
            if (t.labels[a] == t.labels[b]) throw Error(T4A_GPU_INVALID_ARGUMENT, "duplicate index in tensor");
}

std::vector<size_t> plan_permute(const TensorView& t, const int64_t* labels)
{
    const size_t r = t.dims.size();
    std::vector<size_t> perm(r);
    std::vector<char> used(r, 0);
    for (size_t k = 0; k < r; ++k) {
        auto it = std::find(t.labels.begin(), t.labels.end(), labels[k]);
        if (it == t.labels.end()) throw Error(T4A_GPU_INVALID_ARGUMENT, "permute: index not found in tensor");
        perm[k] = (size_t)(it - t.labels.begin());
        if (used[perm[k]]) throw Error(T4A_GPU_INVALID_ARGUMENT, "permute: duplicate index");
        used[perm[k]] = 1;
    }
    return perm;
}

size_t plan_relabel(const TensorView& t, int64_t from, int64_t to)
{
    auto it = std::find(t.labels.begin(), t.labels.end(), from);
    if (it == t.labels.end()) throw Error(T4A_GPU_INVALID_ARGUMENT, "relabel: index not found in tensor");
    if (from != to && std::find(t.labels.begin(), t.labels.end(), to) != t.labels.end())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "relabel: the new label is already present");
    return (size_t)(it - t.labels.begin());
}

ContractPlan plan_outer_product(const TensorView& a, const TensorView& b)
{
    for (int64_t l : a.labels)
        if (std::find(b.labels.begin(), b.labels.end(), l) != b.labels.end())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "outer_product: the operands share an index; use contract for a contraction");
    return plan_contract_pair(a, b);
}

ContractPlan plan_tensordot(const TensorView& a, TensorView& b, const int64_t* labels_a, const int64_t* labels_b, size_t n_pairs)
{
    if (n_pairs == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "tensordot: No pairs specified for contraction");
    std::vector<size_t> ax_a, ax_b;
    for (size_t p = 0; p < n_pairs; ++p) {
        const auto ia = std::find(a.labels.begin(), a.labels.end(), labels_a[p]);
        const auto ib = std::find(b.labels.begin(), b.labels.end(), labels_b[p]);
        if (ia == a.labels.end()) throw Error(T4A_GPU_INVALID_ARGUMENT, "tensordot: Index not found in self tensor");
        if (ib == b.labels.end()) throw Error(T4A_GPU_INVALID_ARGUMENT, "tensordot: Index not found in other tensor");
        const size_t pa = (size_t)(ia - a.labels.begin()), pb = (size_t)(ib - b.labels.begin());
        if (std::find(ax_a.begin(), ax_a.end(), pa) != ax_a.end())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "tensordot: Duplicate axis " + std::to_string(pa) + " in self tensor");
        if (std::find(ax_b.begin(), ax_b.end(), pb) != ax_b.end())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "tensordot: Duplicate axis " + std::to_string(pb) + " in other tensor");
        if (a.dims[pa] != b.dims[pb])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "tensordot: Dimension mismatch: self[" + std::to_string(pa) + "]=" + std::to_string(a.dims[pa]) +
                                                      " != other[" + std::to_string(pb) + "]=" + std::to_string(b.dims[pb]));
        ax_a.push_back(pa);
        ax_b.push_back(pb);
    }
    for (size_t i = 0; i < a.labels.size(); ++i)
        for (size_t j = 0; j < b.labels.size(); ++j)
            if (a.labels[i] == b.labels[j]) {
                bool paired = false;
                for (size_t p = 0; p < n_pairs; ++p) paired = paired || (ax_a[p] == i && ax_b[p] == j);
                if (!paired)
                    throw Error(T4A_GPU_NOT_IMPLEMENTED,
                                "tensordot: Common index found but not in contraction pairs. Batch contraction is not yet implemented.");
            }
    // unpaired axes keep their labels (none is shared, checked above)
    for (size_t p = 0; p < n_pairs; ++p) b.labels[ax_b[p]] = a.labels[ax_a[p]];
    return plan_contract_pair(a, b);
}

void require_distinct_chain_labels(const int64_t* site_labels, const int64_t* bond_labels, size_t n)
{
    std::vector<int64_t> all(site_labels, site_labels + n);
    if (n > 1) all.insert(all.end(), bond_labels, bond_labels + n - 1);
    std::sort(all.begin(), all.end());
    if (std::adjacent_find(all.begin(), all.end()) != all.end())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "tensor_train_to_treetn: site and bond indices must be distinct");
}

std::vector<OwnedTensor> chain_to_tensors(Engine& e, Engine& src, const std::vector<DevCore>& cores, const int64_t* site_labels, const int64_t* bond_labels)
{
    const size_t n = cores.size();
    src.sync();
    std::vector<OwnedTensor> made;
    for (size_t s = 0; s < n; ++s) {
        const DevCore& c = cores[s];
        std::vector<size_t> dims;
        std::vector<int64_t> labels;
        if (s > 0) {
            dims.push_back(c.l);
            labels.push_back(bond_labels[s - 1]);
        }
        dims.push_back(c.s);
        labels.push_back(site_labels[s]);
        if (s + 1 < n) {
            dims.push_back(c.r);
            labels.push_back(bond_labels[s]);
        }
        OwnedTensor t(dims, labels); // boundary legs have dimension 1: the column-major data is unchanged
        if (c.size())
            T4A_HIP(hipMemcpyAsync(t.buf.get(), c.buf.get(), c.size() * sizeof(double), hipMemcpyDeviceToDevice, e.stream()));
        made.push_back(std::move(t));
    }
    e.sync();
    return made;
}

ChainPlan plan_tensors_to_chain(const std::vector<TensorView>& tensors)
{
    const size_t n_sites = tensors.size();
    auto shared = [&](size_t a, size_t b) { // the one label two neighbours share
        std::vector<int64_t> common;
        for (int64_t l : tensors[a].labels)
            if (std::find(tensors[b].labels.begin(), tensors[b].labels.end(), l) != tensors[b].labels.end()) common.push_back(l);
        if (common.size() != 1)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "treetn_to_tensor_train: missing chain edge between nodes " + std::to_string(a) + " and " +
                                                      std::to_string(b));
        return common[0];
    };
    std::vector<int64_t> bonds(n_sites > 0 ? n_sites - 1 : 0);
    for (size_t s = 0; s + 1 < n_sites; ++s) bonds[s] = shared(s, s + 1);
    for (size_t a = 0; a < n_sites; ++a) // a chain: no label may connect nodes that are not neighbours
        for (size_t b = a + 2; b < n_sites; ++b)
            for (int64_t l : tensors[a].labels)
                if (std::find(tensors[b].labels.begin(), tensors[b].labels.end(), l) != tensors[b].labels.end())
                    throw Error(T4A_GPU_INVALID_ARGUMENT, "treetn_to_tensor_train: expected a chain with " + std::to_string(n_sites - 1) + " edges");
    ChainPlan plan;
    for (size_t s = 0; s < n_sites; ++s) {
        const TensorView& t = tensors[s];
        const size_t want = 1 + (s > 0 ? 1 : 0) + (s + 1 < n_sites ? 1 : 0);
        if (t.labels.size() != want)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "treetn_to_tensor_train: node " + std::to_string(s) + " must have exactly one site index");
        std::vector<size_t> perm;
        auto pos = [&](int64_t l) { return (size_t)(std::find(t.labels.begin(), t.labels.end(), l) - t.labels.begin()); };
        size_t site_axis = 0;
        for (size_t a = 0; a < t.labels.size(); ++a)
            if ((s == 0 || t.labels[a] != bonds[s - 1]) && (s + 1 >= n_sites || t.labels[a] != bonds[s])) site_axis = a;
        if (s > 0) perm.push_back(pos(bonds[s - 1]));
        perm.push_back(site_axis);
        if (s + 1 < n_sites) perm.push_back(pos(bonds[s]));
        const std::array<size_t, 3> d = {s > 0 ? t.dims[perm[0]] : 1, t.dims[site_axis], s + 1 < n_sites ? t.dims[perm.back()] : 1};
        if (d[0] == 0 || d[1] == 0 || d[2] == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "treetn_to_tensor_train: a resulting core has a zero dimension");
        plan.perm.push_back(perm);
        plan.dims.push_back(d);
    }
    return plan;
}

std::vector<DevCore> tensors_to_chain(Engine& e, const std::vector<TensorView>& tensors, const ChainPlan& plan)
{
    std::vector<DevCore> cores(tensors.size());
    for (size_t s = 0; s < tensors.size(); ++s) {
        DevCore& c = cores[s];
        c.l = plan.dims[s][0];
        c.s = plan.dims[s][1];
        c.r = plan.dims[s][2];
        c.buf.reserve(c.size());
        tensor_permute(e, tensors[s], plan.perm[s], c.buf.get());
    }
    T4A_HIP(hipGetLastError());
    e.sync();
    return cores;
}

NetworkPlan plan_contract_network(const std::vector<TensorView>& ts, const std::vector<int64_t>& retain) // contract.rs:530-572, :885-941
{
    if (ts.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "No tensors to contract");
    for (const TensorView& t : ts) validate(t, "contract operand");
    auto has = [](const TensorView& t, int64_t l) { return std::find(t.labels.begin(), t.labels.end(), l) != t.labels.end(); };
    for (int64_t r : retain) { // validate_retained_indices_exist :943-959
        bool found = false;
        for (const TensorView& t : ts) found = found || has(t, r);
        if (!found) throw Error(T4A_GPU_INVALID_ARGUMENT, "Retained index " + std::to_string(r) + " does not appear in the input tensors");
    }
    NetworkPlan p;
    if (ts.size() == 1) { // (:539-541: a single operand is returned as it is)
        p.out_labels = ts[0].labels;
        p.out_dims = ts[0].dims;
        return p;
    }
    // connected components: operands that share a label (contractable or retained) are joined (:1167-1230)
    const size_t n = ts.size();
    std::vector<size_t> parent(n);
    for (size_t i = 0; i < n; ++i) parent[i] = i;
    auto find = [&](size_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j)
            for (int64_t l : ts[i].labels)
                if (has(ts[j], l)) parent[find(i)] = find(j);
    size_t components = 0;
    for (size_t i = 0; i < n; ++i) components += find(i) == i ? 1 : 0;
    if (components > 1)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Disconnected tensor network: " + std::to_string(components) + " components found");
    // sizes and occurrence counts per label (:728-750, :892-897)
    std::vector<int64_t> seen;
    std::vector<size_t> seen_dim, count;
    for (const TensorView& t : ts)
        for (size_t a = 0; a < t.labels.size(); ++a) {
            const auto it = std::find(seen.begin(), seen.end(), t.labels[a]);
            if (it == seen.end()) {
                seen.push_back(t.labels[a]);
                seen_dim.push_back(t.dims[a]);
                count.push_back(1);
            } else {
                const size_t k = (size_t)(it - seen.begin());
                if (seen_dim[k] != t.dims[a])
                    throw Error(T4A_GPU_INVALID_ARGUMENT, "Internal label shape mismatch: label " + std::to_string(t.labels[a]) + " has dimensions " +
                                                              std::to_string(seen_dim[k]) + " and " + std::to_string(t.dims[a]));
                ++count[k];
            }
        }
    for (size_t k = 0; k < seen.size(); ++k) { // first appearance order is the order of `seen`
        const bool retained = std::find(retain.begin(), retain.end(), seen[k]) != retain.end();
        if (count[k] == 1 || retained) {
            p.out_labels.push_back(seen[k]);
            p.out_dims.push_back(seen_dim[k]);
        }
    }
    if (p.out_labels.size() > (size_t)TENSOR_MAX_RANK) throw Error(T4A_GPU_NOT_IMPLEMENTED, "contract: result rank too large");
    return p;
}

OwnedTensor tensor_contract_network(Engine& e, const std::vector<TensorView>& ts, const std::vector<int64_t>& retain)
{
    const NetworkPlan plan = plan_contract_network(ts, retain);
    hipStream_t st = e.stream();
    struct Node {
        TensorView v;
        std::shared_ptr<DevBuf<double>> own; // null: an input operand
    };
    std::vector<Node> work;
    for (const TensorView& t : ts) work.push_back(Node{t, nullptr});
    auto has = [](const TensorView& t, int64_t l) { return std::find(t.labels.begin(), t.labels.end(), l) != t.labels.end(); };
    auto in_out = [&](int64_t l) { return std::find(plan.out_labels.begin(), plan.out_labels.end(), l) != plan.out_labels.end(); };
    while (work.size() > 1) {
        // the connected pair with the smallest result (ties: the first such pair)
        size_t bi = 0, bj = 0;
        double best = -1.0;
        for (size_t i = 0; i < work.size(); ++i)
            for (size_t j = i + 1; j < work.size(); ++j) {
                bool shares = false;
                for (int64_t l : work[i].v.labels) shares = shares || has(work[j].v, l);
                if (!shares) continue;
                double sz = 1.0;
                auto needed = [&](int64_t l) {
                    if (in_out(l)) return true;
                    for (size_t q = 0; q < work.size(); ++q)
                        if (q != i && q != j && has(work[q].v, l)) return true;
                    return false;
                };
                for (size_t a = 0; a < work[i].v.labels.size(); ++a) {
                    const int64_t l = work[i].v.labels[a];
                    if (!has(work[j].v, l) || needed(l)) sz *= (double)work[i].v.dims[a];
                }
                for (size_t a = 0; a < work[j].v.labels.size(); ++a)
                    if (!has(work[i].v, work[j].v.labels[a])) sz *= (double)work[j].v.dims[a];
                if (best < 0.0 || sz < best) {
                    best = sz;
                    bi = i;
                    bj = j;
                }
            }
        if (best < 0.0) throw Error(T4A_GPU_INTERNAL_ERROR, "contract: no connected pair left in a connected network");
        const TensorView& A = work[bi].v;
        const TensorView& B = work[bj].v;
        auto needed = [&](int64_t l) {
            if (in_out(l)) return true;
            for (size_t q = 0; q < work.size(); ++q)
                if (q != bi && q != bj && has(work[q].v, l)) return true;
            return false;
        };
        // A -> [free A, summed, batch], B -> [summed, free B, batch]; result [free A, free B, batch]
        std::vector<size_t> pa_free, pa_sum, pa_batch, pb_sum, pb_free, pb_batch;
        size_t M = 1, K = 1, N = 1, Bt = 1;
        for (size_t a = 0; a < A.labels.size(); ++a) {
            const int64_t l = A.labels[a];
            if (!has(B, l)) {
                pa_free.push_back(a);
                M *= A.dims[a];
            } else if (needed(l)) {
                pa_batch.push_back(a);
                Bt *= A.dims[a];
            } else {
                pa_sum.push_back(a);
                K *= A.dims[a];
            }
        }
        auto pos_in_b = [&](int64_t l) { return (size_t)(std::find(B.labels.begin(), B.labels.end(), l) - B.labels.begin()); };
        for (size_t a : pa_sum) pb_sum.push_back(pos_in_b(A.labels[a]));
        for (size_t a : pa_batch) pb_batch.push_back(pos_in_b(A.labels[a]));
        for (size_t b = 0; b < B.labels.size(); ++b)
            if (!has(A, B.labels[b])) {
                pb_free.push_back(b);
                N *= B.dims[b];
            }
        if (M > 0x7FFFFFFFull || N > 0x7FFFFFFFull || K > 0x7FFFFFFFull || Bt > 0x7FFFFFFFull)
            throw Error(T4A_GPU_NOT_IMPLEMENTED, "contract: fused dimension above 2^31");
        std::vector<size_t> perm_a, perm_b;
        perm_a.insert(perm_a.end(), pa_free.begin(), pa_free.end());
        perm_a.insert(perm_a.end(), pa_sum.begin(), pa_sum.end());
        perm_a.insert(perm_a.end(), pa_batch.begin(), pa_batch.end());
        perm_b.insert(perm_b.end(), pb_sum.begin(), pb_sum.end());
        perm_b.insert(perm_b.end(), pb_free.begin(), pb_free.end());
        perm_b.insert(perm_b.end(), pb_batch.begin(), pb_batch.end());
        Node res;
        for (size_t a : pa_free) {
            res.v.dims.push_back(A.dims[a]);
            res.v.labels.push_back(A.labels[a]);
        }
        for (size_t b : pb_free) {
            res.v.dims.push_back(B.dims[b]);
            res.v.labels.push_back(B.labels[b]);
        }
        for (size_t a : pa_batch) {
            res.v.dims.push_back(A.dims[a]);
            res.v.labels.push_back(A.labels[a]);
        }
        if (res.v.dims.size() > (size_t)TENSOR_MAX_RANK) throw Error(T4A_GPU_NOT_IMPLEMENTED, "contract: intermediate rank too large");
        res.own = std::make_shared<DevBuf<double>>();
        res.own->reserve(std::max<size_t>(M * N * Bt, 1));
        res.v.d_data = res.own->get();
        if (M * N * Bt > 0) {
            e.d_tmp.reserve(std::max<size_t>(A.size(), 1));
            e.d_tmp2.reserve(std::max<size_t>(B.size(), 1));
            tensor_permute(e, A, perm_a, e.d_tmp.get());
            tensor_permute(e, B, perm_b, e.d_tmp2.get());
            GemmDesc g = gemm_desc((int)M, (int)N, (int)K, e.d_tmp.get(), (int)M, e.d_tmp2.get(), (int)K, res.own->get(), (int)M);
            g.strideA = (long long)(M * K);
            g.strideB = (long long)(K * N);
            g.strideC = (long long)(M * N);
            g.batch = (int)Bt;
            gemm_launch(g, st);
            T4A_HIP(hipGetLastError());
            e.sync(); // (the permutation scratch is reused by the next step)
        }
        work.erase(work.begin() + (long)bj);
        work.erase(work.begin() + (long)bi);
        work.push_back(std::move(res));
    }
    // into the reference's index order
    const TensorView& F = work[0].v;
    OwnedTensor out(plan.out_dims, plan.out_labels);
    std::vector<size_t> perm;
    for (int64_t l : plan.out_labels) {
        const auto it = std::find(F.labels.begin(), F.labels.end(), l);
        if (it == F.labels.end()) throw Error(T4A_GPU_INTERNAL_ERROR, "contract: a result index was lost");
        perm.push_back((size_t)(it - F.labels.begin()));
    }
    if (perm.size() != F.labels.size()) throw Error(T4A_GPU_INTERNAL_ERROR, "contract: an index was left uncontracted");
    if (F.dims.empty()) T4A_HIP(hipMemcpyAsync(out.buf.get(), F.d_data, sizeof(double), hipMemcpyDeviceToDevice, st)); // (a scalar)
    else if (F.size() > 0) tensor_permute(e, F, perm, out.buf.get());
    e.sync();
    return out;
}

UnfoldPlan plan_unfold_split(const TensorView& t, const std::vector<int64_t>& left) // idx_tensor.rs:5278-5345
{
    validate(t, "unfold_split");
    const size_t rank = t.dims.size();
    if (!(rank >= 2)) throw Error(T4A_GPU_INVALID_ARGUMENT, "Tensor must have rank >= 2, got rank " + std::to_string(rank));
    if (!(left.size() > 0 && left.size() < rank))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Left indices must be a non-empty proper subset of tensor indices (0 < left_len < rank), got left_len=" +
                                                  std::to_string(left.size()) + ", rank=" + std::to_string(rank));
    UnfoldPlan p;
    for (size_t a = 0; a < left.size(); ++a) {
        auto it = std::find(t.labels.begin(), t.labels.end(), left[a]);
        if (it == t.labels.end()) throw Error(T4A_GPU_INVALID_ARGUMENT, "Index in left_inds not found in tensor");
        for (size_t b = 0; b < a; ++b)
            if (left[a] == left[b]) throw Error(T4A_GPU_INVALID_ARGUMENT, "Duplicate index in left_inds");
        p.perm.push_back((size_t)(it - t.labels.begin()));
    }
    const size_t nl = left.size();
    for (size_t k = 0; k < rank; ++k)
        if (std::find(p.perm.begin(), p.perm.begin() + nl, k) == p.perm.begin() + nl) p.perm.push_back(k);
    for (size_t k = 0; k < rank; ++k) {
        const size_t d = t.dims[p.perm[k]];
        if (k < nl) {
            p.left_dims.push_back(d);
            p.left_labels.push_back(t.labels[p.perm[k]]);
            p.m *= d;
        } else {
            p.right_dims.push_back(d);
            p.right_labels.push_back(t.labels[p.perm[k]]);
            p.n *= d;
        }
    }
    return p;
}

OwnedTensor bonded_tensor(std::vector<size_t> dims, std::vector<int64_t> labels, size_t r, int64_t bond, bool bond_first)
{
    dims.insert(bond_first ? dims.begin() : dims.end(), r);
    labels.insert(bond_first ? labels.begin() : labels.end(), bond);
    return OwnedTensor(dims, labels);
}

void require_factorizable(const UnfoldPlan& un, const char* op, const char* empty_what)
{
    if (un.m * un.n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(empty_what) + " of an empty tensor");
    Engine::require_factor_dims(un.m, un.n, std::string(op) + ": unfolded dimensions");
}

void SvdOptions::validate() const
{
    if (!truncate) return;
    if (has_max_bond_dim && max_bond_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "max_bond_dim must be positive when specified");
    if (!std::isfinite(policy.threshold) || policy.threshold < 0.0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid SVD truncation threshold: threshold must be finite and non-negative");
}

void QrOptions::validate() const
{
    if (truncate && (!std::isfinite(rtol) || rtol < 0.0))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid rtol value: rtol must be finite and non-negative");
}

void FactorizeOptions::validate() const
{
    if (alg == 0) svd.validate();
    if (alg == 1) qr.validate();
}

// the m x n unfolding of `t`, behind the caller's half of the staging block
static double* unfold(Engine& e, const TensorView& t, const UnfoldPlan& un)
{
    double* d_mat = tensor_staging(e, un.m * un.n) + un.m * un.n;
    tensor_permute(e, t, un.perm, d_mat);
    return d_mat;
}
static void download(Engine& e, double* dst, const double* src, size_t count)
{
    T4A_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, e.stream()));
    e.sync();
}

UnfoldedFactors tensor_svd(Engine& e, const TensorView& t, const UnfoldPlan& un, const SvdOptions& o)
{
    const size_t m = un.m, n = un.n, k = std::min(m, n);
    const double* d_mat = unfold(e, t, un);
    e.d_tmp.reserve(m * k + k + k * n);
    double* d_u = e.d_tmp.get();
    double* d_s = d_u + m * k;
    double* d_vt = d_s + k;
    e.svd(d_mat, (int)m, (int)n, d_u, d_s, d_vt);
    std::vector<double> hs(k);
    download(e, hs.data(), d_s, k);
    size_t keep = k;
    if (o.truncate) { // svd.rs:279-292
        keep = svd_retained_rank(hs.data(), k, o.policy);
        if (o.has_max_bond_dim) keep = std::min(keep, o.max_bond_dim);
    }
    keep = std::min(std::max<size_t>(keep, 1), k);
    return UnfoldedFactors{m, n, k, keep, d_u, d_vt, d_s, std::move(hs)};
}

UnfoldedFactors tensor_qr(Engine& e, const TensorView& t, const UnfoldPlan& un, const QrOptions& o)
{
    const size_t m = un.m, n = un.n, k = std::min(m, n);
    const double* d_mat = unfold(e, t, un);
    e.d_tmp.reserve(m * k + k * n);
    double* d_q = e.d_tmp.get();
    double* d_r = d_q + m * k;
    e.qr(d_mat, (int)m, (int)n, d_q, d_r);
    size_t keep = k;
    if (o.truncate) {
        std::vector<double> hr(k * n);
        download(e, hr.data(), d_r, k * n);
        keep = std::min(qr_retained_rank(hr.data(), k, n, o.rtol), k);
    }
    return UnfoldedFactors{m, n, k, keep, d_q, d_r, nullptr, {}};
}

FactorizeResult tensor_factorize(Engine& e, const TensorView& t, const UnfoldPlan& un, const FactorizeOptions& o, int64_t bond_label)
{
    const size_t m = un.m, n = un.n;
    hipStream_t st = e.stream();
    FactorizeResult res;
    auto finish = [&](size_t keep, const double* d_l, size_t ldl, const double* d_r, size_t ldr) {
        // d_l: m x keep (ld ldl), d_r: keep x n (ld ldr) -> tensors
        res.left = bonded_tensor(un.left_dims, un.left_labels, keep, bond_label);
        res.right = bonded_tensor(un.right_dims, un.right_labels, keep, bond_label, true);
        gather_launch(d_l, (int)ldl, nullptr, (int)m, nullptr, (int)keep, res.left.buf.get(), (int)m, st);
        gather_launch(d_r, (int)ldr, nullptr, (int)keep, nullptr, (int)n, res.right.buf.get(), (int)keep, st);
        T4A_HIP(hipGetLastError());
        e.sync();
        res.rank = keep;
    };
    if (o.alg == 0) { // SVD
        const UnfoldedFactors f = tensor_svd(e, t, un, o.svd);
        e.d_tmp2.reserve(std::max(m, n) * f.keep);
        res.singular_values.assign(f.s.begin(), f.s.begin() + (long)f.keep);
        if (o.canonical == 0) { // right = S V^H
            diag_scale_launch(f.d_right, (int)f.k, (int)f.keep, (int)n, f.d_s, true, e.d_tmp2.get(), (int)f.keep, st);
            finish(f.keep, f.d_left, m, e.d_tmp2.get(), f.keep);
        } else { // left = U S
            diag_scale_launch(f.d_left, (int)m, (int)m, (int)f.keep, f.d_s, false, e.d_tmp2.get(), (int)m, st);
            finish(f.keep, e.d_tmp2.get(), m, f.d_right, f.k);
        }
    } else if (o.alg == 1) { // QR
        const UnfoldedFactors f = tensor_qr(e, t, un, o.qr);
        finish(f.keep, f.d_left, m, f.d_right, f.k);
    } else { // LU / CI on the rrLU kernels
        const double* d_mat = unfold(e, t, un);
        const bool trunc = o.svd.truncate;
        RrLUOptions lo;
        lo.max_bond_dim = (trunc && o.svd.has_max_bond_dim) ? o.svd.max_bond_dim : std::numeric_limits<size_t>::max();
        lo.rel_tol = trunc ? 1e-14 : 0.0; // factorize.rs:644, :755
        lo.abs_tol = 0.0;
        lo.left_orthogonal = o.canonical == 0;
        const bool lu = o.alg == 2;
        const LuciResult r = e.luci(d_mat, (int)m, (int)n, lo, !lu, lu);
        if (lu) e.lu_permuted_factors(r, lo.left_orthogonal);
        const size_t keep = (size_t)r.rank;
        if (keep == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "Failed to create bond index: dimension 0");
        finish(keep, e.left(), m, e.right(), keep);
    }
    return res;
}

void diag_scale_launch(const double* in, int ldi, int rows, int cols, const double* sv, bool by_row, double* out, int ldo,
                       hipStream_t stream)
{
    const size_t total = (size_t)rows * cols;
    if (total == 0) return;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(diag_scale_kernel, dim3(blocks), dim3(256), 0, stream, in, ldi, rows, cols, sv, by_row ? 1 : 0, out, ldo);
}

} // namespace t4a
