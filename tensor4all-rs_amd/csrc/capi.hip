// capi.hip — extern "C" surface declared in include/t4a_gpu.h.
// No exception crosses the boundary (tensor4all-capi/src/lib.rs:139-162 convention): every entry point
// runs inside `guarded`, which stores the message in a thread-local slot and returns a status code.
#include "stdrng.hpp"
#include "smallrng.hpp"
#include <memory>
#include <initializer_list>
#include <mutex>

#include "patching.hpp"
#include "tci2.hpp"
#include "tree.hpp"
#include "quantics.hpp"
#include "tensorops.hpp"
#include "dense.hpp"
#include "aci.hpp"
#include "globalsearch.hpp"
#include "mpo.hpp"
#include "contraction.hpp"
#include "quanticstransform.hpp"
#include "tt_canonical.hpp"
#include "dmrg.hpp"
#include "tdvp.hpp"
#include "gse.hpp"
#include "pmpo.hpp"
#include "pmpo_patching.hpp"
#include "linsolve.hpp"
#include "swap.hpp"
#include "restructure.hpp"
#include "fit_sum.hpp"
#include "linop.hpp"

struct t4a_gpu_tci2 {
    t4a::Tci2 impl;
    explicit t4a_gpu_tci2(const std::vector<size_t>& d) : impl(d) {}
};

struct t4a_gpu_treetci {
    t4a::TreeTci impl;
    t4a_gpu_treetci(const std::vector<size_t>& d, const t4a::TreeGraph& g) : impl(d, g) {}
};

struct t4a_gpu_tensor : t4a::OwnedTensor {
    explicit t4a_gpu_tensor(t4a::OwnedTensor&& t) : t4a::OwnedTensor(std::move(t)) {}
};

struct t4a_gpu_qtci {
    std::unique_ptr<t4a::QuanticsTci> impl;
};

struct t4a_gpu_ptt {
    std::unique_ptr<t4a::PartitionedTT> impl;
};

struct t4a_gpu_tt {
    t4a::TensorTrain impl;
    t4a_gpu_tt(const std::vector<std::array<size_t, 3>>& d, const double* data) : impl(d, data) {}
    t4a_gpu_tt(const std::vector<t4a::DevCore>& cores, hipStream_t src) : impl(cores, src) {}
};

struct t4a_gpu_site_tt {
    t4a::SiteTrain impl;
    t4a_gpu_site_tt(const std::vector<t4a::DevCore>& cores, hipStream_t src, size_t center) : impl(cores, src, center) {}
};

struct t4a_gpu_vidal_tt {
    std::unique_ptr<t4a::VidalTrain> impl;
};

struct t4a_gpu_inverse_tt {
    std::unique_ptr<t4a::InverseTrain> impl;
};

struct t4a_gpu_mpo {
    std::unique_ptr<t4a::Mpo> impl;
};

struct t4a_gpu_pmpo {
    std::unique_ptr<t4a::PartitionedMpo> impl;
};

struct t4a_gpu_qt_op {
    t4a::QtOperator impl; // host data only
};

struct t4a_gpu_contraction {
    std::unique_ptr<t4a::MpoContraction> impl;
};

struct t4a_gpu_swap_schedule {
    t4a::SwapSchedule impl; // host data only
};

struct t4a_gpu_projected_operator {
    std::unique_ptr<t4a::ProjectedOperator> impl;
};

struct t4a_gpu_aci_problem {
    std::unique_ptr<t4a::AciProblem> impl;
};

namespace t4a {
const std::string& last_error_ref();

namespace {

template <class F> t4a_gpu_status guarded(F&& body)
{
    try {
        body();
        return T4A_GPU_SUCCESS;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory");
        return T4A_GPU_INTERNAL_ERROR;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return T4A_GPU_INTERNAL_ERROR;
    } catch (...) {
        set_last_error("unknown internal error");
        return T4A_GPU_INTERNAL_ERROR;
    }
}

#define T4A_REQUIRE_PTR(p)                                                       \
    do {                                                                         \
        if ((p) == nullptr) throw ::t4a::Error(T4A_GPU_NULL_POINTER, #p " is null"); \
    } while (0)

std::mutex g_dense_mutex;
Engine* g_dense_engine = nullptr;

// One process-global engine for the handle-less dense entry points, serialised by a mutex exactly like the
// reference's global default backend (tensorbackend/src/context.rs:318-338).  It is never destroyed: a destructor that runs
// during static destruction would call into a HIP runtime that may already be gone (under rocprofv3 that teardown does not
// return); the process exit reclaims stream and buffers.
Engine& dense_engine()
{
    if (!g_dense_engine) g_dense_engine = new Engine();
    return *g_dense_engine;
}

TCI2Options convert_options(const t4a_gpu_tci2_options* o)
{
    if (!o) throw Error(T4A_GPU_NULL_POINTER, "options is null");
    TCI2Options r;
    r.tolerance = o->tolerance;
    r.max_iter = o->max_iter;
    r.max_bond_dim = o->max_bond_dim;
    r.pivot_search = o->pivot_search;
    r.normalize_error = o->normalize_error != 0;
    r.verbosity = o->verbosity;
    r.max_nglobal_pivot = o->max_nglobal_pivot;
    r.nsearch = o->nsearch;
    r.sweep_strategy = o->sweep_strategy;
    r.ncheck_history = o->ncheck_history;
    r.strictly_nested = o->strictly_nested != 0;
    r.tol_margin_global_search = o->tol_margin_global_search;
    r.has_seed = o->has_seed != 0;
    r.seed = o->seed;
    if (r.sweep_strategy < 0 || r.sweep_strategy > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid sweep_strategy");
    if (r.pivot_search < 0 || r.pivot_search > 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid pivot_search");
    return r;
}

t4a_gpu_svd_policy to_c(const SvdPolicy& p) { return t4a_gpu_svd_policy{p.threshold, p.scale, p.measure, p.rule}; }
SvdPolicy from_c(const t4a_gpu_svd_policy& p) { return SvdPolicy{p.threshold, p.scale, p.measure, p.rule}; }

// the shape lists of the check_shapes entry points
std::vector<std::array<size_t, 3>> dims3_list(const size_t* d, size_t n)
{
    std::vector<std::array<size_t, 3>> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    return v;
}
std::vector<std::array<size_t, 4>> dims4_list(const size_t* d, size_t n)
{
    std::vector<std::array<size_t, 4>> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = {d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]};
    return v;
}

// the dense test hooks of the Krylov solvers: the n x n matrix and the basis of basis_cols columns are indexed with ints
void require_dense_hook_dims(const char* who, size_t n, size_t basis_cols)
{
    if (n == 0 || n > 46340 || (unsigned long long)n * basis_cols > (unsigned long long)INT_MAX)
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": n must be positive and the matrix and the basis must hold at most INT_MAX elements");
}
// the hooks on a len x nb basis: "<who>: <too_large>" for nb above nb_max or more than INT_MAX elements
void require_basis_dims(const char* who, size_t len, size_t nb, size_t nb_max, const std::string& too_large)
{
    if (len == 0 || nb == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": len and nb must be positive");
    if (nb > nb_max || (unsigned long long)len * nb > (unsigned long long)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": " + too_large);
}

void upload(Engine& e, double* dst, const double* src, size_t count)
{
    if (count == 0) return;
    T4A_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, e.stream()));
    T4A_HIP(hipStreamSynchronize(e.stream()));
}
void download(Engine& e, double* dst, const double* src, size_t count)
{
    if (count == 0) return;
    T4A_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, e.stream()));
    T4A_HIP(hipStreamSynchronize(e.stream()));
}
// The same copies in stream order WITHOUT a host synchronisation of their own, for entry points that end with a synchronising download():
// the caller's buffers stay valid until the entry point returns, and everything between is ordered on the engine's stream (round 6: an SVD
// call paid five stream synchronisations for its copies, a QR call three, a product three).
// ... and the guard that makes "until the entry point returns" true on EVERY path: an exception thrown between the first queued copy and
// the final download (a non-finite input, a HIP error) must not let the entry point return while a copy from or into the caller's memory
// is still in flight.  On the normal path the stream is already idle: one more (empty) synchronisation.  Measured (profiles/r06_svd_small.txt
// section 8): SVD calls of tiny matrices 17 - 20 us shorter (3 x 2: 125 -> 108 us), 64 x 64 and the QR calls unchanged within noise.
struct StreamSyncOnExit {
    Engine& e;
    explicit StreamSyncOnExit(Engine& eng) : e(eng) {}
    ~StreamSyncOnExit() { (void)hipStreamSynchronize(e.stream()); }
    StreamSyncOnExit(const StreamSyncOnExit&) = delete;
    StreamSyncOnExit& operator=(const StreamSyncOnExit&) = delete;
};
void upload_async(Engine& e, double* dst, const double* src, size_t count)
{
    if (count == 0) return;
    T4A_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, e.stream()));
}
void download_async(Engine& e, double* dst, const double* src, size_t count)
{
    if (count == 0) return;
    T4A_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, e.stream()));
}

// the kernels index with 32-bit integers: larger dimensions are refused before any narrowing cast
void require_int_dims(std::initializer_list<size_t> dims, const char* what)
{
    for (size_t d : dims)
        if (d > (size_t)std::numeric_limits<int>::max())
            throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(what) + ": dimension exceeds the 32-bit index range of the device kernels");
}

size_t checked_mul(size_t a, size_t b, const char* what)
{
    if (a != 0 && b > std::numeric_limits<size_t>::max() / a)
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(what) + " overflows usize");
    return a * b;
}

// caller indices -> the 32-bit indices of the device: `count` of them in one list ...
std::vector<uint32_t> narrow_indices(const size_t* idx, size_t count, const char* out_of_bounds = "index out of bounds")
{
    std::vector<uint32_t> u(count);
    for (size_t k = 0; k < count; ++k) {
        if (idx[k] > 0xFFFFFFFFull) throw Error(T4A_GPU_INVALID_ARGUMENT, out_of_bounds);
        u[k] = (uint32_t)idx[k];
    }
    return u;
}
// ... and n_pivots pivots of n_sites indices each
std::vector<std::vector<uint32_t>> narrow_pivots(const size_t* pivots, size_t n_pivots, size_t n_sites, const char* out_of_bounds)
{
    std::vector<std::vector<uint32_t>> p(n_pivots, std::vector<uint32_t>(n_sites));
    for (size_t k = 0; k < n_pivots; ++k)
        for (size_t s = 0; s < n_sites; ++s) {
            const size_t v = pivots[s + n_sites * k];
            if (v > 0xFFFFFFFFull) throw Error(T4A_GPU_INVALID_ARGUMENT, out_of_bounds);
            p[k][s] = (uint32_t)v;
        }
    return p;
}

// an array of handles -> what `get` takes from each; a null entry throws NULL_POINTER with `null_message`
template <class H, class Get> auto handle_list(H* const* handles, size_t n, const char* null_message, Get get)
{
    std::vector<decltype(get(*handles[0]))> v;
    v.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        if (!handles[i]) throw Error(T4A_GPU_NULL_POINTER, null_message);
        v.push_back(get(*handles[i]));
    }
    return v;
}

// what the three LUCI entry points check before they take the lock (the source is the matrix `a` or the callback `fill_block`;
// rook: the 65535 limit of the rook routes).  Returns m * n.
size_t luci_prologue(size_t m, size_t n, const size_t* rank, const size_t* rows, const size_t* cols, const double* pivot_errors,
                     bool source_is_null, const char* source_is_null_message, const double* left, const double* right, bool rook)
{
    T4A_REQUIRE_PTR(rank);
    T4A_REQUIRE_PTR(rows);
    T4A_REQUIRE_PTR(cols);
    T4A_REQUIRE_PTR(pivot_errors);
    const size_t count = checked_mul(m, n, "matrix shape");
    require_int_dims({m, n}, "matrix shape");
    if (count) {
        if (source_is_null) throw Error(T4A_GPU_NULL_POINTER, source_is_null_message);
        T4A_REQUIRE_PTR(left);
        T4A_REQUIRE_PTR(right);
    }
    if (rook && (m > 65535 || n > 65535)) throw Error(T4A_GPU_NOT_IMPLEMENTED, "luci: dimensions above 65535 are not supported");
    return count;
}

void luci_outputs(Engine& e, const LuciResult& r, size_t m, size_t n, size_t* rank, size_t* rows, size_t* cols,
                  double* pivot_errors, double* left, double* right)
{
    *rank = (size_t)r.rank;
    for (int i = 0; i < r.rank; ++i) {
        rows[i] = (size_t)r.row_perm[i];
        cols[i] = (size_t)r.col_perm[i];
    }
    for (size_t i = 0; i < r.pivot_errors.size(); ++i) pivot_errors[i] = r.pivot_errors[i];
    if (r.rank > 0) {
        download(e, left, e.left(), m * (size_t)r.rank);
        download(e, right, e.right(), n * (size_t)r.rank);
    }
}

RookWork& dense_rook_work()
{
    static RookWork w; // guarded by g_dense_mutex like the dense engine itself
    return w;
}

} // namespace
} // namespace t4a

using namespace t4a;

namespace {

// what t4a_gpu_gemm_desc_f64 refuses, all of it on the host: "gemm_desc[i]: <what>"
void require_gemm_desc(const t4a_gpu_gemm_desc& d, size_t i, size_t na, size_t nb, size_t nc)
{
    auto refuse = [&](const std::string& what) { throw Error(T4A_GPU_INVALID_ARGUMENT, "gemm_desc[" + std::to_string(i) + "]: " + what); };
    const int64_t imax = std::numeric_limits<int>::max();
    for (int64_t v : {d.m, d.n, d.k, d.lda, d.ldb, d.ldc, d.batch, d.stride_a, d.stride_b, d.stride_c, d.off_a, d.off_b, d.off_c})
        if (v < 0) refuse("negative size, leading dimension, stride or offset");
    for (int64_t v : {d.m, d.n, d.k, d.lda, d.ldb, d.ldc, d.batch})
        if (v > imax) refuse("dimension exceeds the 32-bit index range of the device kernels");
    // (the kernel rounds m, n and k up to whole tiles in int)
    for (int64_t v : {d.m, d.n, d.k})
        if (v > imax - 63) refuse("m, n and k must be at most INT_MAX - 63: the kernel rounds them up to whole tiles in 32-bit integers");
    if ((d.trans_a != 0 && d.trans_a != 1) || (d.trans_b != 0 && d.trans_b != 1)) refuse("trans_a and trans_b must be 0 or 1");
    const int64_t a_rows = d.trans_a ? d.k : d.m, a_cols = d.trans_a ? d.m : d.k;
    const int64_t b_rows = d.trans_b ? d.n : d.k, b_cols = d.trans_b ? d.k : d.n;
    if (d.lda < std::max<int64_t>(a_rows, 1)) refuse("lda is smaller than the rows of the stored A");
    if (d.ldb < std::max<int64_t>(b_rows, 1)) refuse("ldb is smaller than the rows of the stored B");
    if (d.ldc < std::max<int64_t>(d.m, 1)) refuse("ldc is smaller than the rows of C");
    // (every factor is below 2^31 except strides and offsets, which are compared step by step: no overflow)
    auto fits = [&](int64_t off, int64_t stride, int64_t rows, int64_t cols, int64_t ld, size_t count) {
        if (rows == 0 || cols == 0 || d.batch == 0) return true;
        const unsigned __int128 end = (unsigned __int128)off + (unsigned __int128)(d.batch - 1) * (unsigned __int128)stride +
                                      (unsigned __int128)(cols - 1) * (unsigned __int128)ld + (unsigned __int128)rows;
        return end <= (unsigned __int128)count;
    };
    if (!fits(d.off_a, d.stride_a, a_rows, a_cols, d.lda, na)) refuse("A runs past its buffer");
    if (!fits(d.off_b, d.stride_b, b_rows, b_cols, d.ldb, nb)) refuse("B runs past its buffer");
    if (!fits(d.off_c, d.stride_c, d.m, d.n, d.ldc, nc)) refuse("C runs past its buffer");
    if (d.m == 0 || d.n == 0 || d.batch == 0) return;
    if (d.batch > 1) {
        // results do not overlap when a problem ends before the next begins, or when the problems interleave inside ldc
        const unsigned __int128 span = (unsigned __int128)(d.n - 1) * (unsigned __int128)d.ldc + (unsigned __int128)d.m;
        const bool apart = (unsigned __int128)d.stride_c >= span;
        const bool interleaved = d.stride_c >= d.m && (unsigned __int128)(d.batch - 1) * (unsigned __int128)d.stride_c + (unsigned __int128)d.m <= (unsigned __int128)d.ldc;
        if (!apart && !interleaved) refuse("stride_c makes the results of two problems overlap");
    }
    const GemmPlan p = gemm_plan((int)d.m, (int)d.n, (int)d.k, (int)d.batch);
    if (d.batch * (int64_t)p.ksplit > 65535 || p.grid_n > 65535) refuse("more problems, split-K slices or tile columns than the 65535 a launch takes");
}

std::vector<Tci2*> tci2_list(t4a_gpu_tci2* const* handles, size_t n_handles)
{
    if (n_handles) T4A_REQUIRE_PTR(handles);
    return handle_list(handles, n_handles, "handles[i] is null", [](t4a_gpu_tci2& h) { return &h.impl; });
}

t4a::SearchFn wrap_search_fn(t4a_gpu_batch_eval_fn f, void* ctx)
{
    return [f, ctx](const uint32_t* idx, size_t n_sites, size_t n_pts, double* out) {
        FnSource::call(f, ctx, idx, n_sites, n_pts, out, "batch callback", "points");
    };
}

std::vector<size_t> dims_vec(const size_t* local_dims, size_t n_sites)
{
    return std::vector<size_t>(local_dims, local_dims + n_sites);
}

t4a_gpu_ptt* run_adaptive(const size_t* local_dims, size_t n_sites, const FnSource& f,
                          const size_t* initial_pivots, size_t n_pivots, const t4a_gpu_tci2_options* tci_options,
                          const size_t* patch_order, size_t n_initial_pivots, int32_t recycle_pivots)
{
    if (n_sites) T4A_REQUIRE_PTR(local_dims);
    if (n_pivots) T4A_REQUIRE_PTR(initial_pivots);
    AdaptiveOptions ao;
    ao.tci = convert_options(tci_options);
    ao.n_initial_pivots = n_initial_pivots;
    ao.recycle_pivots = recycle_pivots != 0;
    if (patch_order) ao.patch_order.assign(patch_order, patch_order + n_sites);
    std::vector<size_t> dims(local_dims, local_dims + n_sites);
    std::vector<std::vector<uint32_t>> piv(n_pivots, std::vector<uint32_t>(n_sites));
    for (size_t k = 0; k < n_pivots; ++k)
        for (size_t s = 0; s < n_sites; ++s) {
            const size_t v = initial_pivots[s + n_sites * k];
            // out-of-range values are reported by the driver's own validation; keep them representable
            piv[k][s] = v > 0xFFFFFFFEull ? 0xFFFFFFFFu : (uint32_t)v;
        }
    require_device();
    std::unique_ptr<t4a_gpu_ptt> h(new t4a_gpu_ptt);
    h->impl = adaptive_interpolate(dims, f, piv, ao);
    return h.release();
}

TreeTciOptions convert_tree_options(const t4a_gpu_treetci_options* o)
{
    TreeTciOptions r;
    if (!o) return r;
    r.tolerance = o->tolerance;
    r.max_iter = o->max_iter;
    r.max_bond_dim = o->max_bond_dim;
    r.normalize_error = o->normalize_error != 0;
    r.enable_global_pivots = o->enable_global_pivots != 0;
    r.nsearch = o->nsearch;
    r.max_nglobal_pivot = o->max_nglobal_pivot;
    r.tol_margin_global_search = o->tol_margin_global_search;
    r.has_seed = o->has_seed != 0;
    r.seed = o->seed;
    return r;
}

void write_index_set(const IndexSet& s, size_t* count, size_t* out)
{
    *count = s.count;
    if (out)
        for (size_t k = 0; k < s.count * s.width; ++k) out[k] = s.d[k];
}

void write_history(const t4a_gpu_treetci* h, size_t* n_iter, size_t* ranks, double* errors)
{
    if (n_iter) *n_iter = h->impl.ranks_hist.size();
    for (size_t k = 0; k < h->impl.ranks_hist.size(); ++k) {
        if (ranks) ranks[k] = h->impl.ranks_hist[k];
        if (errors) errors[k] = h->impl.errors_hist[k];
    }
}

QtciOptions convert_qtci_options(const t4a_gpu_qtci_options* o)
{
    QtciOptions r;
    if (!o) return r;
    r.tolerance = o->tolerance;
    r.max_bond_dim = o->max_bond_dim;
    r.max_iter = o->max_iter;
    r.n_random_init_pivot = o->n_random_init_pivot;
    if (o->unfolding_scheme != 0 && o->unfolding_scheme != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown unfolding scheme");
    r.unfolding = o->unfolding_scheme ? Unfolding::Fused : Unfolding::Interleaved;
    r.normalize_error = o->normalize_error != 0;
    r.has_seed = o->has_seed != 0;
    r.seed = o->seed;
    r.to_treetci_options().validate();
    return r;
}

std::vector<std::vector<size_t>> qtci_pivots(const size_t* pivots, size_t n_pivots, size_t n_vars)
{
    std::vector<std::vector<size_t>> p;
    for (size_t k = 0; k < n_pivots; ++k) p.emplace_back(pivots + k * n_vars, pivots + (k + 1) * n_vars);
    return p;
}

void qtci_run(t4a_gpu_qtci** out, std::unique_ptr<QuanticsTci> q, int32_t has_pivots, const size_t* pivots,
              size_t n_pivots, const QtciOptions& o)
{
    const auto pv = qtci_pivots(pivots, has_pivots ? n_pivots : 0, q->grid.n_vars());
    q->run(has_pivots ? &pv : nullptr, o);
    auto* h = new t4a_gpu_qtci();
    h->impl = std::move(q);
    *out = h;
}

SvdPolicy convert_policy(const t4a_gpu_svd_policy* p)
{
    SvdPolicy r;
    if (!p) return r;
    r.threshold = p->threshold;
    r.scale = p->scale;
    r.measure = p->measure;
    r.rule = p->rule;
    if (r.scale < 0 || r.scale > 1 || r.measure < 0 || r.measure > 1 || r.rule < 0 || r.rule > 1)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown SVD truncation policy field");
    return r;
}

TensorView host_view(const size_t* dims, const int64_t* labels, size_t rank)
{
    TensorView v;
    v.d_data = nullptr;
    if (rank) {
        T4A_REQUIRE_PTR(dims);
        T4A_REQUIRE_PTR(labels);
    }
    v.dims.assign(dims, dims + rank);
    v.labels.assign(labels, labels + rank);
    size_t n = 1;
    for (size_t d : v.dims) n = checked_mul(n, d, "tensor shape");
    return v;
}

std::unique_ptr<t4a_gpu_tensor> make_tensor(OwnedTensor&& t) { return std::make_unique<t4a_gpu_tensor>(std::move(t)); }

std::unique_ptr<t4a_gpu_tensor> make_tensor(const std::vector<size_t>& dims, const std::vector<int64_t>& labels)
{
    return make_tensor(OwnedTensor(dims, labels));
}

// the tail of the pairwise products: the product of two device tensors as a new handle
t4a_gpu_tensor* contract_to_handle(const TensorView& va, const TensorView& vb, const ContractPlan& plan)
{
    std::lock_guard<std::mutex> lock(g_dense_mutex);
    Engine& e = dense_engine();
    auto t = make_tensor(plan.out_dims, plan.out_labels);
    tensor_contract_pair(e, va, vb, plan, t->buf.get());
    e.sync();
    return t.release();
}

t4a_gpu_tt* wrap_tt(std::unique_ptr<TensorTrain> r)
{
    r->eng.sync();
    return new t4a_gpu_tt(r->cores, r->eng.stream());
}

void cores_dims(const std::vector<DevCore>& cores, size_t* dims3)
{
    if (!cores.empty()) T4A_REQUIRE_PTR(dims3);
    for (size_t s = 0; s < cores.size(); ++s) {
        dims3[3 * s] = cores[s].l;
        dims3[3 * s + 1] = cores[s].s;
        dims3[3 * s + 2] = cores[s].r;
    }
}

void core_to_host(Engine* eng, const std::vector<DevCore>& cores, size_t site, double* out)
{
    if (site >= cores.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "site " + std::to_string(site) + " is out of range for " + std::to_string(cores.size()) + " tensors");
    const DevCore& c = cores[site];
    if (c.size() == 0) return;
    T4A_REQUIRE_PTR(out);
    T4A_HIP(hipMemcpyAsync(out, c.buf.get(), c.size() * sizeof(double), hipMemcpyDeviceToHost, eng->stream()));
    eng->sync();
}

void vector_out(const std::vector<double>& v, double* out, size_t capacity, size_t* len)
{
    T4A_REQUIRE_PTR(len);
    *len = v.size();
    if (!out) return;
    if (capacity < v.size())
        throw Error(T4A_GPU_BUFFER_TOO_SMALL, "output capacity " + std::to_string(capacity) + " is below " + std::to_string(v.size()));
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(double));
}

t4a_gpu_tt* tt_from_cores(const std::vector<DevCore>& cores, hipStream_t stream) { return new t4a_gpu_tt(cores, stream); }

AciOptions convert_aci(const t4a_gpu_aci_options* o)
{
    AciOptions a;
    if (o) {
        a.max_iters = o->max_iters;
        a.min_iters = o->min_iters;
        a.has_max_bond_dim = o->has_max_bond_dim != 0;
        a.max_bond_dim = o->max_bond_dim;
        a.tolerance = o->tolerance;
        a.scale_tolerance = o->scale_tolerance != 0;
        a.rng_seed = o->rng_seed;
        a.enable_global_guard = o->enable_global_guard != 0;
        a.nsearch_global_pivots = o->nsearch_global_pivots;
        a.max_nglobal_pivot = o->max_nglobal_pivot;
        a.nsweeps_global_search = o->nsweeps_global_search;
        a.tol_margin_global_search = o->tol_margin_global_search;
    }
    return a;
}

AciOpKind aci_op_kind(int32_t kind, const char* unknown_message)
{
    if (kind < 0 || kind > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, unknown_message);
    return (AciOpKind)kind;
}

std::vector<TensorTrain*> aci_inputs(const t4a_gpu_tt* const* inputs, size_t n)
{
    if (n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "inputs must not be empty");
    if (!inputs) throw Error(T4A_GPU_NULL_POINTER, "inputs is null");
    return handle_list(inputs, n, "input tensor train is null", [](const t4a_gpu_tt& t) { return const_cast<TensorTrain*>(&t.impl); });
}

// the positions of every operator of t4a_gpu_linop_exclusive / _compose, one list per operator
std::vector<std::vector<size_t>> linop_supports(const size_t* sites, const size_t* lens, size_t n_ops)
{
    std::vector<std::vector<size_t>> s(n_ops);
    size_t off = 0;
    for (size_t q = 0; q < n_ops; ++q) {
        s[q].assign(sites + off, sites + off + lens[q]);
        off += lens[q];
    }
    return s;
}

PartialSpec partial_spec(const size_t* contract_pairs, size_t n_contract, const size_t* diagonal_pairs, size_t n_diagonal, size_t n_output_order)
{
    PartialSpec spec;
    if (n_contract) T4A_REQUIRE_PTR(contract_pairs);
    if (n_diagonal) T4A_REQUIRE_PTR(diagonal_pairs);
    for (size_t i = 0; i < n_contract; ++i)
        spec.contract_pairs.push_back({contract_pairs[4 * i], contract_pairs[4 * i + 1], contract_pairs[4 * i + 2], contract_pairs[4 * i + 3]});
    for (size_t i = 0; i < n_diagonal; ++i)
        spec.diagonal_pairs.push_back({diagonal_pairs[4 * i], diagonal_pairs[4 * i + 1], diagonal_pairs[4 * i + 2], diagonal_pairs[4 * i + 3]});
    spec.has_output_order = n_output_order != 0;
    return spec;
}

void contraction_environment(t4a_gpu_contraction* h, bool left, size_t n, const size_t* idx, size_t n_pts, double* out, size_t* dims2)
{
    T4A_REQUIRE_PTR(h);
    T4A_REQUIRE_PTR(dims2);
    const std::array<size_t, 2> d = left ? h->impl->left_dims(n) : h->impl->right_dims(n); // n out of range is refused here
    dims2[0] = d[0];
    dims2[1] = d[1];
    if (n_pts == 0) return;
    T4A_REQUIRE_PTR(idx);
    T4A_REQUIRE_PTR(out);
    std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, 2 * h->impl->len(), "index buffer"));
    if (left)
        h->impl->evaluate_left(n, u.data(), n_pts, out, dims2);
    else
        h->impl->evaluate_right(n, u.data(), n_pts, out, dims2);
}

// the entry points of the candidate matrices of A·B answer INVALID_ARGUMENT for NULL (t4a_gpu.h)
#define T4A_REQUIRE_ARG(p)                                                            \
    do {                                                                              \
        if ((p) == nullptr) throw ::t4a::Error(T4A_GPU_INVALID_ARGUMENT, #p " is null"); \
    } while (0)

LinsolveOptions convert_linsolve_options(const t4a_gpu_linsolve_options* p)
{
    LinsolveOptions o;
    o.nfullsweeps = p->nfullsweeps;
    o.has_max_bond_dim = p->has_max_bond_dim != 0;
    o.max_bond_dim = p->max_bond_dim;
    o.has_svd_policy = p->has_svd_policy != 0;
    if (o.has_svd_policy) o.svd_policy = from_c(p->svd_policy);
    o.gmres_tol = p->gmres_tol;
    if (p->gmres_tolerance_mode != 0 && p->gmres_tolerance_mode != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown gmres_tolerance_mode");
    o.gmres_tolerance_mode = (GmresToleranceMode)p->gmres_tolerance_mode;
    o.gmres_max_restarts = p->gmres_max_restarts;
    o.gmres_restart_dim = p->gmres_restart_dim;
    o.a0 = p->a0;
    o.a1 = p->a1;
    o.has_convergence_tol = p->has_convergence_tol != 0;
    o.convergence_tol = p->convergence_tol;
    o.check_residual = p->check_residual != 0;
    o.validate();
    return o;
}

LanczosOptions convert_lanczos_options(const t4a_gpu_lanczos_options& p)
{
    LanczosOptions o;
    o.max_iter = p.max_iter;
    o.rtol = p.rtol;
    o.atol = p.atol;
    o.breakdown_tol = p.breakdown_tol;
    o.hermitian_tol = p.hermitian_tol;
    return o;
}

DmrgOptions convert_dmrg_options(const t4a_gpu_dmrg_options* p)
{
    DmrgOptions o;
    o.nsite = p->nsite;
    o.nsweeps = p->nsweeps;
    o.has_max_bond_dim = p->has_max_bond_dim != 0;
    o.max_bond_dim = p->max_bond_dim;
    o.has_svd_policy = p->has_svd_policy != 0;
    if (o.has_svd_policy) o.svd_policy = from_c(p->svd_policy);
    o.lanczos = convert_lanczos_options(p->lanczos);
    o.has_energy_tol = p->has_energy_tol != 0;
    o.energy_tol = p->energy_tol;
    o.real_scalar_tol = p->real_scalar_tol;
    o.validate();
    return o;
}

FitSumOptions convert_fit_sum_options(const t4a_gpu_fit_sum_options* p)
{
    FitSumOptions o;
    o.nfullsweeps = p->nfullsweeps;
    o.has_max_bond_dim = p->has_max_bond_dim != 0;
    o.max_bond_dim = p->max_bond_dim;
    o.has_svd_policy = p->has_svd_policy != 0;
    if (o.has_svd_policy) o.svd_policy = from_c(p->svd_policy);
    o.has_qr_rtol = p->has_qr_rtol != 0;
    o.qr_rtol = p->qr_rtol;
    o.factorize_alg = p->factorize_alg;
    o.has_convergence_tol = p->has_convergence_tol != 0;
    o.convergence_tol = p->convergence_tol;
    o.validate();
    return o;
}

FitSumRoute convert_fit_sum_route(int32_t route, bool allow_auto)
{
    if (route < (allow_auto ? 0 : 1) || route > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, allow_auto ? "fit_sum: unknown route" : "fit_sum: the route must be fused or gemm");
    return (FitSumRoute)route;
}

KrylovExpmOptions convert_krylov_expm_options(const t4a_gpu_krylov_expm_options& p)
{
    KrylovExpmOptions o;
    o.max_iter = p.max_iter;
    o.max_time_splits = p.max_time_splits;
    o.tol = p.tol;
    o.breakdown_tol = p.breakdown_tol;
    o.hermitian_tol = p.hermitian_tol;
    return o;
}

TdvpOptions convert_tdvp_options(const t4a_gpu_tdvp_options* p, TdvpMode mode)
{
    TdvpOptions o;
    o.nsite = p->nsite;
    o.nsweeps = p->nsweeps;
    o.order = p->order;
    o.exponent_step_re = p->exponent_step_re;
    o.exponent_step_im = p->exponent_step_im;
    o.has_max_bond_dim = p->has_max_bond_dim != 0;
    o.max_bond_dim = p->max_bond_dim;
    o.has_svd_policy = p->has_svd_policy != 0;
    if (o.has_svd_policy) o.svd_policy = from_c(p->svd_policy);
    o.krylov = convert_krylov_expm_options(p->krylov);
    o.validate(mode);
    return o;
}

// ---- what the two-site and the one-site TDVP entry points share: each is its mode, its name and its own stats struct
void check_tdvp_shapes(TdvpMode mode, const size_t* op_dims4, size_t n_op, const size_t* state_dims3, size_t n_state, size_t center, size_t max_iter)
{
    if (n_op) T4A_REQUIRE_PTR(op_dims4);
    if (n_state) T4A_REQUIRE_PTR(state_dims3);
    KrylovExpmOptions ko;
    ko.max_iter = max_iter;
    ko.validate();
    tdvp_validate_shapes(mode, dims4_list(op_dims4, n_op), dims3_list(state_dims3, n_state), center, max_iter);
}

// The plan into the caller's arrays; all four null: the count only.  `who` names the entry point in BUFFER_TOO_SMALL.
void write_tdvp_plan(const char* who, const std::vector<TdvpStep>& plan, size_t capacity, int32_t* kinds, size_t* nodes, size_t* new_centers, double* exponents,
                     size_t* n_steps)
{
    *n_steps = plan.size();
    if (!kinds && !nodes && !new_centers && !exponents) return;
    if (capacity < plan.size()) throw Error(T4A_GPU_BUFFER_TOO_SMALL, std::string(who) + ": the plan has " + std::to_string(plan.size()) + " steps");
    T4A_REQUIRE_PTR(kinds);
    T4A_REQUIRE_PTR(nodes);
    T4A_REQUIRE_PTR(new_centers);
    T4A_REQUIRE_PTR(exponents);
    for (size_t k = 0; k < plan.size(); ++k) {
        kinds[k] = (int32_t)plan[k].kind;
        nodes[2 * k] = plan[k].nodes[0];
        nodes[2 * k + 1] = plan[k].nodes[1];
        new_centers[k] = plan[k].new_center;
        exponents[k] = plan[k].exponent;
    }
}

// -> the counters of the run, for the entry point's own stats struct
TdvpStats run_tdvp(TdvpMode mode, const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_tdvp_options* options, t4a_gpu_tt** state,
                   size_t* sweeps_completed, size_t* local_updates, double* max_error_estimate, size_t* max_krylov_iterations)
{
    T4A_REQUIRE_PTR(state);
    *state = nullptr;
    T4A_REQUIRE_PTR(options);
    const TdvpOptions o = convert_tdvp_options(options, mode); // the options are checked on the host before an operand is looked at
    T4A_REQUIRE_PTR(op);
    T4A_REQUIRE_PTR(init);
    T4A_REQUIRE_PTR(sweeps_completed);
    T4A_REQUIRE_PTR(local_updates);
    T4A_REQUIRE_PTR(max_error_estimate);
    T4A_REQUIRE_PTR(max_krylov_iterations);
    TdvpResult r = tdvp(mode, *op->impl, const_cast<t4a_gpu_tt*>(init)->impl, center, o);
    *state = new t4a_gpu_tt(r.state->cores, r.state->eng.stream());
    *sweeps_completed = r.sweeps_completed;
    *local_updates = r.local_updates;
    *max_error_estimate = r.max_error_estimate;
    *max_krylov_iterations = r.max_krylov_iterations;
    return r.stats;
}

GseOptions convert_gse_options(const t4a_gpu_gse_options* p)
{
    GseOptions o;
    o.krylov_dim = p->krylov_dim;
    o.has_reference_max_bond_dim = p->has_reference_max_bond_dim != 0;
    o.reference_max_bond_dim = p->reference_max_bond_dim;
    o.has_reference_svd_policy = p->has_reference_svd_policy != 0;
    if (o.has_reference_svd_policy) o.reference_svd_policy = from_c(p->reference_svd_policy);
    o.density_weight_cutoff = p->density_weight_cutoff;
    o.hermitian_tol = p->hermitian_tol;
    o.normalize_references = p->normalize_references != 0;
    o.expand_before_first_sweep = p->expand_before_first_sweep != 0;
    o.validate();
    return o;
}

void gse_counters(const GseResult& r, size_t* references_built, size_t* edges_processed, size_t* bonds_expanded, size_t* max_added_basis)
{
    *references_built = r.references_built;
    *edges_processed = r.edges_processed;
    *bonds_expanded = r.bonds_expanded;
    *max_added_basis = r.max_added_basis;
}

// t4a_gpu_gse_tdvp and t4a_gpu_gse_tdvp_one_site but for the mode
void run_gse_tdvp(TdvpMode mode, const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_gse_options* gse, const t4a_gpu_tdvp_options* tdvp_options,
                  t4a_gpu_tt** state, size_t* sweeps_completed, size_t* local_updates, size_t* gse_expansions, double* max_error_estimate,
                  size_t* max_krylov_iterations)
{
    T4A_REQUIRE_PTR(state);
    *state = nullptr;
    T4A_REQUIRE_PTR(gse);
    T4A_REQUIRE_PTR(tdvp_options);
    GseTdvpOptions o;
    o.gse = convert_gse_options(gse); // the options are checked on the host before an operand is looked at
    o.tdvp = convert_tdvp_options(tdvp_options, mode);
    T4A_REQUIRE_PTR(op);
    T4A_REQUIRE_PTR(init);
    T4A_REQUIRE_PTR(sweeps_completed);
    T4A_REQUIRE_PTR(local_updates);
    T4A_REQUIRE_PTR(gse_expansions);
    T4A_REQUIRE_PTR(max_error_estimate);
    T4A_REQUIRE_PTR(max_krylov_iterations);
    GseTdvpResult r = gse_tdvp(mode, *op->impl, const_cast<t4a_gpu_tt*>(init)->impl, center, o);
    *state = new t4a_gpu_tt(r.state->cores, r.state->eng.stream());
    *sweeps_completed = r.sweeps_completed;
    *local_updates = r.local_updates;
    *gse_expansions = r.gse_expansions;
    *max_error_estimate = r.max_error_estimate;
    *max_krylov_iterations = r.max_krylov_iterations;
}

// the ragged shape lists of the hooks as ints: every entry positive, at most `max_jobs` of them
std::vector<int> gse_int_list(const size_t* v, size_t n, size_t max_jobs, const char* who)
{
    if (n == 0 || n > max_jobs) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": between 1 and " + std::to_string(max_jobs) + " operands");
    T4A_REQUIRE_PTR(v);
    std::vector<int> out(n);
    for (size_t i = 0; i < n; ++i) {
        if (v[i] == 0 || v[i] > (size_t)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": every dimension must be positive and at most INT_MAX");
        out[i] = (int)v[i];
    }
    return out;
}

void gse_require_fits(size_t a, size_t b, const char* who)
{
    if (a == 0 || b == 0 || a > (size_t)INT_MAX || b > (size_t)INT_MAX / a)
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(who) + ": every dimension must be positive and every matrix within INT_MAX elements");
}

std::vector<LegProjector> projector_list(const size_t* entries, const size_t* counts, size_t n)
{
    std::vector<LegProjector> v(n);
    if (n) T4A_REQUIRE_PTR(counts);
    size_t off = 0;
    for (size_t k = 0; k < n; ++k) {
        v[k] = projector_from_triples(entries ? entries + 3 * off : nullptr, counts[k]);
        off += counts[k];
    }
    return v;
}

void projector_out(const LegProjector& p, size_t* out, size_t* out_count)
{
    T4A_REQUIRE_PTR(out_count);
    *out_count = p.size();
    if (!out) return;
    size_t i = 0;
    for (const auto& kv : p) {
        out[3 * i] = kv.first.first;
        out[3 * i + 1] = kv.first.second;
        out[3 * i + 2] = kv.second;
        ++i;
    }
}

SiteDims site_dims_list(const size_t* site_dims, size_t n_sites)
{
    if (n_sites) T4A_REQUIRE_PTR(site_dims);
    SiteDims sd(n_sites);
    for (size_t i = 0; i < n_sites; ++i) sd[i] = {site_dims[2 * i], site_dims[2 * i + 1]};
    return sd;
}

MpoContractionOptions pmpo_options(double tolerance, size_t max_bond_dim, int32_t method)
{
    if (method < 0 || method > 3) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown factorize method");
    MpoContractionOptions o;
    o.tolerance = tolerance;
    o.max_bond_dim = max_bond_dim;
    o.method = (MpoFactorizeMethod)method;
    return o;
}

CompressRoute compress_route(int32_t route)
{
    if (route < 0 || route > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown compress route");
    return (CompressRoute)route;
}

std::vector<Mpo*> mpo_list(const t4a_gpu_mpo* const* mpos, size_t count, const char* what)
{
    if (count == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(what) + ": the list is empty");
    T4A_REQUIRE_PTR(mpos);
    std::vector<Mpo*> items(count);
    for (size_t k = 0; k < count; ++k) {
        if (!mpos[k]) throw Error(T4A_GPU_NULL_POINTER, std::string(what) + ": item " + std::to_string(k) + " is null");
        items[k] = mpos[k]->impl.get();
    }
    return items;
}

std::vector<BtRule> truncate_rules(const t4a_gpu_svd_policy* policies, const size_t* max_bond_dims, size_t count)
{
    if (count) T4A_REQUIRE_PTR(policies);
    std::vector<BtRule> rules(count);
    for (size_t k = 0; k < count; ++k) {
        const SvdPolicy p{policies[k].threshold, policies[k].scale, policies[k].measure, policies[k].rule}; // (fields are checked by the driver, per item)
        rules[k] = bt_rule(p, max_bond_dims ? max_bond_dims[k] : 0);
    }
    return rules;
}

void truncate_out(std::vector<std::unique_ptr<Mpo>>& res, const std::vector<std::vector<size_t>>& b, const TruncateManyStats& st, bool ranks_only,
                  t4a_gpu_mpo** out, size_t* bonds, size_t* counts4)
{
    if (!ranks_only) {
        std::vector<t4a_gpu_mpo*> handles;
        for (auto& m : res) handles.push_back(new t4a_gpu_mpo{std::move(m)});
        for (size_t k = 0; k < res.size(); ++k) out[k] = handles[k];
    }
    if (bonds) {
        size_t at = 0;
        for (const auto& v : b)
            for (size_t x : v) bonds[at++] = x;
    }
    if (counts4) {
        counts4[0] = st.launches;
        counts4[1] = st.syncs;
        counts4[2] = st.n_batched;
        counts4[3] = st.n_serial;
    }
}

PatchingOptions patching_options(const t4a_gpu_patching_options* o)
{
    PatchingOptions r;
    if (!o) return r;
    r.rtol = o->rtol;
    r.has_max_bond_dim = o->has_max_bond_dim != 0;
    r.max_bond_dim = o->max_bond_dim;
    if (o->n_patch_order) T4A_REQUIRE_PTR(o->patch_order);
    for (size_t k = 0; k < o->n_patch_order; ++k) r.patch_order.push_back({o->patch_order[2 * k], o->patch_order[2 * k + 1]});
    if (o->split_strategy < 0 || o->split_strategy > 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown patch split strategy");
    r.split_strategy = (PatchSplitStrategy)o->split_strategy;
    return r;
}

void patching_counts(const PatchingStats& st, size_t* counts6)
{
    if (!counts6) return;
    counts6[0] = st.rounds, counts6[1] = st.truncate_calls, counts6[2] = st.ranks_only_calls;
    counts6[3] = st.launches, counts6[4] = st.syncs, counts6[5] = st.splits;
}

SiteLegs site_legs(size_t n, const size_t* leg_counts, const int64_t* keys, const size_t* dims)
{
    SiteLegs legs(n);
    if (n) T4A_REQUIRE_PTR(leg_counts);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < leg_counts[i]; ++k, ++at) {
            T4A_REQUIRE_PTR(keys);
            T4A_REQUIRE_PTR(dims);
            legs[i].push_back({keys[at], dims[at]});
        }
    return legs;
}

void write_legs(const SiteLegs& legs, size_t* leg_counts, int64_t* keys, size_t* dims)
{
    size_t at = 0;
    for (size_t i = 0; i < legs.size(); ++i) {
        if (leg_counts) leg_counts[i] = legs[i].size();
        for (const SwapLeg& g : legs[i]) {
            if (keys) keys[at] = g.key;
            if (dims) dims[at] = g.dim;
            ++at;
        }
    }
}

SwapAssignment assignment(const int64_t* keys, const size_t* sites, size_t count)
{
    SwapAssignment a;
    if (count) {
        T4A_REQUIRE_PTR(keys);
        T4A_REQUIRE_PTR(sites);
    }
    for (size_t k = 0; k < count; ++k) a.push_back({keys[k], sites[k]});
    return a;
}

std::vector<SwapLeg> leg_list(const int64_t* keys, const size_t* dims, size_t count)
{
    std::vector<SwapLeg> v;
    if (count) {
        T4A_REQUIRE_PTR(keys);
        T4A_REQUIRE_PTR(dims);
    }
    for (size_t k = 0; k < count; ++k) v.push_back({keys[k], dims[k]});
    return v;
}

RestructureTarget restructure_target(size_t n_groups, const size_t* group_counts, const int64_t* group_keys)
{
    RestructureTarget t(n_groups);
    if (n_groups) T4A_REQUIRE_PTR(group_counts);
    size_t at = 0;
    for (size_t j = 0; j < n_groups; ++j)
        for (size_t k = 0; k < group_counts[j]; ++k, ++at) {
            T4A_REQUIRE_PTR(group_keys);
            t[j].push_back(group_keys[at]);
        }
    return t;
}

SplitOptions split_options(int32_t form, const t4a_gpu_svd_policy* policy, int32_t has_max_bond_dim, size_t max_bond_dim, int32_t final_sweep)
{
    SplitOptions o;
    o.form = form;
    o.has_policy = policy != nullptr;
    if (policy) o.policy = SvdPolicy{policy->threshold, policy->scale, policy->measure, policy->rule};
    o.has_max_bond_dim = has_max_bond_dim != 0, o.max_bond_dim = max_bond_dim;
    o.final_sweep = final_sweep != 0;
    return o;
}

size_t center_in(int64_t center, size_t n)
{
    if (center < 0) return NO_CENTER;
    if ((size_t)center >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "the centre " + std::to_string(center) + " is not a site of the train");
    return (size_t)center;
}

t4a_gpu_status tt_fuse_to(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims, int64_t center,
                          size_t n_groups, const size_t* group_counts, const int64_t* group_keys, t4a_gpu_tt** out, size_t* out_leg_counts,
                          int64_t* out_keys, size_t* out_dims, int64_t* out_center, size_t* launches)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(tt);
        SiteLegs legs = site_legs(tt->impl.len(), leg_counts, keys, dims);
        const RestructureTarget target = restructure_target(n_groups, group_counts, group_keys);
        const size_t c = center_in(center, tt->impl.len());
        std::vector<size_t> links;
        for (size_t i = 0; i + 1 < tt->impl.len(); ++i) links.push_back(tt->impl.cores[i].r);
        fuse_plan(legs, target, &links); // the refusals, before the device is touched
        // the work happens on a copy with an engine of its own; the input stays as it is
        std::unique_ptr<t4a_gpu_tt> res(new t4a_gpu_tt(tt->impl.cores, tt->impl.eng.stream()));
        const RestructureResult r = fuse_to(res->impl.eng, res->impl.cores, legs, target, c);
        res->impl.eng.sync();
        write_legs(legs, out_leg_counts, out_keys, out_dims);
        if (out_center) *out_center = r.center == NO_CENTER ? -1 : (int64_t)r.center;
        if (launches) *launches = r.launches;
        *out = res.release();
    });
}

// what t4a_gpu_tt_fit_sum and t4a_gpu_mpo_fit_sum share: the checks in their order, the operands of the handles, the scalar outputs
template <class H, class Cores, class Eng, class Pre, class Wrap>
void fit_sum_entry(const H* const* targets, size_t n_targets, const double* coefficients, const H* initial, size_t center,
                   const t4a_gpu_fit_sum_options* options, int32_t route, size_t* sweeps_completed, size_t* local_updates, int32_t* converged,
                   double* norms, Cores&& cores_of, Eng&& engine_of, Pre&& pre, Wrap&& wrap)
{
    T4A_REQUIRE_PTR(options);
    const FitSumOptions o = convert_fit_sum_options(options); // the options are checked on the host before an operand is looked at
    const FitSumRoute rt = convert_fit_sum_route(route, true);
    if (n_targets == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "fit_sum: targets must not be empty");
    T4A_REQUIRE_PTR(targets);
    T4A_REQUIRE_PTR(sweeps_completed);
    T4A_REQUIRE_PTR(local_updates);
    T4A_REQUIRE_PTR(converged);
    std::vector<const std::vector<DevCore>*> cores;
    std::vector<Engine*> engines;
    for (size_t k = 0; k < n_targets; ++k) {
        if (!targets[k]) throw Error(T4A_GPU_NULL_POINTER, "fit_sum: target " + std::to_string(k) + " is null");
        cores.push_back(cores_of(targets[k]));
        engines.push_back(engine_of(targets[k]));
    }
    pre();
    FitSumResult r = fit_sum(cores, engines, coefficients, initial ? cores_of(initial) : nullptr, initial ? engine_of(initial) : nullptr, center, o, rt);
    wrap(r);
    *sweeps_completed = r.sweeps_completed;
    *local_updates = r.local_updates;
    *converged = r.converged;
    if (norms)
        for (size_t i = 0; i < r.norms.size(); ++i) norms[i] = r.norms[i];
}

} // namespace

extern "C" {

t4a_gpu_status t4a_gpu_last_error_message(char* buf, size_t buf_len, size_t* required_len)
{
    const std::string& msg = last_error_ref();
    const size_t need = msg.size() + 1;
    if (required_len) *required_len = need;
    if (!buf) return required_len ? T4A_GPU_SUCCESS : T4A_GPU_NULL_POINTER;
    if (buf_len < need) return T4A_GPU_BUFFER_TOO_SMALL;
    std::memcpy(buf, msg.c_str(), need);
    return T4A_GPU_SUCCESS;
}

t4a_gpu_status t4a_gpu_stdrng_sample(uint64_t seed, const size_t* dims, size_t n, size_t* out)
{
    return guarded([&] {
        if (n == 0) return;
        T4A_REQUIRE_PTR(dims);
        T4A_REQUIRE_PTR(out);
        for (size_t i = 0; i < n; ++i)
            if (dims[i] == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "random_range(0..0): empty range");
        StdRng rng(seed);
        for (size_t i = 0; i < n; ++i) out[i] = rng.random_range(dims[i]);
    });
}

t4a_gpu_status t4a_gpu_chacha_block(const uint32_t* key8, uint64_t counter, uint64_t stream, int32_t rounds, uint32_t* out16)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(key8);
        T4A_REQUIRE_PTR(out16);
        if (rounds <= 0 || (rounds & 1)) throw Error(T4A_GPU_INVALID_ARGUMENT, "ChaCha rounds must be a positive even number");
        StdRng::block(key8, counter, (uint32_t)stream, (uint32_t)(stream >> 32), rounds, out16);
    });
}

// ---- the other two random streams of the reference (smallrng.hpp): known-answer entry points, host only ----
t4a_gpu_status t4a_gpu_siphash(const uint8_t* msg, size_t len, uint64_t k0, uint64_t k1, int32_t c_rounds, int32_t d_rounds, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        if (len > 0) T4A_REQUIRE_PTR(msg);
        if (c_rounds == 1 && d_rounds == 3) {
            SipHasher<1, 3> h(k0, k1);
            h.write(msg, len);
            *out = h.finish();
        } else if (c_rounds == 2 && d_rounds == 4) {
            SipHasher<2, 4> h(k0, k1);
            h.write(msg, len);
            *out = h.finish();
        } else {
            throw Error(T4A_GPU_INVALID_ARGUMENT, "SipHash-1-3 or SipHash-2-4");
        }
    });
}

t4a_gpu_status t4a_gpu_smallrng_words(uint64_t seed, const uint64_t* state4, size_t n, uint64_t* out)
{
    return guarded([&] {
        if (n == 0) return;
        T4A_REQUIRE_PTR(out);
        SmallRng rng = state4 ? SmallRng::from_state(state4) : SmallRng(seed);
        for (size_t i = 0; i < n; ++i) out[i] = rng.next_u64();
    });
}

t4a_gpu_status t4a_gpu_smallrng_sample(uint64_t seed, const size_t* dims, size_t n, size_t* out)
{
    return guarded([&] {
        if (n == 0) return;
        T4A_REQUIRE_PTR(dims);
        T4A_REQUIRE_PTR(out);
        for (size_t i = 0; i < n; ++i)
            if (dims[i] == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "random_range(0..0): empty range");
        SmallRng rng(seed);
        for (size_t i = 0; i < n; ++i) out[i] = rng.random_range(dims[i]);
    });
}

t4a_gpu_status t4a_gpu_smallrng_shuffle(uint64_t seed, size_t n, size_t* out)
{
    return guarded([&] {
        if (n == 0) return;
        T4A_REQUIRE_PTR(out);
        std::vector<size_t> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = i;
        SmallRng rng(seed);
        rng.shuffle(v);
        for (size_t i = 0; i < n; ++i) out[i] = v[i];
    });
}

t4a_gpu_status t4a_gpu_tree_edge_seed(uint64_t seed, const char* tag, size_t u, size_t v, size_t history_len, size_t n_pivots_i, size_t n_pivots_j, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tag);
        T4A_REQUIRE_PTR(out);
        DefaultHasher h;
        h.write_u64(seed);
        h.write_str(tag, std::strlen(tag));
        h.write_usize(std::min(u, v));
        h.write_usize(std::max(u, v));
        h.write_usize(history_len);
        h.write_usize(n_pivots_i);
        h.write_usize(n_pivots_j);
        *out = h.finish();
    });
}

t4a_gpu_status t4a_gpu_chacha8_standard_normal(uint64_t seed, size_t n, double* out, size_t n_words, uint32_t* out_words)
{
    return guarded([&] {
        if (n > 0) {
            T4A_REQUIRE_PTR(out);
            ChaCha8Rng rng(seed);
            for (size_t i = 0; i < n; ++i) out[i] = StandardNormal::sample(rng);
        }
        if (n_words > 0) {
            T4A_REQUIRE_PTR(out_words);
            ChaCha8Rng rng(seed);
            for (size_t i = 0; i < n_words; ++i) out_words[i] = rng.next_u32();
        }
    });
}

t4a_gpu_status t4a_gpu_device_count(int32_t* out_count)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out_count);
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
        *out_count = c;
    });
}

t4a_gpu_status t4a_gpu_set_device(int32_t device)
{
    return guarded([&] {
        require_device();
        T4A_HIP(hipSetDevice(device));
    });
}

const char* t4a_gpu_version(void) { return "t4a-mi355x 0.1.0 (gfx950)"; }

int32_t t4a_gpu_diag_switches_enabled(void) { return 0; }

// ------------------------------------------------------------------------------------------------ dense
t4a_gpu_status t4a_gpu_rrlu_f64(double* a_inout, size_t m, size_t n, size_t max_bond_dim, double rel_tol,
                                double abs_tol, int32_t left_orthogonal, size_t* row_perm, size_t* col_perm,
                                size_t* npivots, double* last_error)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(row_perm);
        T4A_REQUIRE_PTR(col_perm);
        T4A_REQUIRE_PTR(npivots);
        T4A_REQUIRE_PTR(last_error);
        const size_t count = checked_mul(m, n, "matrix shape");
        require_int_dims({m, n}, "matrix shape");
        if (count) T4A_REQUIRE_PTR(a_inout);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_a = e.pi(std::max<size_t>(count, 1));
        upload(e, d_a, a_inout, count);
        LuciResult r = e.luci(d_a, (int)m, (int)n, RrLUOptions::from_abi(max_bond_dim, rel_tol, abs_tol, left_orthogonal != 0), false, true);
        if (count) download(e, a_inout, e.lu_buf(), count);
        for (size_t i = 0; i < m; ++i) row_perm[i] = (size_t)r.row_perm[i];
        for (size_t j = 0; j < n; ++j) col_perm[j] = (size_t)r.col_perm[j];
        *npivots = (size_t)r.rank;
        *last_error = r.last_error;
    });
}

t4a_gpu_status t4a_gpu_luci_f64(const double* a, size_t m, size_t n, size_t max_bond_dim, double rel_tol,
                                double abs_tol, int32_t left_orthogonal, size_t* rank, size_t* rows, size_t* cols,
                                double* pivot_errors, double* left, double* right)
{
    return guarded([&] {
        const size_t count = luci_prologue(m, n, rank, rows, cols, pivot_errors, a == nullptr, "a is null", left, right, false);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_a = e.pi(std::max<size_t>(count, 1));
        upload(e, d_a, a, count);
        LuciResult r = e.luci(d_a, (int)m, (int)n, RrLUOptions::from_abi(max_bond_dim, rel_tol, abs_tol, left_orthogonal != 0), true, false);
        luci_outputs(e, r, m, n, rank, rows, cols, pivot_errors, left, right);
    });
}

t4a_gpu_status t4a_gpu_gemm_batched_f64(size_t batch, size_t m, size_t k, size_t n, const double* a, const double* b,
                                        double* c)
{
    return guarded([&] {
        const size_t na = checked_mul(checked_mul(m, k, "a shape"), batch, "a shape");
        const size_t nb = checked_mul(checked_mul(k, n, "b shape"), batch, "b shape");
        const size_t nc = checked_mul(checked_mul(m, n, "c shape"), batch, "c shape");
        require_int_dims({m, n, k, batch}, "gemm shape");
        if (na) T4A_REQUIRE_PTR(a);
        if (nb) T4A_REQUIRE_PTR(b);
        if (nc) T4A_REQUIRE_PTR(c);
        if (nc == 0) return;
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        e.d_tmp.reserve(std::max<size_t>(na + nb, 1));
        e.d_tmp2.reserve(nc);
        double* da = e.d_tmp.get();
        double* db = da + na;
        StreamSyncOnExit sync_on_exit(e);
        upload_async(e, da, a, na);
        upload_async(e, db, b, nb);
        if (k == 0) {
            fill_launch(e.d_tmp2.get(), nc, 0.0, e.stream());
        } else {
            GemmDesc g = gemm_desc((int)m, (int)n, (int)k, da, (int)m, db, (int)k, e.d_tmp2.get(), (int)m);
            g.strideA = (long long)(m * k);
            g.strideB = (long long)(k * n);
            g.strideC = (long long)(m * n);
            g.batch = (int)batch;
            gemm_launch(g, e.stream());
        }
        T4A_HIP(hipGetLastError());
        download(e, c, e.d_tmp2.get(), nc);
    });
}

t4a_gpu_status t4a_gpu_gemm_f64(const double* a, const double* b, size_t m, size_t k, size_t n, double* c)
{
    return t4a_gpu_gemm_batched_f64(1, m, k, n, a, b, c);
}

t4a_gpu_status t4a_gpu_gemm_route(size_t m, size_t n, size_t k, size_t batch, int32_t* bn, int32_t* ksplit, int32_t* grid_m, int32_t* grid_n,
                                  int32_t* remapped)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(bn);
        T4A_REQUIRE_PTR(ksplit);
        T4A_REQUIRE_PTR(grid_m);
        T4A_REQUIRE_PTR(grid_n);
        T4A_REQUIRE_PTR(remapped);
        require_int_dims({m, n, k, batch}, "gemm_route");
        if (m == 0 || n == 0 || batch == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "gemm_route: m, n and batch must be positive (an empty product launches nothing)");
        const GemmPlan p = gemm_plan((int)m, (int)n, (int)k, (int)batch);
        *bn = p.bn;
        *ksplit = p.ksplit;
        *grid_m = p.grid_m;
        *grid_n = p.grid_n;
        *remapped = p.remapped ? 1 : 0;
    });
}

t4a_gpu_status t4a_gpu_gemm_desc_f64(const t4a_gpu_gemm_desc* descs, size_t n_descs, const double* a, size_t na, const double* b, size_t nb,
                                     double* c, size_t nc)
{
    return guarded([&] {
        if (n_descs) T4A_REQUIRE_PTR(descs);
        if (na) T4A_REQUIRE_PTR(a);
        if (nb) T4A_REQUIRE_PTR(b);
        if (nc) T4A_REQUIRE_PTR(c);
        checked_mul(checked_mul(std::max(std::max(na, nb), nc), 2, "gemm_desc buffers"), sizeof(double), "gemm_desc buffers");
        for (size_t i = 0; i < n_descs; ++i) require_gemm_desc(descs[i], i, na, nb, nc);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        e.d_tmp.reserve(std::max<size_t>(na + nb, 1));
        e.d_tmp2.reserve(std::max<size_t>(nc, 1));
        double* da = e.d_tmp.get();
        double* db = da + na;
        double* dc = e.d_tmp2.get();
        StreamSyncOnExit sync_on_exit(e);
        upload_async(e, da, a, na);
        upload_async(e, db, b, nb);
        upload_async(e, dc, c, nc);
        for (size_t i = 0; i < n_descs; ++i) {
            const t4a_gpu_gemm_desc& d = descs[i];
            GemmDesc g = gemm_desc((int)d.m, (int)d.n, (int)d.k, da + d.off_a, (int)d.lda, db + d.off_b, (int)d.ldb, dc + d.off_c, (int)d.ldc);
            g.transA = d.trans_a;
            g.transB = d.trans_b;
            g.strideA = (long long)d.stride_a;
            g.strideB = (long long)d.stride_b;
            g.strideC = (long long)d.stride_c;
            g.alpha = d.alpha;
            g.beta = d.beta;
            g.batch = (int)d.batch;
            gemm_launch(g, e.stream()); // (queued behind its predecessor: no synchronisation between the products)
        }
        T4A_HIP(hipGetLastError());
        download(e, c, dc, nc);
    });
}

t4a_gpu_status t4a_gpu_trsm_f64(const double* a, size_t na, const double* b, size_t bm, size_t bn, int32_t left_side,
                                int32_t lower, int32_t transpose_a, int32_t unit_diagonal, double* x)
{
    return guarded([&] {
        const size_t acount = checked_mul(na, na, "a shape");
        const size_t bcount = checked_mul(bm, bn, "b shape");
        require_int_dims({na, bm, bn}, "trsm shape");
        if (left_side ? (bm != na) : (bn != na))
            throw Error(T4A_GPU_INVALID_ARGUMENT, "triangular_solve: dimension mismatch between A and B");
        if (acount) T4A_REQUIRE_PTR(a);
        if (bcount) {
            T4A_REQUIRE_PTR(b);
            T4A_REQUIRE_PTR(x);
        }
        if (bcount == 0) return;
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        e.d_tmp.reserve(2 * acount + 1);
        e.d_tmp2.reserve(2 * bcount + 1);
        upload(e, e.d_tmp.get(), a, acount);
        upload(e, e.d_tmp2.get(), b, bcount);
        trsm(e, e.d_tmp.get(), na, e.d_tmp2.get(), bm, bn, left_side != 0, lower != 0, transpose_a != 0, unit_diagonal != 0);
        download(e, x, e.d_tmp2.get(), bcount);
    });
}

t4a_gpu_status t4a_gpu_solve_f64(const double* a, size_t n, const double* b, size_t nrhs, double* x)
{
    return guarded([&] {
        const size_t acount = checked_mul(n, n, "a shape");
        const size_t bcount = checked_mul(n, nrhs, "b shape");
        require_int_dims({n, nrhs}, "solve shape");
        if (acount) T4A_REQUIRE_PTR(a);
        if (bcount) {
            T4A_REQUIRE_PTR(b);
            T4A_REQUIRE_PTR(x);
        }
        if (bcount == 0) return;
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        e.d_tmp.reserve(acount + 1);
        e.d_tmp2.reserve(bcount + 1);
        upload(e, e.d_tmp.get(), a, acount);
        upload(e, e.d_tmp2.get(), b, bcount);
        solve(e, e.d_tmp.get(), n, e.d_tmp2.get(), nrhs);
        download(e, x, e.d_tmp2.get(), bcount);
    });
}

t4a_gpu_status t4a_gpu_fn_eval(int32_t fid, int32_t n_acc, const double* params, const uint64_t* weights,
                               const size_t* local_dims, size_t n_sites, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(params);
        T4A_REQUIRE_PTR(weights);
        T4A_REQUIRE_PTR(local_dims);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        if (fid < 0 || fid >= T4A_FN_COUNT || n_acc < 1 || n_acc > T4A_FN_MAX_ACC)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown built-in function");
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        FnSource f(std::vector<size_t>(local_dims, local_dims + n_sites));
        f.set_builtin(fid, n_acc, params, weights);
        // fold every full index into its accumulators as a "row"; a single all-zero "column"
        IndexSet rows;
        rows.width = n_sites;
        rows.count = n_pts;
        rows.d.resize(n_pts * n_sites);
        for (size_t p = 0; p < n_pts; ++p)
            for (size_t s = 0; s < n_sites; ++s) {
                const size_t v = idx[p * n_sites + s];
                if (v >= local_dims[s]) throw Error(T4A_GPU_INVALID_ARGUMENT, "index out of bounds");
                rows.d[p * n_sites + s] = (uint32_t)v;
            }
        std::vector<uint64_t> acc, zero((size_t)n_acc, 0);
        f.accumulate(rows, f.offset.data(), acc);
        DevBuf<uint64_t> dacc;
        dacc.reserve(acc.size() + zero.size());
        T4A_HIP(hipMemcpyAsync(dacc.get(), acc.data(), acc.size() * 8, hipMemcpyHostToDevice, e.stream()));
        T4A_HIP(hipMemcpyAsync(dacc.get() + acc.size(), zero.data(), zero.size() * 8, hipMemcpyHostToDevice, e.stream()));
        T4A_HIP(hipStreamSynchronize(e.stream()));
        e.d_tmp.reserve(n_pts);
        pi_eval_launch(f.dev, dacc.get(), (int)n_pts, dacc.get() + acc.size(), 1, e.d_tmp.get(), (int)n_pts, false, nullptr,
                       e.stream());
        T4A_HIP(hipGetLastError());
        download(e, out, e.d_tmp.get(), n_pts);
    });
}

// ------------------------------------------------------------------------------------------------ TCI2
t4a_gpu_status t4a_gpu_tci2_options_default(t4a_gpu_tci2_options* o)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(o);
        std::memset(o, 0, sizeof(*o));
        o->tolerance = 1e-8;
        o->max_iter = 20;
        o->max_bond_dim = 0;
        o->pivot_search = 0;
        o->normalize_error = 1;
        o->verbosity = 0;
        o->max_nglobal_pivot = 5;
        o->nsearch = 5;
        o->sweep_strategy = 2;
        o->strictly_nested = 0;
        o->ncheck_history = 3;
        o->tol_margin_global_search = 10.0;
        o->has_seed = 0;
        o->seed = 0;
    });
}

t4a_gpu_status t4a_gpu_tci2_new(const size_t* local_dims, size_t n_sites, t4a_gpu_tci2** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sites) T4A_REQUIRE_PTR(local_dims);
        std::vector<size_t> d(local_dims, local_dims + n_sites);
        if (d.size() < 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "local_dims should have at least 2 elements");
        for (size_t s = 0; s < d.size(); ++s) {
            if (d[s] == 0)
                throw Error(T4A_GPU_INVALID_ARGUMENT, "local dimension at site " + std::to_string(s) + " must be positive");
            if (d[s] > 0xFFFFFFFFull) throw Error(T4A_GPU_INVALID_ARGUMENT, "local dimension too large");
        }
        *out = new t4a_gpu_tci2(d);
    });
}

void t4a_gpu_tci2_release(t4a_gpu_tci2* h) { delete h; }

t4a_gpu_status t4a_gpu_tci2_set_builtin_function(t4a_gpu_tci2* h, int32_t fid, int32_t n_acc, const double* params,
                                                 const uint64_t* weights)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(params);
        T4A_REQUIRE_PTR(weights);
        h->impl.set_builtin(fid, n_acc, params, weights);
    });
}

t4a_gpu_status t4a_gpu_tci2_set_callback(t4a_gpu_tci2* h, t4a_gpu_batch_eval_fn cb, void* ctx)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.set_callback(cb, ctx);
    });
}

t4a_gpu_status t4a_gpu_tci2_add_global_pivots(t4a_gpu_tci2* h, const size_t* pivots, size_t n_pivots)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pivots) T4A_REQUIRE_PTR(pivots);
        h->impl.add_global_pivots(narrow_pivots(pivots, n_pivots, h->impl.len(), "pivot value out of bounds"));
    });
}

t4a_gpu_status t4a_gpu_tci2_crossinterpolate2(t4a_gpu_tci2* h, const size_t* initial_pivots, size_t n_pivots,
                                              const t4a_gpu_tci2_options* options)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pivots) T4A_REQUIRE_PTR(initial_pivots);
        TCI2Options o = convert_options(options);
        o.validate(); // options are validated before any callback runs (tensorci2/tests/mod.rs:7-144)
        h->impl.crossinterpolate2(narrow_pivots(initial_pivots, n_pivots, h->impl.len(), "pivot value out of bounds"), o);
    });
}

t4a_gpu_status t4a_gpu_tci2_optimize(t4a_gpu_tci2* h, const t4a_gpu_tci2_options* options, int32_t final_sweep1site)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.optimize(convert_options(options), final_sweep1site != 0);
    });
}

t4a_gpu_status t4a_gpu_tci2_optimize_group(t4a_gpu_tci2* const* handles, size_t n_handles, const t4a_gpu_tci2_options* options,
                                           int32_t final_sweep1site)
{
    return guarded([&] {
        const std::vector<Tci2*> hs = tci2_list(handles, n_handles); // (a null handle is reported before null options)
        Tci2::optimize_group(hs, convert_options(options), final_sweep1site != 0);
    });
}

t4a_gpu_status t4a_gpu_tci2_fill_site_tensors_group(t4a_gpu_tci2* const* handles, size_t n_handles)
{
    return guarded([&] {
        Tci2::fill_site_tensors_group(tci2_list(handles, n_handles));
    });
}

t4a_gpu_status t4a_gpu_tci2_sweep2site(t4a_gpu_tci2* h, int32_t forward, const t4a_gpu_tci2_options* options)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.sweep2site(forward != 0, convert_options(options));
    });
}

t4a_gpu_status t4a_gpu_tci2_sweep1site(t4a_gpu_tci2* h, int32_t forward, double rel_tol, double abs_tol,
                                       size_t max_bond_dim, int32_t update_tensors)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.sweep1site(forward != 0, rel_tol, abs_tol, bond_cap(max_bond_dim), update_tensors != 0);
    });
}

t4a_gpu_status t4a_gpu_tci2_fill_site_tensors(t4a_gpu_tci2* h)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.fill_site_tensors();
    });
}

t4a_gpu_status t4a_gpu_tci2_make_canonical(t4a_gpu_tci2* h, double rel_tol, double abs_tol, size_t max_bond_dim)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.make_canonical(rel_tol, abs_tol, bond_cap(max_bond_dim));
    });
}

t4a_gpu_status t4a_gpu_tci2_len(const t4a_gpu_tci2* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.len();
    });
}

t4a_gpu_status t4a_gpu_tci2_rank(const t4a_gpu_tci2* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.rank();
    });
}

t4a_gpu_status t4a_gpu_tci2_link_dims(const t4a_gpu_tci2* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        const auto v = h->impl.link_dims();
        for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    });
}

t4a_gpu_status t4a_gpu_tci2_max_sample_value(const t4a_gpu_tci2* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.max_sample_value;
    });
}

t4a_gpu_status t4a_gpu_tci2_max_bond_error(const t4a_gpu_tci2* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.max_bond_error();
    });
}

t4a_gpu_status t4a_gpu_tci2_bond_errors(const t4a_gpu_tci2* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (size_t i = 0; i < h->impl.bond_errors.size(); ++i) out[i] = h->impl.bond_errors[i];
    });
}

t4a_gpu_status t4a_gpu_tci2_pivot_errors(const t4a_gpu_tci2* h, size_t* count, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        *count = h->impl.pivot_errors.size();
        if (out)
            for (size_t i = 0; i < h->impl.pivot_errors.size(); ++i) out[i] = h->impl.pivot_errors[i];
    });
}

t4a_gpu_status t4a_gpu_tci2_index_set(const t4a_gpu_tci2* h, int32_t which, size_t site, size_t* count, size_t* width,
                                      size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        T4A_REQUIRE_PTR(width);
        if (site >= h->impl.len() || which < 0 || which > 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "site/which out of range");
        if (out) const_cast<t4a_gpu_tci2*>(h)->impl.sync_digits(); // (after a device-side bond chain the digit tables are decoded on demand)
        const IndexSet& s = which == 0 ? h->impl.i_set[site] : h->impl.j_set[site];
        *count = s.count;
        *width = s.width;
        if (out)
            for (size_t k = 0; k < s.count * s.width; ++k) out[k] = s.d[k];
    });
}

t4a_gpu_status t4a_gpu_tci2_set_index_set(t4a_gpu_tci2* h, int32_t which, size_t site, size_t count, const size_t* data)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.set_index_set(which, site, count, data);
    });
}

t4a_gpu_status t4a_gpu_tci2_set_max_sample_value(t4a_gpu_tci2* h, double value)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.max_sample_value = value;
    });
}

t4a_gpu_status t4a_gpu_tci2_clear_history(t4a_gpu_tci2* h)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.clear_history();
    });
}

t4a_gpu_status t4a_gpu_tci2_site_tensor(const t4a_gpu_tci2* h, size_t site, size_t* dims3, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3);
        if (site >= h->impl.len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "site out of range");
        t4a_gpu_tci2* hh = const_cast<t4a_gpu_tci2*>(h);
        hh->impl.fill_wait();
        if (!out) {
            dims3[0] = h->impl.cores[site].l;
            dims3[1] = h->impl.cores[site].s;
            dims3[2] = h->impl.cores[site].r;
            return;
        }
        std::vector<double> v = hh->impl.site_tensor_host(site, dims3);
        std::memcpy(out, v.data(), v.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_tci2_site_tensor_device(const t4a_gpu_tci2* h, size_t site, void* out_device)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out_device);
        const_cast<t4a_gpu_tci2*>(h)->impl.site_tensor_device(site, static_cast<double*>(out_device));
    });
}

t4a_gpu_status t4a_gpu_tci2_set_site_tensor_device(t4a_gpu_tci2* h, size_t site, const size_t* dims3,
                                                   const void* in_device)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3);
        h->impl.set_site_tensor_device(site, dims3, static_cast<const double*>(in_device));
    });
}

t4a_gpu_status t4a_gpu_tci2_export_site_tensors_async(t4a_gpu_tci2* h, void* dst_device, size_t stride,
                                                      void* consumer_stream)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dst_device);
        h->impl.export_site_tensors_async(static_cast<double*>(dst_device), stride,
                                          static_cast<hipStream_t>(consumer_stream));
    });
}

t4a_gpu_status t4a_gpu_tci2_n_iterations(const t4a_gpu_tci2* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.errors_hist.size();
    });
}

t4a_gpu_status t4a_gpu_tci2_history(const t4a_gpu_tci2* h, size_t* ranks, double* errors)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        for (size_t i = 0; i < h->impl.errors_hist.size(); ++i) {
            if (ranks) ranks[i] = h->impl.ranks_hist[i];
            if (errors) errors[i] = h->impl.errors_hist[i];
        }
    });
}

t4a_gpu_status t4a_gpu_tci2_termination(const t4a_gpu_tci2* h, int32_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.termination;
    });
}

t4a_gpu_status t4a_gpu_tci2_evaluate(t4a_gpu_tci2* h, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        const std::vector<uint32_t> u = narrow_indices(idx, n_pts * h->impl.len(), "evaluate: index out of bounds");
        std::vector<double> v = h->impl.evaluate(u.data(), n_pts);
        std::memcpy(out, v.data(), n_pts * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_tci2_sum(t4a_gpu_tci2* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.sum();
    });
}

t4a_gpu_status t4a_gpu_tci2_set_site_shard(t4a_gpu_tci2* h, size_t rank, size_t world)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.set_site_shard(rank, world);
    });
}

t4a_gpu_status t4a_gpu_tci2_set_pi_shard(t4a_gpu_tci2* h, size_t rank, size_t world, t4a_gpu_allgather_fn gather, void* ctx)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.set_pi_shard(rank, world, gather, ctx);
    });
}

t4a_gpu_status t4a_gpu_tci2_pi_shard_stats(t4a_gpu_tci2* h, size_t* out2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out2);
        out2[0] = h->impl.pi_shard.n_gathers;
        out2[1] = h->impl.pi_shard.bytes_sent;
    });
}

t4a_gpu_status t4a_gpu_pi_shard_eval(size_t rank, size_t world, t4a_gpu_batch_eval_fn cb, void* cb_ctx, t4a_gpu_allgather_fn gather,
                                     void* gather_ctx, size_t n_sites, const uint32_t* a, size_t wa, size_t a0, size_t na,
                                     const uint32_t* b, size_t wb, size_t b0, size_t nb, double* out)
{
    return guarded([&] { // host only: no device is touched
        if (!cb) throw Error(T4A_GPU_NULL_POINTER, "batch callback is NULL");
        if (world == 0 || rank >= world) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid shard (rank, world)");
        if (na == 0 || nb == 0) return;
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        if (wa + wb != n_sites || a0 + wa > n_sites || b0 + wb > n_sites) throw Error(T4A_GPU_INVALID_ARGUMENT, "index halves do not cover all sites");
        if (world > 1 && !gather) throw Error(T4A_GPU_NULL_POINTER, "a column-block shard over more than one rank needs an all-gather callback");
        PiShard ps;
        ps.rank = rank;
        ps.world = world;
        ps.gather = gather;
        ps.gather_ctx = gather_ctx;
        pi_shard_evaluate(ps, cb, cb_ctx, n_sites, a, wa, a0, na, b, wb, b0, nb, out);
    });
}

t4a_gpu_status t4a_gpu_tci2_export_site_shard_async(t4a_gpu_tci2* h, void* dst_device, size_t stride, void* consumer_stream)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dst_device);
        h->impl.export_site_shard_async(static_cast<double*>(dst_device), stride, static_cast<hipStream_t>(consumer_stream));
    });
}

t4a_gpu_status t4a_gpu_tci2_import_site_shard_async(t4a_gpu_tci2* h, const void* src_device, size_t stride, size_t per_rank,
                                                    void* producer_stream)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(src_device);
        h->impl.import_site_shard_async(static_cast<const double*>(src_device), stride, per_rank, static_cast<hipStream_t>(producer_stream));
    });
}

t4a_gpu_status t4a_gpu_tci2_set_keep_site_tensors(t4a_gpu_tci2* h, int32_t keep)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.keep_site_tensors = keep != 0;
    });
}

t4a_gpu_status t4a_gpu_tci2_last_sweep_shapes(const t4a_gpu_tci2* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (size_t b = 0; b < h->impl.last_sweep_shapes.size(); ++b)
            for (int k = 0; k < 3; ++k) out[3 * b + k] = h->impl.last_sweep_shapes[b][k];
    });
}

t4a_gpu_status t4a_gpu_tci2_profile_enable(t4a_gpu_tci2* h, int32_t enable)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.eng.prof.enabled = enable != 0;
    });
}

t4a_gpu_status t4a_gpu_tci2_profile_reset(t4a_gpu_tci2* h)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        for (double& v : h->impl.eng.prof.v) v = 0.0;
        h->impl.eng.variant_stats_.clear();
    });
}

t4a_gpu_status t4a_gpu_tci2_profile_get(const t4a_gpu_tci2* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (int i = 0; i < T4A_GPU_PROFILE_SLOTS; ++i) out[i] = h->impl.eng.prof.v[i];
        // slots 12..15: the rrLU kernel instantiation with the largest total time
        double best = -1.0;
        for (const auto& kv : h->impl.eng.variant_stats_)
            if (kv.second[0] > best) {
                best = kv.second[0];
                out[12] = kv.second[0];
                out[13] = kv.second[1];
                out[14] = kv.second[2];
                out[15] = (double)kv.first;
            }
    });
}

t4a_gpu_status t4a_gpu_tci2_profile_variants(const t4a_gpu_tci2* h, double* out, size_t cap_rows, size_t* n_rows)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(n_rows);
        const auto& vs = h->impl.eng.variant_stats_;
        *n_rows = vs.size();
        if (out == nullptr) return; // query
        if (cap_rows < vs.size()) throw Error(T4A_GPU_BUFFER_TOO_SMALL, "profile_variants: buffer too small");
        size_t i = 0;
        for (const auto& kv : vs) {
            out[5 * i + 0] = (double)kv.first;
            for (int j = 0; j < 4; ++j) out[5 * i + 1 + j] = kv.second[j];
            ++i;
        }
    });
}

t4a_gpu_status t4a_gpu_tci2_chain_stats(const t4a_gpu_tci2* h, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (int k = 0; k < 5; ++k) out[k] = h->impl.chain_stats[k];
    });
}

t4a_gpu_status t4a_gpu_tci2_chain_stats_ext(const t4a_gpu_tci2* h, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (int k = 0; k < 4; ++k) out[k] = h->impl.chain_stats_ext[k];
    });
}

t4a_gpu_status t4a_gpu_tci2_chain_segments(const t4a_gpu_tci2* h, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (int k = 0; k < 2; ++k) out[k] = h->impl.chain_segments[k];
    });
}

t4a_gpu_status t4a_gpu_tci2_chain_plan_segments(const size_t* dep_ub, const size_t* ind_ub, const size_t* order, size_t n_bonds, size_t capacity,
                                                size_t* first, size_t* count, int32_t* walked, size_t* n_segments)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(n_segments);
        if (n_bonds > 0) {
            T4A_REQUIRE_PTR(dep_ub);
            T4A_REQUIRE_PTR(ind_ub);
            T4A_REQUIRE_PTR(order);
        }
        for (size_t k = 0; k < n_bonds; ++k)
            if (order[k] >= n_bonds) throw t4a::Error(T4A_GPU_INVALID_ARGUMENT, "chain_plan_segments: order[" + std::to_string(k) + "] is not a bond of the chain");
        const std::vector<t4a::ChainSegment> segs = t4a::chain_plan_segments(dep_ub, ind_ub, order, n_bonds);
        *n_segments = segs.size();
        if (!first && !count && !walked) return;
        T4A_REQUIRE_PTR(first);
        T4A_REQUIRE_PTR(count);
        T4A_REQUIRE_PTR(walked);
        if (capacity < segs.size()) throw t4a::Error(T4A_GPU_BUFFER_TOO_SMALL, "chain_plan_segments: " + std::to_string(segs.size()) + " segments, room for " + std::to_string(capacity));
        for (size_t s = 0; s < segs.size(); ++s) {
            first[s] = segs[s].first;
            count[s] = segs[s].count;
            walked[s] = segs[s].walked ? 1 : 0;
        }
    });
}

t4a_gpu_status t4a_gpu_tci2_rook_stats(const t4a_gpu_tci2* h, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        const RookWork& w = h->impl.rook_work();
        out[0] = w.n_device_searches;
        out[1] = w.n_device_visits;
        out[2] = w.n_host_searches;
        out[3] = w.n_host_syncs;
    });
}

t4a_gpu_status t4a_gpu_tci2_fill_stats(const t4a_gpu_tci2* h, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (int k = 0; k < 3; ++k) out[k] = h->impl.fill_stats()[k];
    });
}

t4a_gpu_status t4a_gpu_tci2_set_chain(t4a_gpu_tci2* h, int32_t enable, int32_t verify)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.chain_enabled = enable != 0;
        h->impl.chain_verify = (verify & 1) != 0;
        h->impl.chain_event_timing = (verify & 2) != 0;
        h->impl.small_enabled = (verify & 4) == 0;
        h->impl.small_stamps = (verify & 8) != 0;
        h->impl.fill_graph_relaxed = (verify & 16) != 0;
        h->impl.small_tile_max = (verify & 32) ? 32 : 16;
    });
}

t4a_gpu_status t4a_gpu_tci2_set_callback_threads(t4a_gpu_tci2* h, size_t n_threads)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_threads < 1 || n_threads > 256) throw Error(T4A_GPU_INVALID_ARGUMENT, "callback threads: between 1 and 256");
        h->impl.callback_threads = n_threads;
    });
}

t4a_gpu_status t4a_gpu_tci2_small_stats(const t4a_gpu_tci2* h, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        for (int k = 0; k < 4; ++k) out[k] = h->impl.small_stats[k];
        for (int k = 0; k < 3; ++k) out[4 + k] = h->impl.small_last_clocks_[k];
        out[7] = (uint64_t)h->impl.small_last_reason_;
        for (int k = 0; k < 8; ++k) out[8 + k] = h->impl.small_last_clocks_[3 + k];
    });
}

// ------------------------------------------------------------------------------------------------ lazy block-rook LUCI
t4a_gpu_status t4a_gpu_luci_blocks_f64(size_t m, size_t n, t4a_gpu_fill_block_fn fill_block, void* ctx,
                                       size_t max_bond_dim, double rel_tol, double abs_tol, int32_t left_orthogonal,
                                       size_t* rank, size_t* rows, size_t* cols, double* pivot_errors, double* left,
                                       double* right)
{
    return guarded([&] {
        luci_prologue(m, n, rank, rows, cols, pivot_errors, fill_block == nullptr, "fill_block is null", left, right, true);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        const RookSource src = rook_source_blocks(e, m, n, fill_block, ctx);
        LuciResult r = rook_luci(e, dense_rook_work(), src, RrLUOptions::from_abi(max_bond_dim, rel_tol, abs_tol, left_orthogonal != 0), nullptr, nullptr);
        luci_outputs(e, r, m, n, rank, rows, cols, pivot_errors, left, right);
    });
}

t4a_gpu_status t4a_gpu_luci_rook_f64(const double* a, size_t m, size_t n, size_t max_bond_dim, double rel_tol,
                                     double abs_tol, int32_t left_orthogonal, size_t* rank, size_t* rows, size_t* cols,
                                     double* pivot_errors, double* left, double* right)
{
    return guarded([&] {
        const size_t count = luci_prologue(m, n, rank, rows, cols, pivot_errors, a == nullptr, "a is null", left, right, true);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        // the dense source lives on the device: A (m x n) and its transpose (rows contiguous)
        e.d_tmp2.reserve(2 * std::max<size_t>(count, 1));
        double* d_a = e.d_tmp2.get();
        upload(e, d_a, a, count);
        const RookSource src = rook_source_device(e, d_a, d_a + count, m, n);
        LuciResult r = rook_luci(e, dense_rook_work(), src, RrLUOptions::from_abi(max_bond_dim, rel_tol, abs_tol, left_orthogonal != 0), nullptr, nullptr);
        luci_outputs(e, r, m, n, rank, rows, cols, pivot_errors, left, right);
    });
}

// ------------------------------------------------------------------------------------------------ svd / qr / full-piv LU
t4a_gpu_status t4a_gpu_svd_f64(const double* a, size_t m, size_t n, double* u, double* s, double* vt)
{
    return guarded([&] {
        const size_t count = checked_mul(m, n, "matrix shape");
        require_int_dims({m, n}, "matrix shape");
        if (count == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "SVD of an empty matrix");
        Engine::require_factor_dims(m, n, "svd: dimensions");
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(u);
        T4A_REQUIRE_PTR(s);
        T4A_REQUIRE_PTR(vt);
        const size_t k = std::min(m, n);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_a = e.pi(count);
        e.d_tmp.reserve(m * k + k + k * n); // (before the copy is queued: a growing buffer is freed and allocated, which synchronises)
        StreamSyncOnExit sync_on_exit(e);
        upload_async(e, d_a, a, count);
        double* d_u = e.d_tmp.get();
        double* d_s = d_u + m * k;
        double* d_vt = d_s + k;
        e.svd(d_a, (int)m, (int)n, d_u, d_s, d_vt);
        download_async(e, u, d_u, m * k);
        download_async(e, s, d_s, k);
        download(e, vt, d_vt, k * n);
    });
}

t4a_gpu_status t4a_gpu_rsvd_f64(const double* a, size_t m, size_t n, size_t k, size_t oversample, size_t power_iters, uint64_t seed,
                                double* u, double* s, double* vt)
{
    return guarded([&] {
        const size_t count = checked_mul(m, n, "matrix shape");
        require_int_dims({m, n}, "matrix shape");
        if (count == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "SVD of an empty matrix");
        Engine::require_factor_dims(m, n, "svd: dimensions");
        if (k == 0 || k > std::min(m, n)) throw Error(T4A_GPU_INVALID_ARGUMENT, "rsvd: the rank must be between 1 and min(m, n)");
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(u);
        T4A_REQUIRE_PTR(s);
        T4A_REQUIRE_PTR(vt);
        const size_t l = std::min(std::min(m, n), k + oversample); // sketch width
        const std::vector<double> omega = rsvd_sketch(n, l, seed);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        RsvdBuffers w;
        w.reserve(m, n, l);
        upload(e, w.A.get(), a, count);
        upload(e, w.omega.get(), omega.data(), omega.size());
        rsvd(e, w, m, n, l, power_iters);
        download(e, u, w.U.get(), m * k);  // the first k columns
        download(e, s, w.S.get(), k);
        // the first k rows of Vt (l x n, column-major: strided) -> k x n
        std::vector<double> hv(l * n);
        download(e, hv.data(), w.Vt.get(), l * n);
        for (size_t j = 0; j < n; ++j)
            for (size_t i = 0; i < k; ++i) vt[i + k * j] = hv[i + l * j];
    });
}

t4a_gpu_status t4a_gpu_qr_f64(const double* a, size_t m, size_t n, double* q, double* r)
{
    return guarded([&] {
        const size_t count = checked_mul(m, n, "matrix shape");
        require_int_dims({m, n}, "matrix shape");
        if (count == 0) return;
        Engine::require_factor_dims(m, n, "qr: dimensions");
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(q);
        T4A_REQUIRE_PTR(r);
        const size_t k = std::min(m, n);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_a = e.pi(count);
        e.d_tmp.reserve(m * k + k * n);
        StreamSyncOnExit sync_on_exit(e);
        upload_async(e, d_a, a, count);
        double* d_q = e.d_tmp.get();
        double* d_r = d_q + m * k;
        e.qr(d_a, (int)m, (int)n, d_q, d_r);
        download_async(e, q, d_q, m * k);
        download(e, r, d_r, k * n);
    });
}

t4a_gpu_status t4a_gpu_full_piv_lu_f64(const double* a, size_t n, double* p, double* l, double* u, double* q)
{
    return guarded([&] {
        const size_t count = checked_mul(n, n, "matrix shape");
        require_int_dims({n}, "matrix shape");
        if (count == 0) return;
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(p);
        T4A_REQUIRE_PTR(l);
        T4A_REQUIRE_PTR(u);
        T4A_REQUIRE_PTR(q);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_a = e.pi(count);
        upload(e, d_a, a, count);
        LuciResult r = e.luci(d_a, (int)n, (int)n, RrLUOptions::from_abi(0, 0.0, 0.0, true), false, true);
        const double* d_l = full_piv_lu_factors(e, r, n);
        download(e, l, d_l, count);
        download(e, u, d_l + count, count);
        std::memset(p, 0, count * sizeof(double));
        std::memset(q, 0, count * sizeof(double));
        for (size_t k = 0; k < n; ++k) {
            p[k + n * (size_t)r.row_perm[k]] = 1.0;
            q[k + n * (size_t)r.col_perm[k]] = 1.0;
        }
    });
}

// ------------------------------------------------------------------------------------------------ SimpleTensorTrain
t4a_gpu_status t4a_gpu_tt_new(const size_t* dims3, size_t n_sites, const double* cores, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sites) T4A_REQUIRE_PTR(dims3);
        require_device();
        std::vector<std::array<size_t, 3>> d(n_sites);
        for (size_t s = 0; s < n_sites; ++s) {
            d[s] = {dims3[3 * s], dims3[3 * s + 1], dims3[3 * s + 2]};
            checked_mul(checked_mul(d[s][0], d[s][1], "tensor shape"), d[s][2], "tensor shape");
        }
        *out = new t4a_gpu_tt(d, cores);
    });
}

void t4a_gpu_tt_release(t4a_gpu_tt* h) { delete h; }

t4a_gpu_status t4a_gpu_tt_clone(const t4a_gpu_tt* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = new t4a_gpu_tt(h->impl.cores, h->impl.eng.stream());
    });
}

t4a_gpu_status t4a_gpu_tt_len(const t4a_gpu_tt* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.len();
    });
}

t4a_gpu_status t4a_gpu_tt_dims(const t4a_gpu_tt* h, size_t* dims3)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (h->impl.len()) T4A_REQUIRE_PTR(dims3);
        for (size_t s = 0; s < h->impl.len(); ++s) {
            dims3[3 * s] = h->impl.cores[s].l;
            dims3[3 * s + 1] = h->impl.cores[s].s;
            dims3[3 * s + 2] = h->impl.cores[s].r;
        }
    });
}

t4a_gpu_status t4a_gpu_tt_site_tensor(const t4a_gpu_tt* h, size_t site, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        std::vector<double> v = const_cast<t4a_gpu_tt*>(h)->impl.site_tensor_host(site);
        if (!v.empty()) {
            T4A_REQUIRE_PTR(out);
            std::memcpy(out, v.data(), v.size() * sizeof(double));
        }
    });
}

t4a_gpu_status t4a_gpu_tt_evaluate(t4a_gpu_tt* h, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, h->impl.len(), "index buffer"));
        std::vector<double> v = h->impl.evaluate(u.data(), n_pts);
        std::memcpy(out, v.data(), n_pts * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_tt_sum(t4a_gpu_tt* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.sum();
    });
}

t4a_gpu_status t4a_gpu_tt_norm2(t4a_gpu_tt* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.norm2();
    });
}

t4a_gpu_status t4a_gpu_tt_compress(t4a_gpu_tt* h, int32_t method, double tolerance, size_t max_bond_dim,
                                   int32_t normalize_error)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (method < 0 || method > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown compression method");
        CompressionOptions o;
        o.method = (CompressionMethod)method;
        o.tolerance = tolerance;
        o.max_bond_dim = max_bond_dim;
        o.normalize_error = normalize_error != 0;
        h->impl.compress(o);
    });
}

t4a_gpu_status t4a_gpu_tt_evaluate_many(t4a_gpu_tt* h, const size_t* idx, size_t n_pts, size_t split, double* out,
                                        size_t* used_split)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (used_split) *used_split = split;
        if (n_pts == 0) return; // cache.rs:563-565
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, h->impl.len(), "index buffer"));
        const size_t s = h->impl.evaluate_many(u.data(), n_pts, split, out);
        if (used_split) *used_split = s;
    });
}

// ---- estimate_true_error / floating_zone / opt_first_pivot (tensorci/src/globalsearch.rs, optfirstpivot.rs) ----
t4a_gpu_status t4a_gpu_tt_floating_zone(t4a_gpu_tt* tt, t4a_gpu_batch_eval_fn f, void* ctx, const size_t* local_dims, size_t n_sites,
                                        const size_t* init_p, uint64_t seed, double early_stop_tol, size_t* pivot_out, double* error_out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tt);
        T4A_REQUIRE_PTR(f);
        T4A_REQUIRE_PTR(pivot_out);
        T4A_REQUIRE_PTR(error_out);
        if (n_sites) T4A_REQUIRE_PTR(local_dims);
        std::vector<uint32_t> init;
        if (init_p) init = narrow_indices(init_p, n_sites);
        auto r = t4a::floating_zone(tt->impl, wrap_search_fn(f, ctx), dims_vec(local_dims, n_sites), init_p ? &init : nullptr, seed, early_stop_tol);
        for (size_t s = 0; s < r.first.size(); ++s) pivot_out[s] = r.first[s];
        *error_out = r.second;
    });
}

t4a_gpu_status t4a_gpu_tt_estimate_true_error(t4a_gpu_tt* tt, t4a_gpu_batch_eval_fn f, void* ctx, size_t nsearch, const size_t* initial_points,
                                              size_t n_initial, uint64_t seed, size_t* pivots_out, double* errors_out, size_t capacity,
                                              size_t* n_out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tt);
        T4A_REQUIRE_PTR(f);
        T4A_REQUIRE_PTR(n_out);
        const size_t n = tt->impl.len();
        std::vector<std::vector<uint32_t>> init;
        if (initial_points) {
            const std::vector<uint32_t> u = narrow_indices(initial_points, checked_mul(n, n_initial, "initial points"));
            for (size_t k = 0; k < n_initial; ++k) init.emplace_back(u.begin() + k * n, u.begin() + (k + 1) * n);
        }
        const auto res = t4a::estimate_true_error(tt->impl, wrap_search_fn(f, ctx), nsearch, initial_points ? &init : nullptr, seed);
        *n_out = res.size();
        if (res.size() > capacity) throw Error(T4A_GPU_BUFFER_TOO_SMALL, "estimate_true_error: output capacity " + std::to_string(capacity) +
                                                                              " < " + std::to_string(res.size()) + " results");
        if (!res.empty()) {
            T4A_REQUIRE_PTR(pivots_out);
            T4A_REQUIRE_PTR(errors_out);
        }
        for (size_t k = 0; k < res.size(); ++k) {
            for (size_t s = 0; s < n; ++s) pivots_out[s + n * k] = res[k].first[s];
            errors_out[k] = res[k].second;
        }
    });
}

t4a_gpu_status t4a_gpu_opt_first_pivot(t4a_gpu_batch_eval_fn f, void* ctx, const size_t* local_dims, size_t n_sites, const size_t* first_pivot,
                                       size_t max_sweep, size_t* pivot_out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(f);
        T4A_REQUIRE_PTR(pivot_out);
        if (n_sites) {
            T4A_REQUIRE_PTR(local_dims);
            T4A_REQUIRE_PTR(first_pivot);
        }
        const std::vector<uint32_t> fp = narrow_indices(first_pivot, n_sites);
        const std::vector<uint32_t> r = t4a::opt_first_pivot(wrap_search_fn(f, ctx), dims_vec(local_dims, n_sites), fp, max_sweep);
        for (size_t s = 0; s < r.size(); ++s) pivot_out[s] = r[s];
    });
}

t4a_gpu_status t4a_gpu_tci2_to_tensor_train(t4a_gpu_tci2* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        h->impl.fill_wait();
        *out = new t4a_gpu_tt(h->impl.cores, h->impl.eng.stream());
    });
}

t4a_gpu_status t4a_gpu_tci2_from_tensor_train(const t4a_gpu_tt* tt, double tolerance, size_t max_bond_dim,
                                              size_t max_iter, t4a_gpu_tci2** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tt);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (tt->impl.len() < 2)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "TensorCI2 conversion requires at least 2 tensor-train sites");
        FromTensorTrainOptions o;
        o.tolerance = tolerance;
        o.max_bond_dim = max_bond_dim;
        o.max_iter = max_iter;
        std::unique_ptr<t4a_gpu_tci2> h(new t4a_gpu_tci2(tt->impl.site_dims()));
        h->impl.assign_from_tensor_train(tt->impl, o);
        *out = h.release();
    });
}

// ------------------------------------------------------------------------------------------------ adaptive patching
t4a_gpu_status t4a_gpu_adaptive_interpolate_builtin(const size_t* local_dims, size_t n_sites, int32_t fid, int32_t n_acc,
                                                    const double* params, const uint64_t* weights,
                                                    const size_t* initial_pivots, size_t n_pivots,
                                                    const t4a_gpu_tci2_options* tci_options, const size_t* patch_order,
                                                    size_t n_initial_pivots, int32_t recycle_pivots, t4a_gpu_ptt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(params);
        T4A_REQUIRE_PTR(weights);
        FnSource f(dims_vec(local_dims, local_dims ? n_sites : 0)); // (run_adaptive reports a missing local_dims)
        f.set_builtin(fid, n_acc, params, weights);
        *out = run_adaptive(local_dims, n_sites, f, initial_pivots, n_pivots, tci_options, patch_order, n_initial_pivots,
                            recycle_pivots);
    });
}

t4a_gpu_status t4a_gpu_adaptive_interpolate_callback(const size_t* local_dims, size_t n_sites, t4a_gpu_batch_eval_fn cb,
                                                     void* ctx, const size_t* initial_pivots, size_t n_pivots,
                                                     const t4a_gpu_tci2_options* tci_options, const size_t* patch_order,
                                                     size_t n_initial_pivots, int32_t recycle_pivots, t4a_gpu_ptt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(cb);
        FnSource f(dims_vec(local_dims, local_dims ? n_sites : 0));
        f.set_callback(cb, ctx);
        *out = run_adaptive(local_dims, n_sites, f, initial_pivots, n_pivots, tci_options, patch_order, n_initial_pivots,
                            recycle_pivots);
    });
}

void t4a_gpu_ptt_release(t4a_gpu_ptt* h) { delete h; }

t4a_gpu_status t4a_gpu_ptt_len(const t4a_gpu_ptt* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->patches.size();
    });
}

t4a_gpu_status t4a_gpu_ptt_projector(const t4a_gpu_ptt* h, size_t k, size_t* count, size_t* positions, size_t* values)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        if (k >= h->impl->patches.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "patch index out of range");
        const auto& pr = h->impl->patches[k].projector;
        *count = pr.size();
        size_t i = 0;
        for (const auto& kv : pr) {
            if (positions) positions[i] = kv.first;
            if (values) values[i] = kv.second;
            ++i;
        }
    });
}

t4a_gpu_status t4a_gpu_ptt_patch_tt(const t4a_gpu_ptt* h, size_t k, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (k >= h->impl->patches.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "patch index out of range");
        *out = new t4a_gpu_tt(h->impl->patches[k].cores, h->impl->eng.stream());
    });
}

t4a_gpu_status t4a_gpu_ptt_evaluate(t4a_gpu_ptt* h, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, h->impl->dims.size(), "index buffer"));
        std::vector<double> v = h->impl->evaluate(u.data(), n_pts);
        std::memcpy(out, v.data(), n_pts * sizeof(double));
    });
}

// ------------------------------------------------------------------------------------------------ TreeTCI
t4a_gpu_status t4a_gpu_treetci_options_default(t4a_gpu_treetci_options* o)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(o);
        std::memset(o, 0, sizeof(*o));
        o->tolerance = 1e-8;
        o->max_iter = 20;
        o->max_bond_dim = 0;
        o->normalize_error = 1;
        o->enable_global_pivots = 1;
        o->nsearch = 5;
        o->max_nglobal_pivot = 5;
        o->tol_margin_global_search = 10.0;
        o->has_seed = 0;
        o->seed = 0;
    });
}

t4a_gpu_status t4a_gpu_treetci_new(const size_t* local_dims, size_t n_sites, const size_t* edges, size_t n_edges,
                                   t4a_gpu_treetci** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sites) T4A_REQUIRE_PTR(local_dims);
        if (n_edges) T4A_REQUIRE_PTR(edges);
        std::vector<TreeEdge> es;
        for (size_t k = 0; k < n_edges; ++k) es.emplace_back(edges[2 * k], edges[2 * k + 1]);
        TreeGraph g(n_sites, es); // graph errors are reported before the device is touched
        std::vector<size_t> d(local_dims, local_dims + n_sites);
        if (!(d.size() > 1)) throw Error(T4A_GPU_INVALID_ARGUMENT, "local_dims should have at least 2 elements");
        for (size_t s = 0; s < d.size(); ++s)
            if (d[s] == 0)
                throw Error(T4A_GPU_INVALID_ARGUMENT, "local dimension at site " + std::to_string(s) + " must be positive");
        *out = new t4a_gpu_treetci(d, g);
    });
}

void t4a_gpu_treetci_release(t4a_gpu_treetci* h) { delete h; }

t4a_gpu_status t4a_gpu_treetci_set_builtin_function(t4a_gpu_treetci* h, int32_t fid, int32_t n_acc, const double* params,
                                                    const uint64_t* weights)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(params);
        T4A_REQUIRE_PTR(weights);
        h->impl.set_builtin(fid, n_acc, params, weights);
    });
}

t4a_gpu_status t4a_gpu_treetci_set_callback(t4a_gpu_treetci* h, t4a_gpu_batch_eval_fn cb, void* ctx)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.set_callback(cb, ctx);
    });
}

t4a_gpu_status t4a_gpu_treetci_add_global_pivots(t4a_gpu_treetci* h, const size_t* pivots, size_t n_pivots)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pivots) T4A_REQUIRE_PTR(pivots);
        h->impl.add_global_pivots(narrow_pivots(pivots, n_pivots, h->impl.local_dims.size(), "pivot value out of bounds"));
    });
}

t4a_gpu_status t4a_gpu_treetci_set_proposer(t4a_gpu_treetci* h, int32_t kind, uint64_t seed)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (kind < 0 || kind > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown proposer");
        h->impl.proposer = kind;
        h->impl.proposer_seed = seed;
    });
}

t4a_gpu_status t4a_gpu_treetci_subregion_vertices(const t4a_gpu_treetci* h, size_t u, size_t v, size_t* n_left,
                                                  size_t* left, size_t* n_right, size_t* right)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(n_left);
        T4A_REQUIRE_PTR(n_right);
        const auto keys = h->impl.graph.subregion_vertices(TreeEdge(u, v));
        *n_left = keys.first.size();
        *n_right = keys.second.size();
        if (left) std::copy(keys.first.begin(), keys.first.end(), left);
        if (right) std::copy(keys.second.begin(), keys.second.end(), right);
    });
}

t4a_gpu_status t4a_gpu_treetci_candidates(const t4a_gpu_treetci* h, size_t u, size_t v, size_t* n_left, size_t* left,
                                          size_t* n_right, size_t* right)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(n_left);
        T4A_REQUIRE_PTR(n_right);
        IndexSet l, r;
        h->impl.candidates(TreeEdge(u, v), l, r);
        write_index_set(l, n_left, left);
        write_index_set(r, n_right, right);
    });
}

t4a_gpu_status t4a_gpu_treetci_update_edge(t4a_gpu_treetci* h, size_t u, size_t v, size_t max_bond_dim, double rel_tol,
                                           double abs_tol, size_t* rank, size_t* rows, size_t* cols, double* pivot_errors)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        const EdgeSelection sel = h->impl.update_edge(TreeEdge(u, v), RrLUOptions::from_abi(max_bond_dim, rel_tol, abs_tol, true));
        if (rank) *rank = sel.rank;
        for (size_t k = 0; k < sel.rank; ++k) {
            if (rows) rows[k] = sel.row_indices[k];
            if (cols) cols[k] = sel.col_indices[k];
        }
        if (pivot_errors)
            for (size_t k = 0; k < sel.pivot_errors.size(); ++k) pivot_errors[k] = sel.pivot_errors[k];
    });
}

t4a_gpu_status t4a_gpu_treetci_optimize(t4a_gpu_treetci* h, const t4a_gpu_treetci_options* options, size_t* n_iter,
                                        size_t* ranks, double* errors)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        const TreeTciOptions o = convert_tree_options(options);
        o.validate(); // before any callback runs (optimize/tests.rs:10-75)
        h->impl.optimize(o);
        write_history(h, n_iter, ranks, errors);
    });
}

t4a_gpu_status t4a_gpu_treetci_crossinterpolate2(t4a_gpu_treetci* h, const size_t* initial_pivots, size_t n_pivots,
                                                 const t4a_gpu_treetci_options* options, size_t* n_iter, size_t* ranks,
                                                 double* errors)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pivots) T4A_REQUIRE_PTR(initial_pivots);
        const TreeTciOptions o = convert_tree_options(options);
        o.validate();
        h->impl.crossinterpolate2(narrow_pivots(initial_pivots, n_pivots, h->impl.local_dims.size(), "pivot value out of bounds"), o);
        write_history(h, n_iter, ranks, errors);
    });
}

t4a_gpu_status t4a_gpu_treetci_find_global_pivots(t4a_gpu_treetci* h, size_t nsearch, size_t max_nglobal_pivot,
                                                  double tol_margin, double abs_tol, uint64_t seed, size_t* count,
                                                  size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        const auto pv = h->impl.find_global_pivots(nsearch, max_nglobal_pivot, tol_margin, abs_tol, seed);
        *count = pv.size();
        const size_t ns = h->impl.local_dims.size();
        if (out)
            for (size_t k = 0; k < pv.size(); ++k)
                for (size_t s = 0; s < ns; ++s) out[s + ns * k] = pv[k][s];
    });
}

t4a_gpu_status t4a_gpu_treetci_pivots(const t4a_gpu_treetci* h, const size_t* key, size_t key_len, size_t* count,
                                      size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        if (key_len) T4A_REQUIRE_PTR(key);
        SubtreeKey k(key, key + key_len);
        std::sort(k.begin(), k.end());
        k.erase(std::unique(k.begin(), k.end()), k.end());
        write_index_set(h->impl.pivots_of(k), count, out);
    });
}

t4a_gpu_status t4a_gpu_treetci_bond_errors(const t4a_gpu_treetci* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        size_t k = 0;
        for (const auto& kv : h->impl.bond_errors) out[k++] = kv.second;
    });
}

t4a_gpu_status t4a_gpu_treetci_pivot_errors(const t4a_gpu_treetci* h, size_t* count, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        *count = h->impl.pivot_errors.size();
        if (out) std::copy(h->impl.pivot_errors.begin(), h->impl.pivot_errors.end(), out);
    });
}

t4a_gpu_status t4a_gpu_treetci_flush_pivot_errors(t4a_gpu_treetci* h)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.flush_pivot_errors();
    });
}

t4a_gpu_status t4a_gpu_treetci_max_sample_value(const t4a_gpu_treetci* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.max_sample_value;
    });
}

t4a_gpu_status t4a_gpu_treetci_set_max_sample_value(t4a_gpu_treetci* h, double value)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.max_sample_value = value;
    });
}

t4a_gpu_status t4a_gpu_treetci_max_bond_error(const t4a_gpu_treetci* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.max_bond_error();
    });
}

t4a_gpu_status t4a_gpu_treetci_max_bond_dim(const t4a_gpu_treetci* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.max_bond_dim();
    });
}

t4a_gpu_status t4a_gpu_treetci_materialize(t4a_gpu_treetci* h, size_t center_site)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.materialize(center_site);
    });
}

t4a_gpu_status t4a_gpu_treetci_site_tensor(t4a_gpu_treetci* h, size_t site, size_t* ndims, size_t* dims, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(ndims);
        std::vector<size_t> d;
        const std::vector<double> v = h->impl.site_tensor_host(site, d);
        *ndims = d.size();
        if (dims) std::copy(d.begin(), d.end(), dims);
        if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_treetci_evaluate(t4a_gpu_treetci* h, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, h->impl.local_dims.size(), "index buffer"));
        std::vector<double> v = h->impl.evaluate(u.data(), n_pts);
        std::memcpy(out, v.data(), n_pts * sizeof(double));
    });
}

// ------------------------------------------------------------------------------------------------ quantics front end
t4a_gpu_status t4a_gpu_qtci_options_default(t4a_gpu_qtci_options* o)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(o);
        std::memset(o, 0, sizeof(*o));
        o->tolerance = 1e-8;
        o->max_bond_dim = 0;
        o->max_iter = 200;
        o->n_random_init_pivot = 5;
        o->unfolding_scheme = 0;
        o->normalize_error = 1;
        o->has_seed = 0;
        o->seed = 0;
    });
}

t4a_gpu_status t4a_gpu_quanticscrossinterpolate(const size_t* rs, size_t n_vars, const double* lower, const double* upper,
                                                int32_t include_endpoint, int32_t grid_unfolding, t4a_gpu_coord_eval_fn f,
                                                void* ctx, int32_t has_pivots, const size_t* initial_pivots, size_t n_pivots,
                                                const t4a_gpu_qtci_options* options, t4a_gpu_qtci** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(rs);
        T4A_REQUIRE_PTR(f);
        if (has_pivots && n_pivots) T4A_REQUIRE_PTR(initial_pivots);
        const QtciOptions o = convert_qtci_options(options);
        QuanticsGrid grid(std::vector<size_t>(rs, rs + n_vars), grid_unfolding ? Unfolding::Fused : Unfolding::Interleaved, true,
                          lower ? std::vector<double>(lower, lower + n_vars) : std::vector<double>(),
                          upper ? std::vector<double>(upper, upper + n_vars) : std::vector<double>(), include_endpoint != 0);
        qtci_run(out, std::unique_ptr<QuanticsTci>(new QuanticsTci(grid, f, nullptr, ctx, {})), has_pivots, initial_pivots,
                 n_pivots, o);
    });
}

t4a_gpu_status t4a_gpu_quanticscrossinterpolate_discrete(const size_t* sizes, size_t n_vars, t4a_gpu_grididx_eval_fn f,
                                                         void* ctx, int32_t has_pivots, const size_t* initial_pivots,
                                                         size_t n_pivots, const t4a_gpu_qtci_options* options,
                                                         t4a_gpu_qtci** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(f);
        if (n_vars == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "this method requires at least one grid dimension, got an empty size");
        T4A_REQUIRE_PTR(sizes);
        if (has_pivots && n_pivots) T4A_REQUIRE_PTR(initial_pivots);
        const QtciOptions o = convert_qtci_options(options);
        const std::vector<size_t> sz(sizes, sizes + n_vars);
        for (size_t s : sz)
            if (s == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "this method only supports grid sizes that are powers of 2");
        qtci_check_sizes(sz);
        const size_t r = (size_t)std::log2((double)sz[0]);
        QuanticsGrid grid(std::vector<size_t>(n_vars, r), o.unfolding, false);
        qtci_run(out, std::unique_ptr<QuanticsTci>(new QuanticsTci(grid, nullptr, f, ctx, {})), has_pivots, initial_pivots,
                 n_pivots, o);
    });
}

t4a_gpu_status t4a_gpu_quanticscrossinterpolate_from_arrays(const double* xvals, const size_t* sizes, size_t n_vars,
                                                            t4a_gpu_coord_eval_fn f, void* ctx, int32_t has_pivots,
                                                            const size_t* initial_pivots, size_t n_pivots,
                                                            const t4a_gpu_qtci_options* options, t4a_gpu_qtci** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(f);
        if (n_vars == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "xvals must not be empty");
        T4A_REQUIRE_PTR(sizes);
        if (has_pivots && n_pivots) T4A_REQUIRE_PTR(initial_pivots);
        const QtciOptions o = convert_qtci_options(options);
        std::vector<std::vector<double>> xv;
        size_t off = 0;
        for (size_t d = 0; d < n_vars; ++d) {
            if (sizes[d]) T4A_REQUIRE_PTR(xvals);
            xv.emplace_back(xvals + off, xvals + off + sizes[d]);
            off += sizes[d];
        }
        qtci_run(out, qtci_from_arrays(xv, f, ctx, o), has_pivots, initial_pivots, n_pivots, o);
    });
}

void t4a_gpu_qtci_release(t4a_gpu_qtci* h) { delete h; }

t4a_gpu_status t4a_gpu_qtci_evaluate(t4a_gpu_qtci* h, const size_t* grididx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(grididx);
        T4A_REQUIRE_PTR(out);
        const std::vector<double> v = h->impl->evaluate(grididx, n_pts);
        std::memcpy(out, v.data(), n_pts * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_qtci_sum(t4a_gpu_qtci* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->sum();
    });
}

t4a_gpu_status t4a_gpu_qtci_integral(t4a_gpu_qtci* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->integral();
    });
}

t4a_gpu_status t4a_gpu_qtci_n_sites(const t4a_gpu_qtci* h, size_t* n_sites, size_t* n_vars, int32_t* is_discretized)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_sites) *n_sites = h->impl->grid.n_sites();
        if (n_vars) *n_vars = h->impl->grid.n_vars();
        if (is_discretized) *is_discretized = h->impl->grid.discretized ? 1 : 0;
    });
}

t4a_gpu_status t4a_gpu_qtci_link_dims(const t4a_gpu_qtci* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        const auto ld = h->impl->tt->link_dims();
        if (!ld.empty()) T4A_REQUIRE_PTR(out);
        std::copy(ld.begin(), ld.end(), out);
    });
}

t4a_gpu_status t4a_gpu_qtci_history(const t4a_gpu_qtci* h, size_t* n_iter, size_t* ranks, double* errors)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        const auto& t = *h->impl->tci;
        if (n_iter) *n_iter = t.ranks_hist.size();
        for (size_t k = 0; k < t.ranks_hist.size(); ++k) {
            if (ranks) ranks[k] = t.ranks_hist[k];
            if (errors) errors[k] = t.errors_hist[k];
        }
    });
}

t4a_gpu_status t4a_gpu_qtci_tensor_train(t4a_gpu_qtci* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_tt(h->impl->tt->cores, h->impl->tt->eng.stream());
    });
}

t4a_gpu_status t4a_gpu_qtci_tree_pivots(const t4a_gpu_qtci* h, const size_t* key, size_t key_len, size_t* count, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        if (key_len) T4A_REQUIRE_PTR(key);
        SubtreeKey k(key, key + key_len);
        std::sort(k.begin(), k.end());
        write_index_set(h->impl->tci->pivots_of(k), count, out);
    });
}

t4a_gpu_status t4a_gpu_qtci_cachedata(const t4a_gpu_qtci* h, size_t* count, size_t* quantics, double* values,
                                      size_t* user_calls, size_t* user_points)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        *count = h->impl->cache.size();
        if (user_calls) *user_calls = h->impl->n_user_calls;
        if (user_points) *user_points = h->impl->n_user_points;
        if (!quantics && !values) return;
        size_t k = 0;
        const size_t ns = h->impl->grid.n_sites();
        for (const auto& kv : h->impl->cache) {
            if (quantics)
                for (size_t s = 0; s < ns; ++s) quantics[k * ns + s] = kv.first[s];
            if (values) values[k] = kv.second;
            ++k;
        }
    });
}

t4a_gpu_status t4a_gpu_qtci_grid(const t4a_gpu_qtci* h, int32_t which, const size_t* in, size_t* out_u, double* out_d)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        const QuanticsGrid& g = h->impl->grid;
        const size_t ns = g.n_sites(), nv = g.n_vars();
        if (which == 0) {
            T4A_REQUIRE_PTR(in);
            T4A_REQUIRE_PTR(out_u);
            std::vector<uint32_t> q(ns);
            g.grididx_to_quantics(in, q.data());
            std::copy(q.begin(), q.end(), out_u);
        } else if (which == 1 || which == 2) {
            T4A_REQUIRE_PTR(in);
            std::vector<uint32_t> q = narrow_indices(in, ns);
            if (which == 1) {
                T4A_REQUIRE_PTR(out_u);
                g.quantics_to_grididx(q.data(), out_u);
            } else {
                T4A_REQUIRE_PTR(out_d);
                // cachedata_origcoord (quantics_tci.rs:156-173): only discretized grids carry coordinates
                if (!g.discretized)
                    throw Error(T4A_GPU_INVALID_ARGUMENT, "original coordinates are only available for discretized grids");
                g.quantics_to_origcoord(q.data(), out_d);
            }
        } else if (which == 3) {
            T4A_REQUIRE_PTR(out_u);
            const auto d = g.local_dimensions();
            std::copy(d.begin(), d.end(), out_u);
        } else if (which == 4) {
            T4A_REQUIRE_PTR(out_d);
            const auto st = g.grid_step();
            std::copy(st.begin(), st.end(), out_d);
        } else {
            throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown grid query");
        }
        (void)nv;
    });
}

t4a_gpu_status t4a_gpu_quanticscrossinterpolate_batched(const size_t* rs, size_t n_vars, const double* lower,
                                                        const double* upper, int32_t include_endpoint, int32_t grid_unfolding,
                                                        t4a_gpu_coord_eval_vec_fn f, void* ctx, const size_t* output_dims,
                                                        size_t n_output_dims, int32_t has_pivots, const size_t* initial_pivots,
                                                        size_t n_pivots, const t4a_gpu_qtci_options* options,
                                                        t4a_gpu_tt** out_tt, size_t* n_iter, size_t* ranks, double* errors,
                                                        size_t* user_points)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out_tt);
        *out_tt = nullptr;
        T4A_REQUIRE_PTR(rs);
        T4A_REQUIRE_PTR(f);
        if (n_output_dims) T4A_REQUIRE_PTR(output_dims);
        if (has_pivots && n_pivots) T4A_REQUIRE_PTR(initial_pivots);
        const QtciOptions o = convert_qtci_options(options);
        QuanticsGrid grid(std::vector<size_t>(rs, rs + n_vars), grid_unfolding ? Unfolding::Fused : Unfolding::Interleaved, true,
                          lower ? std::vector<double>(lower, lower + n_vars) : std::vector<double>(),
                          upper ? std::vector<double>(upper, upper + n_vars) : std::vector<double>(), include_endpoint != 0);
        const auto pv = qtci_pivots(initial_pivots, has_pivots ? n_pivots : 0, n_vars);
        QuanticsBatchedResult r = quantics_batched(grid, f, ctx, std::vector<size_t>(output_dims, output_dims + n_output_dims),
                                                   has_pivots ? &pv : nullptr, o);
        if (n_iter) *n_iter = r.ranks.size();
        for (size_t k = 0; k < r.ranks.size(); ++k) {
            if (ranks) ranks[k] = r.ranks[k];
            if (errors) errors[k] = r.errors[k];
        }
        if (user_points) *user_points = r.n_user_points;
        *out_tt = new t4a_gpu_tt(r.tt->cores, r.tt->eng.stream());
    });
}

// ------------------------------------------------------------------------------------------------ dense labelled tensors
t4a_gpu_status t4a_gpu_svd_retained_rank(const double* s, size_t n, const t4a_gpu_svd_policy* policy, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        if (n) T4A_REQUIRE_PTR(s);
        *out = svd_retained_rank(s, n, convert_policy(policy));
    });
}

t4a_gpu_status t4a_gpu_qr_retained_rank(const double* r, size_t k, size_t n, double rtol, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        if (checked_mul(k, n, "R shape")) T4A_REQUIRE_PTR(r);
        *out = qr_retained_rank(r, k, n, rtol);
    });
}

t4a_gpu_status t4a_gpu_tensor_contract_f64(const double* a, const size_t* a_dims, const int64_t* a_labels, size_t a_rank,
                                           const double* b, const size_t* b_dims, const int64_t* b_labels, size_t b_rank,
                                           double* out, size_t* out_dims, int64_t* out_labels, size_t* out_rank)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out_rank);
        TensorView va = host_view(a_dims, a_labels, a_rank), vb = host_view(b_dims, b_labels, b_rank);
        const ContractPlan plan = plan_contract_pair(va, vb); // index errors before the device is touched
        *out_rank = plan.out_dims.size();
        for (size_t k = 0; k < plan.out_dims.size(); ++k) {
            if (out_dims) out_dims[k] = plan.out_dims[k];
            if (out_labels) out_labels[k] = plan.out_labels[k];
        }
        if (!out) return;
        const size_t na = va.size(), nb = vb.size(), nc = checked_mul(plan.M, plan.N, "result shape");
        if (nc == 0) return;
        if (na) T4A_REQUIRE_PTR(a);
        if (nb) T4A_REQUIRE_PTR(b);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_in = e.pi(na + nb + nc);
        upload(e, d_in, a, na);
        upload(e, d_in + na, b, nb);
        va.d_data = d_in;
        vb.d_data = d_in + na;
        tensor_contract_pair(e, va, vb, plan, d_in + na + nb);
        download(e, out, d_in + na + nb, nc);
    });
}

t4a_gpu_status t4a_gpu_tensor_svd_f64(const double* t, const size_t* dims, const int64_t* labels, size_t rank,
                                      const int64_t* left_labels, size_t n_left, int32_t truncate,
                                      const t4a_gpu_svd_policy* policy, int32_t has_max_bond_dim, size_t max_bond_dim,
                                      size_t* r, double* u, double* s, double* v)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(r);
        TensorView tv = host_view(dims, labels, rank);
        if (n_left) T4A_REQUIRE_PTR(left_labels);
        const UnfoldPlan un = plan_unfold_split(tv, std::vector<int64_t>(left_labels, left_labels + n_left));
        const SvdOptions opts{truncate != 0, convert_policy(policy), has_max_bond_dim != 0, max_bond_dim};
        opts.validate();
        require_factorizable(un, "svd", "SVD");
        T4A_REQUIRE_PTR(t);
        T4A_REQUIRE_PTR(u);
        T4A_REQUIRE_PTR(s);
        T4A_REQUIRE_PTR(v);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_t = tensor_staging(e, tv.size());
        upload(e, d_t, t, tv.size());
        tv.d_data = d_t;
        const UnfoldedFactors f = tensor_svd(e, tv, un, opts);
        *r = f.keep;
        std::copy(f.s.begin(), f.s.begin() + f.keep, s);
        download(e, u, f.d_left, f.m * f.keep);
        // V [n x keep] = (first `keep` rows of V^T)^T
        e.d_tmp2.reserve(f.n * f.keep);
        transpose_launch(f.d_right, (int)f.keep, (int)f.n, (int)f.k, e.d_tmp2.get(), (int)f.n, e.stream());
        T4A_HIP(hipGetLastError());
        download(e, v, e.d_tmp2.get(), f.n * f.keep);
    });
}

t4a_gpu_status t4a_gpu_tensor_qr_f64(const double* t, const size_t* dims, const int64_t* labels, size_t rank,
                                     const int64_t* left_labels, size_t n_left, int32_t truncate, int32_t has_rtol, double rtol,
                                     size_t* r, double* q, double* r_factor)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(r);
        TensorView tv = host_view(dims, labels, rank);
        if (n_left) T4A_REQUIRE_PTR(left_labels);
        const UnfoldPlan un = plan_unfold_split(tv, std::vector<int64_t>(left_labels, left_labels + n_left));
        const QrOptions opts{truncate != 0, has_rtol ? rtol : QrOptions().rtol};
        opts.validate();
        require_factorizable(un, "qr", "QR");
        T4A_REQUIRE_PTR(t);
        T4A_REQUIRE_PTR(q);
        T4A_REQUIRE_PTR(r_factor);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        double* d_t = tensor_staging(e, tv.size());
        upload(e, d_t, t, tv.size());
        tv.d_data = d_t;
        const UnfoldedFactors f = tensor_qr(e, tv, un, opts);
        *r = f.keep;
        download(e, q, f.d_left, f.m * f.keep);
        // leading `keep` rows of R with leading dimension keep
        e.d_tmp2.reserve(f.keep * f.n);
        gather_launch(f.d_right, (int)f.k, nullptr, (int)f.keep, nullptr, (int)f.n, e.d_tmp2.get(), (int)f.keep, e.stream());
        T4A_HIP(hipGetLastError());
        download(e, r_factor, e.d_tmp2.get(), f.keep * f.n);
    });
}

// ------------------------------------------------------------------------------------------------ device-resident labelled tensors
t4a_gpu_status t4a_gpu_tensor_new(const double* data, const size_t* dims, const int64_t* labels, size_t rank,
                                  t4a_gpu_tensor** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        TensorView hv = host_view(dims, labels, rank);
        if (rank > (size_t)TENSOR_MAX_RANK) throw Error(T4A_GPU_NOT_IMPLEMENTED, "tensor rank above 16");
        require_distinct_labels(hv);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        auto t = make_tensor(hv.dims, hv.labels);
        if (t->size()) {
            T4A_REQUIRE_PTR(data);
            upload(e, t->buf.get(), data, t->size());
        }
        *out = t.release();
    });
}

void t4a_gpu_tensor_release(t4a_gpu_tensor* h) { delete h; }

t4a_gpu_status t4a_gpu_tensor_rank(const t4a_gpu_tensor* h, size_t* rank)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(rank);
        *rank = h->dims.size();
    });
}

t4a_gpu_status t4a_gpu_tensor_dims(const t4a_gpu_tensor* h, size_t* dims, int64_t* labels)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (dims) std::copy(h->dims.begin(), h->dims.end(), dims);
        if (labels) std::copy(h->labels.begin(), h->labels.end(), labels);
    });
}

t4a_gpu_status t4a_gpu_tensor_to_host(const t4a_gpu_tensor* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (h->size() == 0) return;
        T4A_REQUIRE_PTR(out);
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        download(dense_engine(), out, h->buf.get(), h->size());
    });
}

t4a_gpu_status t4a_gpu_tensor_permute(const t4a_gpu_tensor* h, const int64_t* labels, t4a_gpu_tensor** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        const size_t r = h->dims.size();
        if (r) T4A_REQUIRE_PTR(labels);
        const std::vector<size_t> perm = plan_permute(h->view(), labels);
        std::vector<size_t> nd(r);
        std::vector<int64_t> nl(r);
        for (size_t k = 0; k < r; ++k) {
            nd[k] = h->dims[perm[k]];
            nl[k] = h->labels[perm[k]];
        }
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        auto t = make_tensor(nd, nl);
        tensor_permute(e, h->view(), perm, t->buf.get());
        e.sync();
        *out = t.release();
    });
}

t4a_gpu_status t4a_gpu_tensor_relabel(t4a_gpu_tensor* h, int64_t from, int64_t to)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->labels[plan_relabel(h->view(), from, to)] = to;
    });
}

t4a_gpu_status t4a_gpu_tensor_contract(const t4a_gpu_tensor* a, const t4a_gpu_tensor* b, t4a_gpu_tensor** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        const TensorView va = a->view(), vb = b->view();
        const ContractPlan plan = plan_contract_pair(va, vb);
        *out = contract_to_handle(va, vb, plan);
    });
}

t4a_gpu_status t4a_gpu_tensor_contract_many(const t4a_gpu_tensor* const* tensors, size_t n_tensors, const int64_t* retain_labels,
                                            size_t n_retain, t4a_gpu_tensor** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_tensors) T4A_REQUIRE_PTR(tensors);
        if (n_retain) T4A_REQUIRE_PTR(retain_labels);
        const std::vector<TensorView> views = handle_list(tensors, n_tensors, "tensors[i] is null", [](const t4a_gpu_tensor& t) { return t.view(); });
        const std::vector<int64_t> retain(retain_labels, retain_labels + n_retain);
        (void)plan_contract_network(views, retain); // (argument errors before the device is touched)
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        *out = make_tensor(tensor_contract_network(dense_engine(), views, retain)).release();
    });
}

t4a_gpu_status t4a_gpu_tensor_outer_product(const t4a_gpu_tensor* a, const t4a_gpu_tensor* b, t4a_gpu_tensor** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        const TensorView va = a->view(), vb = b->view();
        *out = contract_to_handle(va, vb, plan_outer_product(va, vb));
    });
}

t4a_gpu_status t4a_gpu_tensor_tensordot(const t4a_gpu_tensor* a, const t4a_gpu_tensor* b, const int64_t* labels_a, const int64_t* labels_b,
                                        size_t n_pairs, t4a_gpu_tensor** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_pairs) {
            T4A_REQUIRE_PTR(labels_a);
            T4A_REQUIRE_PTR(labels_b);
        }
        const TensorView va = a->view();
        TensorView vb = b->view();
        const ContractPlan plan = plan_tensordot(va, vb, labels_a, labels_b, n_pairs);
        *out = contract_to_handle(va, vb, plan);
    });
}

t4a_gpu_status t4a_gpu_tensor_svd(const t4a_gpu_tensor* t, const int64_t* left_labels, size_t n_left, int32_t truncate,
                                  const t4a_gpu_svd_policy* policy, int32_t has_max_bond_dim, size_t max_bond_dim,
                                  int64_t bond_label, int64_t bond_label_v, t4a_gpu_tensor** u, t4a_gpu_tensor** s,
                                  t4a_gpu_tensor** v)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(t);
        T4A_REQUIRE_PTR(u);
        T4A_REQUIRE_PTR(s);
        T4A_REQUIRE_PTR(v);
        *u = *s = *v = nullptr;
        if (n_left) T4A_REQUIRE_PTR(left_labels);
        const TensorView tv = t->view();
        const UnfoldPlan un = plan_unfold_split(tv, std::vector<int64_t>(left_labels, left_labels + n_left));
        const SvdOptions opts{truncate != 0, convert_policy(policy), has_max_bond_dim != 0, max_bond_dim};
        opts.validate();
        require_factorizable(un, "svd", "SVD");
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        const UnfoldedFactors f = tensor_svd(e, tv, un, opts);
        auto tu = make_tensor(bonded_tensor(un.left_dims, un.left_labels, f.keep, bond_label)), ts = make_tensor({f.keep}, {bond_label}),
             tvv = make_tensor(bonded_tensor(un.right_dims, un.right_labels, f.keep, bond_label_v));
        T4A_HIP(hipMemcpyAsync(tu->buf.get(), f.d_left, f.m * f.keep * sizeof(double), hipMemcpyDeviceToDevice, e.stream()));
        T4A_HIP(hipMemcpyAsync(ts->buf.get(), f.d_s, f.keep * sizeof(double), hipMemcpyDeviceToDevice, e.stream()));
        transpose_launch(f.d_right, (int)f.keep, (int)f.n, (int)f.k, tvv->buf.get(), (int)f.n, e.stream());
        T4A_HIP(hipGetLastError());
        e.sync();
        *u = tu.release();
        *s = ts.release();
        *v = tvv.release();
    });
}

t4a_gpu_status t4a_gpu_tensor_qr(const t4a_gpu_tensor* t, const int64_t* left_labels, size_t n_left, int32_t truncate,
                                 int32_t has_rtol, double rtol, int64_t bond_label, t4a_gpu_tensor** q, t4a_gpu_tensor** r)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(t);
        T4A_REQUIRE_PTR(q);
        T4A_REQUIRE_PTR(r);
        *q = *r = nullptr;
        if (n_left) T4A_REQUIRE_PTR(left_labels);
        const TensorView tv = t->view();
        const UnfoldPlan un = plan_unfold_split(tv, std::vector<int64_t>(left_labels, left_labels + n_left));
        const QrOptions opts{truncate != 0, has_rtol ? rtol : QrOptions().rtol};
        opts.validate();
        require_factorizable(un, "qr", "QR");
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        const UnfoldedFactors f = tensor_qr(e, tv, un, opts);
        auto tq = make_tensor(bonded_tensor(un.left_dims, un.left_labels, f.keep, bond_label)),
             tr = make_tensor(bonded_tensor(un.right_dims, un.right_labels, f.keep, bond_label, true));
        T4A_HIP(hipMemcpyAsync(tq->buf.get(), f.d_left, f.m * f.keep * sizeof(double), hipMemcpyDeviceToDevice, e.stream()));
        gather_launch(f.d_right, (int)f.k, nullptr, (int)f.keep, nullptr, (int)f.n, tr->buf.get(), (int)f.keep, e.stream());
        T4A_HIP(hipGetLastError());
        e.sync();
        *q = tq.release();
        *r = tr.release();
    });
}

t4a_gpu_status t4a_gpu_tensor_factorize(const t4a_gpu_tensor* t, const int64_t* left_labels, size_t n_left, int32_t alg,
                                        int32_t canonical, int32_t full_rank, const t4a_gpu_svd_policy* policy,
                                        int32_t has_max_bond_dim, size_t max_bond_dim, int32_t has_qr_rtol, double qr_rtol,
                                        int64_t bond_label, t4a_gpu_tensor** left, t4a_gpu_tensor** right, size_t* rank,
                                        double* singular_values)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(t);
        T4A_REQUIRE_PTR(left);
        T4A_REQUIRE_PTR(right);
        *left = *right = nullptr;
        if (n_left) T4A_REQUIRE_PTR(left_labels);
        if (alg < 0 || alg > 3) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown factorization algorithm");
        if (canonical < 0 || canonical > 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown canonical direction");
        const TensorView tv = t->view();
        const UnfoldPlan un = plan_unfold_split(tv, std::vector<int64_t>(left_labels, left_labels + n_left));
        const FactorizeOptions opts{alg, canonical, SvdOptions{!full_rank, convert_policy(policy), has_max_bond_dim != 0, max_bond_dim},
                                    QrOptions{!full_rank, has_qr_rtol ? qr_rtol : QrOptions().rtol}};
        opts.validate();
        require_factorizable(un, "factorize", "factorization");
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        FactorizeResult f = tensor_factorize(dense_engine(), tv, un, opts, bond_label);
        if (rank) *rank = f.rank;
        if (singular_values) std::copy(f.singular_values.begin(), f.singular_values.end(), singular_values);
        auto tl = make_tensor(std::move(f.left)), tr = make_tensor(std::move(f.right));
        *left = tl.release();
        *right = tr.release();
    });
}

// ---- SimpleTensorTrain arithmetic ----
t4a_gpu_status t4a_gpu_tt_add(const t4a_gpu_tt* a, const t4a_gpu_tt* b, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = wrap_tt(const_cast<t4a_gpu_tt*>(a)->impl.add(const_cast<t4a_gpu_tt*>(b)->impl, false));
    });
}

t4a_gpu_status t4a_gpu_tt_sub(const t4a_gpu_tt* a, const t4a_gpu_tt* b, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = wrap_tt(const_cast<t4a_gpu_tt*>(a)->impl.add(const_cast<t4a_gpu_tt*>(b)->impl, true));
    });
}

t4a_gpu_status t4a_gpu_tt_scale(t4a_gpu_tt* h, double factor)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.scale(factor);
    });
}

t4a_gpu_status t4a_gpu_tt_inner_product(const t4a_gpu_tt* a, const t4a_gpu_tt* b, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = const_cast<t4a_gpu_tt*>(a)->impl.inner_product(const_cast<t4a_gpu_tt*>(b)->impl);
    });
}

t4a_gpu_status t4a_gpu_tt_reverse(const t4a_gpu_tt* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = wrap_tt(const_cast<t4a_gpu_tt*>(h)->impl.reverse());
    });
}

t4a_gpu_status t4a_gpu_tt_partial_sum(const t4a_gpu_tt* h, const size_t* dims, size_t n_dims, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_dims) T4A_REQUIRE_PTR(dims);
        *out = wrap_tt(const_cast<t4a_gpu_tt*>(h)->impl.partial_sum(std::vector<size_t>(dims, dims + n_dims)));
    });
}

// ---- gauge forms: SiteTensorTrain, VidalTensorTrain, InverseTensorTrain (tt_canonical.hip) ----
t4a_gpu_status t4a_gpu_site_tt_from_tt(const t4a_gpu_tt* tt, size_t center, t4a_gpu_site_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(tt);
        SiteTrain::check_new(tt->impl.len(), center);
        *out = new t4a_gpu_site_tt(tt->impl.cores, tt->impl.eng.stream(), center);
    });
}

void t4a_gpu_site_tt_release(t4a_gpu_site_tt* h) { delete h; }

t4a_gpu_status t4a_gpu_site_tt_len(const t4a_gpu_site_tt* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.len();
    });
}

t4a_gpu_status t4a_gpu_site_tt_dims(const t4a_gpu_site_tt* h, size_t* dims3)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        cores_dims(h->impl.cores, dims3);
    });
}

t4a_gpu_status t4a_gpu_site_tt_site_tensor(const t4a_gpu_site_tt* h, size_t site, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        core_to_host(&const_cast<t4a_gpu_site_tt*>(h)->impl.eng, h->impl.cores, site, out);
    });
}

t4a_gpu_status t4a_gpu_site_tt_center(const t4a_gpu_site_tt* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.center();
    });
}

t4a_gpu_status t4a_gpu_site_tt_move_center_left(t4a_gpu_site_tt* h)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.move_center_left();
    });
}

t4a_gpu_status t4a_gpu_site_tt_move_center_right(t4a_gpu_site_tt* h)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.move_center_right();
    });
}

t4a_gpu_status t4a_gpu_site_tt_set_center(t4a_gpu_site_tt* h, size_t center)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl.set_center(center);
    });
}

t4a_gpu_status t4a_gpu_site_tt_set_site_tensor(t4a_gpu_site_tt* h, size_t site, const size_t* dims3, const double* data)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3);
        h->impl.set_site_tensor(site, dims3, data);
    });
}

t4a_gpu_status t4a_gpu_site_tt_set_two_site_tensors(t4a_gpu_site_tt* h, size_t site, const size_t* dims3_1, const double* data1,
                                                    const size_t* dims3_2, const double* data2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3_1);
        T4A_REQUIRE_PTR(dims3_2);
        h->impl.set_two_site_tensors(site, dims3_1, data1, dims3_2, data2);
    });
}

t4a_gpu_status t4a_gpu_site_tt_to_tt(const t4a_gpu_site_tt* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(h);
        *out = tt_from_cores(h->impl.cores, h->impl.eng.stream());
    });
}

t4a_gpu_status t4a_gpu_site_tt_tensors_tt(const t4a_gpu_site_tt* h, t4a_gpu_tt** out) { return t4a_gpu_site_tt_to_tt(h, out); }

t4a_gpu_status t4a_gpu_tt_center_canonicalize(t4a_gpu_tt* tt, size_t center)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tt);
        center_canonicalize(tt->impl, center);
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_from_tt(const t4a_gpu_tt* tt, size_t start, size_t end, t4a_gpu_vidal_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(tt);
        VidalTrain::check_partition(tt->impl.len(), end);
        auto h = std::make_unique<t4a_gpu_vidal_tt>();
        h->impl = std::make_unique<VidalTrain>(tt->impl.cores, tt->impl.eng.stream(), start, end);
        *out = h.release();
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_new(const size_t* dims3, size_t n_sites, const double* cores, const size_t* sv_lens, size_t n_svs,
                                    const double* svs, t4a_gpu_vidal_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        auto h = std::make_unique<t4a_gpu_vidal_tt>();
        if (n_sites == 0) { // vidal.rs:405-411: the empty object whatever the vectors are
            h->impl = std::make_unique<VidalTrain>();
            *out = h.release();
            return;
        }
        T4A_REQUIRE_PTR(dims3);
        VidalTrain::check_new(n_sites, n_svs);
        if (n_svs) T4A_REQUIRE_PTR(sv_lens);
        std::vector<std::array<size_t, 3>> d(n_sites);
        for (size_t s = 0; s < n_sites; ++s) {
            d[s] = {dims3[3 * s], dims3[3 * s + 1], dims3[3 * s + 2]};
            checked_mul(checked_mul(d[s][0], d[s][1], "tensor shape"), d[s][2], "tensor shape");
        }
        h->impl = std::make_unique<VidalTrain>(d, cores, std::vector<size_t>(sv_lens, sv_lens + n_svs), svs);
        *out = h.release();
    });
}

void t4a_gpu_vidal_tt_release(t4a_gpu_vidal_tt* h) { delete h; }

t4a_gpu_status t4a_gpu_vidal_tt_len(const t4a_gpu_vidal_tt* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->len();
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_dims(const t4a_gpu_vidal_tt* h, size_t* dims3)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        cores_dims(h->impl->cores, dims3);
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_site_tensor(const t4a_gpu_vidal_tt* h, size_t site, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        core_to_host(h->impl->eng.get(), h->impl->cores, site, out);
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_set_site_tensor(t4a_gpu_vidal_tt* h, size_t site, const size_t* dims3, const double* data)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3);
        h->impl->set_site_tensor(site, dims3, data);
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_partition(const t4a_gpu_vidal_tt* h, size_t* start, size_t* end)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(start);
        T4A_REQUIRE_PTR(end);
        *start = h->impl->part_start;
        *end = h->impl->part_end;
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_singular_values(const t4a_gpu_vidal_tt* h, size_t bond, double* out, size_t capacity, size_t* len)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(len);
        vector_out(h->impl->singular_values_host(bond), out, capacity, len);
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_set_singular_values(t4a_gpu_vidal_tt* h, size_t bond, const double* values, size_t len)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl->set_singular_values(bond, values, len);
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_to_tt(const t4a_gpu_vidal_tt* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(h);
        std::vector<DevCore> cores = h->impl->to_tensor_train_cores();
        *out = tt_from_cores(cores, h->impl->eng ? h->impl->eng->stream() : nullptr);
    });
}

t4a_gpu_status t4a_gpu_vidal_tt_tensors_tt(const t4a_gpu_vidal_tt* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(h);
        *out = tt_from_cores(h->impl->cores, h->impl->eng ? h->impl->eng->stream() : nullptr);
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_from_vidal(const t4a_gpu_vidal_tt* vidal, t4a_gpu_inverse_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(vidal);
        auto h = std::make_unique<t4a_gpu_inverse_tt>();
        h->impl = std::make_unique<InverseTrain>(*vidal->impl);
        *out = h.release();
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_from_tt(const t4a_gpu_tt* tt, t4a_gpu_inverse_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(tt);
        VidalTrain vidal(tt->impl.cores, tt->impl.eng.stream(), 0, tt->impl.len());
        auto h = std::make_unique<t4a_gpu_inverse_tt>();
        h->impl = std::make_unique<InverseTrain>(vidal);
        *out = h.release();
    });
}

void t4a_gpu_inverse_tt_release(t4a_gpu_inverse_tt* h) { delete h; }

t4a_gpu_status t4a_gpu_inverse_tt_len(const t4a_gpu_inverse_tt* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->len();
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_dims(const t4a_gpu_inverse_tt* h, size_t* dims3)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        cores_dims(h->impl->cores, dims3);
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_site_tensor(const t4a_gpu_inverse_tt* h, size_t site, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        core_to_host(h->impl->eng.get(), h->impl->cores, site, out);
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_partition(const t4a_gpu_inverse_tt* h, size_t* start, size_t* end)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(start);
        T4A_REQUIRE_PTR(end);
        *start = h->impl->part_start;
        *end = h->impl->part_end;
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_inverse_singular_values(const t4a_gpu_inverse_tt* h, size_t bond, double* out, size_t capacity,
                                                          size_t* len)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(len);
        vector_out(h->impl->inverse_singular_values_host(bond), out, capacity, len);
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_set_two_site_tensors(t4a_gpu_inverse_tt* h, size_t site, const size_t* dims3_1, const double* data1,
                                                       const double* inv_sv, size_t inv_len, const size_t* dims3_2, const double* data2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3_1);
        T4A_REQUIRE_PTR(dims3_2);
        h->impl->set_two_site_tensors(site, dims3_1, data1, inv_sv, inv_len, dims3_2, data2);
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_to_tt(const t4a_gpu_inverse_tt* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(h);
        std::vector<DevCore> cores = h->impl->to_tensor_train_cores();
        *out = tt_from_cores(cores, h->impl->eng ? h->impl->eng->stream() : nullptr);
    });
}

t4a_gpu_status t4a_gpu_inverse_tt_tensors_tt(const t4a_gpu_inverse_tt* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(h);
        *out = tt_from_cores(h->impl->cores, h->impl->eng ? h->impl->eng->stream() : nullptr);
    });
}

// ---- simplett_bridge.rs: chain of labelled tensors <-> tensor train ----
t4a_gpu_status t4a_gpu_tt_to_tensors(const t4a_gpu_tt* tt, const int64_t* site_labels, const int64_t* bond_labels,
                                     t4a_gpu_tensor** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tt);
        const size_t n = tt->impl.len();
        if (n == 0) return;
        T4A_REQUIRE_PTR(site_labels);
        T4A_REQUIRE_PTR(out);
        if (n > 1) T4A_REQUIRE_PTR(bond_labels);
        for (size_t s = 0; s < n; ++s) out[s] = nullptr;
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        require_distinct_chain_labels(site_labels, bond_labels, n);
        std::vector<OwnedTensor> made = chain_to_tensors(dense_engine(), const_cast<t4a_gpu_tt*>(tt)->impl.eng, tt->impl.cores, site_labels, bond_labels);
        std::vector<std::unique_ptr<t4a_gpu_tensor>> handles;
        for (OwnedTensor& t : made) handles.push_back(make_tensor(std::move(t)));
        for (size_t s = 0; s < n; ++s) out[s] = handles[s].release();
    });
}

t4a_gpu_status t4a_gpu_tensors_to_tt(const t4a_gpu_tensor* const* tensors, size_t n_sites, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        require_device();
        if (n_sites == 0) {
            *out = new t4a_gpu_tt(std::vector<std::array<size_t, 3>>{}, nullptr);
            return;
        }
        T4A_REQUIRE_PTR(tensors);
        const std::vector<TensorView> views = handle_list(tensors, n_sites, "tensors[s] is null", [](const t4a_gpu_tensor& t) { return t.view(); });
        const ChainPlan plan = plan_tensors_to_chain(views); // (argument errors before the device is touched)
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        Engine& e = dense_engine();
        *out = new t4a_gpu_tt(tensors_to_chain(e, views, plan), e.stream());
    });
}

// ---- tensor4all-aci ----
t4a_gpu_status t4a_gpu_aci_options_default(t4a_gpu_aci_options* o)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(o);
        const AciOptions d;
        o->max_iters = d.max_iters;
        o->min_iters = d.min_iters;
        o->has_max_bond_dim = 0;
        o->max_bond_dim = 0;
        o->tolerance = d.tolerance;
        o->scale_tolerance = 1;
        o->rng_seed = 0;
        o->enable_global_guard = 1;
        o->nsearch_global_pivots = d.nsearch_global_pivots;
        o->max_nglobal_pivot = d.max_nglobal_pivot;
        o->nsweeps_global_search = d.nsweeps_global_search;
        o->tol_margin_global_search = d.tol_margin_global_search;
    });
}

t4a_gpu_status t4a_gpu_aci_elementwise(const t4a_gpu_tt* const* inputs, size_t n_inputs, int32_t op_kind, t4a_gpu_aci_op_fn op,
                                       void* user, const t4a_gpu_aci_options* options, const t4a_gpu_tt* initial_guess,
                                       t4a_gpu_tt** result, size_t* n_iters, size_t* ranks, double* errors,
                                       size_t* nglobal_pivots, int32_t* termination)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(result);
        *result = nullptr;
        const AciOptions o = convert_aci(options);
        o.validate();
        std::vector<TensorTrain*> in = aci_inputs(inputs, n_inputs);
        AciHostOp hop = aci_host_op(aci_op_kind(op_kind, "unknown ACI operator kind"), op, user, "operator callback is null", "operator callback reported an error");
        require_device();
        if (n_iters) *n_iters = 0;
        if (in[0] && in[0]->len() == 1) {
            std::unique_ptr<TensorTrain> tt = aci_one_site(in, (AciOpKind)op_kind, hop);
            *result = new t4a_gpu_tt(tt->cores, tt->eng.stream());
            if (termination) *termination = 0;
            return;
        }
        AciProblem p(in, initial_guess ? &initial_guess->impl : nullptr, o, (AciOpKind)op_kind, hop);
        p.run();
        std::unique_ptr<TensorTrain> tt = p.solution_tt();
        tt->eng.sync();
        *result = new t4a_gpu_tt(tt->cores, tt->eng.stream());
        if (n_iters) *n_iters = p.ranks.size();
        for (size_t i = 0; i < p.ranks.size(); ++i) {
            if (ranks) ranks[i] = p.ranks[i];
            if (errors) errors[i] = p.errors[i];
            if (nglobal_pivots) nglobal_pivots[i] = p.nglobal_pivots[i];
        }
        if (termination) *termination = (int32_t)p.termination;
    });
}

t4a_gpu_status t4a_gpu_aci_problem_new(const t4a_gpu_tt* const* inputs, size_t n_inputs, int32_t op_kind, t4a_gpu_aci_op_fn op,
                                       void* user, const t4a_gpu_aci_options* options, const t4a_gpu_tt* initial_guess,
                                       t4a_gpu_aci_problem** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        const AciOptions o = convert_aci(options);
        o.validate();
        std::vector<TensorTrain*> in = aci_inputs(inputs, n_inputs);
        AciHostOp hop = aci_host_op(aci_op_kind(op_kind, "unknown ACI operator kind"), op, user, "operator callback is null", "operator callback reported an error");
        require_device();
        auto h = std::make_unique<t4a_gpu_aci_problem>();
        h->impl = std::make_unique<AciProblem>(in, initial_guess ? &initial_guess->impl : nullptr, o, (AciOpKind)op_kind, hop);
        *out = h.release();
    });
}

void t4a_gpu_aci_problem_release(t4a_gpu_aci_problem* h) { delete h; }

t4a_gpu_status t4a_gpu_treeaci_local_update_f64(size_t n_inputs, const size_t* bond_dims, const double* const* row_frames,
                                                const double* const* col_frames, size_t row_count, size_t col_count, int32_t op_kind,
                                                t4a_gpu_aci_op_fn op, void* user, size_t max_bond_dim, double tolerance,
                                                int32_t scale_tolerance, int32_t left_orthogonal, size_t* rank, size_t* row_indices,
                                                size_t* col_indices, double* pivot_errors, size_t* n_pivot_errors, double* left,
                                                double* right, double* sampled_scale, double* local_values)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(bond_dims);
        T4A_REQUIRE_PTR(row_frames);
        T4A_REQUIRE_PTR(col_frames);
        T4A_REQUIRE_PTR(rank);
        T4A_REQUIRE_PTR(row_indices);
        T4A_REQUIRE_PTR(col_indices);
        T4A_REQUIRE_PTR(pivot_errors);
        T4A_REQUIRE_PTR(n_pivot_errors);
        T4A_REQUIRE_PTR(left);
        T4A_REQUIRE_PTR(right);
        T4A_REQUIRE_PTR(sampled_scale);
        const AciOpKind kind = aci_op_kind(op_kind, "unknown operator kind");
        checked_mul(row_count, col_count, "local matrix elements");
        require_int_dims({row_count, col_count}, "local matrix shape");
        std::vector<size_t> bd(bond_dims, bond_dims + n_inputs);
        std::vector<const double*> rf(n_inputs), cf(n_inputs);
        for (size_t k = 0; k < n_inputs; ++k) {
            if (bd[k] && (!row_frames[k] || !col_frames[k])) throw Error(T4A_GPU_NULL_POINTER, "frame block is null");
            rf[k] = row_frames[k];
            cf[k] = col_frames[k];
        }
        const AciHostOp host = aci_host_op(kind, op, user, "op is null", "elementwise operator callback failed");
        std::lock_guard<std::mutex> lock(g_dense_mutex);
        TreeAciLocalResult r = treeaci_local_update(dense_engine(), bd, rf, cf, row_count, col_count, kind, host, max_bond_dim,
                                                    tolerance, scale_tolerance != 0, left_orthogonal != 0);
        *rank = r.rank;
        for (size_t i = 0; i < r.rank; ++i) {
            row_indices[i] = r.row_indices[i];
            col_indices[i] = r.col_indices[i];
        }
        *n_pivot_errors = r.pivot_errors.size();
        for (size_t i = 0; i < r.pivot_errors.size(); ++i) pivot_errors[i] = r.pivot_errors[i];
        std::copy(r.left.begin(), r.left.end(), left);
        std::copy(r.right.begin(), r.right.end(), right);
        *sampled_scale = r.sampled_scale;
        if (local_values) std::copy(r.local_values.begin(), r.local_values.end(), local_values);
    });
}

t4a_gpu_status t4a_gpu_aci_problem_local_update(t4a_gpu_aci_problem* h, size_t bond, int32_t left_orthogonal)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl->local_update(bond, left_orthogonal != 0);
    });
}

t4a_gpu_status t4a_gpu_aci_problem_add_global_pivots(t4a_gpu_aci_problem* h, const size_t* pivots, size_t n_pivots, size_t* added)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pivots) T4A_REQUIRE_PTR(pivots);
        const size_t a = h->impl->add_global_pivots(narrow_pivots(pivots, n_pivots, h->impl->len(), "global pivot index out of bounds"));
        if (added) *added = a;
    });
}

t4a_gpu_status t4a_gpu_aci_problem_find_global_pivots(t4a_gpu_aci_problem* h, uint64_t seed, size_t* count, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(count);
        const auto pv = h->impl->find_global_pivots(seed);
        *count = pv.size();
        const size_t n = h->impl->len();
        if (out)
            for (size_t p = 0; p < pv.size(); ++p)
                for (size_t s = 0; s < n; ++s) out[s + n * p] = pv[p][s];
    });
}

t4a_gpu_status t4a_gpu_aci_problem_solution(t4a_gpu_aci_problem* h, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        std::unique_ptr<TensorTrain> tt = h->impl->solution_tt();
        tt->eng.sync();
        *out = new t4a_gpu_tt(tt->cores, tt->eng.stream());
    });
}

t4a_gpu_status t4a_gpu_aci_problem_frame(t4a_gpu_aci_problem* h, int32_t right, size_t input, size_t site, size_t* rows,
                                         size_t* cols, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(rows);
        T4A_REQUIRE_PTR(cols);
        const std::vector<double> f = h->impl->frame_host(right != 0, input, site, rows, cols);
        if (out) std::copy(f.begin(), f.end(), out);
    });
}

t4a_gpu_status t4a_gpu_aci_problem_errors(const t4a_gpu_aci_problem* h, double* pivot_errors, double* pivot_scales)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (pivot_errors) std::copy(h->impl->pivot_errors.begin(), h->impl->pivot_errors.end(), pivot_errors);
        if (pivot_scales) std::copy(h->impl->pivot_scales.begin(), h->impl->pivot_scales.end(), pivot_scales);
    });
}

// ---- MPO<f64> and its contraction (tensor4all-simplett/src/mpo/) ----
t4a_gpu_status t4a_gpu_mpo_new(const size_t* dims4, size_t n_sites, const double* cores, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sites) T4A_REQUIRE_PTR(dims4);
        std::vector<std::array<size_t, 4>> d(n_sites);
        for (size_t s = 0; s < n_sites; ++s) d[s] = {dims4[4 * s], dims4[4 * s + 1], dims4[4 * s + 2], dims4[4 * s + 3]};
        mpo_validate_dims(d); // shape errors come before the device is touched
        if (n_sites) T4A_REQUIRE_PTR(cores);
        require_device();
        *out = new t4a_gpu_mpo{std::make_unique<Mpo>(d, cores)};
    });
}

void t4a_gpu_mpo_release(t4a_gpu_mpo* h) { delete h; }

t4a_gpu_status t4a_gpu_mpo_clone(const t4a_gpu_mpo* h, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_mpo{std::make_unique<Mpo>(h->impl->tt.cores, h->impl->tt.eng.stream(), h->impl->sd)};
    });
}

t4a_gpu_status t4a_gpu_mpo_len(const t4a_gpu_mpo* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->len();
    });
}

t4a_gpu_status t4a_gpu_mpo_dims(const t4a_gpu_mpo* h, size_t* dims4)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        const auto d = h->impl->dims4();
        if (!d.empty()) T4A_REQUIRE_PTR(dims4);
        for (size_t s = 0; s < d.size(); ++s)
            for (int k = 0; k < 4; ++k) dims4[4 * s + k] = d[s][k];
    });
}

t4a_gpu_status t4a_gpu_mpo_site_tensor(const t4a_gpu_mpo* h, size_t site, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        std::vector<double> v = h->impl->tt.site_tensor_host(site);
        if (!v.empty()) {
            T4A_REQUIRE_PTR(out);
            std::memcpy(out, v.data(), v.size() * sizeof(double));
        }
    });
}

t4a_gpu_status t4a_gpu_mpo_evaluate(t4a_gpu_mpo* h, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, 2 * h->impl->len(), "index buffer"));
        std::vector<double> v = h->impl->evaluate(u.data(), n_pts);
        std::memcpy(out, v.data(), n_pts * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_mpo_sum(t4a_gpu_mpo* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->sum();
    });
}

t4a_gpu_status t4a_gpu_mpo_contract(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, int32_t algorithm, int32_t compress, int32_t method,
                                    double tolerance, size_t max_bond_dim, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (algorithm < 0 || algorithm > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown contraction algorithm");
        if (method < 0 || method > 3) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown factorize method");
        MpoContractionOptions o;
        o.tolerance = tolerance;
        o.max_bond_dim = max_bond_dim;
        o.method = (MpoFactorizeMethod)method;
        *out = new t4a_gpu_mpo{mpo_contract(*a->impl, *b->impl, (MpoAlgorithm)algorithm, compress != 0, o)};
    });
}

t4a_gpu_status t4a_gpu_mpo_from_tt(const t4a_gpu_tt* tt, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tt);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        std::vector<std::array<size_t, 2>> sd;
        for (const auto& c : tt->impl.cores) sd.push_back({c.s, 1});
        *out = new t4a_gpu_mpo{std::make_unique<Mpo>(tt->impl.cores, tt->impl.eng.stream(), sd)};
    });
}

t4a_gpu_status t4a_gpu_mpo_to_tt(const t4a_gpu_mpo* mpo, t4a_gpu_tt** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(mpo);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_tt(mpo->impl->tt.cores, mpo->impl->tt.eng.stream());
    });
}

t4a_gpu_status t4a_gpu_mpo_transpose(const t4a_gpu_mpo* mpo, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(mpo);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_mpo{mpo->impl->transpose()};
    });
}

// ---- variational (fit) contraction of two MPOs (mpo.hpp: mpo_contract_fit) ----
t4a_gpu_status t4a_gpu_mpo_fit_options_default(t4a_gpu_mpo_fit_options* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const MpoFitOptions d;
        out->tolerance = d.tolerance;
        out->has_max_bond_dim = d.max_bond_dim != 0;
        out->max_bond_dim = d.max_bond_dim;
        out->max_sweeps = d.max_sweeps;
        out->convergence_tol = d.convergence_tol;
        out->factorize_method = (int32_t)d.method;
    });
}

t4a_gpu_status t4a_gpu_mpo_contract_fit(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const t4a_gpu_mpo_fit_options* options,
                                        const t4a_gpu_mpo* initial, t4a_gpu_mpo** out, size_t* n_sweeps, double* norms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sweeps) *n_sweeps = 0;
        T4A_REQUIRE_PTR(options);
        // the options are checked on the host before an operand is looked at
        if (options->factorize_method < 0 || options->factorize_method > 3) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown factorize method");
        MpoFitOptions o;
        o.tolerance = options->tolerance;
        o.max_bond_dim = options->has_max_bond_dim ? options->max_bond_dim : 0;
        if (options->has_max_bond_dim && options->max_bond_dim == 0)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "contract_fit: max_bond_dim must be at least 1");
        o.max_sweeps = options->max_sweeps;
        o.convergence_tol = options->convergence_tol;
        o.method = (MpoFactorizeMethod)options->factorize_method;
        mpo_fit_validate_options(o);
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        MpoFitInfo info;
        *out = new t4a_gpu_mpo{mpo_contract_fit(*a->impl, *b->impl, o, initial ? initial->impl.get() : nullptr, info)};
        if (n_sweeps) *n_sweeps = info.n_sweeps;
        if (norms) std::copy(info.norms.begin(), info.norms.end(), norms);
    });
}

t4a_gpu_status t4a_gpu_mpo_fit_half(const double* env, size_t n_env, int32_t side, const t4a_gpu_mpo* a, const t4a_gpu_mpo* b,
                                    size_t site, double* out)
{
    return guarded([&] {
        if (side != 0 && side != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "fit_half: side must be 0 (left) or 1 (right)");
        if (n_env == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "fit_half: the environment has a zero dimension");
        T4A_REQUIRE_PTR(env);
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        std::vector<double> v = mpo_fit_half(env, n_env, side == 1, *a->impl, *b->impl, site);
        std::memcpy(out, v.data(), v.size() * sizeof(double));
    });
}

// ---- partial contraction of two MPOs (mpo.hpp: mpo_partial_contract) ----
t4a_gpu_status t4a_gpu_mpo_partial_plan(const size_t* a_site_dims, size_t n_a, const size_t* b_site_dims, size_t n_b,
                                        const size_t* contract_pairs, size_t n_contract, const size_t* diagonal_pairs, size_t n_diagonal,
                                        size_t n_output_order, size_t* out_site_dims, size_t* out_leg_dims)
{
    return guarded([&] {
        if (n_a) T4A_REQUIRE_PTR(a_site_dims);
        if (n_b) T4A_REQUIRE_PTR(b_site_dims);
        std::vector<std::array<size_t, 2>> sa(n_a), sb(n_b);
        for (size_t i = 0; i < n_a; ++i) sa[i] = {a_site_dims[2 * i], a_site_dims[2 * i + 1]};
        for (size_t i = 0; i < n_b; ++i) sb[i] = {b_site_dims[2 * i], b_site_dims[2 * i + 1]};
        const std::vector<PartialSitePlan> plan =
            mpo_partial_plan(sa, sb, partial_spec(contract_pairs, n_contract, diagonal_pairs, n_diagonal, n_output_order));
        for (size_t i = 0; i < plan.size(); ++i) {
            if (out_site_dims) out_site_dims[2 * i] = plan[i].S, out_site_dims[2 * i + 1] = plan[i].T;
            if (out_leg_dims)
                for (int k = 0; k < 4; ++k) out_leg_dims[4 * i + k] = plan[i].leg_dims[k];
        }
    });
}

t4a_gpu_status t4a_gpu_mpo_partial_contract(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const size_t* contract_pairs, size_t n_contract,
                                            const size_t* diagonal_pairs, size_t n_diagonal, size_t n_output_order, int32_t algorithm,
                                            int32_t compress, int32_t method, double tolerance, size_t max_bond_dim, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (algorithm < 0 || algorithm > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown contraction algorithm");
        if (method < 0 || method > 3) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown factorize method");
        MpoContractionOptions o;
        o.tolerance = tolerance;
        o.max_bond_dim = max_bond_dim;
        o.method = (MpoFactorizeMethod)method;
        const PartialSpec spec = partial_spec(contract_pairs, n_contract, diagonal_pairs, n_diagonal, n_output_order);
        *out = new t4a_gpu_mpo{mpo_partial_contract(*a->impl, *b->impl, spec, (MpoAlgorithm)algorithm, compress != 0, o)};
    });
}

t4a_gpu_status t4a_gpu_mpo_partial_contract_fit(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const size_t* contract_pairs, size_t n_contract,
                                                const size_t* diagonal_pairs, size_t n_diagonal, size_t n_output_order,
                                                const t4a_gpu_mpo_fit_options* options, const t4a_gpu_mpo* initial, t4a_gpu_mpo** out,
                                                size_t* n_sweeps, double* norms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sweeps) *n_sweeps = 0;
        T4A_REQUIRE_PTR(options);
        // the options are checked on the host before an operand is looked at, as in t4a_gpu_mpo_contract_fit
        if (options->factorize_method < 0 || options->factorize_method > 3) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown factorize method");
        MpoFitOptions o;
        o.tolerance = options->tolerance;
        o.max_bond_dim = options->has_max_bond_dim ? options->max_bond_dim : 0;
        if (options->has_max_bond_dim && options->max_bond_dim == 0)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "contract_fit: max_bond_dim must be at least 1");
        o.max_sweeps = options->max_sweeps;
        o.convergence_tol = options->convergence_tol;
        o.method = (MpoFactorizeMethod)options->factorize_method;
        mpo_fit_validate_options(o);
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        const PartialSpec spec = partial_spec(contract_pairs, n_contract, diagonal_pairs, n_diagonal, n_output_order);
        MpoFitInfo info;
        *out = new t4a_gpu_mpo{mpo_partial_contract_fit(*a->impl, *b->impl, spec, o, initial ? initial->impl.get() : nullptr, info)};
        if (n_sweeps) *n_sweeps = info.n_sweeps;
        if (norms) std::copy(info.norms.begin(), info.norms.end(), norms);
    });
}

t4a_gpu_status t4a_gpu_mpo_partial_half(const double* env, size_t n_env, int32_t side, const t4a_gpu_mpo* a, const t4a_gpu_mpo* b,
                                        const size_t* contract_pairs, size_t n_contract, const size_t* diagonal_pairs, size_t n_diagonal,
                                        size_t site, double* out)
{
    return guarded([&] {
        if (side != 0 && side != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_half: side must be 0 (left) or 1 (right)");
        if (n_env == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_half: the environment has a zero dimension");
        T4A_REQUIRE_PTR(env);
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        const PartialSpec spec = partial_spec(contract_pairs, n_contract, diagonal_pairs, n_diagonal, 0);
        std::vector<double> v = mpo_partial_half(env, n_env, side == 1, *a->impl, *b->impl, spec, site);
        std::memcpy(out, v.data(), v.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_mpo_relabel_site_dims(t4a_gpu_mpo* mpo, const size_t* site_dims, size_t n_sites)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(mpo);
        if (n_sites) T4A_REQUIRE_PTR(site_dims);
        std::vector<std::array<size_t, 2>> sd(n_sites);
        for (size_t i = 0; i < n_sites; ++i) sd[i] = {site_dims[2 * i], site_dims[2 * i + 1]};
        mpo->impl->relabel_site_dims(sd);
    });
}

// ---- Contraction<f64>: the lazy product of two MPOs (tensor4all-simplett/src/mpo/contraction.rs:60-383) ----
t4a_gpu_status t4a_gpu_contraction_new(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, t4a_gpu_contraction** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_contraction{std::make_unique<MpoContraction>(*a->impl, *b->impl)};
    });
}

void t4a_gpu_contraction_release(t4a_gpu_contraction* h) { delete h; }

t4a_gpu_status t4a_gpu_contraction_len(const t4a_gpu_contraction* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->len();
    });
}

t4a_gpu_status t4a_gpu_contraction_result_site_dims(const t4a_gpu_contraction* h, size_t* dims2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        const auto d = h->impl->result_site_dims();
        if (!d.empty()) T4A_REQUIRE_PTR(dims2);
        for (size_t s = 0; s < d.size(); ++s) {
            dims2[2 * s] = d[s][0];
            dims2[2 * s + 1] = d[s][1];
        }
    });
}

t4a_gpu_status t4a_gpu_contraction_evaluate(t4a_gpu_contraction* h, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, 2 * h->impl->len(), "index buffer"));
        h->impl->evaluate(u.data(), n_pts, out);
    });
}

t4a_gpu_status t4a_gpu_contraction_evaluate_left(t4a_gpu_contraction* h, size_t n, const size_t* idx, size_t n_pts, double* out, size_t* dims2)
{
    return guarded([&] { contraction_environment(h, true, n, idx, n_pts, out, dims2); });
}

t4a_gpu_status t4a_gpu_contraction_evaluate_right(t4a_gpu_contraction* h, size_t n, const size_t* idx, size_t n_pts, double* out, size_t* dims2)
{
    return guarded([&] { contraction_environment(h, false, n, idx, n_pts, out, dims2); });
}

t4a_gpu_status t4a_gpu_contraction_evaluate_many(t4a_gpu_contraction* h, const size_t* idx, size_t n_pts, size_t split, double* out,
                                                 size_t* used_split)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (used_split) *used_split = split;
        if (n_pts == 0) return; // cache.rs:563-565
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, 2 * h->impl->len(), "index buffer"));
        const size_t s = h->impl->evaluate_many(u.data(), n_pts, split, out);
        if (used_split) *used_split = s;
    });
}

t4a_gpu_status t4a_gpu_contraction_clear_cache(t4a_gpu_contraction* h)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl->clear_cache();
    });
}

t4a_gpu_status t4a_gpu_contraction_n_evaluated(const t4a_gpu_contraction* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->n_evaluated();
    });
}

int64_t t4a_gpu_contraction_batch_eval(void* ctx, const uint32_t* idx, size_t n_sites, size_t n_pts, double* out)
{
    const t4a_gpu_status st = guarded([&] {
        T4A_REQUIRE_PTR(ctx);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        static_cast<t4a_gpu_contraction*>(ctx)->impl->evaluate_fused(idx, n_sites, n_pts, out);
    });
    return st == T4A_GPU_SUCCESS ? (int64_t)n_pts : (int64_t)st; // status codes are negative
}

t4a_gpu_status t4a_gpu_mpo_contract_tci(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const t4a_gpu_tci2_options* options,
                                        const size_t* initial_pivots, size_t n_pivots, t4a_gpu_mpo** out_mpo, double* info)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(options);
        T4A_REQUIRE_PTR(out_mpo);
        T4A_REQUIRE_PTR(info);
        *out_mpo = nullptr;
        if (n_pivots) T4A_REQUIRE_PTR(initial_pivots);
        const TCI2Options o = convert_options(options);
        std::vector<std::vector<uint32_t>> piv = narrow_pivots(initial_pivots, n_pivots, a->impl->len(), "pivot value out of bounds");
        *out_mpo = new t4a_gpu_mpo{mpo_contract_tci(*a->impl, *b->impl, o, std::move(piv), info)};
    });
}

// ---- candidate matrices of A·B on the device: the entries below answer INVALID_ARGUMENT for NULL (t4a_gpu.h) ----
t4a_gpu_status t4a_gpu_contraction_evaluate_matrix(t4a_gpu_contraction* h, size_t cut, const size_t* rows, size_t n_rows, const size_t* cols,
                                                   size_t n_cols, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_ARG(h);
        const size_t n = h->impl->len();
        const size_t wl = 2 * std::min(cut, n), wr = 2 * (n - std::min(cut, n));
        if (n_rows && wl) T4A_REQUIRE_ARG(rows);
        if (n_cols && wr) T4A_REQUIRE_ARG(cols);
        if (n_rows && n_cols) T4A_REQUIRE_ARG(out);
        const std::vector<uint32_t> r = narrow_indices(rows, checked_mul(n_rows, wl, "index buffer"));
        const std::vector<uint32_t> c = narrow_indices(cols, checked_mul(n_cols, wr, "index buffer"));
        checked_mul(n_rows, n_cols, "matrix");
        h->impl->evaluate_matrix_host(cut, r.data(), n_rows, c.data(), n_cols, out);
    });
}

t4a_gpu_status t4a_gpu_tci2_set_contraction_source(t4a_gpu_tci2* tci2, t4a_gpu_contraction* contraction)
{
    return guarded([&] {
        T4A_REQUIRE_ARG(tci2);
        T4A_REQUIRE_ARG(contraction);
        tci2->impl.set_source(contraction->impl.get());
    });
}

t4a_gpu_status t4a_gpu_tci2_source_stats(const t4a_gpu_tci2* tci2, uint64_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_ARG(tci2);
        T4A_REQUIRE_ARG(out);
        for (int k = 0; k < 3; ++k) out[k] = tci2->impl.source_stats[k];
    });
}

t4a_gpu_status t4a_gpu_mpo_contract_tci_device(const t4a_gpu_mpo* a, const t4a_gpu_mpo* b, const t4a_gpu_tci2_options* options,
                                               const size_t* initial_pivots, size_t n_pivots, t4a_gpu_mpo** out_mpo, double* info)
{
    return guarded([&] {
        T4A_REQUIRE_ARG(out_mpo);
        *out_mpo = nullptr;
        T4A_REQUIRE_ARG(a);
        T4A_REQUIRE_ARG(b);
        T4A_REQUIRE_ARG(options);
        T4A_REQUIRE_ARG(info);
        if (n_pivots) T4A_REQUIRE_ARG(initial_pivots);
        const TCI2Options o = convert_options(options);
        std::vector<std::vector<uint32_t>> piv = narrow_pivots(initial_pivots, n_pivots, a->impl->len(), "pivot value out of bounds");
        *out_mpo = new t4a_gpu_mpo{mpo_contract_tci(*a->impl, *b->impl, o, std::move(piv), info, true)};
    });
}

// ---- quantics transform operators (tensor4all-quanticstransform): host builders, one upload, the difference kernel ----
t4a_gpu_status t4a_gpu_qt_shift_operator(size_t r, int64_t offset, int32_t bc, t4a_gpu_qt_op** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_qt_op{qt_shift(r, offset, (BoundaryCondition)bc)};
    });
}

t4a_gpu_status t4a_gpu_qt_shift_operator_multivar(size_t r, int64_t offset, int32_t bc, size_t nvariables, size_t target_var,
                                                  t4a_gpu_qt_op** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_qt_op{qt_embed(qt_shift(r, offset, (BoundaryCondition)bc), nvariables, target_var)};
    });
}

t4a_gpu_status t4a_gpu_qt_flip_operator(size_t r, int32_t bc, t4a_gpu_qt_op** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_qt_op{qt_flip(r, (BoundaryCondition)bc)};
    });
}

t4a_gpu_status t4a_gpu_qt_flip_operator_multivar(size_t r, int32_t bc, size_t nvariables, size_t target_var, t4a_gpu_qt_op** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_qt_op{qt_embed(qt_flip(r, (BoundaryCondition)bc), nvariables, target_var)};
    });
}

t4a_gpu_status t4a_gpu_qt_triangle_operator(size_t r, int32_t triangle, t4a_gpu_qt_op** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_qt_op{qt_triangle(r, (TriangleType)triangle)};
    });
}

t4a_gpu_status t4a_gpu_qt_cumsum_operator(size_t r, t4a_gpu_qt_op** out) { return t4a_gpu_qt_triangle_operator(r, T4A_GPU_QT_LOWER, out); }

t4a_gpu_status t4a_gpu_qt_affine_operator(size_t r, const int64_t* a, size_t a_len, const int64_t* b, size_t b_len, int64_t scale,
                                          size_t m, size_t n, const int32_t* bc, size_t n_bc, t4a_gpu_qt_op** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (a_len) T4A_REQUIRE_PTR(a);
        if (b_len) T4A_REQUIRE_PTR(b);
        if (n_bc) T4A_REQUIRE_PTR(bc);
        std::vector<BoundaryCondition> conditions(n_bc);
        for (size_t i = 0; i < n_bc; ++i) conditions[i] = (BoundaryCondition)bc[i];
        *out = new t4a_gpu_qt_op{qt_affine(r, std::vector<int64_t>(a, a + a_len), std::vector<int64_t>(b, b + b_len), scale, m, n, conditions)};
    });
}

void t4a_gpu_qt_op_release(t4a_gpu_qt_op* h) { delete h; }

t4a_gpu_status t4a_gpu_qt_op_len(const t4a_gpu_qt_op* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl.len();
    });
}

t4a_gpu_status t4a_gpu_qt_op_dims(const t4a_gpu_qt_op* h, size_t* dims4)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (h->impl.len()) T4A_REQUIRE_PTR(dims4);
        for (size_t s = 0; s < h->impl.len(); ++s)
            for (int k = 0; k < 4; ++k) dims4[4 * s + k] = h->impl.dims[s][k];
    });
}

t4a_gpu_status t4a_gpu_qt_op_site_tensor(const t4a_gpu_qt_op* h, size_t site, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        if (site >= h->impl.len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "site out of range");
        const std::vector<double>& v = h->impl.sites[site];
        std::memcpy(out, v.data(), v.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_qt_op_to_mpo(const t4a_gpu_qt_op* h, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_mpo{qt_upload(h->impl)};
    });
}

t4a_gpu_status t4a_gpu_qt_difference_kernel(const t4a_gpu_tt* f, int32_t bc, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(f);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_mpo{qt_difference_kernel(const_cast<t4a_gpu_tt*>(f)->impl, (BoundaryCondition)bc)};
    });
}

// ---- square_linsolve: (a0 + a1 A) x = b by two-site sweeps with a local GMRES (linsolve.hpp) ----
t4a_gpu_status t4a_gpu_linsolve_options_default(t4a_gpu_linsolve_options* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const LinsolveOptions d;
        *out = t4a_gpu_linsolve_options{};
        out->nfullsweeps = d.nfullsweeps;
        out->has_max_bond_dim = d.has_max_bond_dim;
        out->max_bond_dim = d.max_bond_dim;
        out->has_svd_policy = d.has_svd_policy;
        out->svd_policy = to_c(d.svd_policy);
        out->gmres_tol = d.gmres_tol;
        out->gmres_tolerance_mode = (int32_t)d.gmres_tolerance_mode;
        out->gmres_max_restarts = d.gmres_max_restarts;
        out->gmres_restart_dim = d.gmres_restart_dim;
        out->a0 = d.a0;
        out->a1 = d.a1;
        out->has_convergence_tol = d.has_convergence_tol;
        out->convergence_tol = d.convergence_tol;
        out->check_residual = d.check_residual;
    });
}

t4a_gpu_status t4a_gpu_linsolve_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* rhs_dims3, size_t n_rhs,
                                             const size_t* state_dims3, size_t n_state, size_t center, size_t gmres_restart_dim)
{
    return guarded([&] {
        if (n_op) T4A_REQUIRE_PTR(op_dims4);
        if (n_rhs) T4A_REQUIRE_PTR(rhs_dims3);
        if (n_state) T4A_REQUIRE_PTR(state_dims3);
        const auto rhs = dims3_list(rhs_dims3, n_rhs);
        linsolve_validate_shapes(dims4_list(op_dims4, n_op), rhs_dims3 ? &rhs : nullptr, dims3_list(state_dims3, n_state), center, gmres_restart_dim);
    });
}

t4a_gpu_status t4a_gpu_square_linsolve(const t4a_gpu_mpo* op, const t4a_gpu_tt* rhs, const t4a_gpu_tt* init, size_t center,
                                       const t4a_gpu_linsolve_options* options, t4a_gpu_tt** solution, size_t* sweeps,
                                       int32_t* has_residual, double* residual, int32_t* converged, t4a_gpu_linsolve_stats* stats)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(solution);
        *solution = nullptr;
        T4A_REQUIRE_PTR(options);
        const LinsolveOptions o = convert_linsolve_options(options); // the options are checked on the host before an operand is looked at
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(rhs);
        T4A_REQUIRE_PTR(init);
        T4A_REQUIRE_PTR(sweeps);
        T4A_REQUIRE_PTR(has_residual);
        T4A_REQUIRE_PTR(residual);
        T4A_REQUIRE_PTR(converged);
        LinsolveResult r = square_linsolve(*op->impl, const_cast<t4a_gpu_tt*>(rhs)->impl, const_cast<t4a_gpu_tt*>(init)->impl, center, o);
        *solution = new t4a_gpu_tt(r.solution->cores, r.solution->eng.stream());
        *sweeps = r.sweeps;
        *has_residual = r.has_residual;
        *residual = r.residual;
        *converged = r.converged;
        if (stats) *stats = t4a_gpu_linsolve_stats{r.stats.local_solves, r.stats.arnoldi_steps, r.stats.apply_calls};
    });
}

t4a_gpu_status t4a_gpu_relative_linear_system_residual(const t4a_gpu_mpo* op, const t4a_gpu_tt* solution, const t4a_gpu_tt* rhs, double a0,
                                                       double a1, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(solution);
        T4A_REQUIRE_PTR(rhs);
        T4A_REQUIRE_PTR(out);
        *out = relative_linear_system_residual(*op->impl, const_cast<t4a_gpu_tt*>(solution)->impl, const_cast<t4a_gpu_tt*>(rhs)->impl, a0, a1);
    });
}

t4a_gpu_status t4a_gpu_projected_operator_new(const t4a_gpu_mpo* op, const t4a_gpu_tt* state, t4a_gpu_projected_operator** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(state);
        *out = new t4a_gpu_projected_operator{std::make_unique<ProjectedOperator>(*op->impl, const_cast<t4a_gpu_tt*>(state)->impl, nullptr)};
    });
}

void t4a_gpu_projected_operator_release(t4a_gpu_projected_operator* h) { delete h; }

t4a_gpu_status t4a_gpu_projected_operator_local_dims(const t4a_gpu_projected_operator* h, size_t site, size_t* dims4)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims4);
        const auto d = h->impl->local_dims(site);
        std::copy(d.begin(), d.end(), dims4);
    });
}

t4a_gpu_status t4a_gpu_projected_operator_apply(t4a_gpu_projected_operator* h, size_t site, const double* v, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(v);
        T4A_REQUIRE_PTR(out);
        const std::vector<double> y = h->impl->apply(site, v);
        std::memcpy(out, y.data(), y.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_projected_operator_apply_one_site(t4a_gpu_projected_operator* h, size_t site, const double* v, double* out, int32_t* reused_hl)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(v);
        T4A_REQUIRE_PTR(out);
        bool reused = false;
        const std::vector<double> y = h->impl->apply_one_site(site, v, &reused);
        std::memcpy(out, y.data(), y.size() * sizeof(double));
        if (reused_hl) *reused_hl = reused;
    });
}

t4a_gpu_status t4a_gpu_projected_operator_time_one_site(t4a_gpu_projected_operator* h, size_t site, size_t reps, double* ms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(ms);
        h->impl->time_one_site(site, reps, ms);
    });
}

t4a_gpu_status t4a_gpu_projected_operator_environment(t4a_gpu_projected_operator* h, int32_t side, size_t bond, size_t* dims3, double* out)
{
    return guarded([&] {
        if (side != 0 && side != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: side must be 0 (left) or 1 (right)");
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3);
        const std::vector<double> e = h->impl->environment(side, bond, dims3);
        if (out) std::memcpy(out, e.data(), e.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_projected_operator_bond_center_env(t4a_gpu_projected_operator* h, size_t site, int32_t toward_right, size_t* dims3, double* out)
{
    return guarded([&] {
        if (toward_right != 0 && toward_right != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "projected operator: toward_right must be 0 or 1");
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3);
        const std::vector<double> e = h->impl->bond_center_environment(site, toward_right != 0, dims3);
        if (out) std::memcpy(out, e.data(), e.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_projected_operator_invalidate(t4a_gpu_projected_operator* h, size_t site)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        h->impl->invalidate(site);
    });
}

t4a_gpu_status t4a_gpu_projected_operator_set_site_tensors(t4a_gpu_projected_operator* h, size_t site, const size_t* dims3_a, const double* t_a,
                                                           const size_t* dims3_b, const double* t_b)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(dims3_a);
        T4A_REQUIRE_PTR(t_a);
        T4A_REQUIRE_PTR(dims3_b);
        T4A_REQUIRE_PTR(t_b);
        h->impl->set_site_tensors(site, dims3_a, t_a, dims3_b, t_b);
    });
}

t4a_gpu_status t4a_gpu_projected_operator_time_step(t4a_gpu_projected_operator* h, size_t site, size_t nb, size_t reps, double* ms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(ms);
        h->impl->time_step(site, nb, reps, ms);
    });
}

t4a_gpu_status t4a_gpu_projected_operator_apply_env(const double* L, const double* R, const size_t* dims, const t4a_gpu_mpo* op, size_t site,
                                                    const double* v, double* out, double* hl, double* hr)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(dims);
        if (dims[0] == 0 || dims[1] == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_env: an environment has a zero dimension");
        T4A_REQUIRE_PTR(L);
        T4A_REQUIRE_PTR(R);
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(v);
        T4A_REQUIRE_PTR(out);
        std::vector<double> vhl, vhr;
        const std::vector<double> y = projected_apply_env(L, R, dims[0], dims[1], *op->impl, site, v, hl ? &vhl : nullptr, hr ? &vhr : nullptr);
        std::memcpy(out, y.data(), y.size() * sizeof(double));
        if (hl) std::memcpy(hl, vhl.data(), vhl.size() * sizeof(double));
        if (hr) std::memcpy(hr, vhr.data(), vhr.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_linsolve_orth(const double* basis, size_t len, size_t nb, double* w_inout, double* h_out, double* norm_out)
{
    return guarded([&] {
        require_basis_dims("linsolve_orth", len, nb, LINSOLVE_RESTART_DIM_MAX + 1, "the basis holds more than INT_MAX elements");
        T4A_REQUIRE_PTR(basis);
        T4A_REQUIRE_PTR(w_inout);
        T4A_REQUIRE_PTR(h_out);
        T4A_REQUIRE_PTR(norm_out);
        require_device();
        linsolve_orth(basis, len, nb, w_inout, h_out, norm_out);
    });
}

t4a_gpu_status t4a_gpu_krylov_orth(const double* basis, size_t len, size_t nb, double* w_inout, int32_t route, double* h_out, double* norm_out)
{
    return guarded([&] {
        require_basis_dims("krylov_orth", len, nb, LINSOLVE_RESTART_DIM_MAX + 1, "the basis holds more than INT_MAX elements");
        if (route < 0 || route > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "krylov_orth: route must be 0 (serial), 1 (wide) or 2 (the rule of krylov_dots_route)");
        T4A_REQUIRE_PTR(basis);
        T4A_REQUIRE_PTR(w_inout);
        T4A_REQUIRE_PTR(h_out);
        T4A_REQUIRE_PTR(norm_out);
        require_device();
        krylov_orth_host(basis, len, nb, w_inout, (KrylovDotsRoute)route, h_out, norm_out);
    });
}

t4a_gpu_status t4a_gpu_krylov_dots_route(size_t len, size_t nb, int32_t* route)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(route);
        if (nb > LINSOLVE_RESTART_DIM_MAX + 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "krylov_dots_route: nb above " + std::to_string(LINSOLVE_RESTART_DIM_MAX + 1));
        *route = (int32_t)krylov_dots_route(len, (int)nb);
    });
}

t4a_gpu_status t4a_gpu_krylov_time_dots(size_t len, size_t nb, size_t reps, double* ms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms);
        krylov_time_dots(len, nb, reps, ms); // checks its arguments, then the device
    });
}

t4a_gpu_status t4a_gpu_linsolve_gmres_dense(const double* H, size_t n, const double* b, const double* x0, double a0, double a1, double tol,
                                            int32_t mode, size_t restart_dim, size_t max_restarts, double* x, size_t* iterations,
                                            double* residual, int32_t* converged)
{
    return guarded([&] {
        if (mode != 0 && mode != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown gmres_tolerance_mode");
        LinsolveOptions o;
        o.gmres_tol = tol;
        o.gmres_restart_dim = restart_dim;
        o.gmres_max_restarts = max_restarts;
        o.validate();
        require_dense_hook_dims("gmres_dense", n, restart_dim + 1);
        T4A_REQUIRE_PTR(H);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(x0);
        T4A_REQUIRE_PTR(x);
        T4A_REQUIRE_PTR(iterations);
        T4A_REQUIRE_PTR(residual);
        T4A_REQUIRE_PTR(converged);
        require_device();
        const GmresResult r = gmres_dense(H, n, b, x0, a0, a1, tol, (GmresToleranceMode)mode, restart_dim, max_restarts, x);
        *iterations = r.iterations;
        *residual = r.residual;
        *converged = r.converged;
    });
}

// ---- two-site DMRG: the lowest eigenpair of an MPO by sweeps with a local Lanczos (dmrg.hpp) ----
t4a_gpu_status t4a_gpu_dmrg_options_default(t4a_gpu_dmrg_options* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const DmrgOptions d;
        *out = t4a_gpu_dmrg_options{};
        out->nsite = d.nsite;
        out->nsweeps = d.nsweeps;
        out->has_max_bond_dim = d.has_max_bond_dim;
        out->max_bond_dim = d.max_bond_dim;
        out->has_svd_policy = d.has_svd_policy;
        out->svd_policy = to_c(d.svd_policy);
        out->lanczos = t4a_gpu_lanczos_options{d.lanczos.max_iter, d.lanczos.rtol, d.lanczos.atol, d.lanczos.breakdown_tol, d.lanczos.hermitian_tol};
        out->has_energy_tol = d.has_energy_tol;
        out->energy_tol = d.energy_tol;
        out->real_scalar_tol = d.real_scalar_tol;
    });
}

t4a_gpu_status t4a_gpu_dmrg_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* state_dims3, size_t n_state, size_t center,
                                         size_t max_iter)
{
    return guarded([&] {
        if (n_op) T4A_REQUIRE_PTR(op_dims4);
        if (n_state) T4A_REQUIRE_PTR(state_dims3);
        LanczosOptions lo;
        lo.max_iter = max_iter;
        lo.validate();
        dmrg_validate_shapes(dims4_list(op_dims4, n_op), dims3_list(state_dims3, n_state), center, max_iter);
    });
}

t4a_gpu_status t4a_gpu_dmrg(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_dmrg_options* options,
                            t4a_gpu_tt** state, double* energy, size_t* sweeps_completed, size_t* local_updates, int32_t* converged,
                            double* max_residual_norm, t4a_gpu_dmrg_stats* stats)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(state);
        *state = nullptr;
        T4A_REQUIRE_PTR(options);
        const DmrgOptions o = convert_dmrg_options(options); // the options are checked on the host before an operand is looked at
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(init);
        T4A_REQUIRE_PTR(energy);
        T4A_REQUIRE_PTR(sweeps_completed);
        T4A_REQUIRE_PTR(local_updates);
        T4A_REQUIRE_PTR(converged);
        T4A_REQUIRE_PTR(max_residual_norm);
        DmrgResult r = dmrg(*op->impl, const_cast<t4a_gpu_tt*>(init)->impl, center, o);
        *state = new t4a_gpu_tt(r.state->cores, r.state->eng.stream());
        *energy = r.energy;
        *sweeps_completed = r.sweeps_completed;
        *local_updates = r.local_updates;
        *converged = r.converged;
        *max_residual_norm = r.max_residual_norm;
        if (stats) *stats = t4a_gpu_dmrg_stats{r.stats.local_solves, r.stats.lanczos_steps, r.stats.apply_calls};
    });
}

t4a_gpu_status t4a_gpu_dmrg_energy(const t4a_gpu_mpo* op, const t4a_gpu_tt* state, size_t center, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(state);
        T4A_REQUIRE_PTR(out);
        *out = dmrg_energy(*op->impl, const_cast<t4a_gpu_tt*>(state)->impl, center);
    });
}

t4a_gpu_status t4a_gpu_lanczos_dense(const double* H, size_t n, const double* v0, const t4a_gpu_lanczos_options* options, double* eigenvalue,
                                     double* eigenvector, size_t* iterations, double* residual_norm, int32_t* converged)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(options);
        const LanczosOptions o = convert_lanczos_options(*options);
        o.validate();
        require_dense_hook_dims("lanczos_dense", n, o.max_iter + 1);
        T4A_REQUIRE_PTR(H);
        T4A_REQUIRE_PTR(v0);
        T4A_REQUIRE_PTR(eigenvalue);
        T4A_REQUIRE_PTR(eigenvector);
        T4A_REQUIRE_PTR(iterations);
        T4A_REQUIRE_PTR(residual_norm);
        T4A_REQUIRE_PTR(converged);
        require_device();
        const LanczosResult r = lanczos_dense(H, n, v0, o, eigenvector);
        *eigenvalue = r.eigenvalue;
        *iterations = r.iterations;
        *residual_norm = r.residual_norm;
        *converged = r.converged;
    });
}

t4a_gpu_status t4a_gpu_krylov_combine(const double* basis, size_t len, size_t nb, const double* coef, double* out, double* norm2)
{
    return guarded([&] {
        require_basis_dims("krylov_combine", len, nb, LINSOLVE_RESTART_DIM_MAX,
                           "nb above " + std::to_string(LINSOLVE_RESTART_DIM_MAX) + " or a basis of more than INT_MAX elements");
        T4A_REQUIRE_PTR(basis);
        T4A_REQUIRE_PTR(coef);
        T4A_REQUIRE_PTR(out);
        T4A_REQUIRE_PTR(norm2);
        require_device();
        krylov_combine_host(basis, len, nb, coef, out, norm2);
    });
}

t4a_gpu_status t4a_gpu_eig_residual(const double* v, const double* hv, size_t len, double lambda, double* r, double* sums3)
{
    return guarded([&] {
        if (len == 0 || len > (size_t)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, "eig_residual: len must be positive and at most INT_MAX");
        T4A_REQUIRE_PTR(v);
        T4A_REQUIRE_PTR(hv);
        T4A_REQUIRE_PTR(sums3);
        require_device();
        eig_residual_host(v, hv, len, lambda, r, sums3);
    });
}

t4a_gpu_status t4a_gpu_lanczos_time_finalise(size_t len, size_t nb, size_t reps, double* ms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms);
        lanczos_time_finalise(len, nb, reps, ms); // checks its arguments, then the device
    });
}

// ---- two-site TDVP: a train evolved under an MPO by sweeps of projected Krylov exponentials (tdvp.hpp) ----
t4a_gpu_status t4a_gpu_tdvp_options_default(t4a_gpu_tdvp_options* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const TdvpOptions d;
        *out = t4a_gpu_tdvp_options{};
        out->nsite = d.nsite;
        out->nsweeps = d.nsweeps;
        out->order = d.order;
        out->exponent_step_re = d.exponent_step_re;
        out->exponent_step_im = d.exponent_step_im;
        out->has_max_bond_dim = d.has_max_bond_dim;
        out->max_bond_dim = d.max_bond_dim;
        out->has_svd_policy = d.has_svd_policy;
        out->svd_policy = to_c(d.svd_policy);
        out->krylov = t4a_gpu_krylov_expm_options{d.krylov.max_iter, d.krylov.max_time_splits, d.krylov.tol, d.krylov.breakdown_tol, d.krylov.hermitian_tol};
    });
}

t4a_gpu_status t4a_gpu_tdvp_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* state_dims3, size_t n_state, size_t center,
                                         size_t max_iter)
{
    return guarded([&] { check_tdvp_shapes(TdvpMode::TwoSite, op_dims4, n_op, state_dims3, n_state, center, max_iter); });
}

t4a_gpu_status t4a_gpu_tdvp_plan(size_t n, size_t center, size_t order, double tau, size_t capacity, int32_t* kinds, size_t* nodes, size_t* new_centers,
                                 double* exponents, size_t* n_steps)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(n_steps);
        write_tdvp_plan("tdvp_plan", tdvp_plan(n, center, order, tau), capacity, kinds, nodes, new_centers, exponents, n_steps);
    });
}

t4a_gpu_status t4a_gpu_tdvp(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_tdvp_options* options, t4a_gpu_tt** state,
                            size_t* sweeps_completed, size_t* local_updates, double* max_error_estimate, size_t* max_krylov_iterations,
                            t4a_gpu_tdvp_stats* stats)
{
    return guarded([&] {
        const TdvpStats s = run_tdvp(TdvpMode::TwoSite, op, init, center, options, state, sweeps_completed, local_updates, max_error_estimate, max_krylov_iterations);
        if (stats) *stats = t4a_gpu_tdvp_stats{s.two_site_steps, s.corrections, s.krylov_steps, s.apply_calls, s.max_time_splits};
    });
}


// ---- one-site TDVP: fixed ranks, a bond-centre correction between two site steps (tdvp.hpp) ----
t4a_gpu_status t4a_gpu_tdvp_one_site_options_default(t4a_gpu_tdvp_options* out)
{
    const t4a_gpu_status st = t4a_gpu_tdvp_options_default(out);
    if (st == T4A_GPU_SUCCESS) out->nsite = 1;
    return st;
}

t4a_gpu_status t4a_gpu_tdvp_one_site_check_shapes(const size_t* op_dims4, size_t n_op, const size_t* state_dims3, size_t n_state, size_t center,
                                                  size_t max_iter)
{
    return guarded([&] { check_tdvp_shapes(TdvpMode::OneSite, op_dims4, n_op, state_dims3, n_state, center, max_iter); });
}

t4a_gpu_status t4a_gpu_tdvp_one_site_plan(size_t n, size_t center, size_t order, double tau, size_t capacity, int32_t* kinds, size_t* nodes,
                                          size_t* new_centers, double* exponents, size_t* n_steps)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(n_steps);
        write_tdvp_plan("tdvp_one_site_plan", tdvp_one_site_plan(n, center, order, tau), capacity, kinds, nodes, new_centers, exponents, n_steps);
    });
}

t4a_gpu_status t4a_gpu_tdvp_one_site(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_tdvp_options* options, t4a_gpu_tt** state,
                                     size_t* sweeps_completed, size_t* local_updates, double* max_error_estimate, size_t* max_krylov_iterations,
                                     t4a_gpu_tdvp_one_site_stats* stats)
{
    return guarded([&] {
        const TdvpStats s = run_tdvp(TdvpMode::OneSite, op, init, center, options, state, sweeps_completed, local_updates, max_error_estimate, max_krylov_iterations);
        if (stats)
            *stats = t4a_gpu_tdvp_one_site_stats{s.one_site_steps, s.bond_corrections, s.qr_steps, s.krylov_steps, s.apply_calls, s.max_time_splits, s.fused_applies,
                                                 s.gemm_applies};
    });
}


t4a_gpu_status t4a_gpu_tdvp_bond_apply_route(size_t ka, size_t kb, size_t W, int32_t* route)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(route);
        if (ka == 0 || kb == 0 || W == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_bond_apply_route: ka, kb and W must be positive");
        *route = (int32_t)tdvp_bond_apply_route(ka, kb, W);
    });
}

t4a_gpu_status t4a_gpu_tdvp_bond_apply_fused_admits(size_t ka, size_t kb, size_t W, int32_t* admits)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(admits);
        *admits = tdvp_bond_apply_fused_admits(ka, kb, W) ? 1 : 0;
    });
}

t4a_gpu_status t4a_gpu_tdvp_set_bond_apply_route(int32_t route)
{
    return guarded([&] { tdvp_set_bond_apply_route(route); });
}

t4a_gpu_status t4a_gpu_tdvp_bond_apply(const double* L, const double* R, const double* C, size_t ka, size_t kb, size_t W, int32_t route, double* out,
                                       int32_t* route_taken)
{
    return guarded([&] {
        if (route < 0 || route > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_bond_apply: route is 0 (fused), 1 (GEMM) or 2 (the rule)");
        if (ka == 0 || kb == 0 || W == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_bond_apply: ka, kb and W must be positive");
        check_bond_center_dims("tdvp_bond_apply", 0, ka, kb, W, 0);
        if (route == 0 && !tdvp_bond_apply_fused_admits(ka, kb, W))
            throw Error(T4A_GPU_INVALID_ARGUMENT, "tdvp_bond_apply: the fused launch holds 16 W k_b doubles in the LDS: W k_b must be at most " +
                                                      std::to_string(TDVP_BOND_FUSED_MAX_PANEL));
        T4A_REQUIRE_PTR(L);
        T4A_REQUIRE_PTR(R);
        T4A_REQUIRE_PTR(C);
        T4A_REQUIRE_PTR(out);
        require_device();
        const BondApplyRoute taken = tdvp_bond_apply_host(L, R, C, ka, kb, W, (BondApplyRoute)route, out);
        if (route_taken) *route_taken = (int32_t)taken;
    });
}

t4a_gpu_status t4a_gpu_tdvp_bond_apply_time(size_t ka, size_t kb, size_t W, size_t reps, double* ms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms);
        tdvp_bond_apply_time(ka, kb, W, reps, ms); // checks its arguments, then the device
    });
}

t4a_gpu_status t4a_gpu_krylov_expm_dense(const double* H, size_t n, const double* v0, double tau, const t4a_gpu_krylov_expm_options* options, double* out,
                                         size_t* iterations, double* error_estimate, int32_t* converged, size_t* time_splits)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(options);
        const KrylovExpmOptions o = convert_krylov_expm_options(*options);
        o.validate();
        if (!std::isfinite(tau)) throw Error(T4A_GPU_INVALID_ARGUMENT, "krylov_expm_dense: tau must be finite");
        require_dense_hook_dims("krylov_expm_dense", n, o.max_iter + 1);
        T4A_REQUIRE_PTR(H);
        T4A_REQUIRE_PTR(v0);
        T4A_REQUIRE_PTR(out);
        T4A_REQUIRE_PTR(iterations);
        T4A_REQUIRE_PTR(error_estimate);
        T4A_REQUIRE_PTR(converged);
        T4A_REQUIRE_PTR(time_splits);
        require_device();
        const KrylovExpmResult r = krylov_expm_dense(H, n, v0, tau, o, out);
        *iterations = r.iterations;
        *error_estimate = r.error_estimate;
        *converged = r.converged;
        *time_splits = r.time_splits;
    });
}

// ---- global subspace expansion and GSE-TDVP (gse.hpp) ----
t4a_gpu_status t4a_gpu_gse_options_default(t4a_gpu_gse_options* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const GseOptions d;
        *out = t4a_gpu_gse_options{};
        out->krylov_dim = d.krylov_dim;
        out->has_reference_max_bond_dim = d.has_reference_max_bond_dim;
        out->reference_max_bond_dim = d.reference_max_bond_dim;
        out->has_reference_svd_policy = d.has_reference_svd_policy;
        out->reference_svd_policy = to_c(d.reference_svd_policy);
        out->density_weight_cutoff = d.density_weight_cutoff;
        out->hermitian_tol = d.hermitian_tol;
        out->normalize_references = d.normalize_references;
        out->expand_before_first_sweep = d.expand_before_first_sweep;
    });
}

t4a_gpu_status t4a_gpu_gse_check_shapes(const t4a_gpu_gse_options* options, const size_t* state_dims3, size_t n_state, const size_t* ref_dims3,
                                        const size_t* ref_lens, size_t n_refs, size_t center)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(options);
        (void)convert_gse_options(options);
        if (n_state) T4A_REQUIRE_PTR(state_dims3);
        if (n_refs) T4A_REQUIRE_PTR(ref_lens);
        std::vector<std::vector<std::array<size_t, 3>>> refs;
        size_t off = 0;
        for (size_t j = 0; j < n_refs; ++j) {
            if (ref_lens[j]) T4A_REQUIRE_PTR(ref_dims3);
            refs.push_back(dims3_list(ref_dims3 + 3 * off, ref_lens[j]));
            off += ref_lens[j];
        }
        gse_validate_shapes(dims3_list(state_dims3, n_state), refs, center);
    });
}

t4a_gpu_status t4a_gpu_gse_krylov_references(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, const t4a_gpu_gse_options* options, size_t capacity,
                                             t4a_gpu_tt** refs, size_t* n_refs)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(n_refs);
        *n_refs = 0;
        T4A_REQUIRE_PTR(options);
        const GseOptions o = convert_gse_options(options);
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(init);
        if (capacity < o.krylov_dim) throw Error(T4A_GPU_BUFFER_TOO_SMALL, "gse_krylov_references: krylov_dim references are returned");
        if (o.krylov_dim) T4A_REQUIRE_PTR(refs);
        std::vector<std::unique_ptr<TensorTrain>> r = gse_krylov_references(*op->impl, const_cast<t4a_gpu_tt*>(init)->impl, o);
        std::vector<std::unique_ptr<t4a_gpu_tt>> hs;
        for (auto& t : r) hs.push_back(std::make_unique<t4a_gpu_tt>(t->cores, t->eng.stream()));
        for (size_t k = 0; k < hs.size(); ++k) refs[k] = hs[k].release();
        *n_refs = r.size();
    });
}

t4a_gpu_status t4a_gpu_gse_expand_with_references(const t4a_gpu_tt* init, const t4a_gpu_tt* const* references, size_t n_refs, size_t center,
                                                  const t4a_gpu_gse_options* options, t4a_gpu_tt** state, size_t* references_built,
                                                  size_t* edges_processed, size_t* bonds_expanded, size_t* max_added_basis)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(state);
        *state = nullptr;
        T4A_REQUIRE_PTR(options);
        const GseOptions o = convert_gse_options(options);
        T4A_REQUIRE_PTR(init);
        T4A_REQUIRE_PTR(references_built);
        T4A_REQUIRE_PTR(edges_processed);
        T4A_REQUIRE_PTR(bonds_expanded);
        T4A_REQUIRE_PTR(max_added_basis);
        if (n_refs) T4A_REQUIRE_PTR(references);
        std::vector<TensorTrain*> refs;
        for (size_t j = 0; j < n_refs; ++j) {
            T4A_REQUIRE_PTR(references[j]);
            refs.push_back(&const_cast<t4a_gpu_tt*>(references[j])->impl);
        }
        GseResult r = global_subspace_expand_with_references(const_cast<t4a_gpu_tt*>(init)->impl, refs, center, o);
        *state = new t4a_gpu_tt(r.state->cores, r.state->eng.stream());
        gse_counters(r, references_built, edges_processed, bonds_expanded, max_added_basis);
    });
}

t4a_gpu_status t4a_gpu_gse_expand(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_gse_options* options, t4a_gpu_tt** state,
                                  size_t* references_built, size_t* edges_processed, size_t* bonds_expanded, size_t* max_added_basis)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(state);
        *state = nullptr;
        T4A_REQUIRE_PTR(options);
        const GseOptions o = convert_gse_options(options);
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(init);
        T4A_REQUIRE_PTR(references_built);
        T4A_REQUIRE_PTR(edges_processed);
        T4A_REQUIRE_PTR(bonds_expanded);
        T4A_REQUIRE_PTR(max_added_basis);
        GseResult r = global_subspace_expand(*op->impl, const_cast<t4a_gpu_tt*>(init)->impl, center, o);
        *state = new t4a_gpu_tt(r.state->cores, r.state->eng.stream());
        gse_counters(r, references_built, edges_processed, bonds_expanded, max_added_basis);
    });
}

t4a_gpu_status t4a_gpu_gse_tdvp(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_gse_options* gse,
                                const t4a_gpu_tdvp_options* tdvp_options, t4a_gpu_tt** state, size_t* sweeps_completed, size_t* local_updates,
                                size_t* gse_expansions, double* max_error_estimate, size_t* max_krylov_iterations)
{
    return guarded([&] {
        run_gse_tdvp(TdvpMode::TwoSite, op, init, center, gse, tdvp_options, state, sweeps_completed, local_updates, gse_expansions, max_error_estimate,
                     max_krylov_iterations);
    });
}

t4a_gpu_status t4a_gpu_gse_tdvp_one_site(const t4a_gpu_mpo* op, const t4a_gpu_tt* init, size_t center, const t4a_gpu_gse_options* gse,
                                         const t4a_gpu_tdvp_options* tdvp_options, t4a_gpu_tt** state, size_t* sweeps_completed, size_t* local_updates,
                                         size_t* gse_expansions, double* max_error_estimate, size_t* max_krylov_iterations)
{
    return guarded([&] {
        run_gse_tdvp(TdvpMode::OneSite, op, init, center, gse, tdvp_options, state, sweeps_completed, local_updates, gse_expansions, max_error_estimate,
                     max_krylov_iterations);
    });
}


t4a_gpu_status t4a_gpu_gse_project(int32_t orient, size_t q, const double* refs, const size_t* rho, size_t K, const double* B, size_t kb, int32_t route,
                                   double* stack, double* trace)
{
    return guarded([&] {
        if ((orient != 0 && orient != 1) || (route != 0 && route != 1)) throw Error(T4A_GPU_INVALID_ARGUMENT, "gse_project: orient and route are 0 or 1");
        const std::vector<int> rh = gse_int_list(rho, K, GSE_MAX_REFERENCES, "gse_project");
        size_t P = 0;
        for (int v : rh) P += (size_t)v;
        gse_require_fits(P, q, "gse_project");
        gse_require_fits(kb, q, "gse_project");
        gse_require_fits(P, kb, "gse_project");
        T4A_REQUIRE_PTR(refs);
        T4A_REQUIRE_PTR(B);
        T4A_REQUIRE_PTR(stack);
        T4A_REQUIRE_PTR(trace);
        require_device();
        gse_project_host(orient, (int)q, refs, rh.data(), (int)K, B, (int)kb, route, stack, trace);
    });
}

t4a_gpu_status t4a_gpu_gse_absorb(int32_t orient, size_t q, const double* children, const size_t* r, const double* parents, const size_t* L, size_t n_trains,
                                  const double* Bn, size_t kn, int32_t route, double* out)
{
    return guarded([&] {
        if ((orient != 0 && orient != 1) || (route != 0 && route != 1)) throw Error(T4A_GPU_INVALID_ARGUMENT, "gse_absorb: orient and route are 0 or 1");
        const std::vector<int> rs = gse_int_list(r, n_trains, GSE_MAX_JOBS, "gse_absorb");
        const std::vector<int> Ls = gse_int_list(L, n_trains, GSE_MAX_JOBS, "gse_absorb");
        size_t sumL = 0, sumR = 0;
        for (size_t j = 0; j < n_trains; ++j) {
            sumL += (size_t)Ls[j];
            sumR += (size_t)rs[j];
            gse_require_fits((size_t)Ls[j], (size_t)rs[j], "gse_absorb");
        }
        gse_require_fits(kn, q, "gse_absorb");
        gse_require_fits(sumL, q, "gse_absorb");
        gse_require_fits(sumL, kn, "gse_absorb");
        gse_require_fits(sumR, q, "gse_absorb");
        gse_require_fits(sumR, kn, "gse_absorb");
        T4A_REQUIRE_PTR(children);
        T4A_REQUIRE_PTR(parents);
        T4A_REQUIRE_PTR(Bn);
        T4A_REQUIRE_PTR(out);
        require_device();
        gse_absorb_host(orient, (int)q, children, rs.data(), parents, Ls.data(), (int)n_trains, Bn, (int)kn, route, out);
    });
}

t4a_gpu_status t4a_gpu_gse_route(size_t q, size_t bond, int32_t* route)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(route);
        gse_require_fits(q, bond, "gse_route");
        *route = gse_use_fused((int)q, (int)bond) ? 0 : 1;
    });
}

t4a_gpu_status t4a_gpu_gse_set_route(int32_t route)
{
    return guarded([&] {
        if (route < -1 || route > 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "gse_set_route: -1 (the rule), 0 (fused) or 1 (GEMM)");
        gse_set_route(route);
    });
}

t4a_gpu_status t4a_gpu_gse_time_routes(size_t chi, size_t d, size_t K, size_t reps, double* ms4)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms4);
        if (chi == 0 || d == 0 || K == 0 || K > (size_t)GSE_MAX_REFERENCES || reps == 0 || chi > 4096 || d > 64)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "gse_time_routes: chi in 1..4096, d in 1..64, K in 1..8 and reps must be positive");
        require_device();
        gse_time_routes(chi, d, K, reps, ms4);
    });
}

// ---- partitioned MPOs (pmpo.hpp): projector.rs, contraction_tasks and the handle ----
t4a_gpu_status t4a_gpu_projector_validate(const size_t* site_dims, size_t n_sites, const size_t* p, size_t count)
{
    return guarded([&] { projector_validate(projector_from_triples(p, count), site_dims_list(site_dims, n_sites)); });
}

t4a_gpu_status t4a_gpu_projector_is_compatible(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = projector_compatible(projector_from_triples(a, count_a), projector_from_triples(b, count_b)) ? 1 : 0;
    });
}

t4a_gpu_status t4a_gpu_projector_intersection(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* compatible,
                                              size_t* out, size_t* out_count)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(compatible);
        T4A_REQUIRE_PTR(out_count);
        LegProjector r;
        *compatible = projector_intersection(projector_from_triples(a, count_a), projector_from_triples(b, count_b), r) ? 1 : 0;
        *out_count = 0;
        if (*compatible) projector_out(r, out, out_count);
    });
}

t4a_gpu_status t4a_gpu_projector_common_restriction(const size_t* a, size_t count_a, const size_t* b, size_t count_b, size_t* out,
                                                    size_t* out_count)
{
    return guarded(
        [&] { projector_out(projector_common_restriction(projector_from_triples(a, count_a), projector_from_triples(b, count_b)), out, out_count); });
}

t4a_gpu_status t4a_gpu_projector_is_subset_of(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = projector_is_subset_of(projector_from_triples(a, count_a), projector_from_triples(b, count_b)) ? 1 : 0;
    });
}

t4a_gpu_status t4a_gpu_projector_are_disjoint(const size_t* entries, const size_t* counts, size_t n_projectors, int32_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = projectors_disjoint(projector_list(entries, counts, n_projectors)) ? 1 : 0;
    });
}

t4a_gpu_status t4a_gpu_projector_filter(const size_t* p, size_t count, const size_t* keys, size_t n_keys, size_t* out, size_t* out_count)
{
    return guarded([&] {
        if (n_keys) T4A_REQUIRE_PTR(keys);
        std::vector<std::pair<size_t, size_t>> k(n_keys);
        for (size_t i = 0; i < n_keys; ++i) k[i] = {keys[2 * i], keys[2 * i + 1]};
        projector_out(projector_filter(projector_from_triples(p, count), k), out, out_count);
    });
}

t4a_gpu_status t4a_gpu_projector_compare(const size_t* a, size_t count_a, const size_t* b, size_t count_b, int32_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = projector_compare(projector_from_triples(a, count_a), projector_from_triples(b, count_b));
    });
}

t4a_gpu_status t4a_gpu_pmpo_contract_plan(const size_t* a_entries, const size_t* a_counts, size_t n_a, const size_t* b_entries,
                                          const size_t* b_counts, size_t n_b, size_t task_capacity, size_t entry_capacity, size_t* n_tasks,
                                          size_t* task_a, size_t* task_b, size_t* task_result, size_t* n_results, size_t* result_counts,
                                          size_t* result_entries, size_t* n_result_entries)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(n_tasks);
        T4A_REQUIRE_PTR(n_results);
        T4A_REQUIRE_PTR(n_result_entries);
        const PmpoPlan plan = pmpo_contract_plan(projector_list(a_entries, a_counts, n_a), projector_list(b_entries, b_counts, n_b));
        size_t ne = 0;
        for (const auto& r : plan.results) ne += r.size();
        *n_tasks = plan.tasks.size();
        *n_results = plan.results.size();
        *n_result_entries = ne;
        if (task_capacity == 0 && entry_capacity == 0) return; // the query
        if (task_capacity < plan.tasks.size() || entry_capacity < ne)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "pmpo_contract_plan: " + std::to_string(plan.tasks.size()) + " tasks and " + std::to_string(ne) +
                                                      " result entries do not fit the capacities " + std::to_string(task_capacity) + " and " +
                                                      std::to_string(entry_capacity));
        if (!plan.tasks.empty()) {
            T4A_REQUIRE_PTR(task_a);
            T4A_REQUIRE_PTR(task_b);
            T4A_REQUIRE_PTR(task_result);
            T4A_REQUIRE_PTR(result_counts);
        }
        if (ne) T4A_REQUIRE_PTR(result_entries);
        for (size_t t = 0; t < plan.tasks.size(); ++t) {
            task_a[t] = plan.tasks[t].a;
            task_b[t] = plan.tasks[t].b;
            task_result[t] = plan.tasks[t].result;
        }
        size_t off = 0;
        for (size_t r = 0; r < plan.results.size(); ++r) {
            size_t c = 0;
            projector_out(plan.results[r], result_entries ? result_entries + 3 * off : nullptr, &c);
            result_counts[r] = c;
            off += c;
        }
    });
}

t4a_gpu_status t4a_gpu_pmpo_check(const size_t* site_dims, size_t n_sites, const size_t* patch_site_dims, const size_t* patch_lens,
                                  size_t n_patches, const size_t* entries, const size_t* counts)
{
    return guarded([&] {
        if (n_patches) T4A_REQUIRE_PTR(patch_lens);
        std::vector<SiteDims> pd(n_patches);
        size_t off = 0;
        for (size_t k = 0; k < n_patches; ++k) {
            pd[k] = site_dims_list(patch_site_dims ? patch_site_dims + 2 * off : nullptr, patch_lens[k]);
            off += patch_lens[k];
        }
        PartitionedMpo::validate(site_dims_list(site_dims, n_sites), pd, projector_list(entries, counts, n_patches));
    });
}

t4a_gpu_status t4a_gpu_pmpo_new(const t4a_gpu_mpo* const* patches, size_t n_patches, const size_t* entries, const size_t* counts,
                                const size_t* site_dims, size_t n_sites, t4a_gpu_pmpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_patches) T4A_REQUIRE_PTR(patches);
        const std::vector<Mpo*> ms = handle_list(patches, n_patches, "patches[k] is null", [](const t4a_gpu_mpo& m) { return m.impl.get(); });
        SiteDims sd;
        if (site_dims) sd = site_dims_list(site_dims, n_sites);
        *out = new t4a_gpu_pmpo{PartitionedMpo::from_patches(ms, projector_list(entries, counts, n_patches), site_dims ? &sd : nullptr)};
    });
}

t4a_gpu_status t4a_gpu_pmpo_from_ptt(const t4a_gpu_ptt* ptt, const size_t* site_dims, t4a_gpu_pmpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ptt);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_pmpo{PartitionedMpo::from_ptt(*ptt->impl, site_dims)};
    });
}

void t4a_gpu_pmpo_release(t4a_gpu_pmpo* h) { delete h; }

t4a_gpu_status t4a_gpu_pmpo_len(const t4a_gpu_pmpo* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->len();
    });
}

t4a_gpu_status t4a_gpu_pmpo_n_sites(const t4a_gpu_pmpo* h, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->sd.size();
    });
}

t4a_gpu_status t4a_gpu_pmpo_site_dims(const t4a_gpu_pmpo* h, size_t* site_dims)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (!h->impl->sd.empty()) T4A_REQUIRE_PTR(site_dims);
        for (size_t i = 0; i < h->impl->sd.size(); ++i) {
            site_dims[2 * i] = h->impl->sd[i][0];
            site_dims[2 * i + 1] = h->impl->sd[i][1];
        }
    });
}

t4a_gpu_status t4a_gpu_pmpo_projector(const t4a_gpu_pmpo* h, size_t k, size_t* count, size_t* entries)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (k >= h->impl->len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "patch index out of range");
        projector_out(h->impl->patches[k].proj, entries, count);
    });
}

t4a_gpu_status t4a_gpu_pmpo_patch(const t4a_gpu_pmpo* h, size_t k, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (k >= h->impl->len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "patch index out of range");
        Mpo& m = *h->impl->patches[k].mpo;
        *out = new t4a_gpu_mpo{std::make_unique<Mpo>(m.tt.cores, m.tt.eng.stream(), m.sd)};
    });
}

t4a_gpu_status t4a_gpu_pmpo_norm(t4a_gpu_pmpo* h, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = h->impl->norm();
    });
}

t4a_gpu_status t4a_gpu_pmpo_evaluate(t4a_gpu_pmpo* h, const size_t* idx, size_t n_pts, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        if (n_pts == 0) return;
        T4A_REQUIRE_PTR(idx);
        T4A_REQUIRE_PTR(out);
        std::vector<uint32_t> u = narrow_indices(idx, checked_mul(n_pts, 2 * h->impl->sd.size(), "index buffer"));
        std::vector<double> v = h->impl->evaluate(u.data(), n_pts);
        std::memcpy(out, v.data(), n_pts * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_pmpo_project(const t4a_gpu_pmpo* h, const size_t* p, size_t count, t4a_gpu_pmpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_pmpo{h->impl->project(projector_from_triples(p, count))};
    });
}

t4a_gpu_status t4a_gpu_pmpo_add(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, double tolerance, size_t max_bond_dim, t4a_gpu_pmpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_pmpo{a->impl->add(*b->impl, pmpo_options(tolerance, max_bond_dim, 0))};
    });
}

t4a_gpu_status t4a_gpu_pmpo_to_mpo(const t4a_gpu_pmpo* h, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_mpo{h->impl->to_mpo()};
    });
}

t4a_gpu_status t4a_gpu_pmpo_to_mpo_route(const t4a_gpu_pmpo* h, int32_t route, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_mpo{h->impl->to_mpo(route)};
    });
}

t4a_gpu_status t4a_gpu_pmpo_contract(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, int32_t algorithm, int32_t compress, int32_t method,
                                     double tolerance, size_t max_bond_dim, t4a_gpu_pmpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (algorithm < 0 || algorithm > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown contraction algorithm");
        const MpoContractionOptions o = pmpo_options(tolerance, max_bond_dim, method);
        *out = new t4a_gpu_pmpo{a->impl->contract(*b->impl, (MpoAlgorithm)algorithm, compress != 0, o)};
    });
}

t4a_gpu_status t4a_gpu_pmpo_pair_products(const size_t* dims, const int64_t* sel, size_t n_jobs, const double* A, const double* B, double* C)
{
    return guarded([&] {
        static_assert(sizeof(long long) == sizeof(int64_t), "selectors are 64-bit");
        pmpo_pair_products(dims, reinterpret_cast<const long long*>(sel), n_jobs, A, B, C);
    });
}

t4a_gpu_status t4a_gpu_pmpo_mask_sites(const size_t* dims, const int64_t* sel, size_t n_jobs, double* X)
{
    return guarded([&] { pmpo_mask_sites(dims, reinterpret_cast<const long long*>(sel), n_jobs, X); });
}

t4a_gpu_status t4a_gpu_pmpo_launch_blocks(size_t total, size_t* blocks)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(blocks);
        *blocks = pmpo_launch_blocks(total);
    });
}

t4a_gpu_status t4a_gpu_pmpo_time_contract(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, double tolerance, size_t max_bond_dim, size_t reps,
                                          double* ms3)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(ms3);
        pmpo_time_contract(*a->impl, *b->impl, pmpo_options(tolerance, max_bond_dim, 0), reps, ms3);
    });
}

// ---- the compress stage as an operation of its own, and for many MPOs in lock step (batch_compress.hpp) ----
t4a_gpu_status t4a_gpu_mpo_compress(const t4a_gpu_mpo* mpo, double tolerance, size_t max_bond_dim, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(mpo);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        *out = new t4a_gpu_mpo{mpo_compress(*mpo->impl, pmpo_options(tolerance, max_bond_dim, 0))};
    });
}

t4a_gpu_status t4a_gpu_mpo_compress_many_counted(const t4a_gpu_mpo* const* mpos, size_t count, double tolerance, size_t max_bond_dim,
                                                 int32_t route, t4a_gpu_mpo** out, size_t* counts4)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        for (size_t k = 0; k < count; ++k) out[k] = nullptr;
        const CompressRoute r = compress_route(route);
        const std::vector<Mpo*> items = mpo_list(mpos, count, "compress_many");
        CompressManyStats st;
        std::vector<std::unique_ptr<Mpo>> res = mpo_compress_many(items, pmpo_options(tolerance, max_bond_dim, 0), r, &st);
        std::vector<t4a_gpu_mpo*> handles;
        for (auto& m : res) handles.push_back(new t4a_gpu_mpo{std::move(m)});
        for (size_t k = 0; k < count; ++k) out[k] = handles[k];
        if (counts4) {
            counts4[0] = st.launches;
            counts4[1] = st.syncs;
            counts4[2] = st.n_batched;
            counts4[3] = st.n_serial;
        }
    });
}

t4a_gpu_status t4a_gpu_mpo_compress_many(const t4a_gpu_mpo* const* mpos, size_t count, double tolerance, size_t max_bond_dim, int32_t route,
                                         t4a_gpu_mpo** out)
{
    return t4a_gpu_mpo_compress_many_counted(mpos, count, tolerance, max_bond_dim, route, out, nullptr);
}

t4a_gpu_status t4a_gpu_mpo_compress_many_plan(const size_t* dims4, const size_t* n_sites, size_t count, double tolerance, size_t max_bond_dim,
                                              int32_t route, int32_t* batched, size_t* bonds, size_t* qr_bonds, size_t* counts3)
{
    return guarded([&] {
        const CompressRoute r = compress_route(route);
        if (count == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many: the list is empty");
        T4A_REQUIRE_PTR(n_sites);
        std::vector<std::vector<std::array<size_t, 4>>> shapes(count);
        size_t at = 0;
        for (size_t k = 0; k < count; ++k) {
            if (n_sites[k]) T4A_REQUIRE_PTR(dims4);
            for (size_t i = 0; i < n_sites[k]; ++i, ++at) shapes[k].push_back({dims4[4 * at], dims4[4 * at + 1], dims4[4 * at + 2], dims4[4 * at + 3]});
        }
        const CompressManyPlan p = compress_many_plan(shapes, pmpo_options(tolerance, max_bond_dim, 0), r);
        size_t ob = 0;
        for (size_t k = 0; k < count; ++k) {
            if (batched) batched[k] = p.batched[k];
            for (size_t i = 0; i < p.bonds[k].size(); ++i, ++ob) {
                if (bonds) bonds[ob] = p.bonds[k][i];
                if (qr_bonds) qr_bonds[ob] = p.qr_bonds[k][i];
            }
        }
        if (counts3) {
            counts3[0] = p.launches;
            counts3[1] = p.syncs;
            counts3[2] = p.n_batched;
        }
    });
}

t4a_gpu_status t4a_gpu_mpo_time_compress_many(const t4a_gpu_mpo* const* mpos, size_t count, double tolerance, size_t max_bond_dim, size_t reps,
                                              double* ms2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms2);
        const std::vector<Mpo*> items = mpo_list(mpos, count, "time_compress_many");
        for (Mpo* m : items)
            if (m->len() != items[0]->len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "time_compress_many: the items differ in length");
        Engine& eng = items[0]->tt.eng;
        std::vector<std::vector<DevCore>> chains;
        for (Mpo* m : items) {
            m->tt.eng.sync();
            chains.push_back(clone_cores(m->tt.cores, eng.stream()));
        }
        eng.sync();
        compress_many_time(eng, chains, pmpo_options(tolerance, max_bond_dim, 0), reps, ms2);
    });
}

t4a_gpu_status t4a_gpu_pmpo_contract_routed(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, int32_t algorithm, int32_t compress, int32_t method,
                                            double tolerance, size_t max_bond_dim, int32_t route, t4a_gpu_pmpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (algorithm < 0 || algorithm > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown contraction algorithm");
        const CompressRoute r = compress_route(route);
        const MpoContractionOptions o = pmpo_options(tolerance, max_bond_dim, method);
        *out = new t4a_gpu_pmpo{a->impl->contract(*b->impl, (MpoAlgorithm)algorithm, compress != 0, o, r)};
    });
}

t4a_gpu_status t4a_gpu_pmpo_time_compress(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, double tolerance, size_t max_bond_dim, size_t reps,
                                          double* ms2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(ms2);
        pmpo_time_compress(*a->impl, *b->impl, pmpo_options(tolerance, max_bond_dim, 0), reps, ms2);
    });
}

// ---- budgeted truncation of many MPOs (batch_truncate.hpp) and adaptive patching (pmpo_patching.hpp) ----
t4a_gpu_status t4a_gpu_mpo_truncate_many_counted(const t4a_gpu_mpo* const* mpos, size_t count, const t4a_gpu_svd_policy* policies,
                                                 const size_t* max_bond_dims, int32_t route, int32_t ranks_only, t4a_gpu_mpo** out,
                                                 size_t* bonds, size_t* counts4)
{
    return guarded([&] {
        if (!ranks_only) T4A_REQUIRE_PTR(out);
        if (out)
            for (size_t k = 0; k < count; ++k) out[k] = nullptr;
        const CompressRoute r = compress_route(route);
        const std::vector<Mpo*> items = mpo_list(mpos, count, "truncate_many");
        const std::vector<BtRule> rules = truncate_rules(policies, max_bond_dims, count);
        TruncateManyStats st;
        std::vector<std::vector<size_t>> b;
        std::vector<std::unique_ptr<Mpo>> res = mpo_truncate_many(items, rules, r, ranks_only != 0, b, &st, nullptr);
        truncate_out(res, b, st, ranks_only != 0, out, bonds, counts4);
    });
}

t4a_gpu_status t4a_gpu_mpo_truncate_many(const t4a_gpu_mpo* const* mpos, size_t count, const t4a_gpu_svd_policy* policies,
                                         const size_t* max_bond_dims, int32_t route, int32_t ranks_only, t4a_gpu_mpo** out, size_t* bonds)
{
    return t4a_gpu_mpo_truncate_many_counted(mpos, count, policies, max_bond_dims, route, ranks_only, out, bonds, nullptr);
}

t4a_gpu_status t4a_gpu_mpo_truncate_many_trace(const t4a_gpu_mpo* const* mpos, size_t count, const t4a_gpu_svd_policy* policies,
                                               const size_t* max_bond_dims, int32_t route, size_t* bonds, size_t* counts4, double* norm2,
                                               int32_t* ranks, double* sv)
{
    return guarded([&] {
        const CompressRoute r = compress_route(route);
        const std::vector<Mpo*> items = mpo_list(mpos, count, "truncate_many");
        const std::vector<BtRule> rules = truncate_rules(policies, max_bond_dims, count);
        TruncateManyStats st;
        TruncateManyTrace tr;
        std::vector<std::vector<size_t>> b;
        std::vector<std::unique_ptr<Mpo>> res = mpo_truncate_many(items, rules, r, true, b, &st, &tr);
        truncate_out(res, b, st, true, nullptr, bonds, counts4);
        const size_t steps2 = items[0]->len() ? 2 * (items[0]->len() - 1) : 0;
        for (size_t k = 0; k < count; ++k) {
            if (norm2) norm2[k] = tr.norm2[k];
            for (size_t t = 0; t < steps2 && t < tr.ranks[k].size(); ++t) {
                if (ranks) ranks[k * steps2 + t] = tr.ranks[k][t];
                if (sv) std::memcpy(sv + (k * steps2 + t) * 64, tr.sv[k].data() + t * 64, 64 * sizeof(double));
            }
        }
    });
}

t4a_gpu_status t4a_gpu_mpo_truncate_many_plan(const size_t* dims4, const size_t* n_sites, size_t count, const size_t* max_bond_dims,
                                              int32_t route, int32_t rules_from_norms, int32_t* batched, size_t* bonds, size_t* qr_bonds,
                                              size_t* counts3)
{
    return guarded([&] {
        const CompressRoute r = compress_route(route);
        if (count == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: the list is empty");
        T4A_REQUIRE_PTR(n_sites);
        std::vector<std::vector<std::array<size_t, 4>>> shapes(count);
        std::vector<size_t> caps(count, 0);
        size_t at = 0;
        for (size_t k = 0; k < count; ++k) {
            if (n_sites[k]) T4A_REQUIRE_PTR(dims4);
            if (max_bond_dims) caps[k] = max_bond_dims[k];
            for (size_t i = 0; i < n_sites[k]; ++i, ++at) shapes[k].push_back({dims4[4 * at], dims4[4 * at + 1], dims4[4 * at + 2], dims4[4 * at + 3]});
        }
        const TruncateManyPlan p = truncate_many_plan(shapes, caps, r, rules_from_norms != 0);
        size_t ob = 0;
        for (size_t k = 0; k < count; ++k) {
            if (batched) batched[k] = p.batched[k];
            for (size_t i = 0; i < p.bonds[k].size(); ++i, ++ob) {
                if (bonds) bonds[ob] = p.bonds[k][i];
                if (qr_bonds) qr_bonds[ob] = p.qr_bonds[k][i];
            }
        }
        if (counts3) {
            counts3[0] = p.launches;
            counts3[1] = p.syncs;
            counts3[2] = p.n_batched;
        }
    });
}

t4a_gpu_status t4a_gpu_pmpo_validate_patching_options(const t4a_gpu_patching_options* options, const size_t* site_dims, size_t n_sites)
{
    return guarded([&] { validate_patching_options(patching_options(options), site_dims_list(site_dims, n_sites)); });
}

t4a_gpu_status t4a_gpu_pmpo_patch_volume(const size_t* entries, size_t count, const size_t* site_dims, size_t n_sites, size_t* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const SiteDims sd = site_dims_list(site_dims, n_sites);
        const LegProjector p = projector_from_triples(entries, count);
        projector_validate(p, sd);
        *out = patch_volume(p, sd);
    });
}

t4a_gpu_status t4a_gpu_pmpo_patch_budgets(const size_t* volumes, const double* norm2, size_t count, double rtol, double* budgets,
                                          int32_t* drop, int32_t* empty)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(empty);
        if (count) {
            T4A_REQUIRE_PTR(volumes);
            T4A_REQUIRE_PTR(norm2);
        }
        validate_truncation_options(rtol, false, 0);
        const PatchBudgets b = patch_budgets(std::vector<size_t>(volumes, volumes + count), std::vector<double>(norm2, norm2 + count), rtol);
        *empty = b.empty ? 1 : 0;
        if (b.empty) return;
        for (size_t k = 0; k < count; ++k) {
            if (budgets) budgets[k] = b.budget[k];
            if (drop) drop[k] = b.drop[k];
        }
    });
}

t4a_gpu_status t4a_gpu_pmpo_split_candidates(const size_t* entries, size_t count, const size_t* site_dims, size_t n_sites,
                                             const t4a_gpu_patching_options* options, size_t* legs, size_t* n_legs)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(n_legs);
        const SiteDims sd = site_dims_list(site_dims, n_sites);
        const PatchingOptions o = patching_options(options);
        validate_patching_options(o, sd);
        const LegProjector p = projector_from_triples(entries, count);
        projector_validate(p, sd);
        const std::vector<PatchLeg> c = split_candidates(p, sd, o);
        *n_legs = c.size();
        if (!legs) return;
        for (size_t k = 0; k < c.size(); ++k) legs[2 * k] = c[k].first, legs[2 * k + 1] = c[k].second;
    });
}

t4a_gpu_status t4a_gpu_pmpo_truncate_adaptive(const t4a_gpu_pmpo* p, double rtol, int32_t has_max_bond_dim, size_t max_bond_dim,
                                              int32_t route, t4a_gpu_pmpo** out, size_t* counts6)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(p);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        const CompressRoute r = compress_route(route);
        validate_truncation_options(rtol, has_max_bond_dim != 0, max_bond_dim);
        PatchingStats st;
        *out = new t4a_gpu_pmpo{truncate_adaptive(*p->impl, rtol, has_max_bond_dim != 0, max_bond_dim, r, &st)};
        patching_counts(st, counts6);
    });
}

t4a_gpu_status t4a_gpu_pmpo_truncate_adaptive_timed(const t4a_gpu_pmpo* p, double rtol, int32_t has_max_bond_dim, size_t max_bond_dim,
                                                    double* ms5)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(p);
        T4A_REQUIRE_PTR(ms5);
        for (int k = 0; k < 5; ++k) ms5[k] = 0.0;
        validate_truncation_options(rtol, has_max_bond_dim != 0, max_bond_dim);
        truncate_adaptive(*p->impl, rtol, has_max_bond_dim != 0, max_bond_dim, CompressRoute::Batched, nullptr, ms5);
    });
}

t4a_gpu_status t4a_gpu_pmpo_add_with_patching(const t4a_gpu_pmpo* subdomains, const t4a_gpu_patching_options* options, int32_t route,
                                              t4a_gpu_pmpo** out, size_t* counts6, size_t* chosen, size_t chosen_capacity,
                                              size_t* n_chosen)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(subdomains);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        const CompressRoute r = compress_route(route);
        const PatchingOptions o = patching_options(options);
        validate_patching_options(o, subdomains->impl->sd);
        PatchingStats st;
        std::vector<PatchLeg> legs;
        std::unique_ptr<PartitionedMpo> res = add_with_patching(*subdomains->impl, o, r, &st, &legs);
        patching_counts(st, counts6);
        if (n_chosen) *n_chosen = legs.size();
        if (chosen)
            for (size_t k = 0; k < legs.size() && k < chosen_capacity; ++k) chosen[2 * k] = legs[k].first, chosen[2 * k + 1] = legs[k].second;
        *out = new t4a_gpu_pmpo{std::move(res)};
    });
}

t4a_gpu_status t4a_gpu_pmpo_contract_adaptive(const t4a_gpu_pmpo* a, const t4a_gpu_pmpo* b, int32_t algorithm, int32_t method, double tolerance,
                                              size_t max_bond_dim, const t4a_gpu_patching_options* options, int32_t route, t4a_gpu_pmpo** out,
                                              size_t* counts6)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (algorithm < 0 || algorithm > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown contraction algorithm");
        const CompressRoute r = compress_route(route);
        const MpoContractionOptions o = pmpo_options(tolerance, max_bond_dim, method);
        const PatchingOptions po = patching_options(options);
        PatchingStats st;
        *out = new t4a_gpu_pmpo{contract_adaptive(*a->impl, *b->impl, (MpoAlgorithm)algorithm, o, po, r, &st)};
        patching_counts(st, counts6);
    });
}

t4a_gpu_status t4a_gpu_pmpo_budget_squared(const t4a_gpu_pmpo* p, size_t k, int32_t* has, double* value)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(p);
        T4A_REQUIRE_PTR(has);
        T4A_REQUIRE_PTR(value);
        if (k >= p->impl->len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "patch index out of range");
        *has = p->impl->patches[k].has_budget ? 1 : 0;
        *value = p->impl->patches[k].budget_squared;
    });
}

// ---- swap_site_indices on a chain (swap.hpp) ----
t4a_gpu_status t4a_gpu_swap_schedule_build(size_t n_sites, const int64_t* cur_keys, const size_t* cur_sites, const size_t* cur_dims,
                                           size_t n_current, const int64_t* target_keys, const size_t* target_sites, size_t n_target,
                                           size_t root, size_t max_passes, const size_t* link_dims, size_t max_bond_dim,
                                           t4a_gpu_swap_schedule** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        const SwapAssignment current = assignment(cur_keys, cur_sites, n_current);
        SwapSchedule sched = swap_schedule_build(n_sites, current, assignment(target_keys, target_sites, n_target), root, max_passes);
        if (cur_dims) {
            SiteLegs legs(n_sites);
            for (size_t k = 0; k < n_current; ++k) legs[current[k].second].push_back({current[k].first, cur_dims[k]});
            std::vector<size_t> links;
            if (link_dims && n_sites) links.assign(link_dims, link_dims + (n_sites - 1));
            swap_plan_check(sched, legs, link_dims ? &links : nullptr, max_bond_dim);
        }
        *out = new t4a_gpu_swap_schedule{std::move(sched)};
    });
}

void t4a_gpu_swap_schedule_release(t4a_gpu_swap_schedule* h) { delete h; }

t4a_gpu_status t4a_gpu_swap_schedule_len(const t4a_gpu_swap_schedule* h, size_t* n_steps)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(n_steps);
        *n_steps = h->impl.steps.size();
    });
}

t4a_gpu_status t4a_gpu_swap_schedule_step_sizes(const t4a_gpu_swap_schedule* h, size_t step, size_t* sizes)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(sizes);
        if (step >= h->impl.steps.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "swap schedule: step out of range");
        const ScheduledSwapStep& s = h->impl.steps[step];
        sizes[0] = s.transport_path.size(), sizes[1] = s.a_side.size(), sizes[2] = s.b_side.size();
    });
}

t4a_gpu_status t4a_gpu_swap_schedule_step(const t4a_gpu_swap_schedule* h, size_t step, size_t* transport_path, size_t* node_ab,
                                          int64_t* a_side, int64_t* b_side)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(h);
        T4A_REQUIRE_PTR(node_ab);
        if (step >= h->impl.steps.size()) throw Error(T4A_GPU_INVALID_ARGUMENT, "swap schedule: step out of range");
        const ScheduledSwapStep& s = h->impl.steps[step];
        if (!s.transport_path.empty()) T4A_REQUIRE_PTR(transport_path);
        if (!s.a_side.empty()) T4A_REQUIRE_PTR(a_side);
        if (!s.b_side.empty()) T4A_REQUIRE_PTR(b_side);
        std::copy(s.transport_path.begin(), s.transport_path.end(), transport_path);
        std::copy(s.a_side.begin(), s.a_side.end(), a_side);
        std::copy(s.b_side.begin(), s.b_side.end(), b_side);
        node_ab[0] = s.node_a, node_ab[1] = s.node_b;
    });
}

t4a_gpu_status t4a_gpu_tt_swap_site_indices(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                            const int64_t* target_keys, const size_t* target_sites, size_t n_target,
                                            int32_t has_max_bond_dim, size_t max_bond_dim, int32_t has_rtol, double rtol, t4a_gpu_tt** out,
                                            size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, int32_t* moved, size_t* center,
                                            size_t* n_steps, double* ms3)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(tt);
        SwapOptions o;
        o.has_max_bond_dim = has_max_bond_dim != 0, o.max_bond_dim = max_bond_dim;
        o.has_rtol = has_rtol != 0, o.rtol = rtol;
        o.validate();
        SiteLegs legs = site_legs(tt->impl.len(), leg_counts, keys, dims);
        const SwapAssignment target = assignment(target_keys, target_sites, n_target);
        // the work happens on a copy with an engine of its own; the input stays as it is
        std::unique_ptr<t4a_gpu_tt> res(new t4a_gpu_tt(tt->impl.cores, tt->impl.eng.stream()));
        SwapTimings tm;
        const SwapResult r = swap_site_indices(res->impl.eng, res->impl.cores, legs, target, o, ms3 ? &tm : nullptr);
        res->impl.eng.sync();
        write_legs(legs, out_leg_counts, out_keys, out_dims);
        if (moved) *moved = r.moved ? 1 : 0;
        if (center) *center = r.center;
        if (n_steps) *n_steps = r.n_steps;
        if (ms3) ms3[0] = tm.kernel_ms, ms3[1] = tm.svd_ms, ms3[2] = tm.qr_ms;
        *out = res.release();
    });
}

t4a_gpu_status t4a_gpu_swap_theta(const double* left, size_t l, size_t m, const double* right, size_t r, const int64_t* left_keys,
                                  const size_t* left_dims, size_t n_left, const int64_t* right_keys, const size_t* right_dims,
                                  size_t n_right, const int64_t* to_left, size_t n_to_left, const int64_t* to_right, size_t n_to_right,
                                  double* out, size_t* mn, int32_t* route)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(left);
        T4A_REQUIRE_PTR(right);
        T4A_REQUIRE_PTR(out);
        if (n_to_left) T4A_REQUIRE_PTR(to_left);
        if (n_to_right) T4A_REQUIRE_PTR(to_right);
        const std::vector<int64_t> tl(to_left, to_left + n_to_left), tr(to_right, to_right + n_to_right);
        size_t M = 0, N = 0;
        int rt = 0;
        require_device();
        const std::vector<double> v = swap_theta(left, l, m, right, r, leg_list(left_keys, left_dims, n_left),
                                                 leg_list(right_keys, right_dims, n_right), tl, tr, M, N, rt);
        std::memcpy(out, v.data(), v.size() * sizeof(double));
        if (mn) mn[0] = M, mn[1] = N;
        if (route) *route = rt;
    });
}

t4a_gpu_status t4a_gpu_swap_theta_time(size_t bond, size_t reps, double* ms2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms2);
        require_device();
        swap_theta_time(bond, (int)std::min<size_t>(reps, 1u << 20), &ms2[0], &ms2[1]);
    });
}

t4a_gpu_status t4a_gpu_legtrain_reorder(t4a_gpu_tt* tt, const size_t* leg_counts, int64_t* keys, size_t* dims, const size_t* sites,
                                        const size_t* order_counts, const int64_t* order_keys, size_t n_named)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(tt);
        SiteLegs legs = site_legs(tt->impl.len(), leg_counts, keys, dims);
        std::vector<std::pair<size_t, std::vector<int64_t>>> orders;
        if (n_named) {
            T4A_REQUIRE_PTR(sites);
            T4A_REQUIRE_PTR(order_counts);
        }
        size_t at = 0;
        for (size_t k = 0; k < n_named; ++k) {
            if (order_counts[k]) T4A_REQUIRE_PTR(order_keys);
            orders.push_back({sites[k], std::vector<int64_t>(order_keys + at, order_keys + at + order_counts[k])});
            at += order_counts[k];
        }
        legtrain_reorder(tt->impl.eng, tt->impl.cores, legs, orders);
        write_legs(legs, nullptr, keys, dims);
    });
}


// ---- fuse_to, split_to, restructure_to on a chain (restructure.hpp) ----
t4a_gpu_status t4a_gpu_restructure_plan(int32_t op, size_t n_sites, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                        const size_t* link_dims, size_t n_groups, const size_t* group_counts, const int64_t* group_keys,
                                        int32_t* kind, size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, size_t* counts4,
                                        int64_t* swap_keys, size_t* swap_sites)
{
    return guarded([&] {
        if (op < 0 || op > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "restructure_plan: op is 0 (restructure_to), 1 (fuse_to) or 2 (split_to)");
        const SiteLegs legs = site_legs(n_sites, leg_counts, keys, dims);
        const RestructureTarget target = restructure_target(n_groups, group_counts, group_keys);
        std::vector<size_t> links;
        if (link_dims && n_sites) links.assign(link_dims, link_dims + (n_sites - 1));
        RestructurePlan p;
        if (op == 1) {
            const FusePlan fp = fuse_plan(legs, target, link_dims ? &links : nullptr);
            p.kind = RestructureKind::FuseOnly;
            p.legs = fp.legs, p.fuse_rounds = fp.rounds, p.fuse_launches = fp.launches;
        } else if (op == 2) {
            const SplitPlan sp = split_plan(legs, target);
            p.kind = RestructureKind::SplitOnly;
            p.legs = sp.legs, p.n_qr = sp.n_qr, p.fuse_launches = sp.launches;
        } else {
            p = restructure_plan(legs, target, link_dims ? &links : nullptr);
        }
        if (kind) *kind = (int32_t)p.kind;
        write_legs(p.legs, out_leg_counts, out_keys, out_dims);
        if (counts4) counts4[0] = p.fuse_rounds, counts4[1] = p.fuse_launches, counts4[2] = p.n_qr, counts4[3] = p.swap_target.size();
        for (size_t k = 0; k < p.swap_target.size(); ++k) {
            if (swap_keys) swap_keys[k] = p.swap_target[k].first;
            if (swap_sites) swap_sites[k] = p.swap_target[k].second;
        }
    });
}

t4a_gpu_status t4a_gpu_tt_fuse_to(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims, int64_t center,
                                  size_t n_groups, const size_t* group_counts, const int64_t* group_keys, t4a_gpu_tt** out,
                                  size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, int64_t* out_center)
{
    return tt_fuse_to(tt, leg_counts, keys, dims, center, n_groups, group_counts, group_keys, out, out_leg_counts, out_keys, out_dims, out_center,
                      nullptr);
}

t4a_gpu_status t4a_gpu_tt_fuse_to_counted(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                          int64_t center, size_t n_groups, const size_t* group_counts, const int64_t* group_keys,
                                          t4a_gpu_tt** out, size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims,
                                          int64_t* out_center, size_t* launches)
{
    return tt_fuse_to(tt, leg_counts, keys, dims, center, n_groups, group_counts, group_keys, out, out_leg_counts, out_keys, out_dims, out_center,
                      launches);
}

t4a_gpu_status t4a_gpu_tt_split_to(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims, size_t n_groups,
                                   const size_t* group_counts, const int64_t* group_keys, int32_t form, const t4a_gpu_svd_policy* policy,
                                   int32_t has_max_bond_dim, size_t max_bond_dim, int32_t final_sweep, t4a_gpu_tt** out,
                                   size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, size_t* n_qr)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(tt);
        const SplitOptions o = split_options(form, policy, has_max_bond_dim, max_bond_dim, final_sweep);
        o.validate();
        SiteLegs legs = site_legs(tt->impl.len(), leg_counts, keys, dims);
        const RestructureTarget target = restructure_target(n_groups, group_counts, group_keys);
        split_plan(legs, target); // the refusals, before the device is touched
        std::unique_ptr<t4a_gpu_tt> res(new t4a_gpu_tt(tt->impl.cores, tt->impl.eng.stream()));
        const RestructureResult r = split_to(res->impl.eng, res->impl.cores, legs, target, o);
        res->impl.eng.sync();
        write_legs(legs, out_leg_counts, out_keys, out_dims);
        if (n_qr) *n_qr = r.n_qr;
        *out = res.release();
    });
}

t4a_gpu_status t4a_gpu_tt_restructure_to(const t4a_gpu_tt* tt, const size_t* leg_counts, const int64_t* keys, const size_t* dims,
                                         int64_t center, size_t n_groups, const size_t* group_counts, const int64_t* group_keys,
                                         int32_t split_form, const t4a_gpu_svd_policy* split_policy, int32_t split_has_max_bond_dim,
                                         size_t split_max_bond_dim, int32_t split_final_sweep, int32_t swap_has_max_bond_dim,
                                         size_t swap_max_bond_dim, int32_t swap_has_rtol, double swap_rtol,
                                         const t4a_gpu_svd_policy* final_policy, size_t final_max_bond_dim, t4a_gpu_tt** out,
                                         size_t* out_leg_counts, int64_t* out_keys, size_t* out_dims, int32_t* kind, int64_t* out_center,
                                         size_t* counts3)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        T4A_REQUIRE_PTR(tt);
        RestructureOptions o;
        o.split = split_options(split_form, split_policy, split_has_max_bond_dim, split_max_bond_dim, split_final_sweep);
        o.swap.has_max_bond_dim = swap_has_max_bond_dim != 0, o.swap.max_bond_dim = swap_max_bond_dim;
        o.swap.has_rtol = swap_has_rtol != 0, o.swap.rtol = swap_rtol;
        o.has_final_truncation = final_policy != nullptr;
        if (final_policy) o.final_policy = SvdPolicy{final_policy->threshold, final_policy->scale, final_policy->measure, final_policy->rule};
        o.final_max_bond_dim = final_max_bond_dim;
        o.validate();
        SiteLegs legs = site_legs(tt->impl.len(), leg_counts, keys, dims);
        const RestructureTarget target = restructure_target(n_groups, group_counts, group_keys);
        const size_t c = center_in(center, tt->impl.len());
        std::vector<size_t> links;
        for (size_t i = 0; i + 1 < tt->impl.len(); ++i) links.push_back(tt->impl.cores[i].r);
        restructure_plan(legs, target, &links); // the refusals, before the device is touched
        std::unique_ptr<t4a_gpu_tt> res(new t4a_gpu_tt(tt->impl.cores, tt->impl.eng.stream()));
        RestructureKind k = RestructureKind::FuseOnly;
        const RestructureResult r = restructure_to(res->impl.eng, res->impl.cores, legs, target, o, c, &k);
        res->impl.eng.sync();
        write_legs(legs, out_leg_counts, out_keys, out_dims);
        if (kind) *kind = (int32_t)k;
        if (out_center) *out_center = r.center == NO_CENTER ? -1 : (int64_t)r.center;
        if (counts3) counts3[0] = r.launches, counts3[1] = r.n_qr, counts3[2] = r.n_swap_steps;
        *out = res.release();
    });
}

t4a_gpu_status t4a_gpu_fuse_round(size_t n_jobs, const double* a, const double* b, const size_t* shapes5, const size_t* leg_counts,
                                  const size_t* leg_dims, const size_t* leg_order, double* out, int32_t* routes)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(shapes5);
        T4A_REQUIRE_PTR(leg_counts);
        T4A_REQUIRE_PTR(out);
        std::vector<FuseRoundHostJob> jobs(n_jobs);
        size_t at_a = 0, at_b = 0, at_leg = 0;
        for (size_t k = 0; k < n_jobs; ++k) {
            FuseRoundHostJob& j = jobs[k];
            j.l = shapes5[5 * k], j.X = shapes5[5 * k + 1], j.m = shapes5[5 * k + 2], j.Y = shapes5[5 * k + 3], j.r = shapes5[5 * k + 4];
            j.A = a + at_a, j.B = b + at_b;
            at_a += j.l * j.X * j.m, at_b += j.m * j.Y * j.r;
            if (leg_counts[k]) {
                T4A_REQUIRE_PTR(leg_dims);
                T4A_REQUIRE_PTR(leg_order);
                j.leg_dims.assign(leg_dims + at_leg, leg_dims + at_leg + leg_counts[k]);
                j.order.assign(leg_order + at_leg, leg_order + at_leg + leg_counts[k]);
                at_leg += leg_counts[k];
            }
        }
        require_device();
        std::vector<int> rt;
        const std::vector<std::vector<double>> res = fuse_round(jobs, rt);
        size_t at = 0;
        for (size_t k = 0; k < n_jobs; ++k) {
            std::memcpy(out + at, res[k].data(), res[k].size() * sizeof(double));
            at += res[k].size();
            if (routes) routes[k] = rt[k];
        }
    });
}

t4a_gpu_status t4a_gpu_fuse_time(size_t n_groups, size_t bond, size_t reps, double* ms2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms2);
        require_device();
        fuse_time(n_groups, bond, (int)std::min<size_t>(reps, 1u << 20), &ms2[0], &ms2[1]);
    });
}

// ---- fit_sum: the variational sum of many trains or MPOs (fit_sum.hpp) ----
t4a_gpu_status t4a_gpu_fit_sum_options_default(t4a_gpu_fit_sum_options* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const FitSumOptions d;
        *out = t4a_gpu_fit_sum_options{};
        out->nfullsweeps = d.nfullsweeps;
        out->has_max_bond_dim = d.has_max_bond_dim;
        out->max_bond_dim = d.max_bond_dim;
        out->has_svd_policy = d.has_svd_policy;
        out->svd_policy = to_c(d.svd_policy);
        out->has_qr_rtol = d.has_qr_rtol;
        out->qr_rtol = d.qr_rtol;
        out->factorize_alg = d.factorize_alg;
        out->has_convergence_tol = d.has_convergence_tol;
        out->convergence_tol = d.convergence_tol;
    });
}

t4a_gpu_status t4a_gpu_fit_sum_check_shapes(const size_t* target_dims3, const size_t* target_lens, size_t n_targets, int32_t has_initial,
                                            const size_t* initial_dims3, size_t n_initial, size_t center, const t4a_gpu_fit_sum_options* options)
{
    return guarded([&] {
        if (options) convert_fit_sum_options(options);
        if (n_targets) T4A_REQUIRE_PTR(target_lens);
        std::vector<std::vector<std::array<size_t, 3>>> targets;
        size_t off = 0;
        for (size_t k = 0; k < n_targets; ++k) {
            if (target_lens[k]) T4A_REQUIRE_PTR(target_dims3);
            targets.push_back(dims3_list(target_dims3 + 3 * off, target_lens[k]));
            off += target_lens[k];
        }
        if (has_initial && n_initial) T4A_REQUIRE_PTR(initial_dims3);
        const auto init = dims3_list(initial_dims3, has_initial ? n_initial : 0);
        fit_sum_validate_shapes(targets, has_initial ? &init : nullptr, center);
    });
}

t4a_gpu_status t4a_gpu_tt_fit_sum(const t4a_gpu_tt* const* targets, size_t n_targets, const double* coefficients, const t4a_gpu_tt* initial,
                                  size_t center, const t4a_gpu_fit_sum_options* options, int32_t route, t4a_gpu_tt** out, size_t* sweeps_completed,
                                  size_t* local_updates, int32_t* converged, double* norms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        fit_sum_entry(
            targets, n_targets, coefficients, initial, center, options, route, sweeps_completed, local_updates, converged, norms,
            [](const t4a_gpu_tt* h) { return &h->impl.cores; }, [](const t4a_gpu_tt* h) { return &const_cast<t4a_gpu_tt*>(h)->impl.eng; },
            [] {}, [&](FitSumResult& r) { *out = new t4a_gpu_tt(r.cores, nullptr); });
    });
}

t4a_gpu_status t4a_gpu_mpo_fit_sum(const t4a_gpu_mpo* const* targets, size_t n_targets, const double* coefficients, const t4a_gpu_mpo* initial,
                                   size_t center, const t4a_gpu_fit_sum_options* options, int32_t route, t4a_gpu_mpo** out, size_t* sweeps_completed,
                                   size_t* local_updates, int32_t* converged, double* norms)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        fit_sum_entry(
            targets, n_targets, coefficients, initial, center, options, route, sweeps_completed, local_updates, converged, norms,
            [](const t4a_gpu_mpo* h) { return &h->impl->tt.cores; }, [](const t4a_gpu_mpo* h) { return &h->impl->tt.eng; },
            [&] {
                // the fused site index is checked by fit_sum; the (s1, s2) pairs behind an equal fused index have to agree as well
                const std::vector<std::array<size_t, 2>>& sd = (initial ? initial : targets[0])->impl->sd;
                for (size_t k = 0; k < n_targets; ++k) {
                    const std::vector<std::array<size_t, 2>>& td = targets[k]->impl->sd;
                    if (td.size() != sd.size()) continue;
                    for (size_t i = 0; i < sd.size(); ++i)
                        if (td[i][0] * td[i][1] == sd[i][0] * sd[i][1] && td[i] != sd[i])
                            throw Error(T4A_GPU_INVALID_ARGUMENT, "fit_sum: target " + std::to_string(k) + " site-space validation failed");
                }
            },
            [&](FitSumResult& r) {
                const std::vector<std::array<size_t, 2>>& sd = (initial ? initial : targets[0])->impl->sd;
                *out = new t4a_gpu_mpo{std::make_unique<Mpo>(std::move(r.cores), sd)};
            });
    });
}

t4a_gpu_status t4a_gpu_fit_sum_half(int32_t right, int32_t route, const double* env, size_t chi, size_t S, const double* cores, const size_t* a,
                                    const size_t* b, size_t K, int32_t has_fill, double fill, double* out)
{
    return guarded([&] {
        const FitSumRoute rt = convert_fit_sum_route(route, false);
        T4A_REQUIRE_PTR(env);
        T4A_REQUIRE_PTR(cores);
        T4A_REQUIRE_PTR(a);
        T4A_REQUIRE_PTR(b);
        T4A_REQUIRE_PTR(out);
        const std::vector<double> r = fit_sum_half(right != 0, rt, env, chi, S, cores, a, b, K, has_fill ? &fill : nullptr);
        std::memcpy(out, r.data(), r.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_fit_sum_route(size_t n_targets, size_t target_bond, size_t result_bond, size_t site_dim, int32_t* route)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(route);
        if (n_targets == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "fit_sum: targets must not be empty");
        *route = (int32_t)fit_sum_route(n_targets, target_bond, result_bond, site_dim);
    });
}

t4a_gpu_status t4a_gpu_fit_sum_plan(size_t n_sites, size_t center, size_t n_targets, size_t site_dim, int32_t route, size_t* out6)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out6);
        const FitSumPlan p = fit_sum_plan(n_sites, center, n_targets, site_dim, convert_fit_sum_route(route, false));
        out6[0] = p.bond_steps_per_sweep, out6[1] = p.half_launches_per_step, out6[2] = p.gemms_per_step, out6[3] = p.svds_per_step;
        out6[4] = p.prepare_half_launches, out6[5] = p.prepare_gemms;
    });
}

t4a_gpu_status t4a_gpu_fit_sum_time_half(int32_t right, size_t K, size_t bond, size_t S, size_t chi, size_t reps, double* ms2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms2);
        fit_sum_time_half(right != 0, K, bond, S, chi, std::min<size_t>(reps, 1u << 20), ms2);
    });
}

// ---- an operator applied on a subset of a state's sites (linop.hpp) ----
t4a_gpu_status t4a_gpu_linop_options_default(t4a_gpu_linop_options* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        const ApplyOptions d;
        out->method = (int32_t)d.method;
        out->tolerance = d.tolerance;
        out->has_max_bond_dim = d.max_bond_dim != 0;
        out->max_bond_dim = d.max_bond_dim;
        out->nfullsweeps = d.max_sweeps;
        out->has_convergence_tol = d.has_convergence_tol;
        out->convergence_tol = d.convergence_tol;
    });
}

t4a_gpu_status t4a_gpu_linop_plan(const size_t* op_dims4, size_t n_op, const size_t* sites, size_t n_sites, const size_t* state_dims3,
                                  size_t n_state, int32_t* kinds, size_t* bonds, size_t* result_dims3)
{
    return guarded([&] {
        if (n_op) T4A_REQUIRE_PTR(op_dims4);
        if (n_sites) T4A_REQUIRE_PTR(sites);
        if (n_state) T4A_REQUIRE_PTR(state_dims3);
        std::vector<std::array<size_t, 4>> od(n_op);
        std::vector<std::array<size_t, 3>> sd(n_state);
        for (size_t i = 0; i < n_op; ++i) od[i] = {op_dims4[4 * i], op_dims4[4 * i + 1], op_dims4[4 * i + 2], op_dims4[4 * i + 3]};
        for (size_t i = 0; i < n_state; ++i) sd[i] = {state_dims3[3 * i], state_dims3[3 * i + 1], state_dims3[3 * i + 2]};
        const std::vector<ApplySitePlan> plan = apply_plan(od, std::vector<size_t>(sites, sites + n_sites), sd);
        for (size_t i = 0; i < plan.size(); ++i) {
            if (kinds) kinds[i] = (int32_t)plan[i].kind;
            if (bonds) bonds[2 * i] = plan[i].m_left, bonds[2 * i + 1] = plan[i].m_right;
            if (result_dims3)
                for (int k = 0; k < 3; ++k) result_dims3[3 * i + k] = plan[i].result[k];
        }
    });
}

t4a_gpu_status t4a_gpu_linop_apply(const t4a_gpu_mpo* op, const size_t* sites, size_t n_sites, const t4a_gpu_tt* state,
                                   const t4a_gpu_linop_options* options, int32_t route, const t4a_gpu_tt* initial, t4a_gpu_tt** out,
                                   size_t* n_sweeps, double* norms, int32_t* route_taken)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sweeps) *n_sweeps = 0;
        T4A_REQUIRE_PTR(options);
        // the options are checked on the host before an operand is looked at
        if (options->method < 0 || options->method > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: unknown method");
        if (route < 0 || route > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: route must be auto, fused or composed");
        if (options->has_max_bond_dim && options->max_bond_dim == 0)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: max_bond_dim must be at least 1");
        ApplyOptions o;
        o.method = (MpoAlgorithm)options->method;
        o.tolerance = options->tolerance;
        o.max_bond_dim = options->has_max_bond_dim ? options->max_bond_dim : 0;
        o.max_sweeps = options->nfullsweeps;
        o.has_convergence_tol = options->has_convergence_tol != 0;
        o.convergence_tol = options->convergence_tol;
        apply_validate_options(o);
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(state);
        if (n_sites) T4A_REQUIRE_PTR(sites);
        TensorTrain& st = const_cast<t4a_gpu_tt*>(state)->impl;
        std::unique_ptr<Mpo> init;
        if (initial && o.method == MpoAlgorithm::Fit) { // the start as an MPO with site dims (d, 1)
            std::vector<std::array<size_t, 2>> sd;
            for (const auto& c : initial->impl.cores) sd.push_back({c.s, 1});
            init = std::make_unique<Mpo>(initial->impl.cores, initial->impl.eng.stream(), sd);
        }
        MpoFitInfo info;
        ApplyRoute taken = ApplyRoute::Composed;
        std::unique_ptr<Mpo> r =
            apply_linear_operator(*op->impl, std::vector<size_t>(sites, sites + n_sites), st, o, (ApplyRoute)route, init.get(), info, &taken);
        *out = new t4a_gpu_tt(r->tt.cores, r->tt.eng.stream());
        if (n_sweeps) *n_sweeps = info.n_sweeps;
        if (norms) std::copy(info.norms.begin(), info.norms.end(), norms);
        if (route_taken) *route_taken = (int32_t)taken;
    });
}

t4a_gpu_status t4a_gpu_linop_extend(const t4a_gpu_mpo* op, const size_t* sites, size_t n_sites, const size_t* state_site_dims, size_t n_state,
                                    t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(op);
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_sites) T4A_REQUIRE_PTR(sites);
        if (n_state) T4A_REQUIRE_PTR(state_site_dims);
        *out = new t4a_gpu_mpo{extend_operator_to_full_space(*op->impl, std::vector<size_t>(sites, sites + n_sites),
                                                              std::vector<size_t>(state_site_dims, state_site_dims + n_state))};
    });
}

t4a_gpu_status t4a_gpu_linop_exclusive(size_t n_state, const size_t* sites, const size_t* lens, size_t n_ops, int32_t* exclusive)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(exclusive);
        if (n_ops) T4A_REQUIRE_PTR(lens);
        if (n_ops) T4A_REQUIRE_PTR(sites);
        *exclusive = are_exclusive_operators(n_state, linop_supports(sites, lens, n_ops)) ? 1 : 0;
    });
}

t4a_gpu_status t4a_gpu_linop_compose(const size_t* state_site_dims, size_t n_state, const t4a_gpu_mpo* const* ops, const size_t* sites,
                                     const size_t* lens, size_t n_ops, t4a_gpu_mpo** out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(out);
        *out = nullptr;
        if (n_state) T4A_REQUIRE_PTR(state_site_dims);
        if (n_ops) T4A_REQUIRE_PTR(ops);
        if (n_ops) T4A_REQUIRE_PTR(lens);
        if (n_ops) T4A_REQUIRE_PTR(sites);
        std::vector<Mpo*> v(n_ops);
        for (size_t q = 0; q < n_ops; ++q) {
            T4A_REQUIRE_PTR(ops[q]);
            v[q] = ops[q]->impl.get();
        }
        *out = new t4a_gpu_mpo{compose_exclusive_linear_operators(std::vector<size_t>(state_site_dims, state_site_dims + n_state), v,
                                                                   linop_supports(sites, lens, n_ops))};
    });
}

t4a_gpu_status t4a_gpu_linop_gap_half(int32_t right, const double* env, size_t n_env, size_t m, const double* x, size_t lb, size_t d,
                                      size_t rb, int32_t has_fill, double fill, double* out)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(env);
        T4A_REQUIRE_PTR(x);
        T4A_REQUIRE_PTR(out);
        const std::vector<double> v = apply_gap_half(right != 0, env, n_env, m, x, lb, d, rb, has_fill ? &fill : nullptr, has_fill ? 64 : 0);
        std::memcpy(out, v.data(), v.size() * sizeof(double));
    });
}

t4a_gpu_status t4a_gpu_linop_route(int32_t method, size_t n_state, size_t n_gap_sites, size_t state_bond, size_t op_bond, int32_t* route)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(route);
        if (method < 0 || method > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: unknown method");
        *route = (int32_t)apply_route((MpoAlgorithm)method, n_state, n_gap_sites, state_bond, op_bond);
    });
}

t4a_gpu_status t4a_gpu_linop_time_half(size_t n_env, size_t m, size_t lb, size_t d, size_t rb, size_t reps, double* ms2)
{
    return guarded([&] {
        T4A_REQUIRE_PTR(ms2);
        linop_time_half(n_env, m, lb, d, rb, std::min<size_t>(reps, 1u << 20), ms2);
    });
}

} // extern "C"
