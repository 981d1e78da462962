// tci2.hip — TensorCI2 driver on the gfx950 engine.
// Mirrors crates/tensor4all-tensorci/src/tensorci2.rs function by function (line references inline).
#include "tci2.hpp"

#include <thread>

#include <exception>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>
#include <unordered_set>

namespace t4a {

extern thread_local double g_chain_wait_seconds; // tci2_chain.hip

// =================================================================================================
// small device kernels: packing of factor matrices into site tensors (column-major [left, site, right])
// =================================================================================================
namespace {

// core[l,s,r] = mat[(l*S+s) + ldm*r] if (l*S+s) < mrows && r < mcols else 0   (tensorci2.rs:1957-1973, :996-1011)
__global__ void __launch_bounds__(256) pack_left_core_kernel(const double* __restrict__ mat, int ldm, int mrows,
                                                             int mcols, double* __restrict__ core, int L, int S, int R)
{
    const size_t total = (size_t)L * S * R;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(e % L);
        const int s = (int)((e / L) % S);
        const int r = (int)(e / ((size_t)L * S));
        const int row = l * S + s;
        core[e] = (row < mrows && r < mcols) ? mat[(size_t)r * ldm + row] : 0.0;
    }
}

// core[l,s,r] = mat[l + ldm*(s*R+r)] if l < mrows && (s*R+r) < mcols else 0   (tensorci2.rs:1983-1999, :1020-1036)
__global__ void __launch_bounds__(256) pack_right_core_kernel(const double* __restrict__ mat, int ldm, int mrows,
                                                              int mcols, double* __restrict__ core, int L, int S, int R)
{
    const size_t total = (size_t)L * S * R;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(e % L);
        const int s = (int)((e / L) % S);
        const int r = (int)(e / ((size_t)L * S));
        const int col = s * R + r;
        core[e] = (l < mrows && col < mcols) ? mat[(size_t)col * ldm + l] : 0.0;
    }
}

inline unsigned blocks_for(size_t total)
{
    size_t b = (total + 255) / 256;
    if (b > 4096) b = 4096;
    if (b == 0) b = 1;
    return (unsigned)b;
}

inline uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

std::string key_of(const uint32_t* v, size_t w) { return std::string(reinterpret_cast<const char*>(v), w * sizeof(uint32_t)); }

std::vector<size_t> non_empty_or_first(const std::vector<int>& perm, int rank) // tensorci2.rs:1813-1819
{
    std::vector<size_t> v;
    for (int i = 0; i < rank; ++i) v.push_back((size_t)perm[i]);
    if (v.empty()) v.push_back(0);
    return v;
}

} // namespace

void TCI2Options::validate() const // tensorci2.rs:140-149
{
    auto nonneg_finite = [](const char* n, double v) {
        if (!(v >= 0.0) || !std::isfinite(v))
            throw Error(T4A_GPU_INVALID_ARGUMENT, std::string(n) + " must be finite and non-negative");
    };
    nonneg_finite("tolerance", tolerance);
    nonneg_finite("tol_margin_global_search", tol_margin_global_search);
    if (max_iter == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "max_iter must be positive");
    if (ncheck_history == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "ncheck_history must be positive");
}

// =================================================================================================
Tci2::Tci2(const std::vector<size_t>& dims) : n_(dims.size()), local_dims(dims), fn_(dims) // tensorci2.rs:380-404
{
    if (dims.size() < 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "local_dims should have at least 2 elements");
    for (size_t s = 0; s < dims.size(); ++s)
        if (dims[s] == 0)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "local dimension at site " + std::to_string(s) + " must be positive");
    i_set.resize(n_);
    j_set.resize(n_);
    for (size_t p = 0; p < n_; ++p) {
        i_set[p].width = p;
        j_set[p].width = n_ - p - 1;
    }
    cores.resize(n_);
    for (size_t p = 0; p < n_; ++p) {
        cores[p].l = 0;
        cores[p].s = dims[p];
        cores[p].r = 0;
    }
    bond_errors.assign(n_ - 1, 0.0);
    last_sweep_shapes.assign(n_ - 1, {0, 0, 0});
    d_maxbits_.reserve(2);
    ev_pi_.init();
    fill_.ev.init();
}

Tci2::~Tci2()
{
    chain_abort();
    for (hipEvent_t e : chain_.t0) (void)hipEventDestroy(e);
    for (hipEvent_t e : chain_.t1) (void)hipEventDestroy(e);
    if (chain_.group_ev) (void)hipEventDestroy(chain_.group_ev);
    if (fill_.export_event) (void)hipEventDestroy(fill_.export_event);
    if (fill_.import_event) (void)hipEventDestroy(fill_.import_event);
    if (fill_.import_stream) pool::stream_put(fill_.import_stream, 2); // (synchronises it)
    if (fill_.graph_exec) (void)hipGraphExecDestroy(fill_.graph_exec);
    if (fill_.stream) pool::stream_put(fill_.stream, 2); // (synchronises it)
    // every buffer of this handle (and of its engine) was only ever used on the three streams that are idle now: the blocks
    // go back to the process-wide cache without a device-wide synchronisation, which would wait for the other handles' chains
    if (hipStreamSynchronize(eng.stream()) == hipSuccess) idle_scope_.arm();
}

void Tci2::set_builtin(int fid, int n_acc, const double* params, const uint64_t* weights)
{
    fn_.set_builtin(fid, n_acc, params, weights); // (refuses bad arguments before anything changes)
    // after a bond chain the pinned mirror is the master copy of the index sets, with accumulators of the OLD weights laid out
    // for the old n_acc: decode the digit tables first (as set_callback does), so that everything below re-accumulates from
    // digits with the new weights
    sync_digits();
    invalidate_fill_cache();
    source_ = nullptr;
    chain_.weights_valid = false; // (the accumulators in the device tables belong to the old weights)
    chain_.tables_valid = false;
    chain_.snap_serial[0] = chain_.snap_serial[1] = ~0ull;
    // the functor's weights and the site table go to the device HERE, with the function they belong to (round 5: the first bond chain of a
    // handle used to upload them — two copies and a stream synchronisation, ~35 us inside the first iteration of every solve)
    {
        hipStream_t st = eng.stream();
        chain_.weights.reserve(fn_.weights.size());
        chain_.siteinfo.reserve(2 * n_);
        std::vector<int> si(2 * n_);
        for (size_t p = 0; p < n_; ++p) {
            si[p] = (int)local_dims[p];
            si[n_ + p] = (int)fn_.offset[p];
        }
        T4A_HIP(hipMemcpyAsync(chain_.weights.get(), fn_.weights.data(), fn_.weights.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        T4A_HIP(hipMemcpyAsync(chain_.siteinfo.get(), si.data(), si.size() * sizeof(int), hipMemcpyHostToDevice, st));
        T4A_HIP(hipStreamSynchronize(st));
        chain_.weights_valid = true;
    }
}

void Tci2::set_callback(t4a_gpu_batch_eval_fn cb, void* ctx)
{
    fn_.set_callback(cb, ctx); // (refuses a null callback before anything changes)
    sync_digits();
    source_ = nullptr;
}

namespace {
// t4a_gpu_batch_eval_fn over a MatrixSource*: its host point evaluator
int64_t source_thunk(void* ctx, const uint32_t* idx, size_t n_sites, size_t n_pts, double* out)
{
    try {
        static_cast<MatrixSource*>(ctx)->eval_points(idx, n_sites, n_pts, out);
        return (int64_t)n_pts;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}
} // namespace

void Tci2::set_source(MatrixSource* src)
{
    if (!src) throw Error(T4A_GPU_NULL_POINTER, "source is null");
    const std::vector<size_t> dims = src->source_local_dims();
    if (dims.size() != n_)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "matrix source: length mismatch: the handle has " + std::to_string(n_) + " sites, the source " +
                                                  std::to_string(dims.size()));
    for (size_t s = 0; s < n_; ++s)
        if (dims[s] != local_dims[s])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "matrix source: local dimension mismatch at site " + std::to_string(s) + ": the handle has " +
                                                      std::to_string(local_dims[s]) + ", the source " + std::to_string(dims[s]));
    set_callback(&source_thunk, src);
    source_ = src;
}

size_t Tci2::rank() const // tensorci2.rs:600-614
{
    size_t r = 0;
    for (size_t p = 1; p < n_; ++p) r = std::max(r, i_set[p].count);
    return r;
}

std::vector<size_t> Tci2::link_dims() const
{
    std::vector<size_t> v;
    for (size_t p = 1; p < n_; ++p) v.push_back(i_set[p].count);
    return v;
}

double Tci2::max_bond_error() const // tensorci2.rs:630
{
    double m = 0.0;
    for (double e : bond_errors) m = std::fmax(m, e);
    return m;
}

void Tci2::invalidate_site_tensors() // tensorci2.rs:724-728
{
    for (size_t p = 0; p < n_; ++p) {
        cores[p].l = 0;
        cores[p].s = local_dims[p];
        cores[p].r = 0;
    }
}

void Tci2::add_global_pivots(const std::vector<std::vector<uint32_t>>& pivots) // tensorci2.rs:668-711
{
    for (const auto& p : pivots) {
        if (p.size() != n_)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Pivot length (" + std::to_string(p.size()) +
                                                      ") must match number of sites (" + std::to_string(n_) + ")");
        for (size_t s = 0; s < n_; ++s)
            if (p[s] >= local_dims[s])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "pivot value " + std::to_string(p[s]) +
                                                          " is out of bounds at site " + std::to_string(s));
    }
    if (!pivots.empty()) sync_digits();
    for (const auto& pivot : pivots) {
        for (size_t p = 0; p < n_; ++p) {
            const uint32_t* pre = pivot.data();
            const uint32_t* suf = pivot.data() + p + 1;
            if (!i_set[p].contains(pre)) {
                i_set[p].push(pre);
                chain_.tables_valid = false;
            }
            if (!j_set[p].contains(suf)) {
                j_set[p].push(suf);
                chain_.tables_valid = false;
            }
        }
    }
    invalidate_site_tensors();
}

IndexSet Tci2::kronecker_i(size_t p) const // tensorci2.rs:1224-1234
{
    IndexSet r;
    r.width = p + 1;
    const IndexSet& src = i_set[p];
    const size_t d = local_dims[p];
    r.count = src.count * d;
    r.d.resize(r.count * r.width);
    uint32_t* out = r.d.data();
    for (size_t k = 0; k < src.count; ++k) {
        const uint32_t* in = src.at(k);
        for (size_t li = 0; li < d; ++li) {
            if (src.width) std::memcpy(out, in, src.width * sizeof(uint32_t));
            out[src.width] = (uint32_t)li;
            out += r.width;
        }
    }
    return r;
}

IndexSet Tci2::kronecker_j(size_t p) const // tensorci2.rs:1236-1246
{
    IndexSet r;
    r.width = n_ - p;
    const IndexSet& src = j_set[p];
    const size_t d = local_dims[p];
    r.count = src.count * d;
    r.d.resize(r.count * r.width);
    uint32_t* out = r.d.data();
    for (size_t li = 0; li < d; ++li)
        for (size_t k = 0; k < src.count; ++k) {
            out[0] = (uint32_t)li;
            if (src.width) std::memcpy(out + 1, src.at(k), src.width * sizeof(uint32_t));
            out += r.width;
        }
    return r;
}

// order-preserving union (tensorci2.rs:1837-1846); hashing replaces the reference's O(M*chi) `contains`
void Tci2::union_extras(IndexSet& base, const IndexSet& extras)
{
    if (extras.count == 0) return;
    if (base.width == 0) {
        if (base.count == 0) base.count = 1;
        return;
    }
    // open-addressing table of (hash, index+1); digits are compared on a hash hit, so the result is exactly the
    // reference's `contains`-based union
    const size_t w = base.width;
    auto hash_of = [w](const uint32_t* v) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (size_t i = 0; i < w; ++i) {
            h ^= v[i];
            h *= 0x100000001b3ull;
        }
        return h ^ (h >> 29);
    };
    size_t cap = 16;
    while (cap < 2 * (base.count + extras.count)) cap <<= 1;
    std::vector<uint32_t> slot(cap, 0);
    base.d.reserve((base.count + extras.count) * w);
    auto insert = [&](size_t idx) {
        size_t pos = hash_of(base.at(idx)) & (cap - 1);
        while (slot[pos]) pos = (pos + 1) & (cap - 1);
        slot[pos] = (uint32_t)idx + 1;
    };
    for (size_t k = 0; k < base.count; ++k) insert(k);
    for (size_t k = 0; k < extras.count; ++k) {
        const uint32_t* e = extras.at(k);
        size_t pos = hash_of(e) & (cap - 1);
        bool found = false;
        while (slot[pos]) {
            if (std::memcmp(base.at(slot[pos] - 1), e, w * sizeof(uint32_t)) == 0) {
                found = true;
                break;
            }
            pos = (pos + 1) & (cap - 1);
        }
        if (!found) {
            base.push(e);
            slot[pos] = (uint32_t)base.count; // index of the new entry + 1
        }
    }
}

// Accumulators of both index sets -> pinned arena -> device (one asynchronous copy on the main stream).
void Tci2::stage_accumulators(const IndexSet& a, size_t a0, const IndexSet& b, size_t b0, const std::vector<uint64_t>* acc_a,
                              const std::vector<uint64_t>* acc_b, const uint64_t** d_ra, const uint64_t** d_rb, bool in_place)
{
    hipStream_t st = eng.stream();
    const size_t K = (size_t)fn_.dev.n_acc;
    std::vector<uint64_t> ra_own, rb_own;
    if (!acc_a) accumulate(a, a0, ra_own);
    if (!acc_b) accumulate(b, b0, rb_own);
    const std::vector<uint64_t>& ra = acc_a ? *acc_a : ra_own;
    const std::vector<uint64_t>& rb = acc_b ? *acc_b : rb_own;
    if (ra.size() != a.count * K || rb.size() != b.count * K)
        throw Error(T4A_GPU_INTERNAL_ERROR, "prepared accumulators have the wrong size");
    // pinned staging arena: entries stay valid until the next stream sync
    const size_t need = ra.size() + rb.size();
    if (acc_used_ + need > h_acc_.cap) {
        T4A_HIP(hipStreamSynchronize(st));
        acc_used_ = 0;
        h_acc_.reserve(std::max(need * 2, (size_t)1 << 16));
    }
    uint64_t* ha = h_acc_.get() + acc_used_;
    acc_used_ += need;
    std::memcpy(ha, ra.data(), ra.size() * sizeof(uint64_t));
    std::memcpy(ha + ra.size(), rb.data(), rb.size() * sizeof(uint64_t));
    if (in_place) { // pinned memory is device-visible under the same address
        *d_ra = ha;
        *d_rb = ha + ra.size();
        return;
    }
    d_rowacc_.reserve(need);
    stage_copy_launch(ha, d_rowacc_.get(), need, st);
    T4A_HIP(hipGetLastError());
    *d_ra = d_rowacc_.get();
    *d_rb = d_rowacc_.get() + ra.size();
}

// out[ia + a.count*ib] = f(index with a's digits at sites [a0, a0+a.width) and b's at [b0, b0+b.width))
void Tci2::eval_matrix(const IndexSet& a, size_t a0, const IndexSet& b, size_t b0, double* d_out,
                       unsigned long long* d_maxbits, const std::vector<uint64_t>* acc_a,
                       const std::vector<uint64_t>* acc_b)
{
    fn_.require("tci2");
    const size_t na = a.count, nb = b.count;
    if (na == 0 || nb == 0) return;
    if (a.width + b.width != n_) throw Error(T4A_GPU_INTERNAL_ERROR, "eval_matrix: index widths do not cover all sites");
    hipStream_t st = eng.stream();
    eng.prof.v[11] += (double)na * (double)nb;
    if (fn_.builtin()) {
        const uint64_t *d_ra = nullptr, *d_rb = nullptr;
        stage_accumulators(a, a0, b, b0, acc_a, acc_b, &d_ra, &d_rb);
        pi_eval_launch(fn_.dev, d_ra, (int)na, d_rb, (int)nb, d_out, (int)na, false, d_maxbits, st);
        T4A_HIP(hipGetLastError());
    } else if (source_ && !pi_shard.active()) {
        // device matrix source: the set that starts at site 0 holds the rows of the source's matrix; when that is `b`, out (na x nb,
        // ia fastest) is the source's matrix transposed
        const bool transposed = a0 != 0;
        const IndexSet& rows = transposed ? b : a;
        const IndexSet& cols = transposed ? a : b;
        source_->fill_matrix(rows.width, rows.d.data(), rows.count, cols.d.data(), cols.count, d_out, na, transposed, st);
        if (d_maxbits) absmax_launch(d_out, na * nb, d_maxbits, st);
        T4A_HIP(hipGetLastError());
        source_stats[0] += 1;
        source_stats[1] += na * nb;
    } else {
        // host batch callback: points in row-major order of (ia, ib) — `ia` outer, `ib` inner — exactly the
        // order the reference hands to batched_f (tensorci2.rs:1862-1869)
        const size_t npts = na * nb;
        cb_vals_.reserve(npts); // (pinned, grow-only: the previous upload out of it was synchronised below)
        double* const vals = cb_vals_.get();
        source_stats[2] += npts;
        if (pi_shard.active()) {
            // column blocks over the ranks of the process group + one all-gather (pishard.hpp)
            pi_shard_evaluate(pi_shard, fn_.cb, fn_.cb_ctx, n_, a.d.data(), a.width, a0, na, b.d.data(), b.width, b0, nb, vals);
        } else {
            // the index buffer of the callback: grow-only and filled by a few host threads (round 5: measured on the native callback of
            // tools/bench_components.py — the backend's share of a cfg3 sweep through a callback was 0.27 s, most of it this buffer)
            if (cb_idx_cap_ < npts * n_) {
                cb_idx_cap_ = npts * n_ + npts * n_ / 4;
                cb_idx_.reset(new uint32_t[cb_idx_cap_]);
            }
            uint32_t* const idx = cb_idx_.get();
            auto fill_rows = [&](size_t ia0, size_t ia1) {
                for (size_t ia = ia0; ia < ia1; ++ia)
                    for (size_t ib = 0; ib < nb; ++ib) {
                        uint32_t* dst = idx + (ia * nb + ib) * n_;
                        std::memcpy(dst + a0, a.at(ia), a.width * sizeof(uint32_t));
                        std::memcpy(dst + b0, b.at(ib), b.width * sizeof(uint32_t));
                    }
            };
            const unsigned hw = std::thread::hardware_concurrency();
            const size_t nthr = (npts * n_ < ((size_t)1 << 21) || hw < 2) ? 1 : std::min<size_t>(std::min<size_t>(8, hw), na);
            if (nthr <= 1) {
                fill_rows(0, na);
            } else {
                std::vector<std::thread> pool;
                for (size_t t = 1; t < nthr; ++t) pool.emplace_back(fill_rows, na * t / nthr, na * (t + 1) / nthr);
                fill_rows(0, na / nthr);
                for (auto& th : pool) th.join();
            }
            // opt-in (t4a_gpu_tci2_set_callback_threads): the point list of ONE candidate matrix split over host threads that call the
            // user function concurrently — outside the reference's contract (it calls f sequentially on one thread on purpose,
            // docs/design/adaptive-tci-interpolation.md:9-11), so only for callbacks that are thread safe.  Same points, same values.
            const size_t cthr = (callback_threads <= 1 || npts < ((size_t)1 << 14)) ? 1 : std::min<size_t>(callback_threads, npts >> 12);
            if (cthr <= 1) {
                fn_.call(idx, n_, npts, vals, "batch callback", "requested entries");
            } else {
                std::vector<int64_t> got(cthr, 0);
                auto call = [&](size_t t) {
                    const size_t p0 = npts * t / cthr, p1 = npts * (t + 1) / cthr;
                    got[t] = fn_.cb(fn_.cb_ctx, idx + p0 * n_, n_, p1 - p0, vals + p0) - (int64_t)(p1 - p0);
                };
                std::vector<std::thread> pool;
                for (size_t t = 1; t < cthr; ++t) pool.emplace_back(call, t);
                call(0);
                for (auto& th : pool) th.join();
                for (size_t t = 0; t < cthr; ++t)
                    if (got[t] != 0)
                        throw Error(T4A_GPU_CALLBACK_ERROR, "batch callback returned a wrong number of values for block " + std::to_string(t) + " of " +
                                                                std::to_string(cthr) + " (callback threads)");
            }
        }
        d_vals_.reserve(npts);
        T4A_HIP(hipMemcpyAsync(d_vals_.get(), vals, npts * sizeof(double), hipMemcpyHostToDevice, st));
        T4A_HIP(hipStreamSynchronize(st)); // (the pinned buffer is reused by the next matrix)
        // vals is (na x nb) row-major == (nb x na) column-major; transpose into the column-major na x nb output
        transpose_launch(d_vals_.get(), (int)nb, (int)na, (int)nb, d_out, (int)na, st);
        if (d_maxbits) absmax_launch(d_out, npts, d_maxbits, st);
        T4A_HIP(hipGetLastError());
    }
}

std::vector<double> Tci2::eval_points_host(const std::vector<uint32_t>& idx, size_t n_pts)
{
    fn_.require("tci2");
    std::vector<double> out(n_pts);
    if (n_pts == 0) return out;
    if (fn_.builtin()) {
        fn_.host_values(idx.data(), n_pts, out.data());
    } else {
        source_stats[2] += n_pts;
        fn_.call(idx.data(), n_, n_pts, out.data(), "batch callback", "requested entries");
    }
    return out;
}

// kron(I_b, d_b) + extras (rows) or kron(d_{b+1}, J_{b+1}) + extras (columns) of bond `bond`, with accumulators
void Tci2::build_side(size_t bond, bool cols, const IndexSet& extra, SidePrep& out) const
{
    out.valid = false;
    out.bond = bond;
    out.cols = cols;
    out.set = cols ? kronecker_j(bond + 1) : kronecker_i(bond);
    union_extras(out.set, extra);
    out.acc.clear();
    if (fn_.builtin()) accumulate(out.set, cols ? bond + 1 : 0, out.acc);
    out.valid = true;
}

LuciResult Tci2::luci_on_sets(const IndexSet& is, const IndexSet& js, const RrLUOptions& o, bool need_factors,
                              const std::vector<uint64_t>* acc_rows, const std::vector<uint64_t>* acc_cols)
{
    const size_t M = is.count, N = js.count;
    hipStream_t st = eng.stream();
    if (fn_.builtin() && M > 0 && N > 0) {
        // built-in functor: only the accumulators travel; the rrLU kernel evaluates Pi into its registers
        FusedPi fp;
        fp.fn = fn_.dev;
        // small bonds (the single-workgroup plan with the fused candidate-matrix build takes them): the kernel reads the few
        // hundred bytes of accumulators straight from the pinned arena — no staging kernel in front of a 10 us factorisation
        fp.host_resident = M * N <= (size_t)64 * 64;
        stage_accumulators(is, 0, js, is.width, acc_rows, acc_cols, &fp.d_rowacc, &fp.d_colacc, fp.host_resident);
        eng.prof.v[11] += (double)M * (double)N;
        LuciResult lu = eng.luci(nullptr, (int)M, (int)N, o, need_factors, false, &fp);
        acc_used_ = 0;
        if (lu.abs_max > max_sample_value) max_sample_value = lu.abs_max;
        return lu;
    }
    double* d_pi = eng.pi(M * N);
    static const bool host_prof = std::getenv("T4A_HOST_PROFILE") != nullptr;
    static double hp_eval = 0;
    static long hp_n = 0;
    const auto hp_t0 = std::chrono::steady_clock::now();
    if (eng.prof.enabled) T4A_HIP(hipEventRecord(ev_pi_.a, st));
    eval_matrix(is, 0, js, is.width, d_pi, nullptr, acc_rows, acc_cols);
    if (eng.prof.enabled) T4A_HIP(hipEventRecord(ev_pi_.b, st));
    if (host_prof) {
        hp_eval += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - hp_t0).count();
        if (++hp_n % 580 == 0) std::fprintf(stderr, "[host profile] eval_matrix host part %.1f us per bond\n", 1e3 * hp_eval / hp_n);
    }
    LuciResult lu = eng.luci(d_pi, (int)M, (int)N, o, need_factors, false);
    acc_used_ = 0; // eng.luci synchronised the stream
    if (eng.prof.enabled) {
        float ms = 0.f;
        T4A_HIP(hipEventElapsedTime(&ms, ev_pi_.a, ev_pi_.b));
        eng.prof.v[2] += ms;
        eng.prof.v[3] += 1.0;
    }
    // update_max_sample_value over every entry of Π (tensorci2.rs:2009-2014)
    if (lu.abs_max > max_sample_value) max_sample_value = lu.abs_max;
    return lu;
}

// PivotSearchStrategy::Rook (tensorci2.rs:1904-1929): the candidate matrix is never materialised; the lazy
// block-rook kernel asks for full rows / columns of Pi, which are evaluated on demand (LazyPiEvaluator, :2035-2142).
LuciResult Tci2::rook_on_sets(const IndexSet& is, const IndexSet& js, const RrLUOptions& o)
{
    fn_.require("tci2");
    const size_t M = is.count, N = js.count;
    hipStream_t st = eng.stream();
    RookSource src;
    src.M = (int)M;
    src.N = (int)N;
    if (fn_.builtin()) {
        const size_t K = (size_t)fn_.dev.n_acc;
        std::vector<uint64_t> ra, rb;
        accumulate(is, 0, ra);
        accumulate(js, is.width, rb);
        // (one copy out of pinned memory: two copies out of pageable vectors and a synchronisation cost ~60 us per bond on small problems;
        // the staging buffer is free again: every rook search ends with a stream synchronisation)
        const auto d_acc = stage_accumulator_pair(ra, rb, h_rookacc_, d_rowacc_, st);
        const uint64_t *d_ra = d_acc.first, *d_rb = d_acc.second;
        src.column = [=](int c, double* out) {
            pi_eval_launch(fn_.dev, d_ra, (int)M, d_rb + (size_t)c * K, 1, out, (int)M, false, nullptr, st);
        };
        src.row = [=](int r, double* out) {
            pi_eval_launch(fn_.dev, d_ra + (size_t)r * K, 1, d_rb, (int)N, out, 1, false, nullptr, st);
        };
        // (a built-in functor costs nothing to evaluate: the search runs device-resident on the materialised matrix, rook.hip)
        static const bool host_driven = std::getenv("T4A_ROOK_HOST") != nullptr; // (A/B and parity of the two search drivers)
        if (!host_driven)
            src.full = [=](double* out) { pi_eval_launch(fn_.dev, d_ra, (int)M, d_rb, (int)N, out, (int)M, false, nullptr, st); };
    } else {
        auto eval_points = [this, st, &is, &js](size_t r0, size_t nr, size_t c0, size_t nc, double* out) {
            const size_t npts = nr * nc;
            std::vector<uint32_t> idx(npts * n_);
            for (size_t a = 0; a < nr; ++a)
                for (size_t b = 0; b < nc; ++b) {
                    uint32_t* dst = idx.data() + (a * nc + b) * n_;
                    std::memcpy(dst, is.at(r0 + a), is.width * sizeof(uint32_t));
                    std::memcpy(dst + is.width, js.at(c0 + b), js.width * sizeof(uint32_t));
                }
            std::vector<double> vals(npts);
            source_stats[2] += npts;
            fn_.call(idx.data(), n_, npts, vals.data(), "batch callback", "requested entries");
            T4A_HIP(hipMemcpyAsync(out, vals.data(), npts * sizeof(double), hipMemcpyHostToDevice, st));
            T4A_HIP(hipStreamSynchronize(st));
        };
        src.column = [=](int c, double* out) { eval_points(0, M, (size_t)c, 1, out); };
        src.row = [=](int r, double* out) { eval_points((size_t)r, 1, 0, N, out); };
    }
    double sampled = max_sample_value;
    LuciResult lu = rook_luci(eng, rook_work_, src, o, &sampled, &eng.prof.v[11]);
    acc_used_ = 0;
    max_sample_value = sampled; // tci.max_sample_value = evaluator.sampled_max() (tensorci2.rs:1926)
    return lu;
}

void Tci2::set_core_zero(size_t site, size_t l, size_t s, size_t r)
{
    DevCore& c = cores[site];
    c.reshape(l, s, r);
    fill_launch(c.buf.get(), l * s * r, 0.0, eng.stream());
}

void Tci2::set_core_from_left(size_t site, size_t left_dim, size_t site_dim, const LuciResult& lu)
{
    const size_t nb = std::max<size_t>((size_t)lu.rank, 1);
    DevCore& c = cores[site];
    c.buf.reserve(left_dim * site_dim * nb);
    c.l = left_dim;
    c.s = site_dim;
    c.r = nb;
    const size_t total = c.size();
    hipLaunchKernelGGL(pack_left_core_kernel, dim3(blocks_for(total)), dim3(256), 0, eng.stream(), eng.left(), lu.M, lu.M,
                       lu.rank, c.buf.get(), (int)left_dim, (int)site_dim, (int)nb);
}

void Tci2::set_core_from_right(size_t site, size_t site_dim, size_t right_dim, const LuciResult& lu)
{
    const size_t nb = std::max<size_t>((size_t)lu.rank, 1);
    DevCore& c = cores[site];
    c.buf.reserve(nb * site_dim * right_dim);
    c.l = nb;
    c.s = site_dim;
    c.r = right_dim;
    const size_t total = c.size();
    const int ldm = lu.rank > 0 ? lu.rank : 1;
    hipLaunchKernelGGL(pack_right_core_kernel, dim3(blocks_for(total)), dim3(256), 0, eng.stream(), eng.right(), ldm,
                       lu.rank, lu.N, c.buf.get(), (int)nb, (int)site_dim, (int)right_dim);
}

void Tci2::update_pivot_errors(const std::vector<double>& e) // tensorci2.rs:801-808
{
    if (pivot_errors.size() < e.size()) pivot_errors.resize(e.size(), 0.0);
    for (size_t i = 0; i < e.size(); ++i) pivot_errors[i] = std::fmax(pivot_errors[i], e[i]);
}

// tensorci2.rs:1821-2007
void Tci2::update_pivots(size_t b, bool left_orthogonal, const TCI2Options& options, const IndexSet& extra_i,
                         const IndexSet& extra_j)
{
    static const bool host_prof = std::getenv("T4A_HOST_PROFILE") != nullptr;
    static double hp_sets = 0, hp_luci = 0, hp_post = 0;
    static long hp_n = 0;
    const auto hp_t0 = std::chrono::steady_clock::now();
    sync_digits();
    // one side may have been built while the previous bond's kernels were running (it does not depend on them)
    SidePrep ready;
    if (prep_.valid && prep_.bond == b) std::swap(ready, prep_);
    prep_.valid = false;
    const bool have_rows = ready.valid && !ready.cols, have_cols = ready.valid && ready.cols;
    IndexSet i_own, j_own;
    if (!have_rows) {
        i_own = kronecker_i(b);
        union_extras(i_own, extra_i);
    }
    if (!have_cols) {
        j_own = kronecker_j(b + 1);
        union_extras(j_own, extra_j);
    }
    const IndexSet& i_comb = have_rows ? ready.set : i_own;
    const IndexSet& j_comb = have_cols ? ready.set : j_own;
    const bool acc_ready = ready.valid && fn_.builtin();
    if (i_comb.count == 0 || j_comb.count == 0) return;
    if (prefetch_.wanted || prefetch_.fill_site >= 0) {
        // host work that does not depend on this bond: the independent side of the NEXT bond and the fill
        // accumulators of a site that is already final; runs while this bond's kernels are in flight
        const Prefetch pf = prefetch_;
        prefetch_.wanted = false;
        prefetch_.fill_site = -1;
        eng.overlap_hook = [this, pf]() {
            if (pf.wanted) build_side(pf.bond, pf.cols, *pf.extra, prep_);
            if (pf.fill_site >= 0) prepare_fill_site((size_t)pf.fill_site);
        };
    }
    const auto hp_t1 = std::chrono::steady_clock::now();

    const bool extras_used = extra_i.count != 0 || extra_j.count != 0;
    RrLUOptions lo;
    lo.max_bond_dim = options.max_bond_dim_or_max();
    lo.rel_tol = options.tolerance;
    lo.abs_tol = 0.0;
    lo.left_orthogonal = left_orthogonal;
    // the reference always builds the factors; they are only CONSUMED when no extras were merged
    // (tensorci2.rs:1942-1949), so the device skips the trsm/gemm otherwise.
    LuciResult lu = options.pivot_search == 0
                        ? luci_on_sets(i_comb, j_comb, lo, !extras_used, (acc_ready && have_rows) ? &ready.acc : nullptr,
                                       (acc_ready && have_cols) ? &ready.acc : nullptr)
                        : rook_on_sets(i_comb, j_comb, lo);
    if (eng.overlap_hook) { // not consumed (rook path / empty matrix): run it now so the next bond still finds it
        std::function<void()> hook;
        hook.swap(eng.overlap_hook);
        hook();
    }
    const auto hp_t2 = std::chrono::steady_clock::now();
    if (b < last_sweep_shapes.size()) last_sweep_shapes[b] = {i_comb.count, j_comb.count, (size_t)lu.rank};

    const std::vector<size_t> rows = non_empty_or_first(lu.row_perm, lu.rank);
    const std::vector<size_t> cols = non_empty_or_first(lu.col_perm, lu.rank);
    IndexSet ni, nj;
    ni.width = i_comb.width;
    nj.width = j_comb.width;
    for (size_t r : rows) ni.push(i_comb.at(r));
    for (size_t c : cols) nj.push(j_comb.at(c));
    i_set[b + 1] = ni;
    j_set[b] = nj;
    chain_.tables_valid = false; // (the host path moved the sets: the device tables of the bond chain are stale)
    if (host_prof) {
        const auto hp_t3 = std::chrono::steady_clock::now();
        hp_sets += std::chrono::duration<double, std::milli>(hp_t1 - hp_t0).count();
        hp_luci += std::chrono::duration<double, std::milli>(hp_t2 - hp_t1).count();
        hp_post += std::chrono::duration<double, std::milli>(hp_t3 - hp_t2).count();
        if (++hp_n % 580 == 0)
            std::fprintf(stderr, "[host profile] per bond: build sets %.1f us, luci_on_sets (host+device) %.1f us, post %.1f us\n",
                         1e3 * hp_sets / hp_n, 1e3 * hp_luci / hp_n, 1e3 * hp_post / hp_n);
    }

    if (extras_used) {
        if (!lu.pivot_errors.empty()) bond_errors[b] = lu.pivot_errors.back();
        return;
    }
    const size_t left_dim = (b == 0) ? 1 : i_set[b].count;
    set_core_from_left(b, left_dim, local_dims[b], lu);
    const size_t right_dim = (b + 1 == n_ - 1) ? 1 : j_set[b + 1].count;
    set_core_from_right(b + 1, local_dims[b + 1], right_dim, lu);
    if (!lu.pivot_errors.empty()) bond_errors[b] = lu.pivot_errors.back();
}

// tensorci2.rs:746-798
void Tci2::sweep2site(bool forward, const TCI2Options& options)
{
    options.validate();
    fn_.require("tci2");
    fill_wait();
    invalidate_site_tensors();
    flush_pivot_errors();
    last_sweep_shapes.assign(n_ - 1, {0, 0, 0});
    prep_.valid = false;
    prefetch_.wanted = false;
    IndexSet ei, ej; // empty extras
    if (chain_enqueue(forward, options, -1, false)) { // built-in functor: the whole half-sweep in one go (tci2_chain.hip)
        chain_finish(options);
        fill_site_tensors();
        return;
    }
    sync_digits();
    if (forward) {
        for (size_t b = 0; b + 1 < n_; ++b) {
            ei.width = b + 1;
            ej.width = n_ - b - 1;
            update_pivots(b, true, options, ei, ej);
        }
    } else {
        for (size_t b = n_ - 1; b-- > 0;) {
            ei.width = b + 1;
            ej.width = n_ - b - 1;
            update_pivots(b, false, options, ei, ej);
        }
    }
    fill_site_tensors();
}

// tensorci2.rs:918-1050
void Tci2::sweep1site_at_bond(size_t b, bool forward, double rel_tol, double abs_tol, size_t max_bond_dim,
                              bool update_tensors)
{
    sync_digits();
    IndexSet is = forward ? kronecker_i(b) : i_set[b];
    IndexSet js = forward ? j_set[b] : kronecker_j(b);
    if (is.count == 0 || js.count == 0) return;
    RrLUOptions lo;
    lo.max_bond_dim = max_bond_dim;
    lo.rel_tol = rel_tol;
    lo.abs_tol = abs_tol;
    lo.left_orthogonal = forward;
    LuciResult lu = luci_on_sets(is, js, lo, update_tensors);
    const std::vector<size_t> rows = non_empty_or_first(lu.row_perm, lu.rank);
    const std::vector<size_t> cols = non_empty_or_first(lu.col_perm, lu.rank);
    IndexSet ni, nj;
    ni.width = is.width;
    nj.width = js.width;
    for (size_t r : rows) ni.push(is.at(r));
    for (size_t c : cols) nj.push(js.at(c));
    if (forward) {
        i_set[b + 1] = ni;
        j_set[b] = nj;
    } else {
        i_set[b] = ni;
        j_set[b - 1] = nj;
    }
    chain_.tables_valid = false;
    if (update_tensors) {
        if (forward) {
            const size_t left_dim = (b == 0) ? 1 : i_set[b].count;
            set_core_from_left(b, left_dim, local_dims[b], lu);
        } else {
            const size_t right_dim = (b == n_ - 1) ? 1 : j_set[b].count;
            set_core_from_right(b, local_dims[b], right_dim, lu);
        }
    }
    if (!lu.pivot_errors.empty()) {
        const size_t bond_idx = forward ? b : b - 1;
        bond_errors[bond_idx] = lu.pivot_errors.back();
    }
    update_pivot_errors(lu.pivot_errors);
}

// tensorci2.rs:865-915
void Tci2::sweep1site(bool forward, double rel_tol, double abs_tol, size_t max_bond_dim, bool update_tensors)
{
    if (!(rel_tol >= 0.0) || !std::isfinite(rel_tol)) throw Error(T4A_GPU_INVALID_ARGUMENT, "rel_tol must be finite and non-negative");
    if (!(abs_tol >= 0.0) || !std::isfinite(abs_tol)) throw Error(T4A_GPU_INVALID_ARGUMENT, "abs_tol must be finite and non-negative");
    if (max_bond_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "max_bond_dim must be positive");
    fn_.require("tci2");
    fill_wait();
    flush_pivot_errors();
    invalidate_site_tensors();
    // built-in functor: the whole sweep as one chain on the device (tci2_chain.hip; the independent side of every bond is the
    // table itself), the site tensors from the factored matrices it leaves behind
    bool chained = false;
    static const bool no_chain1 = std::getenv("T4A_NO_CHAIN_1SITE") != nullptr;
    if (!no_chain1 && n_ >= 2) {
        TCI2Options o1;
        o1.tolerance = rel_tol;
        o1.max_bond_dim = max_bond_dim == std::numeric_limits<size_t>::max() ? 0 : max_bond_dim;
        o1.pivot_search = 0;
        o1.nsearch = 0;
        prep_.valid = false;
        prefetch_.wanted = false;
        chain_.one_site = true;
        chain_.one_factors = update_tensors;
        chain_.abs_tol = abs_tol;
        try {
            chained = chain_enqueue(forward, o1, -1, false);
            if (chained) chain_finish(o1);
        } catch (...) {
            chain_abort(); // (nothing may stay in flight, no XCD reserved)
            chain_.one_site = false;
            throw;
        }
        chain_.one_site = false;
    }
    if (chained) {
        // (every bond went through the chain or through its per-bond tail)
    } else if (forward) {
        for (size_t b = 0; b + 1 < n_; ++b) sweep1site_at_bond(b, true, rel_tol, abs_tol, max_bond_dim, update_tensors);
    } else {
        for (size_t b = n_ - 1; b >= 1; --b) sweep1site_at_bond(b, false, rel_tol, abs_tol, max_bond_dim, update_tensors);
    }
    if (update_tensors) { // tensorci2.rs:902-912 + fill_tensor :813-850
        const size_t last = forward ? n_ - 1 : 0;
        const bool on_device = chained && forward && chain_.last_core_ok; // (evaluated from the tables behind the chain: chain_last_core_kernel)
        chain_.last_core_ok = false;
        const size_t A = i_set[last].count, S = local_dims[last], C = j_set[last].count; // (counts are current behind a chain, digits need not be)
        DevCore& c = cores[last];
        if (!on_device) c.buf.reserve(std::max<size_t>(A * S * C, 1));
        c.l = A;
        c.s = S;
        c.r = C;
        if (A * S * C > 0 && !on_device) {
            sync_digits();
            IndexSet rows = kronecker_i(last);
            const IndexSet& jl = j_set[last];
            double* d_m = eng.pi(A * S * C);
            eval_matrix(rows, 0, jl, rows.width, d_m, nullptr);
            hipLaunchKernelGGL(pack_left_core_kernel, dim3(blocks_for(c.size())), dim3(256), 0, eng.stream(), d_m,
                               (int)(A * S), (int)(A * S), (int)C, c.buf.get(), (int)A, (int)S, (int)C);
            T4A_HIP(hipStreamSynchronize(eng.stream()));
            acc_used_ = 0;
        }
    }
}

// tensorci2.rs:1201-1221
void Tci2::make_canonical(double rel_tol, double abs_tol, size_t max_bond_dim)
{
    if (!(rel_tol >= 0.0) || !std::isfinite(rel_tol)) throw Error(T4A_GPU_INVALID_ARGUMENT, "rel_tol must be finite and non-negative");
    if (!(abs_tol >= 0.0) || !std::isfinite(abs_tol)) throw Error(T4A_GPU_INVALID_ARGUMENT, "abs_tol must be finite and non-negative");
    if (max_bond_dim == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "max_bond_dim must be positive");
    sweep1site(true, 0.0, 0.0, std::numeric_limits<size_t>::max(), false);
    sweep1site(false, rel_tol, abs_tol, max_bond_dim, false);
    sweep1site(true, rel_tol, abs_tol, max_bond_dim, true);
}

// =================================================================================================
// TT evaluation / sum
// =================================================================================================
std::vector<double> Tci2::site_tensor_host(size_t site, size_t dims3[3])
{
    fill_wait();
    const DevCore& c = cores[site];
    dims3[0] = c.l;
    dims3[1] = c.s;
    dims3[2] = c.r;
    std::vector<double> h(c.size());
    if (!h.empty()) {
        T4A_HIP(hipMemcpyAsync(h.data(), c.buf.get(), h.size() * sizeof(double), hipMemcpyDeviceToHost, eng.stream()));
        T4A_HIP(hipStreamSynchronize(eng.stream()));
    }
    return h;
}

void Tci2::site_tensor_device(size_t site, double* d_out)
{
    if (site >= len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "site out of range");
    fill_wait();
    const DevCore& c = cores[site];
    if (c.size()) {
        T4A_HIP(hipMemcpyAsync(d_out, c.buf.get(), c.size() * sizeof(double), hipMemcpyDeviceToDevice, eng.stream()));
        T4A_HIP(hipStreamSynchronize(eng.stream()));
    }
}

void Tci2::set_site_tensor_device(size_t site, const size_t dims3[3], const double* d_in)
{
    if (site >= len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "site out of range");
    if (dims3[1] != local_dims[site]) throw Error(T4A_GPU_INVALID_ARGUMENT, "site dimension mismatch");
    fill_wait();
    DevCore& c = cores[site];
    const size_t count = dims3[0] * dims3[1] * dims3[2];
    c.reshape(dims3[0], dims3[1], dims3[2]);
    if (count) {
        if (!d_in) throw Error(T4A_GPU_NULL_POINTER, "in_device is null");
        T4A_HIP(hipMemcpyAsync(c.buf.get(), d_in, count * sizeof(double), hipMemcpyDeviceToDevice, eng.stream()));
        T4A_HIP(hipStreamSynchronize(eng.stream()));
    }
}

void Tci2::set_index_set(int which, size_t site, size_t count, const size_t* data)
{
    if (site >= len() || which < 0 || which > 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "site/which out of range");
    sync_digits();
    IndexSet& s = which == 0 ? i_set[site] : j_set[site];
    const size_t first_site = which == 0 ? 0 : site + 1;
    if (count * s.width && !data) throw Error(T4A_GPU_NULL_POINTER, "data is null");
    IndexSet n;
    n.width = s.width;
    n.count = count;
    n.d.resize(count * s.width);
    for (size_t k = 0; k < count; ++k)
        for (size_t q = 0; q < s.width; ++q) {
            const size_t v = data[k * s.width + q];
            if (v >= local_dims[first_site + q]) throw Error(T4A_GPU_INVALID_ARGUMENT, "index out of bounds");
            n.d[k * s.width + q] = (uint32_t)v;
        }
    s = n;
    invalidate_site_tensors();
    mark_sets_changed();
}

void Tci2::set_site_shard(size_t rank, size_t world)
{
    if (world == 0 || rank >= world) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid shard (rank, world)");
    shard_rank = rank;
    shard_world = world;
}

void Tci2::set_pi_shard(size_t rank, size_t world, t4a_gpu_allgather_fn gather, void* ctx)
{
    if (world == 0 || rank >= world) throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid shard (rank, world)");
    if (world > 1 && !gather) throw Error(T4A_GPU_NULL_POINTER, "a column-block shard over more than one rank needs an all-gather callback");
    pi_shard = PiShard();
    pi_shard.rank = rank;
    pi_shard.world = world;
    pi_shard.gather = world > 1 ? gather : nullptr;
    pi_shard.gather_ctx = ctx;
}

static void check_tt_chain(const std::vector<DevCore>& cores) // SimpleTensorTrain::new, simplett/src/tensortrain.rs:97
{
    if (cores.front().l != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "First tensor must have left dimension 1");
    if (cores.back().r != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "Last tensor must have right dimension 1");
    for (size_t i = 0; i + 1 < cores.size(); ++i)
        if (cores[i].r != cores[i + 1].l || cores[i].r == 0)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "tensor train bond dimension mismatch at bond " + std::to_string(i));
}

std::vector<double> Tci2::evaluate(const uint32_t* idx, size_t n_pts)
{
    fill_wait();
    check_tt_chain(cores);
    std::vector<double> out(n_pts);
    if (n_pts == 0) return out;
    for (size_t p = 0; p < n_pts; ++p)
        for (size_t s = 0; s < n_; ++s)
            if (idx[p * n_ + s] >= local_dims[s]) throw Error(T4A_GPU_INVALID_ARGUMENT, "evaluate: index out of bounds");
    hipStream_t st = eng.stream();
    std::vector<TtCoreDesc> desc(n_);
    int max_bond = 1;
    for (size_t s = 0; s < n_; ++s) {
        desc[s].data = cores[s].buf.get();
        desc[s].l = (int)cores[s].l;
        desc[s].d = (int)cores[s].s;
        desc[s].r = (int)cores[s].r;
        max_bond = std::max(max_bond, std::max(desc[s].l, desc[s].r));
    }
    d_coredesc_.reserve(n_);
    d_idx_.reserve(n_pts * n_);
    d_vals_.reserve(n_pts);
    T4A_HIP(hipMemcpyAsync(d_coredesc_.get(), desc.data(), n_ * sizeof(TtCoreDesc), hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(d_idx_.get(), idx, n_pts * n_ * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    T4A_HIP(hipStreamSynchronize(st));
    tt_evaluate_launch(d_coredesc_.get(), (int)n_, max_bond, d_idx_.get(), (int)n_pts, d_vals_.get(), st);
    T4A_HIP(hipMemcpyAsync(out.data(), d_vals_.get(), n_pts * sizeof(double), hipMemcpyDeviceToHost, st));
    T4A_HIP(hipStreamSynchronize(st));
    T4A_HIP(hipGetLastError());
    return out;
}

double Tci2::sum() // simplett/src/traits.rs:231-275 (host-side: O(n chi^2 d), not on the hot path)
{
    check_tt_chain(cores);
    std::vector<double> cur;
    for (size_t site = 0; site < n_; ++site) {
        size_t d3[3];
        std::vector<double> t = site_tensor_host(site, d3);
        const size_t L = d3[0], S = d3[1], R = d3[2];
        if (site == 0) {
            cur.assign(R, 0.0);
            for (size_t s = 0; s < S; ++s)
                for (size_t r = 0; r < R; ++r) cur[r] = cur[r] + t[0 + L * (s + S * r)];
            continue;
        }
        std::vector<double> site_sum(L * R, 0.0);
        for (size_t l = 0; l < L; ++l)
            for (size_t s = 0; s < S; ++s)
                for (size_t r = 0; r < R; ++r) site_sum[l * R + r] = site_sum[l * R + r] + t[l + L * (s + S * r)];
        std::vector<double> next(R, 0.0);
        for (size_t r = 0; r < R; ++r) {
            double sum = 0.0;
            for (size_t l = 0; l < L; ++l) sum = sum + cur[l] * site_sum[l * R + r];
            next[r] = sum;
        }
        cur.swap(next);
    }
    return cur[0];
}

// =================================================================================================
// global pivot search + optimisation loop
// =================================================================================================
// DefaultGlobalPivotFinder::find_global_pivots (tensorci/src/globalpivot.rs:160-219).  All candidate points
// of all searches are independent (the reference resets the coordinate after each 1-D scan), so f and the
// TT are evaluated in two batches.  RNG: rand 0.9 StdRng + random_range(0..d), restated in stdrng.hpp (initial points are drawn
// search by search, site by site, exactly as globalpivot.rs:174-180 does).
std::vector<std::vector<uint32_t>> Tci2::find_global_pivots(double abs_tol, const TCI2Options& o, StdRng& rng)
{
    std::vector<std::vector<uint32_t>> found;
    if (o.nsearch == 0) return found;
    std::vector<std::vector<uint32_t>> initial(o.nsearch, std::vector<uint32_t>(n_));
    for (auto& p : initial)
        for (size_t s = 0; s < n_; ++s) p[s] = (uint32_t)rng.random_range(local_dims[s]);
    std::vector<uint32_t> idx;
    for (const auto& point : initial)
        for (size_t p = 0; p < n_; ++p)
            for (size_t v = 0; v < local_dims[p]; ++v) {
                const size_t base = idx.size();
                idx.insert(idx.end(), point.begin(), point.end());
                idx[base + p] = (uint32_t)v;
            }
    const size_t npts = idx.size() / n_;
    std::vector<double> fv = eval_points_host(idx, npts);
    std::vector<double> tv;
    try {
        tv = evaluate(idx.data(), npts);
    } catch (const Error&) {
        tv.assign(npts, 0.0); // `.unwrap_or(T::zero())`
    }
    size_t q = 0;
    for (const auto& point : initial) {
        double best_error = 0.0;
        std::vector<uint32_t> best_point = point;
        for (size_t p = 0; p < n_; ++p)
            for (size_t v = 0; v < local_dims[p]; ++v, ++q) {
                const double diff = fv[q] - tv[q];
                const double err = std::sqrt(diff * diff);
                if (err > best_error) {
                    best_error = err;
                    best_point.assign(idx.begin() + q * n_, idx.begin() + (q + 1) * n_);
                }
            }
        if (best_error > abs_tol * o.tol_margin_global_search) found.push_back(best_point);
    }
    if (found.size() > o.max_nglobal_pivot) found.resize(o.max_nglobal_pivot);
    return found;
}

static bool convergence_criterion(const std::vector<size_t>& ranks, const std::vector<double>& errors,
                                  const std::vector<size_t>& nglobal, double tolerance, size_t max_bond_dim,
                                  size_t ncheck_history, int& out) // tensorci2.rs:1407-1437
{
    if (errors.size() < ncheck_history) return false;
    const size_t n = errors.size();
    bool errors_converged = true, no_global = true, at_max = true;
    size_t min_rank = std::numeric_limits<size_t>::max();
    for (size_t i = n - ncheck_history; i < n; ++i) {
        if (!(errors[i] < tolerance)) errors_converged = false;
        if (nglobal[i] != 0) no_global = false;
        if (!(ranks[i] >= max_bond_dim)) at_max = false;
        min_rank = std::min(min_rank, ranks[i]);
    }
    const bool rank_stable = (min_rank == ranks[n - 1]);
    if (at_max) {
        out = T4A_GPU_TCI2_MAX_BOND_DIMENSION;
        return true;
    }
    if (errors_converged && no_global && rank_stable) {
        out = T4A_GPU_TCI2_CONVERGED;
        return true;
    }
    return false;
}

// optimize_with_finder (tensorci2.rs:1626-1802)
// T4A_OPT_PROF=1: host time of the pieces of an iteration (microseconds, accumulated; printed by optimize())
static double g_opt_seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
struct OptSeg {
    int k;
    std::chrono::steady_clock::time_point t0;
    explicit OptSeg(int k_) : k(k_), t0(std::chrono::steady_clock::now()) {}
    ~OptSeg() { g_opt_seg[k] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
};

// optimize_with_finder (tensorci2.rs:1626-1802) as a resumable run: opt_begin, then per iteration opt_iter_start (prelude + the
// half-sweep enqueued as a bond chain, without waiting) and opt_iter_finish (the rest of the iteration), then opt_end.  optimize()
// drives one handle; optimize_group() drives up to eight in lock-step from one host thread — every handle's chain runs on its
// own XCD, so their bond updates overlap on the device while the host only ever waits for the slowest.
void Tci2::opt_begin(OptRun& r)
{
    const TCI2Options& options = r.options;

    options.validate();
    fn_.require("tci2");
    if (rank() == 0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "TensorCI2 state must contain at least one pivot before optimization");
    // pipelined mode (keep_site_tensors): a fill left in flight by the previous call keeps running beside the bond
    // updates below (they only touch the index sets); it is completed by the next fill or the first reader of a core
    if (!keep_site_tensors) fill_wait();
    ranks_hist.clear();
    errors_hist.clear();
    r.nglobal_hist.clear();
    termination = T4A_GPU_TCI2_MAX_ITERATIONS;
    r.rng.reseed(options.has_seed ? options.seed : 0x1234567ull); // (no seed: OS entropy in the reference — any stream will do)
    r.pending_fill = false;
    r.iter = 0;
    r.done = false;
    r.small_complete = false;
    // small problems: the whole loop in ONE launch (tci2_small.hip); it may finish the call, run the first iterations and hand the
    // rest back, or decline
    if (small_engine_run(r) && r.small_complete) return;
    fill_presize(options); // (bounded rank, built-in functor: site tensors and fill workspaces get their final size now)
}

bool Tci2::opt_iter_start(OptRun& r, bool defer_launch)
{
    const TCI2Options& options = r.options;
    if (r.done || r.iter >= options.max_iter) return false;
    const size_t iter = r.iter;
    (void)iter;
        r.norm = (options.normalize_error && max_sample_value > 0.0) ? max_sample_value : 1.0;
        r.abs_tol = options.tolerance * r.norm;
        bool is_forward = true;
        if (options.sweep_strategy == 1) is_forward = false;
        else if (options.sweep_strategy == 2) is_forward = (iter % 2 == 0);

        // extras of this iteration: the sets at the start of the previous one (:1675-1685); then the sets as they are now join
        // the history (:1686-1689).  After a bond chain only codes and counts are current: the entry carries those.
        long ext_idx = (!options.strictly_nested && !history.empty()) ? (long)history.size() - 1 : -1;
        {
            OptSeg seg_(0);
            HistEntry cur;
            cur.serial = ++chain_.hist_serial;
            if (chain_.digits_stale) {
                cur.digits_valid = false;
                cur.cap = chain_.cap;
                cur.is.resize(n_);
                cur.js.resize(n_);
                for (size_t p = 0; p < n_; ++p) {
                    cur.is[p].width = i_set[p].width;
                    cur.is[p].count = i_set[p].count;
                    cur.js[p].width = j_set[p].width;
                    cur.js[p].count = j_set[p].count;
                }
                const ChainTab mi = chain_mirror(chain_.mcur, 0), mj = chain_mirror(chain_.mcur, 1);
                cur.code.resize(2 * n_ * chain_.cap);
                std::memcpy(cur.code.data(), mi.code, n_ * chain_.cap * sizeof(uint64_t));
                std::memcpy(cur.code.data() + n_ * chain_.cap, mj.code, n_ * chain_.cap * sizeof(uint64_t));
            } else {
                cur.is = i_set;
                cur.js = j_set;
            }
            history.push_back(std::move(cur));
            // only the most recent snapshot is ever read (:1677-1681): cap the memory held by older ones
            if (history.size() > 2) {
                history.erase(history.begin());
                if (ext_idx >= 0) --ext_idx;
            }
        }
        {
            OptSeg seg_(1);
            invalidate_site_tensors();
            flush_pivot_errors();
            last_sweep_shapes.assign(n_ - 1, {0, 0, 0});
            prep_.valid = false;
            invalidate_fill_cache();
        }
        const bool fill_ahead = fn_.builtin() && options.pivot_search == 0;
        // built-in functor, full pivot search: the whole half-sweep is enqueued at once (tci2_chain.hip) ...
        r.is_forward = is_forward;
        r.ext_idx = ext_idx;
        r.fill_ahead = fill_ahead;
        {
            OptSeg seg_(2);
            r.chained = chain_enqueue(is_forward, options, ext_idx, true, !defer_launch);
        }
    return true;
}

void Tci2::opt_iter_finish(OptRun& r)
{
    const TCI2Options& options = r.options;
    const size_t iter = r.iter;
    const double norm = r.norm, abs_tol = r.abs_tol;
    const bool is_forward = r.is_forward, chained = r.chained, fill_ahead = r.fill_ahead;
    const long ext_idx = r.ext_idx;
    do { // (one pass; `break` = the convergence exit of the reference's loop)
        {
            OptSeg seg_(3);
            opt_issue_pending_fill(r);
        }
        if (chained) {
            OptSeg seg_(4);
            chain_finish(options);
        } else {
            // ... otherwise bond by bond
            sync_digits();
            std::vector<IndexSet> no_i(n_), no_j(n_);
            for (size_t p = 0; p < n_; ++p) {
                no_i[p].width = p;
                no_j[p].width = n_ - p - 1;
            }
            if (ext_idx >= 0) hist_digits(history[(size_t)ext_idx]);
            const std::vector<IndexSet>& extra_i = ext_idx >= 0 ? history[(size_t)ext_idx].is : no_i;
            const std::vector<IndexSet>& extra_j = ext_idx >= 0 ? history[(size_t)ext_idx].js : no_j;
            if (is_forward) {
                for (size_t b = 0; b + 1 < n_; ++b) {
                    // bond b+1 reads J_{b+2}, which bond b does not touch: its column side can be built ahead
                    prefetch_.wanted = b + 2 < n_;
                    prefetch_.bond = b + 1;
                    prefetch_.cols = true;
                    prefetch_.extra = prefetch_.wanted ? &extra_j[b + 1] : nullptr;
                    // site b-1 only reads I_{b-1}, J_{b-1}, I_b: final since bond b-1 (forward bonds write I_{b+1}, J_b)
                    prefetch_.fill_site = (fill_ahead && b >= 1) ? (long)(b - 1) : -1;
                    update_pivots(b, true, options, extra_i[b + 1], extra_j[b]);
                }
            } else {
                for (size_t b = n_ - 1; b-- > 0;) {
                    // bond b-1 reads I_{b-1}, which bond b does not touch: its row side can be built ahead
                    prefetch_.wanted = b > 0;
                    prefetch_.bond = b - 1;
                    prefetch_.cols = false;
                    prefetch_.extra = prefetch_.wanted ? &extra_i[b] : nullptr;
                    // site b+2 reads I_{b+2}, J_{b+2}, I_{b+3}: final since bond b+1 (backward bonds write I_{b+1}, J_b)
                    prefetch_.fill_site = (fill_ahead && b + 2 < n_) ? (long)(b + 2) : -1;
                    update_pivots(b, false, options, extra_i[b + 1], extra_j[b]);
                }
            }
        }
        prefetch_.wanted = false;
        prefetch_.fill_site = -1;
        prep_.valid = false;
        // the cores are not needed by the next half-sweep unless the global pivot search evaluates the TT
        const bool fill_async = options.nsearch == 0 && !options.strictly_nested;
        if (chained && chain_.digits_stale && fill_async) {
            // this fill's accumulators (out of the mirror), descriptors and launches go out after the NEXT iteration's chain
            // has been enqueued (or after the loop): the device is busy with that chain while the host prepares the fill
            r.pending_fill = true;
        } else {
            fill_run(FillOptions{fill_async, /*trust_cache*/ fill_ahead && !chained, /*no_main_sync*/ chained && chain_.digits_stale});
        }
        OptSeg seg_tail_(5);
        const double error = max_bond_error();
        errors_hist.push_back(error / norm);

        std::vector<std::vector<uint32_t>> gp = find_global_pivots(abs_tol, options, r.rng);
        // invalidates the site tensors even for an empty list (tensorci2.rs:707-708) unless the caller opted out
        if (!(gp.empty() && keep_site_tensors)) add_global_pivots(gp);
        r.nglobal_hist.push_back(gp.size());
        ranks_hist.push_back(rank());
        if (options.verbosity > 0)
            std::printf("iteration = %zu, rank = %zu, error = %.2e, maxsamplevalue = %.2e, nglobalpivot = %zu\n", iter + 1,
                        rank(), error / norm, max_sample_value, gp.size());
        int reason;
        if (convergence_criterion(ranks_hist, errors_hist, r.nglobal_hist, options.tolerance, options.max_bond_dim_or_max(),
                                  options.ncheck_history, reason)) {
            termination = reason;
            r.done = true;
            break;
        }
    } while (false);
    ++r.iter;
}

void Tci2::opt_end(OptRun& r)
{
    const TCI2Options& options = r.options;
    const bool final_sweep1site = r.final_sweep1site;
    opt_issue_pending_fill(r); // the last iteration's fill
    // the cores of the last iteration are complete (deferred solve errors surface here); in pipelined mode the wait
    // is left to the first reader (site_tensor*, evaluate, export_site_tensors_async, the next fill)
    if (!keep_site_tensors || final_sweep1site) fill_wait();
    if (final_sweep1site) { // :1781-1794
        const double norm = (options.normalize_error && max_sample_value > 0.0) ? max_sample_value : 1.0;
        const double abs_tol = options.tolerance * norm;
        sweep1site(true, 1e-14, abs_tol, options.max_bond_dim_or_max(), true);
    }
}

void Tci2::optimize(const TCI2Options& options, bool final_sweep1site)
{
    OptRun r;
    r.options = options;
    r.final_sweep1site = final_sweep1site;
    static const bool prof = std::getenv("T4A_OPT_PROF") != nullptr; // host time between two chains (stderr, once per call)
    try {
        opt_begin(r);
        if (!prof) {
            while (opt_iter_start(r)) opt_iter_finish(r);
        } else {
            double t_start = 0.0, t_finish = 0.0;
            const double wait0 = g_chain_wait_seconds;
            size_t iters = 0;
            for (;;) {
                const auto ta = std::chrono::steady_clock::now();
                if (!opt_iter_start(r)) break;
                const auto tb = std::chrono::steady_clock::now();
                opt_iter_finish(r);
                const auto tc = std::chrono::steady_clock::now();
                t_start += std::chrono::duration<double>(tb - ta).count();
                t_finish += std::chrono::duration<double>(tc - tb).count();
                ++iters;
            }
            std::fprintf(stderr, "[t4a] optimize segments (us per iteration): history snapshot %.1f, invalidate + flush %.1f, chain_enqueue %.1f | pending fill %.1f, chain_finish incl. the wait %.1f, error + global pivots + convergence %.1f\n",
                         g_opt_seg[0] / std::max<size_t>(iters, 1), g_opt_seg[1] / std::max<size_t>(iters, 1), g_opt_seg[2] / std::max<size_t>(iters, 1), g_opt_seg[3] / std::max<size_t>(iters, 1),
                         g_opt_seg[4] / std::max<size_t>(iters, 1), g_opt_seg[5] / std::max<size_t>(iters, 1));
            for (double& v : g_opt_seg) v = 0.0;
            const double wait = g_chain_wait_seconds - wait0;
            std::fprintf(stderr, "[t4a] optimize: %zu iterations: start (prepare + launch the chain) %.1f us, finish %.1f us of which waiting for the device %.1f us, per iteration\n",
                         iters, 1e6 * t_start / std::max<size_t>(iters, 1), 1e6 * t_finish / std::max<size_t>(iters, 1), 1e6 * wait / std::max<size_t>(iters, 1));
        }
        opt_end(r);
    } catch (...) {
        chain_abort(); // (a chain may be in flight: the error came from the fill of the previous iteration)
        throw;
    }
}

// Up to eight handles (one XCD each) optimised in lock-step by the calling thread: every iteration first enqueues all the bond
// chains, then finishes them one after the other.  Results are exactly those of optimize() on every handle.
void Tci2::optimize_group(const std::vector<Tci2*>& hs, const TCI2Options& options, bool final_sweep1site)
{
    if (hs.empty()) return;
    if (hs.size() > 8) throw Error(T4A_GPU_INVALID_ARGUMENT, "optimize_group: at most eight handles (one per XCD)");
    for (size_t i = 0; i < hs.size(); ++i) {
        if (!hs[i]) throw Error(T4A_GPU_NULL_POINTER, "optimize_group: null handle");
        for (size_t j = 0; j < i; ++j)
            if (hs[j] == hs[i]) throw Error(T4A_GPU_INVALID_ARGUMENT, "optimize_group: a handle appears twice");
        hs[i]->eng.set_xcc((int)i); // (distinct XCDs: a handle keeps its reservation from enqueue to finish)
    }
    std::vector<OptRun> runs(hs.size());
    try {
    for (size_t i = 0; i < hs.size(); ++i) {
        runs[i].options = options;
        runs[i].final_sweep1site = final_sweep1site;
        runs[i].allow_small = false; // (the group's point is eight chains side by side: one engine launch per handle would serialise them)
        hs[i]->opt_begin(runs[i]);
    }
    static const bool prof = std::getenv("T4A_GROUP_PROF") != nullptr; // host time per phase, printed once per call
    double t_start = 0.0, t_launch = 0.0, t_finish = 0.0, t_fill = 0.0;
    const double wait0 = g_chain_wait_seconds;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    size_t iters = 0;
    for (;;) {
        std::vector<size_t> active;
        std::vector<Tci2*> chained;
        const auto ta = now();
        for (size_t i = 0; i < hs.size(); ++i)
            if (hs[i]->opt_iter_start(runs[i], true)) {
                active.push_back(i);
                if (runs[i].chained) chained.push_back(hs[i]);
            }
        if (active.empty()) break;
        const auto tb = now();
        chain_group_launch(chained); // one chain of launches for all of them (or one each when they do not line up)
        const auto tc = now();
        // the chained handles first, the group's leader first of all: it holds the chip until its chain has completed, and a
        // handle on the per-bond path needs an XCD of its own
        for (size_t i : active)
            if (runs[i].chained) hs[i]->opt_issue_pending_fill(runs[i]); // (all of them while the group's chain still runs)
        t_fill += secs(tc, now());
        for (size_t i : active)
            if (runs[i].chained) hs[i]->opt_iter_finish(runs[i]);
        for (size_t i : active)
            if (!runs[i].chained) hs[i]->opt_iter_finish(runs[i]);
        const auto td = now();
        t_start += secs(ta, tb);
        t_launch += secs(tb, tc);
        t_finish += secs(tc, td);
        ++iters;
    }
    if (prof)
        std::fprintf(stderr, "[t4a] optimize_group: %zu handles, %zu iterations: start %.2f ms, launch %.2f ms, finish %.2f ms (of which issuing the previous iteration's fills %.2f ms, waiting for the device %.2f ms)\n",
                     hs.size(), iters, 1e3 * t_start, 1e3 * t_launch, 1e3 * t_finish, 1e3 * t_fill, 1e3 * (g_chain_wait_seconds - wait0));
    // the last iteration's fills of ALL handles first (each on its own fill stream), then the waits: handle by handle the device
    // idled while the host issued the next handle's dozen launches
    for (size_t i = 0; i < hs.size(); ++i) hs[i]->opt_issue_pending_fill(runs[i]);
    for (size_t i = 0; i < hs.size(); ++i) hs[i]->opt_end(runs[i]);
    } catch (...) {
        for (Tci2* h : hs) h->chain_abort(); // (the leader's abort waits for the group's stream and gives the chip back)
        throw;
    }
}

// crossinterpolate2 (tensorci2.rs:1513-1563)
void Tci2::crossinterpolate2(std::vector<std::vector<uint32_t>> pivots, const TCI2Options& options)
{
    options.validate();
    fn_.require("tci2");
    if (pivots.empty()) pivots.push_back(std::vector<uint32_t>(n_, 0));
    add_global_pivots(pivots);
    std::vector<uint32_t> flat;
    for (const auto& p : pivots) flat.insert(flat.end(), p.begin(), p.end());
    std::vector<double> vals = eval_points_host(flat, pivots.size());
    for (double v : vals) {
        const double a = std::sqrt(v * v);
        if (a > max_sample_value) max_sample_value = a;
    }
    if (max_sample_value < 1e-30) throw Error(T4A_GPU_INVALID_ARGUMENT, "Initial pivots have zero function values");
    optimize(options, true);
}

} // namespace t4a
