// contraction.hip — Contraction<f64> on the device (see contraction.hpp).  Index bookkeeping (validation, unique halves, the split)
// is host integer work; every floating-point operation runs in the gfx950 kernels of kernels_contraction.hip (environments) and
// kernels_tt.hip (pairing).
#include "contraction.hpp"
#include "globalsearch.hpp"
#include "tci2.hpp"

#include <algorithm>
#include <climits>
#include <string>

namespace t4a {

namespace {
constexpr int ENV_MAX_BLOCKS = 8192;          // workgroups of an environment launch whose working set is in the LDS
constexpr int ENV_MAX_BLOCKS_SCRATCH = 1024;  // ... in global scratch
constexpr size_t ENV_SCRATCH_MAX_BYTES = (size_t)2 << 30;
} // namespace

MpoContraction::MpoContraction(Mpo& a, Mpo& b)
{
    if (a.len() != b.len())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO length mismatch: expected " + std::to_string(a.len()) + ", got " + std::to_string(b.len()));
    n_ = a.len();
    for (size_t i = 0; i < n_; ++i)
        if (a.sd[i][1] != b.sd[i][0])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Shared shape mismatch at site " + std::to_string(i) + ": MPO A has site_dim_2=" +
                                                      std::to_string(a.sd[i][1]) + ", MPO B has site_dim_1=" + std::to_string(b.sd[i][0]));
    sites_.resize(n_);
    for (size_t i = 0; i < n_; ++i) {
        const DevCore& x = a.tt.cores[i];
        const DevCore& y = b.tt.cores[i];
        sites_[i] = Site{x.l, a.sd[i][0], a.sd[i][1], x.r, y.l, b.sd[i][1], y.r};
        // an environment, the K intermediates of a site step and the strides of the two site tensors are int in the kernels
        const unsigned long long lim = INT_MAX;
        const unsigned long long k = a.sd[i][1];
        if ((unsigned long long)x.l * y.l > lim || (unsigned long long)x.r * y.r > lim || k * x.r * y.l > lim || k * x.l * y.r > lim)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Contraction: site " + std::to_string(i) + " has a bond pair of more than INT_MAX entries");
        if ((unsigned long long)x.l * a.sd[i][0] * k * x.r > lim || (unsigned long long)y.l * k * b.sd[i][1] * y.r > lim)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Contraction: site " + std::to_string(i) + " holds more than INT_MAX elements");
    }
    a_ = std::make_unique<Mpo>(a.tt.cores, a.tt.eng.stream(), a.sd);
    b_ = std::make_unique<Mpo>(b.tt.cores, b.tt.eng.stream(), b.sd);
    b_->tt.eng.sync(); // b_'s cores are read on a_'s stream from here on
    eng_ = &a_->tt.eng;
}

MpoContraction::~MpoContraction()
{
    if (eng_) (void)hipStreamSynchronize(eng_->stream()); // (a matrix a consumer never waited for)
    for (hipEvent_t e : {ev_upload_, ev_consumer_, ev_done_})
        if (e) (void)hipEventDestroy(e);
}

std::vector<std::array<size_t, 2>> MpoContraction::result_site_dims() const
{
    std::vector<std::array<size_t, 2>> d(n_);
    for (size_t i = 0; i < n_; ++i) d[i] = {sites_[i].s1, sites_[i].s2};
    return d;
}

std::vector<size_t> MpoContraction::fused_local_dims() const
{
    std::vector<size_t> d(n_);
    for (size_t i = 0; i < n_; ++i) d[i] = sites_[i].s1 * sites_[i].s2;
    return d;
}

std::array<size_t, 2> MpoContraction::left_dims(size_t n) const
{
    if (n > n_) throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid operation: Site " + std::to_string(n) + " is out of range [0, " + std::to_string(n_) + "]");
    if (n == 0) return {1, 1};
    return {sites_[n - 1].ra, sites_[n - 1].rb};
}

std::array<size_t, 2> MpoContraction::right_dims(size_t n) const
{
    if (n > n_) throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid operation: Site " + std::to_string(n) + " is out of range [0, " + std::to_string(n_) + "]");
    if (n == n_) return {1, 1};
    return {sites_[n].la, sites_[n].lb};
}

void MpoContraction::validate_indices(const uint32_t* idx, size_t n_pts, size_t first, size_t last) const
{
    for (size_t p = 0; p < n_pts; ++p)
        for (size_t s = first; s < last; ++s) {
            const uint32_t i = idx[2 * n_ * p + 2 * s], j = idx[2 * n_ * p + 2 * s + 1];
            if (i >= sites_[s].s1 || j >= sites_[s].s2)
                throw Error(T4A_GPU_INVALID_ARGUMENT, "Index out of bounds: index " + std::to_string(std::max(i, j)) + " at site " +
                                                          std::to_string(s) + " (max: " + std::to_string(std::max(sites_[s].s1, sites_[s].s2)) + ")");
        }
}

void MpoContraction::validate_halves(const uint32_t* packed, size_t n_items, size_t first, size_t last) const
{
    const size_t w = last - first;
    for (size_t p = 0; p < n_items; ++p)
        for (size_t s = first; s < last; ++s) {
            const uint32_t i = packed[2 * w * p + 2 * (s - first)], j = packed[2 * w * p + 2 * (s - first) + 1];
            if (i >= sites_[s].s1 || j >= sites_[s].s2)
                throw Error(T4A_GPU_INVALID_ARGUMENT, "Index out of bounds: index " + std::to_string(std::max(i, j)) + " at site " +
                                                          std::to_string(s) + " (max: " + std::to_string(std::max(sites_[s].s1, sites_[s].s2)) + ")");
        }
}

void MpoContraction::upload_descs()
{
    if (descs_uploaded_) return; // the operands are this object's own copies: their addresses never change
    std::vector<ContractionSiteDesc> desc(n_);
    for (size_t s = 0; s < n_; ++s) {
        const Site& t = sites_[s];
        ContractionSiteDesc& d = desc[s];
        d = ContractionSiteDesc{};
        d.A = a_->tt.cores[s].buf.get();
        d.B = b_->tt.cores[s].buf.get();
        d.la = (int)t.la;
        d.s1 = (int)t.s1;
        d.k = (int)t.k;
        d.ra = (int)t.ra;
        d.lb = (int)t.lb;
        d.s2 = (int)t.s2;
        d.rb = (int)t.rb;
    }
    d_desc_.reserve(std::max<size_t>(n_, 1));
    T4A_HIP(hipMemcpyAsync(d_desc_.get(), desc.data(), n_ * sizeof(ContractionSiteDesc), hipMemcpyHostToDevice, eng_->stream()));
    eng_->sync(); // `desc` is pageable host memory
    descs_uploaded_ = true;
}

// The working set of one workgroup over sites [first, last): 2 * env_cap + t_cap doubles.  Returns the global scratch it lives in
// (nullptr: it fits the LDS) and how many workgroups to launch.
double* MpoContraction::working_set(size_t n_items, int& env_cap, int& t_cap, int& blocks, size_t first, size_t last, bool left)
{
    size_t env = 1, t = 1;
    for (size_t s = first; s < last; ++s) {
        const Site& x = sites_[s];
        env = std::max({env, x.la * x.lb, x.ra * x.rb});
        t = std::max(t, left ? x.k * x.ra * x.lb : x.k * x.la * x.rb);
    }
    env_cap = (int)env;
    t_cap = (int)t;
    const size_t ws = 2 * env + t;
    if (ws <= CONTRACTION_LDS_DOUBLES) {
        blocks = (int)std::min<size_t>(n_items, ENV_MAX_BLOCKS);
        return nullptr;
    }
    if (ws * sizeof(double) > ENV_SCRATCH_MAX_BYTES)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Contraction: a site step needs a working set of " + std::to_string(ws) +
                                                  " doubles (2 * max(la*lb) + K * lb * ra), above the limit of " +
                                                  std::to_string(ENV_SCRATCH_MAX_BYTES / sizeof(double)));
    blocks = (int)std::min<size_t>({n_items, (size_t)ENV_MAX_BLOCKS_SCRATCH, ENV_SCRATCH_MAX_BYTES / (ws * sizeof(double))});
    // one buffer per direction: growing a buffer that the other launch of the same call still uses would hand it back to the pool
    DevBuf<double>& buf = left ? d_scratch_l_ : d_scratch_r_;
    buf.reserve((size_t)blocks * ws);
    return buf.get();
}

void MpoContraction::launch_left(size_t n, const uint32_t* d_idx, size_t n_items, double* d_out, size_t ld)
{
    int env_cap, t_cap, blocks;
    double* scratch = working_set(n_items, env_cap, t_cap, blocks, 0, n, true);
    contraction_env_left_launch(d_desc_.get(), (int)n, d_idx, (int)n_items, d_out, (int)ld, env_cap, t_cap, scratch, blocks, eng_->stream());
}

void MpoContraction::launch_right(size_t n, const uint32_t* d_idx, size_t n_items, double* d_out, size_t ld)
{
    int env_cap, t_cap, blocks;
    double* scratch = working_set(n_items, env_cap, t_cap, blocks, n, n_, false);
    contraction_env_right_launch(d_desc_.get(), (int)n_, (int)n, d_idx, (int)n_items, d_out, (int)ld, env_cap, t_cap, scratch, blocks,
                                 eng_->stream());
}

namespace {
void check_batch(size_t n_pts)
{
    if (n_pts > (size_t)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, "Contraction: more than INT_MAX points in one call");
}
} // namespace

// environments of every point (no unique map: a caller who wants shared halves computed once uses evaluate_many)
void MpoContraction::environments(bool left, size_t n, const uint32_t* idx, size_t n_pts, double* out)
{
    const std::array<size_t, 2> dims = left ? left_dims(n) : right_dims(n);
    const size_t len = dims[0] * dims[1];
    const bool trivial = left ? n == 0 : n == n_;
    if (trivial) { // contraction.rs:269-273, :332-336
        std::fill(out, out + n_pts, 1.0);
        return;
    }
    if (n_pts == 0) return;
    check_batch(n_pts);
    const size_t first = left ? 0 : n, last = left ? n : n_, w = last - first;
    validate_indices(idx, n_pts, first, last);
    std::vector<uint32_t> h(n_pts * 2 * w);
    for (size_t p = 0; p < n_pts; ++p) std::copy_n(idx + 2 * n_ * p + 2 * first, 2 * w, h.data() + p * 2 * w);
    hipStream_t st = eng_->stream();
    upload_descs();
    d_idx_.reserve(h.size());
    d_envl_.reserve(n_pts * len);
    T4A_HIP(hipMemcpyAsync(d_idx_.get(), h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (left)
        launch_left(n, d_idx_.get(), n_pts, d_envl_.get(), len);
    else
        launch_right(n, d_idx_.get(), n_pts, d_envl_.get(), len);
    T4A_HIP(hipMemcpyAsync(out, d_envl_.get(), n_pts * len * sizeof(double), hipMemcpyDeviceToHost, st));
    eng_->sync();
    T4A_HIP(hipGetLastError());
}

void MpoContraction::evaluate(const uint32_t* idx, size_t n_pts, double* out)
{
    std::lock_guard<std::mutex> lock(mu_);
    if (n_ == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO is empty"); // contraction.rs:194-196
    environments(true, n_, idx, n_pts, out);                            // the last right bonds are 1: one value per point
    n_evaluated_ += n_pts;
}

void MpoContraction::evaluate_left(size_t n, const uint32_t* idx, size_t n_pts, double* out, size_t dims2[2])
{
    std::lock_guard<std::mutex> lock(mu_);
    const std::array<size_t, 2> d = left_dims(n);
    dims2[0] = d[0];
    dims2[1] = d[1];
    environments(true, n, idx, n_pts, out);
}

void MpoContraction::evaluate_right(size_t n, const uint32_t* idx, size_t n_pts, double* out, size_t dims2[2])
{
    std::lock_guard<std::mutex> lock(mu_);
    const std::array<size_t, 2> d = right_dims(n);
    dims2[0] = d[0];
    dims2[1] = d[1];
    environments(false, n, idx, n_pts, out);
}

size_t MpoContraction::evaluate_many(const uint32_t* idx, size_t n_pts, size_t split, double* out)
{
    std::lock_guard<std::mutex> lock(mu_);
    const size_t n = n_;
    if (n_pts == 0) return split; // cache.rs:563-565
    if (n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO is empty");
    check_batch(n_pts);
    validate_indices(idx, n_pts, 0, n);
    if (split == 0) split = find_split_heuristic(idx, n, 2, n_pts);
    if (split == 0 || split > n)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid split position: " + std::to_string(split) + " (n_sites=" + std::to_string(n) + ")");
    hipStream_t st = eng_->stream();
    UniqueMap ul, ur;
    ul.build(idx, 2 * n, 0, 2 * split, n_pts);
    ur.build(idx, 2 * n, 2 * split, 2 * (n - split), n_pts);
    const size_t nl = ul.first.size(), nr = ur.first.size();
    const size_t wl = 2 * split, wr = 2 * (n - split);
    std::vector<uint32_t> hl(nl * wl), hr(std::max<size_t>(nr * wr, 1));
    for (size_t u = 0; u < nl; ++u) std::copy_n(idx + (size_t)ul.first[u] * 2 * n, wl, hl.data() + u * wl);
    for (size_t u = 0; u < nr; ++u) std::copy_n(idx + (size_t)ur.first[u] * 2 * n + wl, wr, hr.data() + u * wr);
    const size_t len = split < n ? sites_[split].la * sites_[split].lb : 1; // entries of an environment at the split
    upload_descs();
    d_idx_.reserve(hl.size() + hr.size());
    d_il_.reserve(n_pts);
    d_ir_.reserve(n_pts);
    d_envl_.reserve(std::max<size_t>(nl * len, 1));
    d_envr_.reserve(std::max<size_t>(nr * len, 1));
    d_vals_.reserve(n_pts);
    uint32_t* d_hl = d_idx_.get();
    uint32_t* d_hr = d_hl + hl.size();
    T4A_HIP(hipMemcpyAsync(d_hl, hl.data(), hl.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (wr) T4A_HIP(hipMemcpyAsync(d_hr, hr.data(), nr * wr * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(d_il_.get(), ul.which.data(), n_pts * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(d_ir_.get(), ur.which.data(), n_pts * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    launch_left(split, d_hl, nl, d_envl_.get(), len);
    if (wr)
        launch_right(split, d_hr, nr, d_envr_.get(), len);
    else
        fill_launch(d_envr_.get(), nr * len, 1.0, st); // evaluate_right(len, .) == [[1]]
    // value[p] = sum_{a, b} L[il[p]][a, b] R[ir[p]][a, b]: both are column-major over the same bond pair
    tt_env_dot_launch(d_envl_.get(), d_envr_.get(), (int)len, (int)len, d_il_.get(), d_ir_.get(), n_pts, d_vals_.get(), st);
    T4A_HIP(hipMemcpyAsync(out, d_vals_.get(), n_pts * sizeof(double), hipMemcpyDeviceToHost, st));
    eng_->sync();
    T4A_HIP(hipGetLastError());
    n_evaluated_ += n_pts;
    return split;
}

void MpoContraction::evaluate_fused(const uint32_t* fidx, size_t n_sites, size_t n_pts, double* out)
{
    if (n_sites != n_)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid operation: Expected " + std::to_string(n_) + " index pairs, got " + std::to_string(n_sites));
    std::vector<uint32_t> idx(2 * n_ * n_pts);
    for (size_t p = 0; p < n_pts; ++p)
        for (size_t s = 0; s < n_; ++s) {
            const uint32_t f = fidx[n_ * p + s], s1 = (uint32_t)sites_[s].s1;
            idx[2 * n_ * p + 2 * s] = f % s1; // an f beyond s1 * s2 gives j >= s2: refused by validate_indices
            idx[2 * n_ * p + 2 * s + 1] = f / s1;
        }
    evaluate_many(idx.data(), n_pts, 0, out);
}

void MpoContraction::matrix_locked(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, bool fused,
                                   double* d_out, size_t ld, bool transposed, hipStream_t consumer)
{
    const size_t n = n_;
    if (n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO is empty");
    if (cut > n) throw Error(T4A_GPU_INVALID_ARGUMENT, "Invalid split position: " + std::to_string(cut) + " (n_sites=" + std::to_string(n) + ")");
    if (n_rows == 0 || n_cols == 0) return;
    check_batch(n_rows);
    check_batch(n_cols);
    if (n_cols > CONTRACTION_PAIR_MAX_COLS)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Contraction: more than " + std::to_string(CONTRACTION_PAIR_MAX_COLS) + " columns in one matrix");
    if (ld < (transposed ? n_cols : n_rows)) throw Error(T4A_GPU_INVALID_ARGUMENT, "Contraction: the leading dimension is below the matrix");
    const size_t wl = 2 * cut, wr = 2 * (n - cut);
    const size_t nl = n_rows * wl, nr = n_cols * wr;
    // the staging buffer is read by the previous call's upload: the one host wait of a call, normally over long ago
    if (upload_pending_) {
        T4A_HIP(hipEventSynchronize(ev_upload_));
        upload_pending_ = false;
    }
    h_halves_.reserve(std::max<size_t>(nl + nr, 1));
    uint32_t* hl = h_halves_.get();
    uint32_t* hr = hl + nl;
    if (fused) {
        auto decode = [this](const uint32_t* f, size_t n_items, size_t first, size_t last, uint32_t* dst) {
            const size_t w = last - first;
            for (size_t p = 0; p < n_items; ++p)
                for (size_t s = first; s < last; ++s) {
                    const uint32_t v = f[w * p + (s - first)], s1 = (uint32_t)sites_[s].s1;
                    dst[2 * w * p + 2 * (s - first)] = v % s1; // an f beyond s1 * s2 gives j >= s2: refused by validate_halves
                    dst[2 * w * p + 2 * (s - first) + 1] = v / s1;
                }
        };
        decode(rows, n_rows, 0, cut, hl);
        decode(cols, n_cols, cut, n, hr);
    } else {
        if (nl) std::copy_n(rows, nl, hl);
        if (nr) std::copy_n(cols, nr, hr);
    }
    validate_halves(hl, n_rows, 0, cut);
    validate_halves(hr, n_cols, cut, n);
    // entries of an environment at the cut (the outer bonds of an MPO are 1: K == 1 at cut == 0 and cut == len)
    const size_t K = cut < n ? sites_[cut].la * sites_[cut].lb : sites_[n - 1].ra * sites_[n - 1].rb;
    hipStream_t st = eng_->stream();
    const bool foreign = consumer != nullptr && consumer != st;
    if (!ev_upload_) {
        T4A_HIP(hipEventCreateWithFlags(&ev_upload_, hipEventDisableTiming));
        T4A_HIP(hipEventCreateWithFlags(&ev_consumer_, hipEventDisableTiming));
        T4A_HIP(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming));
    }
    upload_descs();
    d_idx_.reserve(std::max<size_t>(nl + nr, 1));
    d_envl_.reserve(n_rows * K);
    d_envr_.reserve(n_cols * K);
    if (nl + nr) {
        T4A_HIP(hipMemcpyAsync(d_idx_.get(), hl, (nl + nr) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        T4A_HIP(hipEventRecord(ev_upload_, st));
        upload_pending_ = true;
    }
    if (wl)
        launch_left(cut, d_idx_.get(), n_rows, d_envl_.get(), K);
    else
        fill_launch(d_envl_.get(), n_rows * K, 1.0, st); // evaluate_left(0, .) == [[1]]
    if (wr)
        launch_right(cut, d_idx_.get() + nl, n_cols, d_envr_.get(), K);
    else
        fill_launch(d_envr_.get(), n_cols * K, 1.0, st); // evaluate_right(len, .) == [[1]]
    if (foreign) { // d_out may still be read or written by what the consumer enqueued before this call
        T4A_HIP(hipEventRecord(ev_consumer_, consumer));
        T4A_HIP(hipStreamWaitEvent(st, ev_consumer_, 0));
    }
    contraction_pair_launch(d_envl_.get(), (int)n_rows, d_envr_.get(), (int)n_cols, (int)K, d_out, ld, transposed, st);
    T4A_HIP(hipGetLastError());
    if (foreign) {
        T4A_HIP(hipEventRecord(ev_done_, st));
        T4A_HIP(hipStreamWaitEvent(consumer, ev_done_, 0));
    }
    n_evaluated_ += n_rows * n_cols;
}

void MpoContraction::evaluate_matrix(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, double* d_out,
                                     size_t ld, bool transposed, hipStream_t consumer)
{
    std::lock_guard<std::mutex> lock(mu_);
    matrix_locked(cut, rows, n_rows, cols, n_cols, false, d_out, ld, transposed, consumer);
}

void MpoContraction::fill_matrix(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, double* d_out,
                                 size_t ld, bool transposed, hipStream_t consumer)
{
    std::lock_guard<std::mutex> lock(mu_);
    matrix_locked(cut, rows, n_rows, cols, n_cols, true, d_out, ld, transposed, consumer);
}

void MpoContraction::evaluate_matrix_host(size_t cut, const uint32_t* rows, size_t n_rows, const uint32_t* cols, size_t n_cols, double* out)
{
    std::lock_guard<std::mutex> lock(mu_);
    const size_t total = n_rows * n_cols;
    d_vals_.reserve(std::max<size_t>(total, 1));
    matrix_locked(cut, rows, n_rows, cols, n_cols, false, d_vals_.get(), n_rows, false, nullptr);
    if (total == 0) return;
    // through pinned memory: a copy straight into the caller's pageable buffer was measured at 30 ms for 2 MiB (the kernels take 0.35 ms)
    h_vals_.reserve(total);
    T4A_HIP(hipMemcpyAsync(h_vals_.get(), d_vals_.get(), total * sizeof(double), hipMemcpyDeviceToHost, eng_->stream()));
    eng_->sync();
    T4A_HIP(hipGetLastError());
    std::copy_n(h_vals_.get(), total, out);
}

namespace {
// t4a_gpu_batch_eval_fn over an MpoContraction*
int64_t contraction_thunk(void* ctx, const uint32_t* idx, size_t n_sites, size_t n_pts, double* out)
{
    try {
        static_cast<MpoContraction*>(ctx)->evaluate_fused(idx, n_sites, n_pts, out);
        return (int64_t)n_pts;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}
} // namespace

std::unique_ptr<Mpo> mpo_contract_tci(Mpo& a, Mpo& b, const TCI2Options& options, std::vector<std::vector<uint32_t>> initial_pivots,
                                      double info[4], bool device_source)
{
    MpoContraction c(a, b);
    const size_t n = c.len();
    const std::vector<size_t> dims = c.fused_local_dims();
    options.validate();
    Tci2 tci(dims); // refuses fewer than two sites (tensorci2.rs:381-385)
    if (device_source)
        tci.set_source(&c);
    else
        tci.set_callback(&contraction_thunk, &c);
    if (initial_pivots.empty()) { // optfirstpivot.rs: a local search for a large first pivot, started at the all-zero index
        const SearchFn f = [&c](const uint32_t* idx, size_t n_sites, size_t n_pts, double* out) { c.evaluate_fused(idx, n_sites, n_pts, out); };
        initial_pivots.push_back(opt_first_pivot(f, dims, std::vector<uint32_t>(n, 0), 1000));
    }
    tci.crossinterpolate2(std::move(initial_pivots), options);
    tci.fill_wait();
    std::unique_ptr<Mpo> out = std::make_unique<Mpo>(tci.cores, tci.eng.stream(), c.result_site_dims()); // the cores are the fused train
    info[0] = (double)tci.termination;
    info[1] = (double)tci.rank();
    info[2] = (double)c.n_evaluated();
    info[3] = tci.errors_hist.empty() ? 0.0 : tci.errors_hist.back();
    return out;
}

} // namespace t4a
