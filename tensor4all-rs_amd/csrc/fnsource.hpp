// fnsource.hpp — the function being interpolated, as every driver sees it: a built-in device functor with its integer weight tables
// (include/t4a_testfunctions.h) or a host batch callback.  One copy of the argument checks, the accumulator loop, the host evaluation
// of a built-in and the count check of a callback, shared by Tci2, TreeTci, the patching driver and the C ABI.
#pragma once

#include <utility>

#include "common.hpp"
#include "kernels.hpp"

namespace t4a {

// A list of multi-indices of fixed width, flat: entry k = d[k*width .. (k+1)*width)
struct IndexSet {
    size_t width = 0;
    size_t count = 0;
    std::vector<uint32_t> d;
    const uint32_t* at(size_t k) const { return d.data() + k * width; }
    void push(const uint32_t* v)
    {
        d.insert(d.end(), v, v + width);
        ++count;
    }
    void clear()
    {
        d.clear();
        count = 0;
    }
    bool contains(const uint32_t* v) const
    {
        if (width == 0) return count > 0;
        for (size_t k = 0; k < count; ++k)
            if (std::memcmp(at(k), v, width * sizeof(uint32_t)) == 0) return true;
        return false;
    }
};

enum class FnKind { None, Builtin, Callback };

struct FnSource {
    std::vector<size_t> offset; // per site into one weight table
    size_t total = 0;           // entries of one weight table: sum of the local dimensions
    FnDevice dev{};
    std::vector<uint64_t> weights; // dev.n_acc * total
    t4a_gpu_batch_eval_fn cb = nullptr;
    void* cb_ctx = nullptr;

    explicit FnSource(const std::vector<size_t>& local_dims) : offset(local_dims.size())
    {
        for (size_t s = 0; s < local_dims.size(); ++s) {
            offset[s] = total;
            total += local_dims[s];
        }
    }

    FnKind kind() const { return kind_; }
    bool builtin() const { return kind_ == FnKind::Builtin; }

    void set_builtin(int fid, int n_acc, const double* params, const uint64_t* w)
    {
        if (fid < 0 || fid >= T4A_FN_COUNT) throw Error(T4A_GPU_INVALID_ARGUMENT, "unknown built-in function id");
        if (n_acc < 1 || n_acc > T4A_FN_MAX_ACC) throw Error(T4A_GPU_INVALID_ARGUMENT, "n_acc out of range");
        dev.fid = fid;
        dev.n_acc = n_acc;
        std::memcpy(dev.params, params, sizeof(double) * T4A_FN_MAX_PARAMS);
        weights.assign(w, w + (size_t)n_acc * total);
        kind_ = FnKind::Builtin;
    }

    void set_callback(t4a_gpu_batch_eval_fn f, void* ctx)
    {
        if (!f) throw Error(T4A_GPU_NULL_POINTER, "callback is null");
        cb = f;
        cb_ctx = ctx;
        kind_ = FnKind::Callback;
    }

    // `name`: the handle family in the C ABI ("tci2", "treetci")
    void require(const char* name) const
    {
        if (kind_ == FnKind::None)
            throw Error(T4A_GPU_INVALID_ARGUMENT, std::string("no function set: call t4a_gpu_") + name + "_set_builtin_function or _set_callback");
    }

    // acc[e * n_acc + k] = sum over the digits s of entry e of weights[k][site_off[s] + digit]: site_off[s] is the weight offset of the
    // site digit s lives on (contiguous sites from `first`: offset.data() + first)
    void accumulate(const IndexSet& set, const size_t* site_off, std::vector<uint64_t>& acc) const
    {
        const int K = dev.n_acc;
        acc.assign(set.count * (size_t)K, 0);
        for (size_t e = 0; e < set.count; ++e) {
            const uint32_t* v = set.at(e);
            for (int k = 0; k < K; ++k) {
                uint64_t a = 0;
                const uint64_t* w = weights.data() + (size_t)k * total;
                for (size_t s = 0; s < set.width; ++s) a += w[site_off[s] + v[s]];
                acc[e * K + k] = a;
            }
        }
    }

    // the built-in at n_pts full multi-indices (idx[p * n_sites + s]), evaluated on the host
    void host_values(const uint32_t* idx, size_t n_pts, double* out) const
    {
        const size_t n = offset.size();
        for (size_t p = 0; p < n_pts; ++p) {
            uint64_t acc[T4A_FN_MAX_ACC] = {0, 0, 0, 0};
            for (int k = 0; k < dev.n_acc; ++k) {
                const uint64_t* w = weights.data() + (size_t)k * total;
                for (size_t s = 0; s < n; ++s) acc[k] += w[offset[s] + idx[p * n + s]];
            }
            out[p] = t4a_fn_value(dev.fid, acc, dev.params);
        }
    }

    // the callback at n_pts multi-indices; anything but n_pts values back is an error: "<who> returned G values for N <what>"
    void call(const uint32_t* idx, size_t n_sites, size_t n_pts, double* out, const char* who, const char* what) const
    {
        call(cb, cb_ctx, idx, n_sites, n_pts, out, who, what);
    }
    static void call(t4a_gpu_batch_eval_fn f, void* ctx, const uint32_t* idx, size_t n_sites, size_t n_pts, double* out, const char* who,
                     const char* what)
    {
        const int64_t got = f(ctx, idx, n_sites, n_pts, out);
        if (got < 0 || (size_t)got != n_pts)
            throw Error(T4A_GPU_CALLBACK_ERROR,
                        std::string(who) + " returned " + std::to_string(got) + " values for " + std::to_string(n_pts) + " " + what);
    }

private:
    FnKind kind_ = FnKind::None;
};

// Row and column accumulators -> one pinned block -> one asynchronous copy to the device; returns the two device pointers.  The
// pinned block is free again after the next synchronisation of `st`.
inline std::pair<const uint64_t*, const uint64_t*> stage_accumulator_pair(const std::vector<uint64_t>& ra, const std::vector<uint64_t>& rb,
                                                                          PinBuf<uint64_t>& pin, DevBuf<uint64_t>& dev, hipStream_t st)
{
    const size_t need = ra.size() + rb.size();
    pin.reserve(need);
    dev.reserve(need);
    std::memcpy(pin.get(), ra.data(), ra.size() * sizeof(uint64_t));
    std::memcpy(pin.get() + ra.size(), rb.data(), rb.size() * sizeof(uint64_t));
    T4A_HIP(hipMemcpyAsync(dev.get(), pin.get(), need * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    return {dev.get(), dev.get() + ra.size()};
}

} // namespace t4a
