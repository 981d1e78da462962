// batch_compress.hip — the host side of batch_compress.hpp: the plan (shapes only), the driver that queues both sweeps of every batched
// chain without a host round trip, and the entry points the C ABI and the partitioned MPO call.  Per call the batched part issues
// n - 1 right-step launches, n - 1 left-step launches, one read-back of all ranks and flags and ONE stream synchronisation; the driver
// counts them itself (CompressManyStats) so that a test can hold them against the plan.
#include "batch_compress.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>

namespace t4a {

namespace {

using Shape3 = std::array<size_t, 3>; // (l, fused s, r)

struct Bounds {
    std::vector<size_t> k; // after the right sweep: k[n] = 1, k[i] = min(l_i, s_i k[i+1]); k[0] = 1
    std::vector<size_t> b; // of the result: b[0] = 1, b[i+1] = min(k[i+1], b[i] s_i, cap)
    bool inside = false;   // n >= 2 and every k[i] <= BATCH_COMPRESS_BMAX
};

Bounds bounds_of(const std::vector<Shape3>& f, size_t cap)
{
    const size_t n = f.size();
    Bounds o;
    o.k.assign(n + 1, 1);
    o.b.assign(n + 1, 1);
    if (n == 0) return o;
    for (size_t i = n - 1; i >= 1; --i) o.k[i] = std::min(f[i][0], f[i][1] * o.k[i + 1]);
    o.inside = n >= 2;
    for (size_t i = 0; i + 1 < n; ++i) {
        size_t v = std::min(o.k[i + 1], o.b[i] * f[i][1]);
        if (cap != 0) v = std::min(v, cap);
        o.b[i + 1] = v;
        if (o.k[i + 1] > (size_t)BATCH_COMPRESS_BMAX) o.inside = false;
    }
    return o;
}

void check_options(const MpoContractionOptions& opt)
{
    if (opt.method == MpoFactorizeMethod::RSVD)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "Factorization failed: RSVD factorization not yet implemented"); // as svd_rank
}

// which items take the kernels
std::vector<int> pick(const std::vector<Bounds>& bd, CompressRoute route)
{
    std::vector<int> batched(bd.size(), 0);
    if (route == CompressRoute::Serial) return batched;
    size_t inside = 0, largest = 0;
    for (const Bounds& b : bd)
        if (b.inside) {
            ++inside;
            largest = std::max(largest, *std::max_element(b.k.begin(), b.k.end()));
        }
    if (route == CompressRoute::Auto && inside < BATCH_COMPRESS_AUTO_MIN_ITEMS && largest > BATCH_COMPRESS_AUTO_SMALL_BOND) return batched;
    for (size_t k = 0; k < bd.size(); ++k) batched[k] = bd[k].inside;
    return batched;
}

std::vector<Shape3> shape_of(const std::vector<DevCore>& c)
{
    std::vector<Shape3> f(c.size());
    for (size_t i = 0; i < c.size(); ++i) f[i] = {c[i].l, c[i].s, c[i].r};
    return f;
}

// Both sweeps of the items `which` (indices into `in`) on the kernels; out[k] receives the result of in[which[k]].  Returns the position in
// `which` of the first item with a non-finite entry, or -1.
long long run_batched(Engine& eng, const std::vector<const std::vector<DevCore>*>& in, const std::vector<size_t>& which,
                      const std::vector<Bounds>& bd, const MpoContractionOptions& opt, std::vector<std::vector<DevCore>>& out,
                      CompressManyStats& stats)
{
    const size_t nb = which.size(), n = in[which[0]]->size(), steps = n - 1;
    const hipStream_t st = eng.stream();
    // the arena: per item Y[0 .. n-2] (the site with R^T absorbed), Z[1 .. n-1] (Q^T), Z'[1 .. n-2] (the site with diag(S) Vt absorbed), scratch
    std::vector<size_t> offY(nb * n, 0), offZ(nb * n, 0), offA(nb * n, 0), offS(nb, 0);
    size_t total = 0;
    for (size_t q = 0; q < nb; ++q) {
        const std::vector<DevCore>& c = *in[which[q]];
        const Bounds& B = bd[which[q]];
        size_t scratch = 0;
        for (size_t i = 0; i < n; ++i) {
            const size_t sr = c[i].s * B.k[i + 1];
            if (i + 1 < n) {
                offY[q * n + i] = total;
                total += c[i].l * sr;
                scratch = std::max(scratch, B.b[i] * sr + (size_t)(BATCH_COMPRESS_BMAX * BATCH_COMPRESS_BMAX + 3 * BATCH_COMPRESS_BMAX)); // left step i
            }
            if (i >= 1) {
                offZ[q * n + i] = total;
                total += B.k[i] * sr;
                scratch = std::max(scratch, sr * c[i].l + sr * B.k[i] + 3 * B.k[i]); // right step i
            }
            if (i >= 1 && i + 1 < n) {
                offA[q * n + i] = total;
                total += B.b[i] * sr;
            }
        }
        offS[q] = total;
        total += scratch;
    }
    DevBuf<double> arena;
    arena.reserve(std::max<size_t>(total, 1));
    double* base = arena.get();
    // the results, allocated at their bounds: the kernels write them compactly, the shapes are set after the read-back
    out.clear();
    out.resize(nb);
    for (size_t q = 0; q < nb; ++q) {
        const std::vector<DevCore>& c = *in[which[q]];
        const Bounds& B = bd[which[q]];
        out[q].resize(n);
        for (size_t i = 0; i < n; ++i) out[q][i] = DevCore::make(B.b[i], c[i].s, i + 1 < n ? B.b[i + 1] : 1);
    }
    // job tables and the read-back go through pinned memory: the copies below are asynchronous for the host too
    PinBuf<BcRightJob> rj_buf;
    PinBuf<BcLeftJob> lj_buf;
    PinBuf<int> h_buf;
    rj_buf.reserve(steps * nb);
    lj_buf.reserve(steps * nb);
    h_buf.reserve(nb * steps + nb);
    BcRightJob* rj = rj_buf.get();
    BcLeftJob* lj = lj_buf.get();
    int* h = h_buf.get();
    for (size_t q = 0; q < nb; ++q) {
        const std::vector<DevCore>& c = *in[which[q]];
        const Bounds& B = bd[which[q]];
        for (size_t step = 0; step < steps; ++step) { // right step `step` works on site i = n - 1 - step
            const size_t i = n - 1 - step;
            BcRightJob& j = rj[step * nb + q];
            j = BcRightJob{};
            j.T = i == n - 1 ? c[i].buf.get() : base + offY[q * n + i];
            j.P = c[i - 1].buf.get();
            j.Z = base + offZ[q * n + i];
            j.Y = base + offY[q * n + i - 1];
            j.scratch = base + offS[q];
            j.l = (int)c[i].l;
            j.sr = (int)(c[i].s * B.k[i + 1]);
            j.pl = (int)(c[i - 1].l * c[i - 1].s);
            j.k = (int)B.k[i];
        }
        for (size_t i = 0; i < steps; ++i) {
            BcLeftJob& j = lj[i * nb + q];
            j = BcLeftJob{};
            j.C = base + (i == 0 ? offY[q * n] : offA[q * n + i]);
            j.Nx = base + offZ[q * n + i + 1];
            j.U = out[q][i].buf.get();
            j.Nout = i + 1 == n - 1 ? out[q][n - 1].buf.get() : base + offA[q * n + i + 1];
            j.scratch = base + offS[q];
            j.s = (int)c[i].s;
            j.r = (int)B.k[i + 1];
            j.rest = (int)(c[i + 1].s * B.k[i + 2]);
            j.lb = (int)B.b[i];
            j.prev = i == 0 ? -1 : (int)(q * steps + i - 1);
            j.cur = (int)(q * steps + i);
        }
    }
    DevBuf<BcRightJob> d_rj;
    DevBuf<BcLeftJob> d_lj;
    DevBuf<int> d_state; // ranks[nb * steps], then flags[nb]
    d_rj.reserve(steps * nb);
    d_lj.reserve(steps * nb);
    d_state.reserve(nb * steps + nb);
    int* d_ranks = d_state.get();
    int* d_flags = d_ranks + nb * steps;
    T4A_HIP(hipMemsetAsync(d_state.get(), 0, sizeof(int) * (nb * steps + nb), st));
    T4A_HIP(hipMemcpyAsync(d_rj.get(), rj, steps * nb * sizeof(BcRightJob), hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(d_lj.get(), lj, steps * nb * sizeof(BcLeftJob), hipMemcpyHostToDevice, st));
    for (size_t step = 0; step < steps; ++step) {
        bc_right_step_launch(d_rj.get() + step * nb, (int)nb, d_flags, st);
        ++stats.launches;
    }
    for (size_t i = 0; i < steps; ++i) {
        bc_left_step_launch(d_lj.get() + i * nb, (int)nb, d_ranks, d_flags, opt.tolerance, (int)std::min<size_t>(opt.max_bond_dim, 1u << 30), st);
        ++stats.launches;
    }
    T4A_HIP(hipGetLastError());
    T4A_HIP(hipMemcpyAsync(h, d_state.get(), sizeof(int) * (nb * steps + nb), hipMemcpyDeviceToHost, st));
    eng.sync(); // the one synchronisation of the batched part: job tables, arena and read-back are all behind it
    ++stats.syncs;
    long long bad = -1;
    for (size_t q = 0; q < nb; ++q) {
        if (h[nb * steps + q]) {
            if (bad < 0) bad = (long long)q;
            continue;
        }
        const std::vector<DevCore>& c = *in[which[q]];
        size_t l = 1;
        for (size_t i = 0; i < n; ++i) {
            const size_t r = i + 1 < n ? (size_t)h[q * steps + i] : 1;
            out[q][i].reshape(l, c[i].s, r);
            l = r;
        }
    }
    return bad;
}

[[noreturn]] void throw_item(size_t k, const std::string& what) { throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many: item " + std::to_string(k) + ": " + what); }

// the results of every item, in order; the inputs are only read
std::vector<std::vector<DevCore>> run(Engine& eng, const std::vector<const std::vector<DevCore>*>& in, const MpoContractionOptions& opt,
                                      CompressRoute route, CompressManyStats* stats)
{
    check_options(opt);
    CompressManyStats local;
    const size_t N = in.size();
    std::vector<std::vector<DevCore>> res(N);
    if (N == 0) {
        if (stats) *stats = local;
        return res;
    }
    const size_t n = in[0]->size();
    std::vector<Bounds> bd(N);
    for (size_t k = 0; k < N; ++k) {
        if (in[k]->size() != n)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many: item " + std::to_string(k) + " has " + std::to_string(in[k]->size()) +
                                                      " sites, item 0 has " + std::to_string(n));
        bd[k] = bounds_of(shape_of(*in[k]), opt.max_bond_dim);
    }
    const std::vector<int> batched = pick(bd, route);
    std::vector<size_t> which;
    for (size_t k = 0; k < N; ++k)
        if (batched[k]) which.push_back(k);
    size_t first_bad = N;
    if (!which.empty()) {
        std::vector<std::vector<DevCore>> out;
        const long long bad = run_batched(eng, in, which, bd, opt, out, local);
        if (bad >= 0) first_bad = which[(size_t)bad];
        for (size_t q = 0; q < which.size(); ++q) res[which[q]] = std::move(out[q]);
        local.n_batched = which.size();
    }
    // the other items, one after the other on the serial stage (an item past a flagged one is never reported: the lowest index is)
    for (size_t k = 0; k < first_bad; ++k) {
        if (batched[k]) continue;
        res[k] = clone_cores(*in[k], eng.stream());
        ++local.n_serial;
        if (n <= 1) continue;
        try {
            mpo_compress_cores(eng, res[k], opt);
        } catch (const Error& e) {
            if (e.code == T4A_GPU_INVALID_ARGUMENT) throw_item(k, e.what());
            throw;
        }
    }
    if (first_bad < N) throw_item(first_bad, "SVD computation failed: non-finite input");
    if (local.n_serial) eng.sync(); // (copies of short chains may be in flight; the batched part has ended synced)
    if (stats) *stats = local;
    return res;
}

} // namespace

CompressManyPlan compress_many_plan(const std::vector<std::vector<std::array<size_t, 4>>>& shapes, const MpoContractionOptions& opt,
                                    CompressRoute route)
{
    if (shapes.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many: the list is empty");
    check_options(opt);
    const size_t N = shapes.size(), n = shapes[0].size();
    CompressManyPlan p;
    std::vector<Bounds> bd(N);
    for (size_t k = 0; k < N; ++k) {
        if (shapes[k].size() != n)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many: item " + std::to_string(k) + " has " + std::to_string(shapes[k].size()) +
                                                      " sites, item 0 has " + std::to_string(n));
        try {
            mpo_validate_dims(shapes[k]);
        } catch (const Error& e) {
            throw_item(k, e.what());
        }
        std::vector<Shape3> f(n);
        for (size_t i = 0; i < n; ++i) f[i] = {shapes[k][i][0], shapes[k][i][1] * shapes[k][i][2], shapes[k][i][3]};
        bd[k] = bounds_of(f, opt.max_bond_dim);
        p.bonds.push_back(bd[k].b);
        p.qr_bonds.push_back(bd[k].k);
    }
    p.batched = pick(bd, route);
    for (int b : p.batched) p.n_batched += b;
    if (p.n_batched) {
        p.launches = 2 * (n - 1);
        p.syncs = 1;
    }
    return p;
}

void compress_many_cores(Engine& eng, const std::vector<std::vector<DevCore>*>& chains, const MpoContractionOptions& opt, CompressRoute route,
                         CompressManyStats* stats)
{
    std::vector<const std::vector<DevCore>*> in(chains.begin(), chains.end());
    std::vector<std::vector<DevCore>> res = run(eng, in, opt, route, stats);
    for (size_t k = 0; k < chains.size(); ++k) *chains[k] = std::move(res[k]);
}

std::vector<std::unique_ptr<Mpo>> mpo_compress_many(const std::vector<Mpo*>& items, const MpoContractionOptions& opt, CompressRoute route,
                                                    CompressManyStats* stats)
{
    if (items.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many: the list is empty");
    for (size_t k = 0; k < items.size(); ++k)
        if (!items[k]) throw Error(T4A_GPU_NULL_POINTER, "compress_many: item " + std::to_string(k) + " is null");
    for (size_t k = 1; k < items.size(); ++k)
        if (items[k]->len() != items[0]->len())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many: item " + std::to_string(k) + " has " + std::to_string(items[k]->len()) +
                                                      " sites, item 0 has " + std::to_string(items[0]->len()));
    check_options(opt);
    std::vector<const std::vector<DevCore>*> in;
    for (Mpo* m : items) {
        m->tt.eng.sync(); // every operand is read on the first one's stream
        in.push_back(&m->tt.cores);
    }
    Engine& eng = items[0]->tt.eng;
    std::vector<std::vector<DevCore>> res = run(eng, in, opt, route, stats);
    std::vector<std::unique_ptr<Mpo>> out;
    for (size_t k = 0; k < items.size(); ++k) out.push_back(std::make_unique<Mpo>(std::move(res[k]), items[k]->sd));
    return out;
}

std::unique_ptr<Mpo> mpo_compress(Mpo& a, const MpoContractionOptions& opt)
{
    check_options(opt);
    Engine& eng = a.tt.eng;
    std::vector<DevCore> cores = clone_cores(a.tt.cores, eng.stream());
    if (cores.size() > 1) mpo_compress_cores(eng, cores, opt);
    eng.sync();
    return std::make_unique<Mpo>(std::move(cores), a.sd);
}

void compress_many_time(Engine& eng, const std::vector<std::vector<DevCore>>& chains, const MpoContractionOptions& opt, size_t reps, double ms[2])
{
    if (reps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many_time: reps must be positive");
    if (chains.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "compress_many_time: no chain");
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    double total[2] = {0.0, 0.0};
    for (size_t r = 0; r < reps + 1; ++r)
        for (int which = 0; which < 2; ++which) {
            std::vector<std::vector<DevCore>> copy(chains.size());
            std::vector<std::vector<DevCore>*> ptr;
            for (size_t t = 0; t < chains.size(); ++t) {
                copy[t] = clone_cores(chains[t], eng.stream());
                ptr.push_back(&copy[t]);
            }
            eng.sync();
            const clk::time_point t0 = clk::now();
            if (which == 0) {
                for (auto& c : copy) mpo_compress_cores(eng, c, opt);
            } else {
                compress_many_cores(eng, ptr, opt, CompressRoute::Batched, nullptr);
            }
            if (r) total[which] += since(t0); // the first round warms up
        }
    ms[0] = total[0] / reps;
    ms[1] = total[1] / reps;
}

} // namespace t4a
