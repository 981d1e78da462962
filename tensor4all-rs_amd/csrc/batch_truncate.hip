// batch_truncate.hip — the host side of batch_truncate.hpp: the plan (shapes only), the two phases of a call (TruncateBatch) and the entry
// point the C ABI calls.  Per call the batched part issues n - 1 QR-step launches and 2 (n - 1) SVD-step launches, one read-back of all
// ranks and flags, and one stream synchronisation — two when the caller reads the norms between the phases.  The driver counts them
// itself (TruncateManyStats) so that a test can hold them against the plan.
#include "batch_truncate.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>

namespace t4a {

namespace {

using Shape3 = std::array<size_t, 3>; // (l, fused s, r)

struct Bounds {
    std::vector<size_t> k;  // after the QR sweep: k[0] = 1, k[i+1] = min(k[i] s_i, r_{i+1}); k[n] = 1
    std::vector<size_t> b2; // after the leftward sweep: b2[n] = 1, b2[i] = min(k[i], s_i b2[i+1], cap)
    std::vector<size_t> b3; // of the result: b3[0] = 1, b3[i+1] = min(b2[i+1], b3[i] s_i, cap)
    bool inside = false;    // n >= 2 and every k[i] <= BATCH_COMPRESS_BMAX
};

Bounds bounds_of(const std::vector<Shape3>& f, size_t cap)
{
    const size_t n = f.size();
    Bounds o;
    o.k.assign(n + 1, 1);
    o.b2.assign(n + 1, 1);
    o.b3.assign(n + 1, 1);
    if (n == 0) return o;
    o.inside = n >= 2;
    for (size_t i = 0; i + 1 < n; ++i) {
        o.k[i + 1] = std::min(o.k[i] * f[i][1], f[i][2]);
        if (o.k[i + 1] > (size_t)BATCH_COMPRESS_BMAX) o.inside = false;
    }
    for (size_t i = n - 1; i >= 1; --i) {
        size_t v = std::min(o.k[i], f[i][1] * o.b2[i + 1]);
        if (cap != 0) v = std::min(v, cap);
        o.b2[i] = v;
    }
    for (size_t i = 0; i + 1 < n; ++i) {
        size_t v = std::min(o.b2[i + 1], o.b3[i] * f[i][1]);
        if (cap != 0) v = std::min(v, cap);
        o.b3[i + 1] = v;
    }
    return o;
}

// which items take the kernels: the rule of compress_many (batch_compress.hpp).  Measured for this call: at 16, 64 and
// 256 items of bonds 16 and 64 the kernels win 5 to 14 times, all on the batched side of the rule; below 16 items of a bond above 16
// nothing was measured, so Auto stays serial there.
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

[[noreturn]] void throw_item(size_t k, const std::string& what) { throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: item " + std::to_string(k) + ": " + what); }
const char* const NONFINITE = "SVD computation failed: non-finite input";

using clk = std::chrono::steady_clock;
double since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

} // namespace

struct TruncateBatch::Impl {
    Engine& eng;
    std::vector<const std::vector<DevCore>*> in;
    bool trace, timing;
    size_t N = 0, n = 0, nb = 0, steps = 0;
    std::vector<Bounds> bd; // with cap = 0: the rules arrive in phase 2
    std::vector<int> batched;
    std::vector<size_t> which;
    // the batched part
    DevBuf<double> arena, d_norm, d_sv;
    std::vector<size_t> offQ, offY, offZ, offP, offA, offS; // per item and site: after QR (Q, with R absorbed Y), leftward (Z, P), rightward (A)
    DevBuf<int> d_state;                                     // ranks[nb * 2 * steps], then flags[nb]
    PinBuf<double> h_norm;
    PinBuf<BtQrJob> qj_buf;
    DevBuf<BtQrJob> d_qj;
    // the serial part
    std::vector<std::vector<DevCore>> serial; // per item (empty for batched ones): the chain, canonical onto the last site after phase 1
    std::vector<int> serial_bad;
    bool canonical = false;

    Impl(Engine& e, std::vector<const std::vector<DevCore>*> i, bool tr, bool tm) : eng(e), in(std::move(i)), trace(tr), timing(tm) {}
    int* d_ranks() { return d_state.get(); }
    int* d_flags() { return d_state.get() + nb * 2 * steps; }
    // bond j (1 .. n - 1) of item q after the leftward (sweep 0) or the rightward (sweep 1) sweep
    int rank_index(size_t q, int sweep, size_t j) const { return (int)(q * 2 * steps + (size_t)sweep * steps + (j - 1)); }
};

TruncateBatch::TruncateBatch(Engine& eng, std::vector<const std::vector<DevCore>*> in, CompressRoute route, bool trace_, bool timing)
    : p_(new Impl(eng, std::move(in), trace_, timing))
{
    Impl& p = *p_;
    p.N = p.in.size();
    p.n = p.N ? p.in[0]->size() : 0;
    p.bd.resize(p.N);
    for (size_t k = 0; k < p.N; ++k) {
        if (p.in[k]->size() != p.n)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: item " + std::to_string(k) + " has " + std::to_string(p.in[k]->size()) +
                                                      " sites, item 0 has " + std::to_string(p.n));
        p.bd[k] = bounds_of(shape_of(*p.in[k]), 0);
    }
    p.batched = pick(p.bd, route);
    for (size_t k = 0; k < p.N; ++k)
        if (p.batched[k]) p.which.push_back(k);
    p.nb = p.which.size();
    p.steps = p.n ? p.n - 1 : 0;
    p.serial.resize(p.N);
    p.serial_bad.assign(p.N, 0);
    norm2_.assign(p.N, 0.0);
    stats.n_batched = p.nb;
    stats.n_serial = p.N - p.nb;
    trace.norm2.assign(p.N, 0.0);
    trace.ranks.resize(p.N);
    trace.sv.resize(p.N);
}

TruncateBatch::~TruncateBatch() = default;

void TruncateBatch::canonicalize(bool read_norms)
{
    Impl& p = *p_;
    const size_t n = p.n, nb = p.nb, steps = p.steps;
    const hipStream_t st = p.eng.stream();
    clk::time_point t0 = clk::now();
    size_t first_bad = p.N; // the lowest flagged item of the batched part
    if (nb) {
        // the arena at the bounds without a cap: per item Q[0 .. n-2], Y[1 .. n-1], Z[1 .. n-1], P[0 .. n-2], A[1 .. n-2], scratch
        p.offQ.assign(nb * n, 0), p.offY.assign(nb * n, 0), p.offZ.assign(nb * n, 0), p.offP.assign(nb * n, 0), p.offA.assign(nb * n, 0);
        p.offS.assign(nb, 0);
        size_t total = 0;
        const size_t fixed = (size_t)(BATCH_COMPRESS_BMAX * BATCH_COMPRESS_BMAX + 3 * BATCH_COMPRESS_BMAX);
        for (size_t q = 0; q < nb; ++q) {
            const std::vector<DevCore>& c = *p.in[p.which[q]];
            const Bounds& B = p.bd[p.which[q]];
            size_t scratch = 0;
            for (size_t i = 0; i < n; ++i) {
                const size_t ls = B.k[i] * c[i].s;
                if (i + 1 < n) {
                    p.offQ[q * n + i] = total;
                    total += ls * B.k[i + 1];
                    p.offP[q * n + i] = total;
                    total += ls * B.b2[i + 1];
                    scratch = std::max(scratch, ls * c[i].r + ls * B.k[i + 1] + 3 * B.k[i + 1]);      // QR step i
                    scratch = std::max(scratch, 2 * (B.b3[i] * c[i].s) * B.b2[i + 1] + fixed);         // rightward step i
                }
                if (i >= 1) {
                    p.offY[q * n + i] = total;
                    total += B.k[i] * c[i].s * c[i].r;
                    p.offZ[q * n + i] = total;
                    total += B.b2[i] * c[i].s * B.b2[i + 1];
                    scratch = std::max(scratch, 2 * (c[i].s * B.b2[i + 1]) * B.k[i] + fixed);          // leftward step i
                }
                if (i >= 1 && i + 1 < n) {
                    p.offA[q * n + i] = total;
                    total += B.b3[i] * c[i].s * B.b2[i + 1];
                }
            }
            p.offS[q] = total;
            total += scratch;
        }
        p.arena.reserve(std::max<size_t>(total, 1));
        double* base = p.arena.get();
        p.d_norm.reserve(nb);
        p.h_norm.reserve(nb);
        p.d_state.reserve(nb * 2 * steps + nb);
        p.qj_buf.reserve(steps * nb); // the job table stays alive into phase 2: a call with given rules does not wait here
        BtQrJob* qj = p.qj_buf.get();
        for (size_t q = 0; q < nb; ++q) {
            const std::vector<DevCore>& c = *p.in[p.which[q]];
            const Bounds& B = p.bd[p.which[q]];
            for (size_t i = 0; i < steps; ++i) {
                BtQrJob& j = qj[i * nb + q];
                j = BtQrJob{};
                j.T = i == 0 ? c[0].buf.get() : base + p.offY[q * n + i];
                j.Nx = c[i + 1].buf.get();
                j.Q = base + p.offQ[q * n + i];
                j.Y = base + p.offY[q * n + i + 1];
                j.scratch = base + p.offS[q];
                j.norm2 = i + 1 == steps ? p.d_norm.get() + q : nullptr;
                j.ls = (int)(B.k[i] * c[i].s);
                j.r = (int)c[i].r;
                j.rest = (int)(c[i + 1].s * c[i + 1].r);
                j.k = (int)B.k[i + 1];
            }
        }
        DevBuf<BtQrJob>& d_qj = p.d_qj;
        d_qj.reserve(steps * nb);
        T4A_HIP(hipMemsetAsync(p.d_state.get(), 0, sizeof(int) * (nb * 2 * steps + nb), st));
        T4A_HIP(hipMemsetAsync(p.d_norm.get(), 0, sizeof(double) * nb, st));
        T4A_HIP(hipMemcpyAsync(d_qj.get(), qj, steps * nb * sizeof(BtQrJob), hipMemcpyHostToDevice, st));
        for (size_t i = 0; i < steps; ++i) {
            bt_qr_step_launch(d_qj.get() + i * nb, (int)nb, p.d_flags(), st);
            ++stats.launches;
        }
        T4A_HIP(hipGetLastError());
        if (p.timing) {
            p.eng.sync();
            stats.ms[0] = since(t0);
            t0 = clk::now();
        }
        if (read_norms) {
            PinBuf<int> h_flags;
            h_flags.reserve(nb);
            T4A_HIP(hipMemcpyAsync(p.h_norm.get(), p.d_norm.get(), sizeof(double) * nb, hipMemcpyDeviceToHost, st));
            T4A_HIP(hipMemcpyAsync(h_flags.get(), p.d_flags(), sizeof(int) * nb, hipMemcpyDeviceToHost, st));
            p.eng.sync(); // the synchronisation a budget costs: job table and read-back are behind it
            ++stats.syncs;
            for (size_t q = 0; q < nb; ++q) {
                norm2_[p.which[q]] = p.h_norm.get()[q];
                if (h_flags.get()[q] && first_bad == p.N) first_bad = p.which[q]; // reported behind the serial items of a lower index
            }
        }
        if (p.timing) stats.ms[1] = since(t0);
    }
    // the serial items: copies, canonical onto the last site
    for (size_t k = 0; k < first_bad; ++k) { // (an item past a flagged one is never reported: the lowest index is)
        if (p.batched[k]) continue;
        p.serial[k] = clone_cores(*p.in[k], st);
        if (n == 0) continue;
        try {
            QrSweep sw(p.eng);
            if (n > 1) sw.canonicalize(p.serial[k], n - 1);
        } catch (const Error& e) {
            if (e.code == T4A_GPU_INVALID_ARGUMENT) throw_item(k, e.what());
            throw;
        }
        if (read_norms || p.trace) {
            const DevCore& last = p.serial[k][n - 1];
            const std::vector<double> h = to_host(p.eng, last.buf.get(), last.size());
            double s = 0.0;
            for (double v : h) s += v * v;
            norm2_[k] = s;
            if (!std::isfinite(s)) {
                bool inf_input = false;
                for (double v : h)
                    if (!std::isfinite(v)) inf_input = true;
                if (inf_input) throw_item(k, NONFINITE);
            }
        }
    }
    if (first_bad < p.N) throw_item(first_bad, NONFINITE);
    trace.norm2 = norm2_;
    p.canonical = true;
}

std::vector<std::vector<DevCore>> TruncateBatch::truncate(const std::vector<BtRule>& rules, bool ranks_only, std::vector<std::vector<size_t>>& bonds)
{
    Impl& p = *p_;
    if (!p.canonical) throw Error(T4A_GPU_INTERNAL_ERROR, "truncate_many: truncate before canonicalize");
    if (rules.size() != p.N) throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: " + std::to_string(rules.size()) + " rules for " + std::to_string(p.N) + " items");
    const size_t n = p.n, nb = p.nb, steps = p.steps;
    const hipStream_t st = p.eng.stream();
    std::vector<std::vector<DevCore>> res(p.N);
    bonds.assign(p.N, {});
    size_t first_bad = p.N;
    if (nb) {
        clk::time_point t0 = clk::now();
        double* base = p.arena.get();
        // the results at their bounds under the item's cap: the kernels write them compactly, the shapes are set after the read-back
        std::vector<Bounds> B(nb);
        std::vector<std::vector<DevCore>> out(nb);
        for (size_t q = 0; q < nb; ++q) {
            const std::vector<DevCore>& c = *p.in[p.which[q]];
            const BtRule& rl = rules[p.which[q]];
            B[q] = bounds_of(shape_of(c), (size_t)rl.cap);
            if (rl.skip) continue;
            out[q].resize(n);
            for (size_t i = 0; i < n; ++i) out[q][i] = DevCore::make(B[q].b3[i], c[i].s, B[q].b3[i + 1]);
        }
        PinBuf<BtSvdJob> sj_buf;
        PinBuf<BtRule> rl_buf;
        PinBuf<int> h_buf;
        sj_buf.reserve(2 * steps * nb);
        rl_buf.reserve(nb);
        h_buf.reserve(nb * 2 * steps + nb);
        if (p.trace) p.d_sv.reserve(nb * 2 * steps * 64);
        BtSvdJob* sj = sj_buf.get();
        for (size_t q = 0; q < nb; ++q) {
            const std::vector<DevCore>& c = *p.in[p.which[q]];
            const Bounds& U = p.bd[p.which[q]]; // without the cap: the arena was laid out with these
            rl_buf.get()[q] = rules[p.which[q]];
            for (size_t t = 0; t < steps; ++t) { // leftward step t works on site i = n - 1 - t and truncates bond i
                const size_t i = n - 1 - t;
                BtSvdJob& j = sj[t * nb + q];
                j = BtSvdJob{};
                j.C = base + (i == n - 1 ? p.offY[q * n + i] : p.offP[q * n + i]);
                j.Nb = base + p.offQ[q * n + i - 1];
                j.U = base + p.offZ[q * n + i];
                j.Nout = base + p.offP[q * n + i - 1];
                j.scratch = base + p.offS[q];
                j.sv = p.trace ? p.d_sv.get() + (q * 2 * steps + t) * 64 : nullptr;
                j.s = (int)c[i].s;
                j.nb_s = (int)c[i - 1].s;
                j.outer_dim = (int)U.b2[i + 1], j.outer_idx = i == n - 1 ? -1 : p.rank_index(q, 0, i + 1);
                j.trunc_dim = (int)U.k[i], j.trunc_idx = -1;
                j.far_dim = (int)U.k[i - 1], j.far_idx = -1;
                j.cur = p.rank_index(q, 0, i);
            }
            for (size_t i = 0; i < steps; ++i) { // rightward step i truncates bond i + 1
                BtSvdJob& j = sj[(steps + i) * nb + q];
                j = BtSvdJob{};
                j.C = base + (i == 0 ? p.offP[q * n] : p.offA[q * n + i]);
                j.Nb = base + p.offZ[q * n + i + 1];
                j.U = out[q].empty() ? nullptr : out[q][i].buf.get();
                j.Nout = i + 1 == n - 1 ? (out[q].empty() ? nullptr : out[q][n - 1].buf.get()) : base + p.offA[q * n + i + 1];
                j.scratch = base + p.offS[q];
                j.sv = p.trace ? p.d_sv.get() + (q * 2 * steps + steps + i) * 64 : nullptr;
                j.s = (int)c[i].s;
                j.nb_s = (int)c[i + 1].s;
                // the result buffers are laid out under the cap, the arena without it: both bound what the kernel may meet
                j.outer_dim = (int)B[q].b3[i], j.outer_idx = i == 0 ? -1 : p.rank_index(q, 1, i);
                j.trunc_dim = (int)B[q].b2[i + 1], j.trunc_idx = p.rank_index(q, 0, i + 1);
                j.far_dim = (int)B[q].b2[i + 2], j.far_idx = i + 2 == n ? -1 : p.rank_index(q, 0, i + 2);
                j.cur = p.rank_index(q, 1, i + 1);
            }
        }
        DevBuf<BtSvdJob> d_sj;
        DevBuf<BtRule> d_rl;
        d_sj.reserve(2 * steps * nb);
        d_rl.reserve(nb);
        T4A_HIP(hipMemcpyAsync(d_sj.get(), sj, 2 * steps * nb * sizeof(BtSvdJob), hipMemcpyHostToDevice, st));
        T4A_HIP(hipMemcpyAsync(d_rl.get(), rl_buf.get(), nb * sizeof(BtRule), hipMemcpyHostToDevice, st));
        if (p.trace) T4A_HIP(hipMemsetAsync(p.d_sv.get(), 0, sizeof(double) * nb * 2 * steps * 64, st));
        for (size_t t = 0; t < 2 * steps; ++t) {
            bt_svd_step_launch(t < steps, d_sj.get() + t * nb, (int)nb, d_rl.get(), p.d_ranks(), p.d_flags(), st);
            ++stats.launches;
            if (p.timing && t + 1 == steps) {
                p.eng.sync();
                stats.ms[2] = since(t0);
                t0 = clk::now();
            }
        }
        T4A_HIP(hipGetLastError());
        if (p.timing) {
            p.eng.sync();
            stats.ms[3] = since(t0);
            t0 = clk::now();
        }
        int* h = h_buf.get();
        T4A_HIP(hipMemcpyAsync(h, p.d_state.get(), sizeof(int) * (nb * 2 * steps + nb), hipMemcpyDeviceToHost, st));
        std::vector<double> hsv;
        p.eng.sync(); // the synchronisation of phase 2: job tables, arena and read-back are all behind it
        ++stats.syncs;
        if (p.timing) stats.ms[4] = since(t0);
        if (p.trace) {
            hsv = to_host(p.eng, p.d_sv.get(), nb * 2 * steps * 64);
            const std::vector<double> hn = to_host(p.eng, p.d_norm.get(), nb); // (the hook's own copies are outside the count)
            for (size_t q = 0; q < nb; ++q) trace.norm2[p.which[q]] = hn[q];
        }
        for (size_t q = 0; q < nb; ++q) {
            const size_t k = p.which[q];
            const int flag = h[nb * 2 * steps + q];
            if (flag == 2) throw Error(T4A_GPU_INTERNAL_ERROR, "truncate_many: item " + std::to_string(k) + ": a rank left its planned bound");
            if (flag) {
                first_bad = std::min(first_bad, k);
                continue;
            }
            if (rules[k].skip) continue;
            const std::vector<DevCore>& c = *p.in[k];
            bonds[k].assign(n + 1, 1);
            for (size_t j = 1; j < n; ++j) bonds[k][j] = (size_t)h[p.rank_index(q, 1, j)];
            if (p.trace) {
                trace.ranks[k].clear(); // in the order the steps run: the leftward sweep meets the bonds n - 1 .. 1
                for (size_t t = 0; t < steps; ++t) trace.ranks[k].push_back(h[p.rank_index(q, 0, n - 1 - t)]);
                for (size_t j = 1; j < n; ++j) trace.ranks[k].push_back(h[p.rank_index(q, 1, j)]);
                trace.sv[k].assign(hsv.begin() + q * 2 * steps * 64, hsv.begin() + (q + 1) * 2 * steps * 64);
            }
            if (ranks_only) continue;
            for (size_t i = 0; i < n; ++i) out[q][i].reshape(bonds[k][i], c[i].s, bonds[k][i + 1]);
            res[k] = std::move(out[q]);
        }
    }
    // the serial stage: the same sequence on one chain (an item past a flagged one is never reported: the lowest index is)
    DevBuf<double> u, s, vt, us;
    std::vector<double> hs;
    bool any_serial = false;
    for (size_t k = 0; k < first_bad; ++k) {
        if (p.batched[k]) continue;
        any_serial = true;
        const BtRule& rl = rules[k];
        if (rl.skip) continue;
        std::vector<DevCore>& c = p.serial[k];
        SvdPolicy pol;
        pol.threshold = rl.threshold, pol.scale = rl.scale, pol.measure = rl.measure, pol.rule = rl.rule;
        auto factor = [&](const double* mat, int M, int Nn) {
            const int kmin = std::min(M, Nn);
            u.reserve((size_t)M * kmin);
            s.reserve(kmin);
            vt.reserve((size_t)kmin * Nn);
            p.eng.svd(mat, M, Nn, u.get(), s.get(), vt.get());
            hs = to_host(p.eng, s.get(), (size_t)kmin);
            size_t keep = svd_retained_rank(hs.data(), (size_t)kmin, pol);
            if (rl.cap != 0) keep = std::min(keep, (size_t)rl.cap);
            if (p.trace) {
                trace.ranks[k].push_back((int)std::min(std::max<size_t>(keep, 1), (size_t)kmin));
                std::vector<double> pad(hs);
                pad.resize(std::max<size_t>(pad.size(), 64), 0.0);
                trace.sv[k].insert(trace.sv[k].end(), pad.begin(), pad.begin() + 64);
            }
            return (int)std::min(std::max<size_t>(keep, 1), (size_t)kmin);
        };
        try {
            for (size_t i = n; i-- > 1;) { // leftward: the site as l x (s r); the site takes Vt, the left neighbour U S
                DevCore& cs = c[i];
                DevCore& pv = c[i - 1];
                const int M = (int)cs.l, Nn = (int)(cs.s * cs.r), kmin = std::min(M, Nn);
                const int keep = factor(cs.buf.get(), M, Nn);
                DevCore ns = DevCore::make((size_t)keep, cs.s, cs.r);
                gather_launch(vt.get(), kmin, nullptr, keep, nullptr, Nn, ns.buf.get(), keep, st);
                us.reserve((size_t)M * keep);
                diag_scale_launch(u.get(), M, M, keep, s.get(), false, us.get(), M, st);
                DevCore np = DevCore::make(pv.l, pv.s, (size_t)keep);
                const int pl = (int)(pv.l * pv.s);
                gemm_launch(gemm_desc(pl, keep, M, pv.buf.get(), pl, us.get(), M, np.buf.get(), pl), st);
                T4A_HIP(hipGetLastError());
                p.eng.sync(); // the two old cores are released below while the gather and the GEMM queued above still read them
                cs = std::move(ns);
                pv = std::move(np);
            }
            for (size_t i = 0; i + 1 < n; ++i) { // rightward: the site as (l s) x r; the site takes U, the right neighbour S Vt
                DevCore& cs = c[i];
                DevCore& nx = c[i + 1];
                const int M = (int)(cs.l * cs.s), Nn = (int)cs.r, kmin = std::min(M, Nn);
                const int keep = factor(cs.buf.get(), M, Nn);
                DevCore ns = DevCore::make(cs.l, cs.s, (size_t)keep);
                gather_launch(u.get(), M, nullptr, M, nullptr, keep, ns.buf.get(), M, st);
                us.reserve((size_t)keep * Nn);
                diag_scale_launch(vt.get(), kmin, keep, Nn, s.get(), true, us.get(), keep, st);
                DevCore nn = DevCore::make((size_t)keep, nx.s, nx.r);
                const int rest = (int)(nx.s * nx.r);
                gemm_launch(gemm_desc(keep, rest, Nn, us.get(), keep, nx.buf.get(), Nn, nn.buf.get(), keep), st);
                T4A_HIP(hipGetLastError());
                p.eng.sync(); // as above: the old cores go back to the pool
                cs = std::move(ns);
                nx = std::move(nn);
            }
        } catch (const Error& e) {
            if (e.code == T4A_GPU_INVALID_ARGUMENT) throw_item(k, e.what());
            throw;
        }
        bonds[k].assign(n + 1, 1);
        for (size_t j = 1; j < n; ++j) bonds[k][j] = c[j].l;
        if (!ranks_only) res[k] = std::move(c);
    }
    if (first_bad < p.N) throw_item(first_bad, NONFINITE);
    if (any_serial) p.eng.sync(); // (copies of short chains may be in flight; the batched part has ended synced)
    p.canonical = false;
    return res;
}

TruncateManyPlan truncate_many_plan(const std::vector<std::vector<std::array<size_t, 4>>>& shapes, const std::vector<size_t>& caps,
                                    CompressRoute route, bool rules_from_norms)
{
    if (shapes.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: the list is empty");
    if (caps.size() != shapes.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: " + std::to_string(caps.size()) + " caps for " + std::to_string(shapes.size()) + " items");
    const size_t N = shapes.size(), n = shapes[0].size();
    TruncateManyPlan p;
    std::vector<Bounds> bd(N);
    for (size_t k = 0; k < N; ++k) {
        if (shapes[k].size() != n)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: item " + std::to_string(k) + " has " + std::to_string(shapes[k].size()) +
                                                      " sites, item 0 has " + std::to_string(n));
        try {
            mpo_validate_dims(shapes[k]);
        } catch (const Error& e) {
            throw_item(k, e.what());
        }
        std::vector<Shape3> f(n);
        for (size_t i = 0; i < n; ++i) f[i] = {shapes[k][i][0], shapes[k][i][1] * shapes[k][i][2], shapes[k][i][3]};
        bd[k] = bounds_of(f, caps[k]);
        p.bonds.push_back(bd[k].b3);
        p.qr_bonds.push_back(bd[k].k);
    }
    p.batched = pick(bd, route);
    for (int b : p.batched) p.n_batched += b;
    if (p.n_batched) {
        p.launches = 3 * (n - 1);
        p.syncs = rules_from_norms ? 2 : 1;
    }
    return p;
}

std::vector<std::unique_ptr<Mpo>> mpo_truncate_many(const std::vector<Mpo*>& items, const std::vector<BtRule>& rules, CompressRoute route,
                                                    bool ranks_only, std::vector<std::vector<size_t>>& bonds, TruncateManyStats* stats,
                                                    TruncateManyTrace* trace)
{
    if (items.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: the list is empty");
    if (rules.size() != items.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: " + std::to_string(rules.size()) + " rules for " + std::to_string(items.size()) + " items");
    for (size_t k = 0; k < items.size(); ++k)
        if (!items[k]) throw Error(T4A_GPU_NULL_POINTER, "truncate_many: item " + std::to_string(k) + " is null");
    for (size_t k = 1; k < items.size(); ++k)
        if (items[k]->len() != items[0]->len())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "truncate_many: item " + std::to_string(k) + " has " + std::to_string(items[k]->len()) +
                                                      " sites, item 0 has " + std::to_string(items[0]->len()));
    for (size_t k = 0; k < rules.size(); ++k) {
        const BtRule& r = rules[k];
        if (!(r.threshold >= 0.0) || !std::isfinite(r.threshold)) throw_item(k, "the threshold must be finite and non-negative");
        if (r.scale < 0 || r.scale > 1 || r.measure < 0 || r.measure > 1 || r.rule < 0 || r.rule > 1) throw_item(k, "unknown truncation policy");
        if (r.cap < 0) throw_item(k, "the cap is negative");
    }
    std::vector<const std::vector<DevCore>*> in;
    for (Mpo* m : items) {
        m->tt.eng.sync(); // every operand is read on the first one's stream
        in.push_back(&m->tt.cores);
    }
    TruncateBatch tb(items[0]->tt.eng, in, route, trace != nullptr, false);
    tb.canonicalize(false);
    std::vector<std::vector<DevCore>> res = tb.truncate(rules, ranks_only, bonds);
    if (stats) *stats = tb.stats;
    if (trace) *trace = std::move(tb.trace);
    std::vector<std::unique_ptr<Mpo>> out;
    for (size_t k = 0; k < items.size(); ++k)
        out.push_back(ranks_only || res[k].empty() ? nullptr : std::make_unique<Mpo>(std::move(res[k]), items[k]->sd));
    return out;
}

} // namespace t4a
