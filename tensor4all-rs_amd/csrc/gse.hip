// gse.hip — global subspace expansion and GSE-TDVP on the device (see gse.hpp).  Shape bookkeeping and the cutoff on the singular values
// are host work; every floating-point operation on a train runs in gfx950 kernels: the QR steps of QrSweep, the Jacobi SVD of the
// engine, the two launches of kernels_gse.hip, the zip-up contraction behind the references and tdvp.
#include "gse.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

namespace {

void require_int(size_t a, size_t b, size_t edge_child, const char* what)
{
    if (a != 0 && b > (size_t)INT_MAX / a)
        throw Error(T4A_GPU_INVALID_ARGUMENT, std::string("gse: ") + what + " of the edge at child " + std::to_string(edge_child) + " would hold more than INT_MAX elements");
}

// The buffers of the edges, grown as needed and reused from edge to edge.
struct EdgeWork {
    DevBuf<double> u1, s1, vt1, u2, s2, vt2, bn, stack, scratch, part, trace;
    DevBuf<unsigned> ticket;
};

} // namespace

// ------------------------------------------------------------------------------------------------ options and shapes
void GseOptions::validate() const
{
    require_tol(density_weight_cutoff, "invalid GSE option density_weight_cutoff: must be finite and non-negative");
    require_tol(hermitian_tol, "invalid GSE option hermitian_tol: must be finite and non-negative");
    if (has_reference_max_bond_dim && reference_max_bond_dim == 0)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid GSE option reference_max_bond_dim: must be greater than zero when set");
    if (has_reference_svd_policy) validate_svd_policy(reference_svd_policy, "GseOptions::reference_svd_policy");
}

void gse_validate_shapes(const std::vector<std::array<size_t, 3>>& state, const std::vector<std::vector<std::array<size_t, 3>>>& refs, size_t center)
{
    const size_t n = state.size();
    if (center >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "GSE center " + std::to_string(center) + " is not a state node");
    if (refs.size() > (size_t)GSE_MAX_REFERENCES)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "gse: more than " + std::to_string(GSE_MAX_REFERENCES) + " references are not implemented");
    for (const auto& r : refs) {
        if (r.size() != n) throw Error(T4A_GPU_INVALID_ARGUMENT, "GSE requires target, references, and operator support to have the same tree topology");
        for (size_t i = 0; i < n; ++i)
            if (r[i][1] != state[i][1])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid GSE mapping at node " + std::to_string(i) + ": reference site dimension does not match target");
    }
}

namespace {
void validate_operator(const std::vector<std::array<size_t, 4>>& op, const std::vector<std::array<size_t, 3>>& state, size_t center)
{
    const size_t n = state.size();
    if (center >= n) throw Error(T4A_GPU_INVALID_ARGUMENT, "GSE center " + std::to_string(center) + " is not a state node");
    if (op.size() != n) throw Error(T4A_GPU_INVALID_ARGUMENT, "GSE requires target, references, and operator support to have the same tree topology");
    for (size_t i = 0; i < n; ++i)
        if (op[i][1] != state[i][1] || op[i][2] != state[i][1])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "invalid GSE mapping at node " + std::to_string(i) + ": operator site dimensions (" + std::to_string(op[i][1]) + ", " +
                                                      std::to_string(op[i][2]) + ") do not match the state's " + std::to_string(state[i][1]));
}
} // namespace

// Measured on an MI355X at d = 2, K = 2 (tools/probe_gse.py): at bond 64 (q = 128) the fused launches take 0.6 of the
// GEMM composition, at bond 128 (q = 256) 1.3 - 1.4 times and at bond 256 (q = 512) 3.2 - 4.7 times as long — a workgroup owns 16 rows
// and the launch has too few of them to fill the device, while the GEMM tiles both output dimensions.  Shapes up to the measured win
// take the fused launches; everything above, the unmeasured shapes between the two included, takes the GEMM.
namespace {
std::atomic<int> g_route{-1};
}
void gse_set_route(int route) { g_route.store(route < 0 || route > 1 ? -1 : route); }
bool gse_use_fused(int q, int bond)
{
    const int forced = g_route.load();
    if (forced >= 0) return forced == 0;
    return (long long)q * bond <= GSE_FUSED_MAX_WORK;
}

// ------------------------------------------------------------------------------------------------ the references
std::vector<std::unique_ptr<TensorTrain>> gse_krylov_references(Mpo& op, TensorTrain& init, const GseOptions& o)
{
    o.validate();
    validate_operator(op.dims4(), dims3_of(init.cores), 0);
    size_t cap = o.reference_max_bond_dim;
    if (!o.has_reference_max_bond_dim) {
        cap = 1;
        for (size_t d : init.link_dims()) cap = std::max(cap, d);
        cap = cap + 1;
    }
    MpoContractionOptions mo;
    mo.tolerance = o.has_reference_svd_policy ? o.reference_svd_policy.threshold : 1e-12;
    mo.max_bond_dim = cap;
    mo.method = MpoFactorizeMethod::SVD;
    std::vector<std::unique_ptr<TensorTrain>> refs;
    TensorTrain* cur = &init;
    for (size_t k = 0; k < o.krylov_dim; ++k) {
        std::vector<std::array<size_t, 2>> sd;
        for (const DevCore& c : cur->cores) sd.push_back({c.s, 1});
        Mpo ket(cur->cores, cur->eng.stream(), sd);
        std::unique_ptr<Mpo> prod = mpo_contract(op, ket, MpoAlgorithm::ZipUp, true, mo);
        auto next = std::make_unique<TensorTrain>(prod->tt.cores, prod->tt.eng.stream());
        if (o.normalize_references) {
            const double nrm = std::sqrt(next->norm2());
            if (nrm > 0.0) next->scale(1.0 / nrm);
        }
        refs.push_back(std::move(next));
        cur = refs.back().get();
    }
    return refs;
}

// ------------------------------------------------------------------------------------------------ the expansion
namespace {

// One edge: the child `ci` of every train is replaced by the expanded basis, the parent `pi` absorbs the coefficients.  orient 0: the
// child is to the right of its parent (its first leg is the bond); 1: to the left (its last leg is the bond).  tr[0] is the target.
// -> the number of rows appended.
size_t expand_one_edge(Engine& e, EdgeWork& w, std::vector<std::vector<DevCore>>& tr, size_t ci, size_t pi, int orient, double cutoff)
{
    hipStream_t st = e.stream();
    const int nt = (int)tr.size(), K = nt - 1;
    const DevCore& tc = tr[0][ci];
    const size_t s = tc.s, far = orient ? tc.l : tc.r;
    const size_t q = s * far;
    int r[GSE_MAX_JOBS], L[GSE_MAX_JOBS];
    const double* child[GSE_MAX_JOBS];
    const double* parent[GSE_MAX_JOBS];
    size_t P = 0, sumL = 0;
    for (int t = 0; t < nt; ++t) {
        const DevCore& c = tr[t][ci];
        const DevCore& p = tr[t][pi];
        if ((orient ? c.l : c.r) != far || c.s != s)
            throw Error(T4A_GPU_INTERNAL_ERROR, "gse: the far bond of child " + std::to_string(ci) + " is not common to all trains");
        const size_t rt = orient ? c.r : c.l, Lt = orient ? p.s * p.r : p.l * p.s;
        require_int(rt, q, ci, "a child matrix");
        require_int(Lt, std::max(rt, q), ci, "a parent matrix");
        r[t] = (int)rt;
        L[t] = (int)Lt;
        child[t] = c.buf.get();
        parent[t] = p.buf.get();
        if (t) P += rt;
        sumL += Lt;
    }
    const size_t rr = (size_t)r[0], k = std::min(rr, q), k2 = std::min(P, q);
    require_int(P, q, ci, "the stack of the projected references");
    require_int(sumL, q, ci, "the scratch of the absorption");
    require_int(k + k2, std::max(q, sumL), ci, "the expanded basis");
    Engine::require_factor_dims(std::max(rr, P), q, "gse: dimensions of an edge");

    // 1. the old basis: the right singular vectors of the child as r x q (orient 1: the left ones of the q x r matricisation)
    grow(e, w.u1, std::max(rr, q) * k);
    grow(e, w.s1, k);
    grow(e, w.vt1, k * std::max(rr, q));
    if (orient)
        e.svd(child[0], (int)q, (int)rr, w.u1.get(), w.s1.get(), w.vt1.get());
    else
        e.svd(child[0], (int)rr, (int)q, w.u1.get(), w.s1.get(), w.vt1.get());
    const double* B = orient ? w.u1.get() : w.vt1.get();

    // 2. the projected references and the trace
    const int tiles = gse_tiles(r + 1, K);
    grow(e, w.stack, P * q);
    grow(e, w.scratch, std::max(P * k, std::max(sumL * q, (size_t)nt * std::max(rr, P) * (k + k2))));
    grow(e, w.part, (size_t)tiles);
    grow(e, w.trace, 1);
    if (!w.ticket.get()) w.ticket.reserve(1);
    T4A_HIP(hipMemsetAsync(w.ticket.get(), 0, sizeof(unsigned), st));
    const bool fused = gse_use_fused((int)q, (int)rr);
    if (fused)
        gse_project_launch(orient, (int)q, child + 1, r + 1, K, B, (int)k, w.stack.get(), w.scratch.get(), w.part.get(), w.ticket.get(), w.trace.get(), st);
    else
        gse_project_gemm(e, orient, (int)q, child + 1, r + 1, K, B, (int)k, w.stack.get(), w.scratch.get(), w.part.get(), w.ticket.get(), w.trace.get());
    T4A_HIP(hipGetLastError());

    // 3. the directions of the stack: the host reads the singular values and the trace
    grow(e, w.u2, std::max(P, q) * k2);
    grow(e, w.s2, k2);
    grow(e, w.vt2, k2 * std::max(P, q));
    if (orient)
        e.svd(w.stack.get(), (int)q, (int)P, w.u2.get(), w.s2.get(), w.vt2.get());
    else
        e.svd(w.stack.get(), (int)P, (int)q, w.u2.get(), w.s2.get(), w.vt2.get());
    std::vector<double> sig(k2);
    double trace = 0.0;
    T4A_HIP(hipMemcpyAsync(sig.data(), w.s2.get(), sizeof(double) * k2, hipMemcpyDeviceToHost, st));
    T4A_HIP(hipMemcpyAsync(&trace, w.trace.get(), sizeof(double), hipMemcpyDeviceToHost, st));
    e.sync();
    size_t m = 0;
    if (trace > 0.0)
        while (m < k2 && sig[m] * sig[m] > cutoff * trace) ++m;

    // 4. the new child B' = [B; kept rows]
    const size_t kn = k + m;
    grow(e, w.bn, kn * q);
    if (orient) {
        T4A_HIP(hipMemcpyAsync(w.bn.get(), w.u1.get(), sizeof(double) * q * k, hipMemcpyDeviceToDevice, st));
        if (m) T4A_HIP(hipMemcpyAsync(w.bn.get() + q * k, w.u2.get(), sizeof(double) * q * m, hipMemcpyDeviceToDevice, st));
    } else {
        T4A_HIP(hipMemcpy2DAsync(w.bn.get(), sizeof(double) * kn, w.vt1.get(), sizeof(double) * k, sizeof(double) * k, q, hipMemcpyDeviceToDevice, st));
        if (m) T4A_HIP(hipMemcpy2DAsync(w.bn.get() + k, sizeof(double) * kn, w.vt2.get(), sizeof(double) * k2, sizeof(double) * m, q, hipMemcpyDeviceToDevice, st));
    }

    // 5. the parents absorb the coefficients, the children become B'
    std::vector<DevCore> np(nt), nc(nt);
    double* out[GSE_MAX_JOBS];
    for (int t = 0; t < nt; ++t) {
        const DevCore& p = tr[t][pi];
        np[t] = orient ? DevCore::make(kn, p.s, p.r) : DevCore::make(p.l, p.s, kn);
        nc[t] = orient ? DevCore::make(far, s, kn) : DevCore::make(kn, s, far);
        out[t] = np[t].buf.get();
    }
    if (fused)
        gse_absorb_launch(orient, (int)q, child, r, parent, L, nt, w.bn.get(), (int)kn, out, w.scratch.get(), st);
    else
        gse_absorb_gemm(e, orient, (int)q, child, r, parent, L, nt, w.bn.get(), (int)kn, out, w.scratch.get());
    T4A_HIP(hipGetLastError());
    for (int t = 0; t < nt; ++t) T4A_HIP(hipMemcpyAsync(nc[t].buf.get(), w.bn.get(), sizeof(double) * kn * q, hipMemcpyDeviceToDevice, st));
    e.sync(); // the old cores are released below
    for (int t = 0; t < nt; ++t) {
        tr[t][ci] = std::move(nc[t]);
        tr[t][pi] = std::move(np[t]);
    }
    return m;
}

} // namespace

GseResult global_subspace_expand_with_references(TensorTrain& init, const std::vector<TensorTrain*>& references, size_t center, const GseOptions& o)
{
    o.validate();
    std::vector<std::vector<std::array<size_t, 3>>> rd;
    for (const TensorTrain* r : references) {
        if (!r) throw Error(T4A_GPU_NULL_POINTER, "gse: a reference is null");
        rd.push_back(dims3_of(r->cores));
    }
    gse_validate_shapes(dims3_of(init.cores), rd, center);
    const size_t n = init.cores.size();
    Engine e;
    hipStream_t st = e.stream();
    GseResult out;
    out.references_built = references.size();
    std::vector<std::vector<DevCore>> tr;
    init.eng.sync();
    tr.push_back(clone_cores(init.cores, st));
    for (TensorTrain* r : references) {
        r->eng.sync();
        tr.push_back(clone_cores(r->cores, st));
    }
    QrSweep sw(e);
    for (auto& t : tr) sw.canonicalize(t, center);
    if (!references.empty()) {
        EdgeWork w;
        auto book = [&](size_t added) {
            ++out.edges_processed;
            if (added) {
                ++out.bonds_expanded;
                out.max_added_basis = std::max(out.max_added_basis, added);
            }
        };
        if (center > 0) { // the left arm: every centre to the leaf 0, then 0->1 .. c-1->c
            for (auto& t : tr)
                for (size_t i = center; i > 0; --i) sw.right_step(t, i);
            for (size_t i = 0; i < center; ++i) book(expand_one_edge(e, w, tr, i, i + 1, 1, o.density_weight_cutoff));
        }
        if (center + 1 < n) { // the right arm: every centre to the leaf n-1, then n-1->n-2 .. c+1->c
            for (auto& t : tr)
                for (size_t i = center; i + 1 < n; ++i) sw.left_step(t, i);
            for (size_t i = n - 1; i > center; --i) book(expand_one_edge(e, w, tr, i, i - 1, 0, o.density_weight_cutoff));
        }
    }
    e.sync();
    out.state = std::make_unique<TensorTrain>(tr[0], st);
    return out;
}

GseResult global_subspace_expand(Mpo& op, TensorTrain& init, size_t center, const GseOptions& o)
{
    o.validate();
    validate_operator(op.dims4(), dims3_of(init.cores), center);
    if (o.krylov_dim > (size_t)GSE_MAX_REFERENCES)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "gse: more than " + std::to_string(GSE_MAX_REFERENCES) + " references are not implemented");
    std::vector<std::unique_ptr<TensorTrain>> refs = gse_krylov_references(op, init, o);
    std::vector<TensorTrain*> ptrs;
    for (auto& r : refs) ptrs.push_back(r.get());
    return global_subspace_expand_with_references(init, ptrs, center, o);
}

GseTdvpResult gse_tdvp(TdvpMode mode, Mpo& op, TensorTrain& init, size_t center, const GseTdvpOptions& o)
{
    o.gse.validate();
    o.tdvp.validate(mode);
    tdvp_validate_shapes(mode, op.dims4(), dims3_of(init.cores), center, o.tdvp.krylov.max_iter);
    if (o.gse.krylov_dim > (size_t)GSE_MAX_REFERENCES)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "gse: more than " + std::to_string(GSE_MAX_REFERENCES) + " references are not implemented");
    GseTdvpResult out;
    std::unique_ptr<TensorTrain> state;
    TensorTrain* cur = &init;
    TdvpOptions one = o.tdvp;
    one.nsweeps = 1;
    for (size_t sweep = 0; sweep < o.tdvp.nsweeps; ++sweep) {
        if (o.gse.krylov_dim > 0 && (sweep > 0 || o.gse.expand_before_first_sweep)) {
            GseResult ex = global_subspace_expand(op, *cur, center, o.gse);
            state = std::move(ex.state);
            cur = state.get();
            ++out.gse_expansions;
        }
        TdvpResult r = tdvp(mode, op, *cur, center, one);
        state = std::move(r.state);
        cur = state.get();
        out.sweeps_completed += r.sweeps_completed;
        out.local_updates += r.local_updates;
        out.max_error_estimate = std::max(out.max_error_estimate, r.max_error_estimate);
        out.max_krylov_iterations = std::max(out.max_krylov_iterations, r.max_krylov_iterations);
    }
    out.state = std::move(state);
    return out;
}

// ------------------------------------------------------------------------------------------------ test hooks and the probe
namespace {
struct HostOperands {
    std::vector<DevBuf<double>> bufs;
    const double* up(hipStream_t st, const double* h, size_t count)
    {
        bufs.emplace_back();
        bufs.back().reserve(std::max<size_t>(count, 1));
        if (count) T4A_HIP(hipMemcpyAsync(bufs.back().get(), h, sizeof(double) * count, hipMemcpyHostToDevice, st));
        return bufs.back().get();
    }
};
} // namespace

void gse_project_host(int orient, int q, const double* refs, const int* rho, int K, const double* B, int kb, int route, double* stack, double* trace)
{
    Engine e;
    hipStream_t st = e.stream();
    HostOperands ops;
    ops.bufs.reserve(GSE_MAX_JOBS + 1);
    const double* d_refs[GSE_MAX_JOBS];
    size_t P = 0;
    for (int j = 0; j < K; ++j) {
        d_refs[j] = ops.up(st, refs + P * q, (size_t)rho[j] * q);
        P += rho[j];
    }
    const double* dB = ops.up(st, B, (size_t)kb * q);
    DevBuf<double> d_stack, scratch, part, d_trace;
    DevBuf<unsigned> ticket;
    d_stack.reserve(P * q);
    scratch.reserve(P * kb);
    part.reserve(gse_tiles(rho, K));
    d_trace.reserve(1);
    ticket.reserve(1);
    T4A_HIP(hipMemsetAsync(ticket.get(), 0, sizeof(unsigned), st));
    if (route == 0)
        gse_project_launch(orient, q, d_refs, rho, K, dB, kb, d_stack.get(), scratch.get(), part.get(), ticket.get(), d_trace.get(), st);
    else
        gse_project_gemm(e, orient, q, d_refs, rho, K, dB, kb, d_stack.get(), scratch.get(), part.get(), ticket.get(), d_trace.get());
    T4A_HIP(hipGetLastError());
    T4A_HIP(hipMemcpyAsync(stack, d_stack.get(), sizeof(double) * P * q, hipMemcpyDeviceToHost, st));
    T4A_HIP(hipMemcpyAsync(trace, d_trace.get(), sizeof(double), hipMemcpyDeviceToHost, st));
    e.sync();
}

void gse_absorb_host(int orient, int q, const double* children, const int* r, const double* parents, const int* L, int n_trains, const double* Bn, int kn,
                     int route, double* out)
{
    Engine e;
    hipStream_t st = e.stream();
    HostOperands ops;
    ops.bufs.reserve(2 * GSE_MAX_JOBS + 1);
    const double* d_child[GSE_MAX_JOBS];
    const double* d_parent[GSE_MAX_JOBS];
    double* d_out[GSE_MAX_JOBS];
    std::vector<DevBuf<double>> outs(n_trains);
    size_t coff = 0, poff = 0, sumL = 0, sumG = 0;
    for (int j = 0; j < n_trains; ++j) {
        d_child[j] = ops.up(st, children + coff, (size_t)r[j] * q);
        d_parent[j] = ops.up(st, parents + poff, (size_t)L[j] * r[j]);
        outs[j].reserve((size_t)L[j] * kn);
        d_out[j] = outs[j].get();
        coff += (size_t)r[j] * q;
        poff += (size_t)L[j] * r[j];
        sumL += L[j];
        sumG += (size_t)r[j] * kn;
    }
    const double* dB = ops.up(st, Bn, (size_t)kn * q);
    DevBuf<double> scratch;
    scratch.reserve(std::max(sumL * q, sumG));
    if (route == 0)
        gse_absorb_launch(orient, q, d_child, r, d_parent, L, n_trains, dB, kn, d_out, scratch.get(), st);
    else
        gse_absorb_gemm(e, orient, q, d_child, r, d_parent, L, n_trains, dB, kn, d_out, scratch.get());
    T4A_HIP(hipGetLastError());
    size_t ooff = 0;
    for (int j = 0; j < n_trains; ++j) {
        T4A_HIP(hipMemcpyAsync(out + ooff, d_out[j], sizeof(double) * (size_t)L[j] * kn, hipMemcpyDeviceToHost, st));
        ooff += (size_t)L[j] * kn;
    }
    e.sync();
}

void gse_time_routes(size_t chi, size_t d, size_t K, size_t reps, double ms[4])
{
    if (chi == 0 || d == 0 || K == 0 || K > (size_t)GSE_MAX_REFERENCES || reps == 0 || chi > 4096 || d > 64)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "gse_time_routes: chi in 1..4096, d in 1..64, K in 1..8 and reps must be positive");
    Engine e;
    hipStream_t st = e.stream();
    const int q = (int)(d * chi), kb = (int)chi, kn = (int)chi + 1, Lp = (int)(d * chi);
    const int nt = (int)K + 1;
    int r[GSE_MAX_JOBS], L[GSE_MAX_JOBS];
    std::vector<DevBuf<double>> ch(nt), pa(nt), ou(nt);
    const double* child[GSE_MAX_JOBS];
    const double* parent[GSE_MAX_JOBS];
    double* out[GSE_MAX_JOBS];
    size_t P = 0, sumL = 0, sumG = 0;
    for (int t = 0; t < nt; ++t) {
        r[t] = t ? (int)chi + 1 : (int)chi;
        L[t] = Lp;
        ch[t].reserve((size_t)r[t] * q);
        pa[t].reserve((size_t)L[t] * r[t]);
        ou[t].reserve((size_t)L[t] * kn);
        fill_launch(ch[t].get(), (size_t)r[t] * q, 1.0 / std::sqrt((double)q), st);
        fill_launch(pa[t].get(), (size_t)L[t] * r[t], 1.0 / std::sqrt((double)r[t]), st);
        child[t] = ch[t].get();
        parent[t] = pa[t].get();
        out[t] = ou[t].get();
        if (t) P += r[t];
        sumL += L[t];
        sumG += (size_t)r[t] * kn;
    }
    DevBuf<double> B, stack, scratch, part, trace;
    DevBuf<unsigned> ticket;
    B.reserve((size_t)kn * q);
    fill_launch(B.get(), (size_t)kn * q, 1.0 / std::sqrt((double)q), st);
    stack.reserve(P * q);
    scratch.reserve(std::max(std::max(P * (size_t)kb, sumL * q), sumG));
    part.reserve(gse_tiles(r + 1, (int)K));
    trace.reserve(1);
    ticket.reserve(1);
    const std::function<void()> pieces[4] = {
        [&] {
            T4A_HIP(hipMemsetAsync(ticket.get(), 0, sizeof(unsigned), st));
            gse_project_launch(0, q, child + 1, r + 1, (int)K, B.get(), kb, stack.get(), scratch.get(), part.get(), ticket.get(), trace.get(), st);
        },
        [&] {
            T4A_HIP(hipMemsetAsync(ticket.get(), 0, sizeof(unsigned), st));
            gse_project_gemm(e, 0, q, child + 1, r + 1, (int)K, B.get(), kb, stack.get(), scratch.get(), part.get(), ticket.get(), trace.get());
        },
        [&] { gse_absorb_launch(0, q, child, r, parent, L, nt, B.get(), kn, out, scratch.get(), st); },
        [&] { gse_absorb_gemm(e, 0, q, child, r, parent, L, nt, B.get(), kn, out, scratch.get()); },
    };
    time_pieces(st, pieces, 4, reps, ms);
    e.sync();
}

} // namespace t4a
