// linop.hip — an operator applied on a subset of a state's sites (linop.hpp): the host plan with every refusal, the full-length
// operator of the composed route, compose.rs for a chain, the one-launch naive apply and the dispatch over method and route.  The
// fused zip-up and fit live in mpo.hip beside the contraction whose recursion and sweeps they are.
#include "linop.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

namespace {

constexpr size_t LINOP_DIM_MAX = 65535; // the tensor train's limit

void check_count(size_t a, size_t b, size_t c, size_t d, const std::string& what)
{
    const unsigned long long lim = INT_MAX;
    unsigned long long n = 1;
    for (size_t x : {a, b, c, d}) {
        if (x > lim || n * x > lim) throw Error(T4A_GPU_INVALID_ARGUMENT, what + " holds more than INT_MAX elements");
        n *= x;
    }
}

std::string list_of(const std::vector<size_t>& v)
{
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

std::vector<std::array<size_t, 3>> dims3_of(const TensorTrain& t)
{
    std::vector<std::array<size_t, 3>> d(t.len());
    for (size_t i = 0; i < t.len(); ++i) d[i] = {t.cores[i].l, t.cores[i].s, t.cores[i].r};
    return d;
}

// a gap site of the full-length operator, delta_{aa'} delta_{yx} as [m, d, d, m] column-major, exact on the host
std::vector<double> bridge_site(size_t m, size_t d)
{
    std::vector<double> h(m * d * d * m, 0.0);
    for (size_t a = 0; a < m; ++a)
        for (size_t x = 0; x < d; ++x) h[a + m * (x + d * (x + d * a))] = 1.0;
    return h;
}

DevCore upload_site(const std::vector<double>& h, size_t l, size_t s, size_t r, hipStream_t st)
{
    DevCore c = DevCore::make(l, s, r);
    T4A_HIP(hipMemcpyAsync(c.buf.get(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st));
    T4A_HIP(hipStreamSynchronize(st)); // `h` is pageable host memory of the caller's frame
    return c;
}

PartialSpec matrix_product_spec(size_t n)
{
    PartialSpec spec;
    for (size_t i = 0; i < n; ++i) spec.contract_pairs.push_back(PartialPair{i, 1, i, 0});
    return spec;
}

// every site of the chain in one launch of apply_site_kernel
std::vector<DevCore> naive_fused(Mpo& op, TensorTrain& state, const std::vector<ApplySitePlan>& plan)
{
    const size_t n = state.len();
    Engine& eng = op.tt.eng;
    const hipStream_t st = eng.stream();
    state.eng.sync(); // the state's cores are read on the operator's stream
    std::vector<DevCore> out(n);
    std::vector<ApplySiteJob> jobs(n);
    unsigned long long off = 0;
    for (size_t i = 0; i < n; ++i) {
        const ApplySitePlan& p = plan[i];
        const DevCore& x = state.cores[i];
        out[i] = DevCore::make(p.result[0], p.result[1], p.result[2]);
        ApplySiteJob& j = jobs[i];
        j = ApplySiteJob{};
        j.gap = p.kind == ApplySiteKind::Op ? 0 : 1;
        j.O = j.gap ? nullptr : op.tt.cores[p.op_site].buf.get();
        j.X = x.buf.get();
        j.Y = out[i].buf.get();
        j.off = off;
        j.ml = (int)p.m_left, j.s1 = (int)p.d_out, j.k = (int)p.d_in, j.mr = (int)p.m_right;
        j.lb = (int)x.l, j.rb = (int)x.r;
        off += out[i].size();
    }
    DevBuf<ApplySiteJob> d_jobs;
    d_jobs.reserve(n);
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), n * sizeof(ApplySiteJob), hipMemcpyHostToDevice, st));
    apply_site_launch(d_jobs.get(), (int)n, off, st);
    T4A_HIP(hipGetLastError());
    eng.sync(); // `jobs` is pageable host memory, d_jobs goes out of scope
    return out;
}

} // namespace

std::vector<ApplySitePlan> apply_plan(const std::vector<std::array<size_t, 4>>& od, const std::vector<size_t>& sites,
                                      const std::vector<std::array<size_t, 3>>& sd)
{
    const size_t k = od.size(), n = sd.size();
    if (k == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: the operator has no sites");
    mpo_validate_dims(od);
    if (sites.size() != k)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: the operator has " + std::to_string(k) + " sites, `sites` names " +
                                                  std::to_string(sites.size()) + " positions");
    for (size_t j = 0; j + 1 < k; ++j)
        if (sites[j] >= sites[j + 1])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: sites must be strictly ascending, got " + list_of(sites));
    if (sites[k - 1] >= n) {
        std::vector<size_t> all(n);
        for (size_t i = 0; i < n; ++i) all[i] = i;
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Operator nodes " + list_of(sites) + " are not a subset of state nodes " + list_of(all));
    }
    for (size_t i = 0; i < n; ++i) {
        const std::string site = "apply_linear_operator: state site " + std::to_string(i);
        if (sd[i][0] == 0 || sd[i][1] == 0 || sd[i][2] == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, site + " has a zero dimension");
        if (i + 1 < n && sd[i][2] != sd[i + 1][0])
            throw Error(T4A_GPU_INVALID_ARGUMENT, site + " has right bond " + std::to_string(sd[i][2]) + ", its neighbour left bond " +
                                                      std::to_string(sd[i + 1][0]));
    }
    if (sd[0][0] != 1 || sd[n - 1][2] != 1) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: the state's outer bonds must be 1");
    for (size_t j = 0; j < k; ++j)
        if (od[j][2] != sd[sites[j]][1])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Shared shape mismatch at site " + std::to_string(sites[j]) + ": operator has input dim " +
                                                      std::to_string(od[j][2]) + ", the state has site dim " + std::to_string(sd[sites[j]][1]));
    std::vector<ApplySitePlan> plan(n);
    size_t j = 0; // the first operator site at or behind i
    for (size_t i = 0; i < n; ++i) {
        ApplySitePlan& p = plan[i];
        p.d_in = sd[i][1];
        if (j < k && sites[j] == i) {
            p.kind = ApplySiteKind::Op;
            p.op_site = j;
            p.m_left = od[j][0], p.m_right = od[j][3];
            p.d_out = od[j][1];
            ++j;
        } else {
            p.kind = (j == 0 || j == k) ? ApplySiteKind::Outside : ApplySiteKind::Bridge;
            p.m_left = p.m_right = p.kind == ApplySiteKind::Bridge ? od[j][0] : 1;
            p.d_out = p.d_in;
        }
        const std::string site = "apply_linear_operator: site " + std::to_string(i);
        for (size_t side = 0; side < 2; ++side) {
            const size_t m = side ? p.m_right : p.m_left, b = side ? sd[i][2] : sd[i][0];
            if (m * b > LINOP_DIM_MAX)
                throw Error(T4A_GPU_INVALID_ARGUMENT, site + ": the fused bond " + std::to_string(m) + " * " + std::to_string(b) + " is above 65535");
        }
        if (p.d_out > LINOP_DIM_MAX || p.d_in > LINOP_DIM_MAX)
            throw Error(T4A_GPU_INVALID_ARGUMENT, site + ": dimensions above 65535 are not supported");
        p.result = {p.m_left * sd[i][0], p.d_out, p.m_right * sd[i][2]};
        check_count(sd[i][0], sd[i][1], sd[i][2], 1, site + ": the state's core");
        check_count(p.result[0], p.result[1], p.result[2], 1, site + ": the result's core");
        check_count(p.m_left, p.d_out, p.d_in, p.m_right, site + ": the operator's core"); // at a gap site: that of the composed route
        // the half products of zip-up and fit with an environment of one row, the smallest they can be
        check_count(p.d_out, p.m_left, sd[i][0], 1, site + ": a work matrix");
        check_count(p.d_out, p.m_right, sd[i][2], 1, site + ": a work matrix");
    }
    return plan;
}

std::unique_ptr<Mpo> extend_operator_to_full_space(Mpo& op, const std::vector<size_t>& sites, const std::vector<size_t>& dims)
{
    std::vector<std::array<size_t, 3>> sd(dims.size());
    for (size_t i = 0; i < dims.size(); ++i) sd[i] = {1, dims[i], 1}; // the plan of a product state: the kinds and operator bonds are those of any state
    const std::vector<ApplySitePlan> plan = apply_plan(op.dims4(), sites, sd);
    const size_t n = dims.size();
    for (size_t i = 0; i < n; ++i)
        if (plan[i].kind != ApplySiteKind::Op && dims[i] > 255) // d * d is the fused site index of an identity
            throw Error(T4A_GPU_INVALID_ARGUMENT, "extend_operator_to_full_space: site " + std::to_string(i) + " has dimension " +
                                                      std::to_string(dims[i]) + ", an identity needs at most 255");
    Engine& eng = op.tt.eng;
    const hipStream_t st = eng.stream();
    std::vector<DevCore> cores(n);
    std::vector<std::array<size_t, 2>> osd(n);
    for (size_t i = 0; i < n; ++i) {
        const ApplySitePlan& p = plan[i];
        osd[i] = {p.d_out, p.d_in};
        if (p.kind == ApplySiteKind::Op) cores[i] = clone_core(op.tt.cores[p.op_site], st);
        else cores[i] = upload_site(bridge_site(p.m_left, p.d_in), p.m_left, p.d_in * p.d_in, p.m_left, st);
    }
    eng.sync();
    return std::make_unique<Mpo>(std::move(cores), osd);
}

bool are_exclusive_operators(size_t n, const std::vector<std::vector<size_t>>& supports)
{
    std::vector<char> taken(n, 0);
    for (const std::vector<size_t>& s : supports) {
        if (s.empty()) return false;
        size_t lo = s[0], hi = s[0];
        for (size_t v : s) {
            if (v >= n || taken[v]) return false; // not a node of the target, or shared with another operator (or named twice)
            taken[v] = 1;
            lo = std::min(lo, v), hi = std::max(hi, v);
        }
        if (hi - lo + 1 != s.size()) return false; // not connected: on a chain a support is an interval
    }
    return true;
}

std::unique_ptr<Mpo> compose_exclusive_linear_operators(const std::vector<size_t>& dims, const std::vector<Mpo*>& ops,
                                                        const std::vector<std::vector<size_t>>& supports)
{
    const size_t n = dims.size();
    if (ops.size() != supports.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "compose_exclusive_linear_operators: one list of sites per operator is needed");
    if (!are_exclusive_operators(n, supports))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "compose_exclusive_linear_operators: operators must be exclusive: Operators are not exclusive: they may "
                                              "overlap or not form connected subtrees");
    for (size_t i = 0; i < n; ++i)
        if (dims[i] == 0 || dims[i] > 255) // d * d is the fused site index of an identity
            throw Error(T4A_GPU_INVALID_ARGUMENT, "compose_exclusive_linear_operators: site " + std::to_string(i) + " has dimension " +
                                                      std::to_string(dims[i]) + ", an identity needs 1 .. 255");
    std::vector<const DevCore*> src(n, nullptr);
    std::vector<std::array<size_t, 2>> osd(n);
    for (size_t i = 0; i < n; ++i) osd[i] = {dims[i], dims[i]};
    for (size_t q = 0; q < ops.size(); ++q) {
        const Mpo& o = *ops[q];
        const std::vector<size_t>& s = supports[q];
        if (o.len() != s.size())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "compose_exclusive_linear_operators: operator " + std::to_string(q) + " has " + std::to_string(o.len()) +
                                                      " sites, its `sites` names " + std::to_string(s.size()) + " positions");
        for (size_t j = 0; j < s.size(); ++j) {
            if (j && s[j] != s[j - 1] + 1)
                throw Error(T4A_GPU_INVALID_ARGUMENT, "compose_exclusive_linear_operators: the sites of operator " + std::to_string(q) + " must ascend");
            if (o.sd[j][1] != dims[s[j]])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "Shared shape mismatch at site " + std::to_string(s[j]) + ": operator has input dim " +
                                                          std::to_string(o.sd[j][1]) + ", the state has site dim " + std::to_string(dims[s[j]]));
            src[s[j]] = &o.tt.cores[j];
            osd[s[j]] = o.sd[j];
        }
    }
    if (n == 0) return std::make_unique<Mpo>(std::vector<DevCore>{}, osd);
    Engine eng;
    const hipStream_t st = eng.stream();
    for (Mpo* o : ops) o->tt.eng.sync();
    std::vector<DevCore> cores(n);
    for (size_t i = 0; i < n; ++i) {
        if (src[i]) cores[i] = clone_core(*src[i], st);
        else cores[i] = upload_site(bridge_site(1, dims[i]), 1, dims[i] * dims[i], 1, st);
    }
    eng.sync();
    return std::make_unique<Mpo>(std::move(cores), osd);
}

void apply_validate_options(const ApplyOptions& opt)
{
    if (!(opt.tolerance >= 0.0) || !std::isfinite(opt.tolerance))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: tolerance must be finite and not negative");
    if (opt.has_convergence_tol && (!(opt.convergence_tol >= 0.0) || !std::isfinite(opt.convergence_tol)))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: convergence_tol must be finite and not negative");
    const int m = (int)opt.method;
    if (m < 0 || m > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: unknown method");
}

ApplyRoute apply_route(MpoAlgorithm method, size_t n_sites, size_t n_gap_sites, size_t state_bond, size_t op_bond)
{
    // The sizes at which tools/probe_linop.py measured the fused route faster than the composed one by more than the spread of either
    // (profiles/linop_probe.json): {method, sites, gap sites, largest state bond, largest operator bond}.  The
    // margins are 1 - 8 % of a call (the SVDs dominate both routes), so nothing is read into the sizes between: everything else,
    // Naive and every unmeasured size included, takes the composed route.
    static const size_t wins[][5] = {
        {2, 16, 8, 16, 2},   {1, 16, 8, 64, 2},   {1, 16, 8, 128, 2},  {2, 16, 8, 128, 2},  {1, 16, 8, 16, 8},   {2, 16, 8, 16, 8},   {1, 16, 8, 64, 8},
        {2, 16, 8, 64, 8},   {1, 16, 8, 128, 8},  {2, 16, 8, 128, 8},  {2, 32, 16, 16, 2},  {2, 32, 16, 64, 2},  {1, 32, 16, 128, 2}, {1, 32, 16, 16, 8},
        {2, 32, 16, 16, 8},  {1, 32, 16, 64, 8},  {2, 32, 16, 64, 8},  {1, 32, 16, 128, 8}, {2, 32, 16, 128, 8},
    };
    for (const auto& w : wins)
        if ((size_t)method == w[0] && n_sites == w[1] && n_gap_sites == w[2] && state_bond == w[3] && op_bond == w[4]) return ApplyRoute::Fused;
    return ApplyRoute::Composed;
}

std::unique_ptr<Mpo> apply_linear_operator(Mpo& op, const std::vector<size_t>& sites, TensorTrain& state, const ApplyOptions& opt, ApplyRoute route,
                                           Mpo* initial, MpoFitInfo& info, ApplyRoute* taken)
{
    info = MpoFitInfo{};
    const std::vector<ApplySitePlan> plan = apply_plan(op.dims4(), sites, dims3_of(state));
    apply_validate_options(opt);
    if ((int)route < 0 || (int)route > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: route must be auto, fused or composed");
    const size_t n = state.len();
    size_t n_gap = 0, state_bond = 1, op_bond = 1;
    for (size_t i = 0; i < n; ++i) {
        n_gap += plan[i].kind != ApplySiteKind::Op;
        state_bond = std::max(state_bond, state.cores[i].r);
        op_bond = std::max(op_bond, plan[i].m_right);
    }
    const ApplyRoute rt = route == ApplyRoute::Auto ? apply_route(opt.method, n, n_gap, state_bond, op_bond) : route;
    if (taken) *taken = rt;
    std::vector<std::array<size_t, 2>> rsd(n);
    for (size_t i = 0; i < n; ++i) rsd[i] = {plan[i].d_out, 1};
    MpoFitOptions fo;
    fo.tolerance = opt.tolerance;
    fo.max_bond_dim = opt.max_bond_dim;
    fo.max_sweeps = opt.max_sweeps;
    // no convergence_tol: every sweep runs (|norm_k / norm_{k-1} - 1| < 0 never holds)
    fo.convergence_tol = opt.has_convergence_tol ? opt.convergence_tol : 0.0;
    if (rt == ApplyRoute::Fused) {
        if (opt.method == MpoAlgorithm::Naive) {
            op.tt.eng.sync();
            return std::make_unique<Mpo>(naive_fused(op, state, plan), rsd);
        }
        return linop_fused_contract(op, state, plan, opt.method == MpoAlgorithm::Fit, fo, initial, info);
    }
    // composed: the full-length operator and the kernels of the MPO-MPO contraction
    std::vector<size_t> dims(n);
    std::vector<std::array<size_t, 2>> ssd(n);
    for (size_t i = 0; i < n; ++i) dims[i] = plan[i].d_in, ssd[i] = {plan[i].d_in, 1};
    std::unique_ptr<Mpo> full = extend_operator_to_full_space(op, sites, dims);
    Mpo st(state.cores, state.eng.stream(), ssd);
    if (opt.method == MpoAlgorithm::Fit) return mpo_contract_fit(*full, st, fo, initial, info);
    MpoContractionOptions co;
    co.tolerance = opt.tolerance;
    co.max_bond_dim = opt.max_bond_dim;
    return mpo_partial_contract(*full, st, matrix_product_spec(n), opt.method, false, co);
}

} // namespace t4a
