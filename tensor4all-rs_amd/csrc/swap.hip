// swap.hip — see swap.hpp.  The schedule and the plan checks are host work; the step runs in swap_theta_kernel (kernels_swap.hip),
// the transport in the Householder QR steps of QrSweep, the factorisation in the Jacobi SVD of the engine, the split in
// split_two_site (tt_chain.hpp).
#include "swap.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <functional>
#include <map>
#include <set>
#include <string>

#include "krylov.hpp"
#include "linsolve.hpp"
#include "tensorops.hpp"

namespace t4a {

namespace {

constexpr size_t SWAP_DIM_MAX = 65535; // the tensor train's limit on a (fused) site dimension

[[noreturn]] void invalid(const std::string& msg) { throw Error(T4A_GPU_INVALID_ARGUMENT, msg); }

// is `target` in the component of node_a once the edge (a, b) of the chain is removed
bool on_a_side(size_t a, size_t b, size_t target) { return a < b ? target <= a : target >= a; }

bool satisfied(const std::map<int64_t, size_t>& position, const std::map<int64_t, size_t>& target)
{
    for (const auto& t : target)
        if (position.at(t.first) != t.second) return false;
    return true;
}

size_t fused_dim(const std::vector<SwapLeg>& legs)
{
    size_t s = 1;
    for (const SwapLeg& g : legs) s *= g.dim;
    return s;
}

} // namespace

void SwapOptions::validate() const
{
    if (has_max_bond_dim && max_bond_dim == 0) invalid("swap_site_indices: max_bond_dim must be positive when specified");
    if (has_rtol && (!std::isfinite(rtol) || rtol < 0.0)) invalid("swap_site_indices: rtol must be finite and non-negative");
}

SwapSchedule swap_schedule_build(size_t n, const SwapAssignment& current, const SwapAssignment& target, size_t root, size_t max_passes)
{
    if (root >= n) invalid("SwapSchedule::build: root " + std::to_string(root) + " not in topology");
    std::map<int64_t, size_t> position, tgt;
    for (const auto& c : current) {
        if (c.second >= n)
            invalid("SwapSchedule::build: current node " + std::to_string(c.second) + " for index " + std::to_string(c.first) +
                    " is not in the topology");
        if (!position.emplace(c.first, c.second).second) invalid("SwapSchedule::build: index " + std::to_string(c.first) + " occurs twice in the network");
    }
    for (const auto& t : target) {
        if (!position.count(t.first))
            invalid("SwapSchedule::build: target_assignment contains index " + std::to_string(t.first) + " which is not in the network");
        if (t.second >= n)
            invalid("SwapSchedule::build: target node " + std::to_string(t.second) + " for index " + std::to_string(t.first) +
                    " is not in the topology");
        if (!tgt.emplace(t.first, t.second).second)
            invalid("SwapSchedule::build: target_assignment contains index " + std::to_string(t.first) + " twice");
    }
    if (max_passes == SWAP_PASSES_DIAMETER) max_passes = n - 1; // tree_diameter of a chain
    SwapSchedule sched;
    sched.root = root;
    size_t center = root;
    for (size_t pass = 0; pass < max_passes; ++pass) {
        if (satisfied(position, tgt)) break;
        bool any_moved = false;
        for_each_bond_from(root, n, [&](size_t i, bool move_right) {
            const size_t a = move_right ? i : i + 1, b = move_right ? i + 1 : i;
            ScheduledSwapStep step;
            bool crossing = false;
            for (const auto& p : position) { // ascending keys
                if (p.second != a && p.second != b) continue;
                const auto t = tgt.find(p.first);
                if (t != tgt.end()) {
                    if (on_a_side(a, b, t->second)) {
                        step.a_side.push_back(p.first);
                        crossing |= p.second == b;
                    } else {
                        step.b_side.push_back(p.first);
                        crossing |= p.second == a;
                    }
                } else if (p.second == a) {
                    step.a_side.push_back(p.first);
                } else {
                    step.b_side.push_back(p.first);
                }
            }
            if (!crossing) return;
            if (center != a && center != b) {
                if (center < a)
                    for (size_t k = center; k <= a; ++k) step.transport_path.push_back(k);
                else
                    for (size_t k = center + 1; k-- > a;) step.transport_path.push_back(k);
            }
            step.node_a = a;
            step.node_b = b;
            for (int64_t k : step.a_side) position[k] = a;
            for (int64_t k : step.b_side) position[k] = b;
            sched.steps.push_back(std::move(step));
            center = b;
            any_moved = true;
        });
        if (!any_moved) break;
    }
    if (!satisfied(position, tgt)) invalid("SwapSchedule::build: did not converge within " + std::to_string(max_passes) + " passes");
    return sched;
}

void swap_plan_check(const SwapSchedule& sched, const SiteLegs& legs, const std::vector<size_t>* link_dims, size_t max_bond_dim)
{
    const size_t n = legs.size();
    std::map<int64_t, size_t> dim;
    for (const auto& site : legs)
        for (const SwapLeg& g : site) dim[g.key] = g.dim;
    std::vector<size_t> bond; // bond[i]: between sites i - 1 and i; bond[0] = bond[n] = 1
    if (link_dims) {
        if (link_dims->size() + 1 != n) invalid("swap_site_indices: the train has " + std::to_string(n) + " sites but " +
                                                std::to_string(link_dims->size()) + " bonds were given");
        bond.assign(n + 1, 1);
        for (size_t i = 0; i + 1 < n; ++i) bond[i + 1] = (*link_dims)[i];
    }
    for (size_t k = 0; k < sched.steps.size(); ++k) {
        const ScheduledSwapStep& s = sched.steps[k];
        const std::string where = "swap_site_indices: step " + std::to_string(k) + " on the edge (" + std::to_string(s.node_a) + ", " +
                                  std::to_string(s.node_b) + ")";
        if (s.a_side.size() + s.b_side.size() > (size_t)SWAP_MAX_LEGS)
            invalid(where + " merges " + std::to_string(s.a_side.size() + s.b_side.size()) + " legs; a step holds at most " +
                    std::to_string(SWAP_MAX_LEGS));
        size_t da = 1, db = 1;
        for (const auto* side : {&s.a_side, &s.b_side}) {
            size_t& d = side == &s.a_side ? da : db;
            for (int64_t key : *side) {
                const size_t g = dim.at(key);
                if (g == 0) invalid(where + ": a leg of dimension 0");
                d = g > SWAP_DIM_MAX || d * g > SWAP_DIM_MAX ? SWAP_DIM_MAX + 1 : d * g;
            }
            if (d > SWAP_DIM_MAX) invalid(where + ": a side would hold a fused site dimension above 65535");
        }
        if (link_dims) {
            const size_t left = std::min(s.node_a, s.node_b);
            const size_t dl = s.node_a < s.node_b ? da : db, dr = s.node_a < s.node_b ? db : da;
            const unsigned long long M = (unsigned long long)bond[left] * dl, N = (unsigned long long)dr * bond[left + 2];
            if (M > (unsigned long long)INT_MAX || N > (unsigned long long)INT_MAX || M * N > (unsigned long long)INT_MAX)
                invalid(where + ": the work matrix would hold more than INT_MAX elements");
            size_t nb = (size_t)std::min(M, N);
            if (max_bond_dim) nb = std::min(nb, max_bond_dim);
            bond[left + 1] = nb;
        }
    }
}

SwapStepPlan swap_step_plan(const std::vector<SwapLeg>& left, const std::vector<SwapLeg>& right, const std::vector<int64_t>& to_left,
                            const std::vector<int64_t>& to_right)
{
    SwapStepPlan p;
    std::map<int64_t, size_t> dim;
    for (const auto* site : {&left, &right})
        for (const SwapLeg& g : *site)
            if (!dim.emplace(g.key, g.dim).second) invalid("swap_on_edge: leg " + std::to_string(g.key) + " occurs twice");
    if (dim.size() > (size_t)SWAP_MAX_LEGS) invalid("swap_on_edge: more than " + std::to_string(SWAP_MAX_LEGS) + " legs on the two sites");
        std::map<int64_t, std::pair<bool, size_t>> where; // key -> (to the columns, stride)
    for (const auto* side : {&to_left, &to_right}) {
        const bool col = side == &to_right;
        std::vector<int64_t> keys(*side);
        std::sort(keys.begin(), keys.end());
        size_t stride = 1;
        for (int64_t key : keys) {
            const auto g = dim.find(key);
            if (where.count(key)) invalid("swap_on_edge: a_side_sites and b_side_sites overlap");
            if (g == dim.end()) invalid("swap_on_edge: scheduled site partition does not match current edge sites");
            where[key] = {col, stride};
            (col ? p.new_right : p.new_left).push_back({key, g->second});
            stride *= g->second;
        }
        (col ? p.Cb : p.Ra) = stride;
    }
    if (where.size() != dim.size()) invalid("swap_on_edge: scheduled site partition does not match current edge sites");
    for (const auto* site : {&left, &right}) {
        size_t stride = 1;
        for (const SwapLeg& g : *site) {
            p.dim.push_back(g.dim);
            p.src.push_back(stride);
            p.from_right.push_back(site == &right);
            p.to_col.push_back(where[g.key].first);
            p.dst.push_back(where[g.key].second);
            stride *= g.dim;
        }
    }
    return p;
}

namespace {

SwapThetaDesc step_desc(const SwapStepPlan& p, const double* A, size_t l, size_t X, size_t m, const double* B, size_t Y, size_t r, double* out)
{
    SwapThetaDesc d{};
    d.A = A, d.B = B, d.out = out;
    d.l = (int)l, d.X = (int)X, d.m = (int)m, d.Y = (int)Y, d.r = (int)r;
    d.Ra = (int)p.Ra, d.Cb = (int)p.Cb;
    d.n_legs = (int)p.dim.size();
    for (int j = 0; j < d.n_legs; ++j) {
        d.dim[j] = (int)p.dim[j], d.src[j] = (int)p.src[j], d.dst[j] = (int)p.dst[j];
        d.from_right[j] = p.from_right[j], d.to_col[j] = p.to_col[j];
    }
    return d;
}

// the sizes a step works with, checked before its launch: every count within int, Ra Cb == X Y
void check_step(const SwapStepPlan& p, size_t l, size_t X, size_t m, size_t Y, size_t r, const std::string& where)
{
    const unsigned long long lim = INT_MAX;
    if (p.Ra * p.Cb != X * Y) invalid(where + ": the legs do not make up the fused site indices of the two sites");
    const unsigned long long M = (unsigned long long)l * p.Ra, N = (unsigned long long)p.Cb * r;
    if (M > lim || N > lim || M * N > lim || (unsigned long long)l * X * m > lim || (unsigned long long)m * Y * r > lim)
        invalid(where + ": the work matrix would hold more than INT_MAX elements");
    Engine::require_factor_dims((size_t)M, (size_t)N, where + ": unfolded dimensions");
}

struct PartTimer { // device ms of what runs between start() and stop(), summed; idle unless `on`
    bool on;
    hipStream_t st;
    hipEvent_t e0{}, e1{};
    PartTimer(bool enable, hipStream_t s) : on(enable), st(s)
    {
        if (on) {
            T4A_HIP(hipEventCreate(&e0));
            T4A_HIP(hipEventCreate(&e1));
        }
    }
    ~PartTimer()
    {
        if (on) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
    }
    void start()
    {
        if (on) T4A_HIP(hipEventRecord(e0, st));
    }
    void stop(double& acc)
    {
        if (!on) return;
        T4A_HIP(hipEventRecord(e1, st));
        T4A_HIP(hipEventSynchronize(e1));
        float ms = 0.0f;
        T4A_HIP(hipEventElapsedTime(&ms, e0, e1));
        acc += ms;
    }
};

} // namespace

void swap_on_edge(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, size_t node_a, size_t node_b, const std::vector<int64_t>& a_side,
                  const std::vector<int64_t>& b_side, const SwapOptions& opt, SwapWork& w, SwapTimings* timings)
{
    const size_t n = cores.size();
    if (node_a >= n || node_b >= n || (node_a + 1 != node_b && node_b + 1 != node_a)) invalid("swap_on_edge: no edge between nodes");
    hipStream_t st = eng.stream();
    PartTimer timer(timings != nullptr, st);
    SwapTimings none;
    SwapTimings& tm = timings ? *timings : none;
    const std::string where = "swap_on_edge (" + std::to_string(node_a) + ", " + std::to_string(node_b) + ")";
    const bool move_right = node_a < node_b;
    const size_t i = std::min(node_a, node_b);
    DevCore& A = cores[i];
    DevCore& B = cores[i + 1];
    const SwapStepPlan p = swap_step_plan(legs[i], legs[i + 1], move_right ? a_side : b_side, move_right ? b_side : a_side);
    check_step(p, A.l, A.s, A.r, B.s, B.r, where);
    const int M = (int)(A.l * p.Ra), N = (int)(p.Cb * B.r), kmin = std::min(M, N);
    grow(eng, w.theta, (size_t)M * N);
    grow(eng, w.u, (size_t)M * kmin);
    grow(eng, w.s, (size_t)kmin);
    grow(eng, w.vt, (size_t)kmin * N);
    timer.start();
    if (!swap_theta_launch(step_desc(p, A.buf.get(), A.l, A.s, A.r, B.buf.get(), B.s, B.r, w.theta.get()), st))
        invalid(where + " needs more than INT_MAX workgroups");
    timer.stop(tm.kernel_ms);
    timer.start();
    eng.svd(w.theta.get(), M, N, w.u.get(), w.s.get(), w.vt.get());
    w.hs.resize(kmin);
    T4A_HIP(hipMemcpyAsync(w.hs.data(), w.s.get(), sizeof(double) * kmin, hipMemcpyDeviceToHost, st));
    eng.sync();
    SvdPolicy policy;
    policy.threshold = opt.has_rtol ? opt.rtol : 0.0; // None is 0, never a global default
    policy.scale = 0, policy.measure = 0, policy.rule = 0;
    size_t keep = svd_retained_rank(w.hs.data(), (size_t)kmin, policy);
    if (opt.has_max_bond_dim) keep = std::min(keep, opt.max_bond_dim);
    keep = std::min(std::max<size_t>(keep, 1), (size_t)kmin);
    DevCore nl = DevCore::make(A.l, p.Ra, keep), nr = DevCore::make(keep, p.Cb, B.r);
    // node_a's site is the isometry, node_b's carries S
    split_two_site(st, w.u.get(), M, w.s.get(), w.vt.get(), kmin, N, (int)keep, move_right, nl, nr);
    T4A_HIP(hipGetLastError());
    eng.sync(); // the old sites are released below
    timer.stop(tm.svd_ms);
    A = std::move(nl);
    B = std::move(nr);
    legs[i] = p.new_left;
    legs[i + 1] = p.new_right;
}

SwapResult swap_site_indices(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const SwapAssignment& target, const SwapOptions& opt,
                             SwapTimings* timings)
{
    opt.validate();
    const size_t n = cores.size();
    if (legs.size() != n) invalid("swap_site_indices: legs are given for " + std::to_string(legs.size()) + " sites of " + std::to_string(n));
    SwapAssignment current;
    for (size_t i = 0; i < n; ++i) {
        if (fused_dim(legs[i]) != cores[i].s)
            invalid("swap_site_indices: the legs of site " + std::to_string(i) + " do not make up its site dimension " + std::to_string(cores[i].s));
        for (const SwapLeg& g : legs[i]) current.push_back({g.key, i});
    }
    SwapResult res;
    if (target.empty()) return res;
    const SwapSchedule sched = swap_schedule_build(n, current, target, 0);
    if (sched.steps.empty()) return res;
    std::vector<size_t> links;
    for (size_t i = 0; i + 1 < n; ++i) links.push_back(cores[i].r);
    swap_plan_check(sched, legs, &links, opt.has_max_bond_dim ? opt.max_bond_dim : 0);

    hipStream_t st = eng.stream();
    PartTimer timer(timings != nullptr, st);
    SwapTimings none;
    SwapTimings& tm = timings ? *timings : none;
    QrSweep sweeper(eng);
    timer.start();
    sweeper.canonicalize(cores, sched.root);
    timer.stop(tm.qr_ms);
    SwapWork work;
    for (const ScheduledSwapStep& step : sched.steps) {
        timer.start();
        for (size_t j = 0; j + 1 < step.transport_path.size(); ++j) { // exact, full rank
            const size_t from = step.transport_path[j], to = step.transport_path[j + 1];
            if (to == from + 1) sweeper.left_step(cores, from);
            else sweeper.right_step(cores, from);
        }
        timer.stop(tm.qr_ms);
        swap_on_edge(eng, cores, legs, step.node_a, step.node_b, step.a_side, step.b_side, opt, work, timings);
        res.center = step.node_b;
    }
    res.moved = true;
    res.n_steps = sched.steps.size();
    return res;
}

std::vector<double> swap_theta(const double* left, size_t l, size_t m, const double* right, size_t r, const std::vector<SwapLeg>& legs_left,
                               const std::vector<SwapLeg>& legs_right, const std::vector<int64_t>& to_left, const std::vector<int64_t>& to_right,
                               size_t& M, size_t& N, int& route)
{
    if (l == 0 || m == 0 || r == 0) invalid("swap_theta: a bond of dimension 0");
    for (const auto* site : {&legs_left, &legs_right})
        for (const SwapLeg& g : *site)
            if (g.dim == 0 || g.dim > SWAP_DIM_MAX) invalid("swap_theta: a leg dimension of 0 or above 65535");
    const SwapStepPlan p = swap_step_plan(legs_left, legs_right, to_left, to_right);
    const size_t X = fused_dim(legs_left), Y = fused_dim(legs_right);
    check_step(p, l, X, m, Y, r, "swap_theta");
    M = l * p.Ra, N = p.Cb * r;
    Engine eng;
    hipStream_t st = eng.stream();
    DevBuf<double> dA = upload_vector(st, left, l * X * m), dB = upload_vector(st, right, m * Y * r), out;
    out.reserve(M * N);
    if (!swap_theta_launch(step_desc(p, dA.get(), l, X, m, dB.get(), Y, r, out.get()), st)) invalid("swap_theta needs more than INT_MAX workgroups");
    T4A_HIP(hipGetLastError());
    route = swap_theta_route((int)l, (int)r);
    return to_host(eng, out.get(), M * N);
}

void swap_theta_time(size_t bond, int reps, double* kernel_ms, double* composed_ms)
{
    if (bond == 0 || bond > 4096 || reps <= 0) invalid("swap_theta_time: bond in 1 .. 4096 and reps > 0 are needed");
    // binary legs 0 (left site) and 1 (right site) exchanged: the full redistribution of the quantics regrouping
    const std::vector<SwapLeg> ll{{0, 2}}, lr{{1, 2}};
    const SwapStepPlan p = swap_step_plan(ll, lr, {1}, {0});
    Engine eng;
    hipStream_t st = eng.stream();
    const size_t len = bond * 2 * bond, total = 4 * bond * bond;
    DevBuf<double> dA, dB, out, mid;
    dA.reserve(len), dB.reserve(len), out.reserve(total), mid.reserve(total);
    fill_launch(dA.get(), len, 0.5, st);
    fill_launch(dB.get(), len, 0.25, st);
    const SwapThetaDesc d = step_desc(p, dA.get(), bond, 2, bond, dB.get(), 2, bond, out.get());
    const int M = (int)(2 * bond), N = M, K = (int)bond;
    const TensorView tv{mid.get(), {bond, 2, 2, bond}, {0, 1, 2, 3}};
    const std::vector<size_t> perm{0, 2, 1, 3};
    const std::function<void()> pieces[2] = {
        [&] { swap_theta_launch(d, st); },
        [&] { // the (l x) x m matricisation of A times the m x (y r) one of B needs no reshape launch on these layouts
            gemm_launch(gemm_desc(M, N, K, dA.get(), M, dB.get(), K, mid.get(), M), st);
            tensor_permute(eng, tv, perm, out.get());
        },
    };
    double ms[2] = {0.0, 0.0};
    time_pieces(st, pieces, 2, (size_t)reps, ms);
    eng.sync();
    *kernel_ms = ms[0];
    *composed_ms = ms[1];
}

void legtrain_reorder(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const std::vector<std::pair<size_t, std::vector<int64_t>>>& orders)
{
    const size_t n = cores.size();
    if (legs.size() != n) invalid("reorder_legs: legs are given for " + std::to_string(legs.size()) + " sites of " + std::to_string(n));
    std::vector<LegReorderJob> jobs;
    std::vector<DevCore> fresh;
    std::vector<std::vector<SwapLeg>> new_legs;
    std::set<size_t> seen;
    unsigned long long off = 0;
    for (const auto& o : orders) {
        const size_t i = o.first;
        if (i >= n) invalid("reorder_legs: site " + std::to_string(i) + " is not in the train");
        if (!seen.insert(i).second) invalid("reorder_legs: site " + std::to_string(i) + " is named twice");
        const std::vector<SwapLeg>& old = legs[i];
        if (old.size() > (size_t)SWAP_MAX_LEGS) invalid("reorder_legs: site " + std::to_string(i) + " holds more than " + std::to_string(SWAP_MAX_LEGS) + " legs");
        if (fused_dim(old) != cores[i].s) invalid("reorder_legs: the legs of site " + std::to_string(i) + " do not make up its site dimension");
        std::vector<int64_t> a(o.second), b;
        for (const SwapLeg& g : old) b.push_back(g.key);
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        if (a != b) invalid("reorder_legs: the order of site " + std::to_string(i) + " is not a permutation of its legs");
        if (cores[i].size() > (size_t)INT_MAX) invalid("reorder_legs: site " + std::to_string(i) + " holds more than INT_MAX elements");
        LegReorderJob j{};
        std::vector<SwapLeg> nl;
        for (int64_t key : o.second) {
            size_t stride = 1;
            for (const SwapLeg& g : old) {
                if (g.key == key) {
                    j.dim[j.n_legs] = (int)g.dim;
                    j.stride[j.n_legs] = (int)stride;
                    ++j.n_legs;
                    nl.push_back(g);
                }
                stride *= g.dim;
            }
        }
        fresh.push_back(DevCore::make(cores[i].l, cores[i].s, cores[i].r));
        j.src = cores[i].buf.get();
        j.dst = fresh.back().buf.get();
        j.off = off;
        j.l = (int)cores[i].l, j.s = (int)cores[i].s, j.r = (int)cores[i].r;
        off += cores[i].size();
        jobs.push_back(j);
        new_legs.push_back(std::move(nl));
    }
    if (jobs.empty()) return;
    hipStream_t st = eng.stream();
    DevBuf<LegReorderJob> d_jobs;
    d_jobs.reserve(jobs.size());
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(LegReorderJob), hipMemcpyHostToDevice, st));
    leg_reorder_launch(d_jobs.get(), (int)jobs.size(), off, st);
    T4A_HIP(hipGetLastError());
    eng.sync(); // the old sites are released below
    for (size_t k = 0; k < orders.size(); ++k) {
        cores[orders[k].first] = std::move(fresh[k]);
        legs[orders[k].first] = std::move(new_legs[k]);
    }
}

} // namespace t4a
