// restructure.hip — see restructure.hpp.  The plans are host work; a fuse round runs in fuse_round_kernel (kernels_restructure.hip),
// leg orders in leg_reorder_kernel (kernels_swap.hip), the peeling of split_to in the Householder QR of the engine, the final sweeps
// in the serial stage of batch_truncate.hpp.
#include "restructure.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <functional>
#include <map>
#include <set>
#include <string>

#include "batch_truncate.hpp"
#include "krylov.hpp"

namespace t4a {

namespace {

constexpr size_t NONE = (size_t)-1;

[[noreturn]] void invalid(const std::string& msg) { throw Error(T4A_GPU_INVALID_ARGUMENT, msg); }

std::string str(size_t v) { return std::to_string(v); }
std::string str(int64_t v) { return std::to_string(v); }

size_t fused_dim(const std::vector<SwapLeg>& legs)
{
    size_t s = 1;
    for (const SwapLeg& g : legs) s *= g.dim;
    return s;
}

std::vector<int64_t> keys_of(const std::vector<SwapLeg>& legs)
{
    std::vector<int64_t> k;
    for (const SwapLeg& g : legs) k.push_back(g.key);
    return k;
}

struct TargetMap {
    std::map<int64_t, size_t> group_of, site_of, dim;
};

// the refusals every entry point shares, with the messages of `op` ("fuse_to", "split_to", "restructure_to")
TargetMap check_target(const std::string& op, const SiteLegs& legs, const RestructureTarget& target)
{
    TargetMap tm;
    for (size_t i = 0; i < legs.size(); ++i)
        for (const SwapLeg& g : legs[i]) {
            if (g.dim == 0) invalid(op + ": site index " + str(g.key) + " has dimension 0");
            if (!tm.site_of.emplace(g.key, i).second)
                invalid(op + ": site index " + str(g.key) + " appears in both current nodes " + str(tm.site_of[g.key]) + " and " + str(i));
            tm.dim[g.key] = g.dim;
        }
    for (size_t j = 0; j < target.size(); ++j) {
        if (target[j].empty()) invalid(op + ": target node " + str(j) + " has no site indices");
        for (int64_t key : target[j])
            if (!tm.group_of.emplace(key, j).second)
                invalid(op + ": site index " + str(key) + " appears in both target nodes " + str(tm.group_of[key]) + " and " + str(j));
    }
    for (const auto& t : tm.group_of)
        if (!tm.site_of.count(t.first)) {
            if (op == "fuse_to")
                invalid("fuse_to: incompatible target structure: target node " + str(t.second) + " has site indices not found in the current train");
            if (op == "split_to") invalid("split_to: target site index " + str(t.first) + " is missing from the current network");
            invalid(op + ": current and target must contain the same site indices");
        }
    for (const auto& c : tm.site_of)
        if (!tm.group_of.count(c.first)) {
            if (op == "fuse_to")
                invalid("fuse_to: missing target for current node " + str(c.second) + ": it has site indices but no corresponding target node");
            if (op == "split_to")
                invalid("split_to: incompatible target structure: site index " + str(c.first) + " in current node " + str(c.second) +
                        " has no corresponding target node");
            invalid(op + ": current and target must contain the same site indices");
        }
    return tm;
}

// the ascending list of the target groups the legs of a site lie in
std::vector<size_t> groups_of_site(const std::vector<SwapLeg>& site, const TargetMap& tm)
{
    std::set<size_t> s;
    for (const SwapLeg& g : site) s.insert(tm.group_of.at(g.key));
    return std::vector<size_t>(s.begin(), s.end());
}

// fuse_to steps 2 - 4b and contract_node_group's connectivity on a chain: the group of every site, or why there is none
bool fuse_assign(const SiteLegs& legs, const TargetMap& tm, size_t n_groups, std::vector<size_t>& group, std::string& why)
{
    const size_t n = legs.size();
    group.assign(n, NONE);
    for (size_t i = 0; i < n; ++i) {
        const std::vector<size_t> gs = groups_of_site(legs[i], tm);
        if (gs.size() > 1) {
            why = "fuse_to: ambiguous mapping: current node " + str(i) + " maps to multiple target nodes: " + str(gs[0]) + " and " + str(gs[1]);
            return false;
        }
        if (gs.size() == 1) group[i] = gs[0];
    }
    // step 4: a site without legs between two members of a group joins it
    std::vector<size_t> first(n_groups, NONE), last(n_groups, NONE);
    for (size_t i = 0; i < n; ++i)
        if (group[i] != NONE) {
            if (first[group[i]] == NONE) first[group[i]] = i;
            last[group[i]] = i;
        }
    for (size_t g = 0; g < n_groups; ++g) {
        if (first[g] == NONE) continue;
        for (size_t i = first[g]; i <= last[g]; ++i)
            if (legs[i].empty() && group[i] == NONE) group[i] = g;
    }
    // step 4b, to a fixed point: a dangling one joins the unique neighbouring group; of two neighbouring groups that are neighbours in
    // the target the smaller index (choose_site_free_absorption_target)
    for (;;) {
        std::vector<std::pair<size_t, size_t>> additions;
        for (size_t i = 0; i < n; ++i) {
            if (group[i] != NONE || !legs[i].empty()) continue;
            const size_t a = i > 0 ? group[i - 1] : NONE, b = i + 1 < n ? group[i + 1] : NONE;
            if (a == NONE && b == NONE) continue;
            if (a == NONE || b == NONE || a == b) additions.push_back({i, a == NONE ? b : a});
            else if (std::max(a, b) - std::min(a, b) == 1) additions.push_back({i, std::min(a, b)});
        }
        if (additions.empty()) break;
        for (const auto& ad : additions) group[ad.first] = ad.second;
    }
    for (size_t i = 0; i < n; ++i)
        if (group[i] == NONE) {
            why = "fuse_to: current node " + str(i) + " has no site indices and lies between target nodes that are no neighbours: it cannot be absorbed";
            return false;
        }
    // the members of a group are contiguous ...
    std::vector<size_t> count(n_groups, 0);
    first.assign(n_groups, NONE), last.assign(n_groups, NONE);
    for (size_t i = 0; i < n; ++i) {
        if (first[group[i]] == NONE) first[group[i]] = i;
        last[group[i]] = i;
        ++count[group[i]];
    }
    for (size_t g = 0; g < n_groups; ++g)
        if (count[g] != last[g] - first[g] + 1) {
            why = "fuse_to: failed to contract nodes for target " + str(g) + ": Nodes to contract do not form a connected subtree";
            return false;
        }
    // ... and the groups ascend along the chain
    for (size_t i = 0; i + 1 < n; ++i)
        if (group[i + 1] < group[i]) {
            why = "fuse_to: the groups of the target are contiguous on the chain but not in chain order (target node " + str(group[i]) +
                  " lies left of target node " + str(group[i + 1]) + "); restructure_to can move them";
            return false;
        }
    return true;
}

FusePlan fuse_plan_from(const SiteLegs& legs, const RestructureTarget& target, const TargetMap& tm, const std::vector<size_t>& group,
                        const std::vector<size_t>* link_dims)
{
    const size_t n = legs.size(), G = target.size();
    if (link_dims && link_dims->size() + 1 != n && n)
        invalid("fuse_to: the train has " + str(n) + " sites but " + str(link_dims->size()) + " bonds were given");
    FusePlan p;
    p.members.resize(G);
    for (size_t i = 0; i < n; ++i) p.members[group[i]].push_back(i);
    p.legs.resize(G);
    size_t kmax = 1;
    for (size_t g = 0; g < G; ++g) {
        const std::string where = "fuse_to: target node " + str(g);
        if (target[g].size() > (size_t)FUSE_MAX_LEGS)
            invalid(where + " holds " + str(target[g].size()) + " legs; a fused site holds at most " + str((size_t)FUSE_MAX_LEGS));
        size_t d = 1;
        for (int64_t key : target[g]) {
            const size_t dk = tm.dim.at(key);
            p.legs[g].push_back({key, dk});
            d = dk > RESTRUCTURE_DIM_MAX || d * dk > RESTRUCTURE_DIM_MAX ? RESTRUCTURE_DIM_MAX + 1 : d * dk;
        }
        if (d > RESTRUCTURE_DIM_MAX) invalid(where + " would hold a fused site dimension above 65535");
        const std::vector<size_t>& mem = p.members[g];
        kmax = std::max(kmax, mem.size());
        if (link_dims) { // every accumulated core of the group, the result included
            const unsigned long long l = mem.front() == 0 ? 1 : (*link_dims)[mem.front() - 1];
            unsigned long long x = 1;
            for (size_t s : mem) {
                x *= fused_dim(legs[s]);
                const unsigned long long r = s + 1 == n ? 1 : (*link_dims)[s];
                if (l > (unsigned long long)INT_MAX || r > (unsigned long long)INT_MAX || l * x > (unsigned long long)INT_MAX ||
                    l * x * r > (unsigned long long)INT_MAX)
                    invalid(where + ": the result core would hold more than INT_MAX elements");
            }
        }
        if (mem.size() == 1 && keys_of(legs[mem[0]]) != target[g]) p.reorder.push_back(g);
    }
    p.rounds = kmax - 1;
    p.launches = p.rounds + (p.reorder.empty() ? 0 : 1);
    return p;
}

// split_to's mapping: the site every group lies on, or why there is none
bool split_assign(const SiteLegs& legs, const TargetMap& tm, const RestructureTarget& target, bool keep_legless, std::vector<size_t>& site,
                  std::string& why)
{
    site.assign(target.size(), NONE);
    for (size_t j = 0; j < target.size(); ++j)
        for (int64_t key : target[j]) {
            const size_t s = tm.site_of.at(key);
            if (site[j] != NONE && site[j] != s) {
                why = "split_to: target node " + str(j) + " spans multiple current nodes; use restructure_to for mixed regrouping";
                return false;
            }
            site[j] = s;
        }
    if (!keep_legless)
        for (size_t i = 0; i < legs.size(); ++i)
            if (legs[i].empty()) {
                why = "split_to: current node " + str(i) + " has no site indices and so has no corresponding target node; fuse_to absorbs such nodes";
                return false;
            }
    for (size_t j = 0; j + 1 < target.size(); ++j)
        if (site[j + 1] < site[j]) {
            why = "split_to: the target is not in chain order (target node " + str(j) + " lies on current node " + str(site[j]) + ", target node " +
                  str(j + 1) + " on current node " + str(site[j + 1]) + "); use restructure_to for mixed regrouping";
            return false;
        }
    return true;
}

SplitPlan split_plan_from(const SiteLegs& legs, const RestructureTarget& target, const TargetMap& tm, const std::vector<size_t>& site)
{
    SplitPlan p;
    p.groups.resize(legs.size());
    for (size_t j = 0; j < target.size(); ++j) p.groups[site[j]].push_back(j);
    for (size_t i = 0; i < legs.size(); ++i) {
        if (p.groups[i].empty()) { // a kept site without legs
            p.legs.push_back({});
            continue;
        }
        std::vector<int64_t> order;
        for (size_t j : p.groups[i]) {
            std::vector<SwapLeg> frag;
            for (int64_t key : target[j]) {
                frag.push_back({key, tm.dim.at(key)});
                order.push_back(key);
            }
            p.legs.push_back(std::move(frag));
        }
        p.n_qr += p.groups[i].size() - 1;
        if (order != keys_of(legs[i])) p.launches = 1;
    }
    return p;
}

void check_train(const std::string& op, const std::vector<DevCore>& cores, const SiteLegs& legs)
{
    if (legs.size() != cores.size()) invalid(op + ": legs are given for " + str(legs.size()) + " sites of " + str(cores.size()));
    for (size_t i = 0; i < cores.size(); ++i)
        if (fused_dim(legs[i]) != cores[i].s)
            invalid(op + ": the legs of site " + str(i) + " do not make up its site dimension " + str(cores[i].s));
}

std::vector<size_t> links_of(const std::vector<DevCore>& cores)
{
    std::vector<size_t> links;
    for (size_t i = 0; i + 1 < cores.size(); ++i) links.push_back(cores[i].r);
    return links;
}

// the leg table of a round that writes the chain-order legs `chain` in the order `order`
void leg_table(FuseRoundJob& j, const std::vector<SwapLeg>& chain, const std::vector<int64_t>& order)
{
    j.n_legs = (int)chain.size();
    for (size_t k = 0; k < chain.size(); ++k) {
        j.dim[k] = (int)chain[k].dim;
        size_t stride = 1;
        for (int64_t key : order) {
            if (key == chain[k].key) break;
            for (const SwapLeg& g : chain)
                if (g.key == key) stride *= g.dim;
        }
        j.dst[k] = (int)stride;
    }
}

RestructureResult fuse_run(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const RestructureTarget& target, const FusePlan& plan,
                           size_t center)
{
    RestructureResult res;
    const size_t G = plan.members.size();
    if (!plan.reorder.empty()) {
        std::vector<std::pair<size_t, std::vector<int64_t>>> orders;
        for (size_t g : plan.reorder) orders.push_back({plan.members[g][0], target[g]});
        legtrain_reorder(eng, cores, legs, orders);
    }
    std::vector<std::vector<DevCore>> acc(G); // per group the accumulated core of every round
    std::vector<FuseRoundJob> jobs;
    std::vector<size_t> first(plan.rounds + 1, 0);
    std::vector<unsigned long long> items(plan.rounds, 0);
    for (size_t g = 0; g < G; ++g) acc[g].reserve(plan.members[g].size());
    for (size_t t = 1; t <= plan.rounds; ++t) {
        for (size_t g = 0; g < G; ++g) {
            const std::vector<size_t>& mem = plan.members[g];
            if (mem.size() <= t) continue;
            const DevCore& A = t == 1 ? cores[mem[0]] : acc[g].back();
            const DevCore& B = cores[mem[t]];
            if (A.r != B.l) invalid("fuse_to: the bond between sites " + str(mem[t] - 1) + " and " + str(mem[t]) + " does not match");
            if (A.l == 0 || A.r == 0 || B.r == 0) invalid("fuse_to: a bond of dimension 0");
            DevCore out = DevCore::make(A.l, A.s * B.s, B.r);
            FuseRoundJob j{};
            j.A = A.buf.get(), j.B = B.buf.get(), j.out = out.buf.get();
            j.off = items[t - 1];
            j.l = (int)A.l, j.X = (int)A.s, j.m = (int)A.r, j.Y = (int)B.s, j.r = (int)B.r;
            if (t + 1 == mem.size()) { // the group's last round writes the target's order
                std::vector<SwapLeg> chain;
                for (size_t s : mem) chain.insert(chain.end(), legs[s].begin(), legs[s].end());
                if (keys_of(chain) != target[g]) leg_table(j, chain, target[g]);
            }
            items[t - 1] += fuse_round_items(j.l, j.X, j.Y, j.r);
            jobs.push_back(j);
            acc[g].push_back(std::move(out));
        }
        first[t] = jobs.size();
        if ((items[t - 1] + 3) / 4 > (unsigned long long)INT_MAX) invalid("fuse_to: a round needs more than INT_MAX workgroups");
    }
    hipStream_t st = eng.stream();
    DevBuf<FuseRoundJob> d_jobs;
    if (!jobs.empty()) {
        d_jobs.reserve(jobs.size());
        T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(FuseRoundJob), hipMemcpyHostToDevice, st));
        for (size_t t = 1; t <= plan.rounds; ++t)
            fuse_round_launch(d_jobs.get() + first[t - 1], (int)(first[t] - first[t - 1]), items[t - 1], st);
        T4A_HIP(hipGetLastError());
        eng.sync(); // the old sites and the intermediate cores are released below
    }
    std::vector<DevCore> fresh;
    for (size_t g = 0; g < G; ++g) {
        const std::vector<size_t>& mem = plan.members[g];
        fresh.push_back(mem.size() == 1 ? std::move(cores[mem[0]]) : std::move(acc[g].back()));
        if (center != NO_CENTER && center >= mem.front() && center <= mem.back()) res.center = g;
    }
    cores = std::move(fresh);
    legs = plan.legs;
    res.launches = plan.launches;
    return res;
}

// the legs after swap_site_indices moved every key to assignment[key]: sites a step touches end in ascending key order, the others keep theirs
SiteLegs legs_after_swap(const SiteLegs& legs, const SwapAssignment& target)
{
    SwapAssignment current;
    std::map<int64_t, size_t> dim;
    for (size_t i = 0; i < legs.size(); ++i)
        for (const SwapLeg& g : legs[i]) {
            current.push_back({g.key, i});
            dim[g.key] = g.dim;
        }
    const SwapSchedule sched = swap_schedule_build(legs.size(), current, target, 0);
    std::set<size_t> touched;
    for (const ScheduledSwapStep& s : sched.steps) touched.insert(s.node_a), touched.insert(s.node_b);
    SiteLegs out(legs.size());
    std::map<size_t, std::vector<int64_t>> at;
    for (const auto& t : target) at[t.second].push_back(t.first);
    for (size_t i = 0; i < legs.size(); ++i) {
        if (!touched.count(i)) {
            out[i] = legs[i];
            continue;
        }
        std::vector<int64_t> keys = at[i];
        std::sort(keys.begin(), keys.end());
        for (int64_t key : keys) out[i].push_back({key, dim.at(key)});
    }
    return out;
}

// build_path_swap_then_fuse_assignment on a chain by position
bool swap_then_fuse_assignment(const SiteLegs& legs, const TargetMap& tm, const RestructureTarget& target, SwapAssignment& out)
{
    std::vector<size_t> contributors(target.size(), 0);
    for (const auto& site : legs) {
        const std::vector<size_t> gs = groups_of_site(site, tm);
        if (gs.size() != 1) return false;
        ++contributors[gs[0]];
    }
    size_t cursor = 0;
    out.clear();
    for (size_t j = 0; j < target.size(); ++j) {
        const size_t len = contributors[j];
        if (len == 0 || cursor + len > legs.size() || target[j].size() < len) return false;
        std::vector<int64_t> keys(target[j]);
        std::sort(keys.begin(), keys.end());
        for (size_t pos = 0; pos < keys.size(); ++pos) out.push_back({keys[pos], cursor + std::min(pos, len - 1)});
        cursor += len;
    }
    return cursor == legs.size();
}

void check_policy(const std::string& op, const SvdPolicy& p)
{
    if (!std::isfinite(p.threshold) || p.threshold < 0.0) invalid(op + ": the threshold must be finite and non-negative");
    if (p.scale < 0 || p.scale > 1 || p.measure < 0 || p.measure > 1 || p.rule < 0 || p.rule > 1) invalid(op + ": unknown truncation policy");
}

} // namespace

void SplitOptions::validate() const
{
    if (form != 0) {
        if (form == 1 || form == 2) throw Error(T4A_GPU_NOT_IMPLEMENTED, "split_to: only the unitary form is implemented (LU / CI are not)");
        invalid("split_to: unknown canonical form");
    }
    if (has_max_bond_dim && max_bond_dim == 0) invalid("split_to: max_bond_dim must be positive when specified");
    if (has_policy) check_policy("split_to", policy);
}

void RestructureOptions::validate() const
{
    split.validate();
    swap.validate();
    if (has_final_truncation) check_policy("restructure_to: final truncation", final_policy);
}

FusePlan fuse_plan(const SiteLegs& legs, const RestructureTarget& target, const std::vector<size_t>* link_dims)
{
    const TargetMap tm = check_target("fuse_to", legs, target);
    std::vector<size_t> group;
    std::string why;
    if (!fuse_assign(legs, tm, target.size(), group, why)) invalid(why);
    return fuse_plan_from(legs, target, tm, group, link_dims);
}

SplitPlan split_plan(const SiteLegs& legs, const RestructureTarget& target, bool keep_legless)
{
    const TargetMap tm = check_target("split_to", legs, target);
    std::vector<size_t> site;
    std::string why;
    if (!split_assign(legs, tm, target, keep_legless, site, why)) invalid(why);
    return split_plan_from(legs, target, tm, site);
}

RestructurePlan restructure_plan(const SiteLegs& legs, const RestructureTarget& target, const std::vector<size_t>* link_dims)
{
    const TargetMap tm = check_target("restructure_to", legs, target);
    const size_t n = legs.size(), G = target.size();
    RestructurePlan p;
    bool unique = true;
    for (const auto& site : legs) unique = unique && groups_of_site(site, tm).size() <= 1;
    std::vector<size_t> map;
    std::string why;
    auto take_fuse = [&](const SiteLegs& before, const std::vector<size_t>* links) {
        const FusePlan fp = fuse_plan(before, target, links);
        p.legs = fp.legs;
        p.fuse_rounds = fp.rounds;
        p.fuse_launches = fp.launches;
    };
    if (unique) {
        if (fuse_assign(legs, tm, G, map, why)) {
            p.kind = RestructureKind::FuseOnly;
            take_fuse(legs, link_dims);
            return p;
        }
        if (swap_then_fuse_assignment(legs, tm, target, p.swap_target)) {
            p.kind = RestructureKind::SwapThenFuse;
            take_fuse(legs_after_swap(legs, p.swap_target), nullptr);
            return p;
        }
        p.swap_target.clear();
    }
    if (split_assign(legs, tm, target, false, map, why)) {
        p.kind = RestructureKind::SplitOnly;
        const SplitPlan sp = split_plan_from(legs, target, tm, map);
        p.legs = sp.legs;
        p.n_qr = sp.n_qr;
        return p;
    }
    if (G == n) {
        p.kind = RestructureKind::SwapOnly;
        for (size_t j = 0; j < G; ++j)
            for (int64_t key : target[j]) p.swap_target.push_back({key, j});
        take_fuse(legs_after_swap(legs, p.swap_target), nullptr);
        return p;
    }
    // split every site into its fragments in ascending target index, then fuse: possible whenever the fragments, in chain order, name
    // the target nodes in non-decreasing order
    bool ordered = true;
    size_t prev = 0;
    for (const auto& site : legs)
        for (size_t g : groups_of_site(site, tm)) {
            ordered = ordered && g >= prev;
            prev = g;
        }
    if (ordered) {
        p.kind = RestructureKind::SplitThenFuse;
        for (const auto& site : legs)
            for (size_t g : groups_of_site(site, tm)) {
                std::vector<int64_t> frag;
                for (int64_t key : target[g])
                    for (const SwapLeg& leg : site)
                        if (leg.key == key) frag.push_back(key);
                p.split_target.push_back(std::move(frag));
            }
        const SplitPlan sp = split_plan(legs, p.split_target, true);
        p.n_qr = sp.n_qr;
        take_fuse(sp.legs, nullptr);
        return p;
    }
    throw Error(T4A_GPU_NOT_IMPLEMENTED,
                "restructure_to: planner placeholder only; split/move/mixed restructure planning is not implemented yet");
}

RestructureResult fuse_to(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const RestructureTarget& target, size_t center)
{
    check_train("fuse_to", cores, legs);
    const std::vector<size_t> links = links_of(cores);
    const FusePlan plan = fuse_plan(legs, target, &links);
    return fuse_run(eng, cores, legs, target, plan, center);
}

void truncate_chain_serial(Engine& eng, std::vector<DevCore>& cores, const SvdPolicy& policy, size_t max_bond_dim)
{
    if (cores.empty()) return;
    eng.sync();
    TruncateBatch tb(eng, {&cores}, CompressRoute::Serial);
    tb.canonicalize(false);
    std::vector<std::vector<size_t>> bonds;
    std::vector<std::vector<DevCore>> res = tb.truncate({bt_rule(policy, max_bond_dim)}, false, bonds);
    eng.sync();
    cores = std::move(res[0]);
}

RestructureResult split_to(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const RestructureTarget& target, const SplitOptions& opt,
                           bool keep_legless)
{
    opt.validate();
    check_train("split_to", cores, legs);
    const SplitPlan plan = split_plan(legs, target, keep_legless);
    const size_t n = cores.size();
    // every unfolding of the peeling, before the device is touched (bonds bounded by min(rows, cols) of the step before)
    for (size_t i = 0; i < n; ++i) {
        unsigned long long l = cores[i].l, rest = cores[i].s;
        for (size_t f = 0; f + 1 < plan.groups[i].size(); ++f) {
            unsigned long long F = 1;
            for (int64_t key : target[plan.groups[i][f]])
                for (const SwapLeg& g : legs[i])
                    if (g.key == key) F *= g.dim;
            rest /= F;
            const unsigned long long rows = l * F, cols = rest * cores[i].r;
            const std::string where = "split_to: current node " + str(i) + ", fragment " + str(f);
            Engine::require_factor_dims((size_t)std::min<unsigned long long>(rows, SIZE_MAX), (size_t)std::min<unsigned long long>(cols, SIZE_MAX),
                                        where + ": unfolded dimensions");
            if (rows * cols > (unsigned long long)INT_MAX) invalid(where + ": the unfolding would hold more than INT_MAX elements");
            l = std::min(rows, cols);
        }
    }
    RestructureResult res;
    // phase 1a: fragment-major legs in target order, one launch over all sites
    std::vector<std::pair<size_t, std::vector<int64_t>>> orders;
    for (size_t i = 0; i < n; ++i) {
        std::vector<int64_t> order;
        for (size_t j : plan.groups[i]) order.insert(order.end(), target[j].begin(), target[j].end());
        if (!plan.groups[i].empty() && order != keys_of(legs[i])) orders.push_back({i, std::move(order)});
    }
    if (!orders.empty()) {
        legtrain_reorder(eng, cores, legs, orders);
        res.launches = 1;
    }
    // phase 1b: peel fragment after fragment from the left
    hipStream_t st = eng.stream();
    std::vector<DevCore> fresh;
    DevBuf<double> q, rr;
    for (size_t i = 0; i < n; ++i) {
        DevCore rem = std::move(cores[i]);
        for (size_t f = 0; f + 1 < plan.groups[i].size(); ++f) {
            const size_t F = fused_dim(plan.legs[fresh.size()]);
            const size_t rest = rem.s / F;
            const int rows = (int)(rem.l * F), cols = (int)(rest * rem.r), k = std::min(rows, cols);
            grow(eng, q, (size_t)rows * k);
            grow(eng, rr, (size_t)k * cols);
            eng.qr(rem.buf.get(), rows, cols, q.get(), rr.get());
            const std::vector<double> hr = to_host(eng, rr.get(), (size_t)k * cols);
            const size_t keep = std::min(std::max<size_t>(qr_retained_rank(hr.data(), (size_t)k, (size_t)cols, 0.0), 1), (size_t)k);
            DevCore frag = DevCore::make(rem.l, F, keep), next = DevCore::make(keep, rest, rem.r);
            T4A_HIP(hipMemcpyAsync(frag.buf.get(), q.get(), sizeof(double) * (size_t)rows * keep, hipMemcpyDeviceToDevice, st));
            gather_launch(rr.get(), k, nullptr, (int)keep, nullptr, cols, next.buf.get(), (int)keep, st);
            T4A_HIP(hipGetLastError());
            eng.sync(); // the old remainder is released below
            fresh.push_back(std::move(frag));
            rem = std::move(next);
            ++res.n_qr;
        }
        fresh.push_back(std::move(rem));
    }
    cores = std::move(fresh);
    legs = plan.legs;
    // phase 2
    if (opt.final_sweep) truncate_chain_serial(eng, cores, opt.has_policy ? opt.policy : SvdPolicy(), opt.has_max_bond_dim ? opt.max_bond_dim : 0);
    return res;
}

RestructureResult restructure_to(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const RestructureTarget& target,
                                 const RestructureOptions& opt, size_t center, RestructureKind* kind)
{
    opt.validate();
    check_train("restructure_to", cores, legs);
    const std::vector<size_t> links = links_of(cores);
    const RestructurePlan plan = restructure_plan(legs, target, &links);
    if (kind) *kind = plan.kind;
    RestructureResult res;
    switch (plan.kind) {
    case RestructureKind::FuseOnly:
        res = fuse_to(eng, cores, legs, target, center);
        break;
    case RestructureKind::SplitOnly:
        res = split_to(eng, cores, legs, target, opt.split);
        break;
    case RestructureKind::SwapOnly:
    case RestructureKind::SwapThenFuse: {
        const SwapResult sr = swap_site_indices(eng, cores, legs, plan.swap_target, opt.swap);
        res = fuse_to(eng, cores, legs, target, sr.moved ? sr.center : center); // after a swap-only phase: the leg orders
        res.n_swap_steps = sr.n_steps;
        break;
    }
    case RestructureKind::SplitThenFuse: {
        const RestructureResult sp = split_to(eng, cores, legs, plan.split_target, opt.split, true);
        res = fuse_to(eng, cores, legs, target, NO_CENTER);
        res.launches += sp.launches;
        res.n_qr = sp.n_qr;
        break;
    }
    }
    if (opt.has_final_truncation) {
        truncate_chain_serial(eng, cores, opt.final_policy, opt.final_max_bond_dim);
        res.center = NO_CENTER;
    }
    return res;
}

std::vector<std::vector<double>> fuse_round(const std::vector<FuseRoundHostJob>& host, std::vector<int>& routes)
{
    if (host.empty()) invalid("fuse_round: no job");
    const unsigned long long lim = INT_MAX;
    std::vector<FuseRoundJob> jobs;
    unsigned long long items = 0;
    for (size_t k = 0; k < host.size(); ++k) {
        const FuseRoundHostJob& h = host[k];
        const std::string where = "fuse_round: job " + str(k);
        if (!h.A || !h.B) throw Error(T4A_GPU_NULL_POINTER, where + ": a core is null");
        if (h.l == 0 || h.m == 0 || h.r == 0 || h.X == 0 || h.Y == 0) invalid(where + ": a dimension of 0");
        if (h.X > RESTRUCTURE_DIM_MAX || h.Y > RESTRUCTURE_DIM_MAX || h.X * h.Y > RESTRUCTURE_DIM_MAX)
            invalid(where + ": a fused site dimension above 65535");
        if ((unsigned long long)h.l * h.X * h.m > lim || (unsigned long long)h.m * h.Y * h.r > lim || (unsigned long long)h.l * h.X * h.Y * h.r > lim)
            invalid(where + ": a core would hold more than INT_MAX elements");
        if (h.leg_dims.size() > (size_t)FUSE_MAX_LEGS) invalid(where + ": more than " + str((size_t)FUSE_MAX_LEGS) + " legs");
        FuseRoundJob j{};
        j.off = items;
        j.l = (int)h.l, j.X = (int)h.X, j.m = (int)h.m, j.Y = (int)h.Y, j.r = (int)h.r;
        if (!h.leg_dims.empty()) {
            size_t prod = 1;
            for (size_t d : h.leg_dims) prod *= std::max<size_t>(d, 1);
            std::vector<size_t> sorted(h.order);
            std::sort(sorted.begin(), sorted.end());
            for (size_t q = 0; q < sorted.size(); ++q)
                if (sorted[q] != q) invalid(where + ": the order is no permutation of the legs");
            if (h.order.size() != h.leg_dims.size() || prod != h.X * h.Y || std::count(h.leg_dims.begin(), h.leg_dims.end(), (size_t)0))
                invalid(where + ": the legs do not make up the fused site index of the result");
            std::vector<SwapLeg> chain;
            std::vector<int64_t> order;
            for (size_t q = 0; q < h.leg_dims.size(); ++q) chain.push_back({(int64_t)q, h.leg_dims[q]});
            for (size_t q : h.order) order.push_back((int64_t)q);
            leg_table(j, chain, order);
        }
        items += fuse_round_items(j.l, j.X, j.Y, j.r);
        jobs.push_back(j);
    }
    if ((items + 3) / 4 > lim) invalid("fuse_round needs more than INT_MAX workgroups");
    Engine eng;
    hipStream_t st = eng.stream();
    std::vector<DevBuf<double>> bufs;
    for (size_t k = 0; k < host.size(); ++k) {
        const FuseRoundHostJob& h = host[k];
        bufs.push_back(upload_vector(st, h.A, h.l * h.X * h.m));
        jobs[k].A = bufs.back().get();
        bufs.push_back(upload_vector(st, h.B, h.m * h.Y * h.r));
        jobs[k].B = bufs.back().get();
        DevBuf<double> out;
        out.reserve(h.l * h.X * h.Y * h.r);
        jobs[k].out = out.get();
        bufs.push_back(std::move(out));
    }
    DevBuf<FuseRoundJob> d_jobs;
    d_jobs.reserve(jobs.size());
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(FuseRoundJob), hipMemcpyHostToDevice, st));
    fuse_round_launch(d_jobs.get(), (int)jobs.size(), items, st);
    T4A_HIP(hipGetLastError());
    std::vector<std::vector<double>> res;
    routes.clear();
    for (size_t k = 0; k < host.size(); ++k) {
        res.push_back(to_host(eng, jobs[k].out, host[k].l * host[k].X * host[k].Y * host[k].r));
        routes.push_back(fuse_round_route(jobs[k].l, jobs[k].r));
    }
    return res;
}

void fuse_time(size_t n_groups, size_t bond, int reps, double* round_ms, double* per_pair_ms)
{
    if (n_groups == 0 || bond == 0 || bond > 4096 || reps <= 0 || n_groups * 4 * bond * bond > ((size_t)1 << 27))
        invalid("fuse_time: n_groups > 0, bond in 1 .. 4096, reps > 0 and at most 2^27 result elements are needed");
    Engine eng;
    hipStream_t st = eng.stream();
    const size_t len = bond * 2 * bond, total = 4 * bond * bond;
    DevBuf<double> dA, dB, out;
    dA.reserve(len), dB.reserve(len), out.reserve(total * n_groups);
    fill_launch(dA.get(), len, 0.5, st);
    fill_launch(dB.get(), len, 0.25, st);
    std::vector<FuseRoundJob> jobs(n_groups);
    std::vector<SwapThetaDesc> descs(n_groups);
    unsigned long long items = 0;
    for (size_t g = 0; g < n_groups; ++g) {
        FuseRoundJob& j = jobs[g];
        j = FuseRoundJob{};
        j.A = dA.get(), j.B = dB.get(), j.out = out.get() + g * total;
        j.off = items;
        j.l = j.m = j.r = (int)bond, j.X = j.Y = 2;
        items += fuse_round_items(j.l, 2, 2, j.r);
        SwapThetaDesc& d = descs[g]; // legs 0 (left site) and 1 (right site), both sent left
        d = SwapThetaDesc{};
        d.A = j.A, d.B = j.B, d.out = j.out;
        d.l = d.m = d.r = (int)bond, d.X = d.Y = 2;
        d.Ra = 4, d.Cb = 1, d.n_legs = 2;
        d.dim[0] = d.dim[1] = 2, d.src[0] = d.src[1] = 1, d.dst[0] = 1, d.dst[1] = 2;
        d.from_right[1] = 1;
    }
    DevBuf<FuseRoundJob> d_jobs;
    d_jobs.reserve(n_groups);
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), n_groups * sizeof(FuseRoundJob), hipMemcpyHostToDevice, st));
    const std::function<void()> pieces[2] = {
        [&] { fuse_round_launch(d_jobs.get(), (int)n_groups, items, st); },
        [&] {
            for (const SwapThetaDesc& d : descs) swap_theta_launch(d, st);
        },
    };
    double ms[2] = {0.0, 0.0};
    time_pieces(st, pieces, 2, (size_t)reps, ms);
    eng.sync();
    *round_ms = ms[0];
    *per_pair_ms = ms[1];
}

} // namespace t4a
