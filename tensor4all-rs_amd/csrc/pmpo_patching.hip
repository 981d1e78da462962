// pmpo_patching.hip — see pmpo_patching.hpp.  A host driver over the mask launch of pmpo.hip and the batched truncation of
// batch_truncate.hpp; it has no kernel of its own.
#include "pmpo_patching.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

namespace t4a {

namespace {

[[noreturn]] void invalid(const std::string& what) { throw Error(T4A_GPU_INVALID_ARGUMENT, what); }

struct Work { // a subdomain of the loop: masked by its own projector once it has been through budgeted()
    LegProjector proj;
    std::unique_ptr<Mpo> mpo;
    double budget = 0.0;
};

size_t max_bond(const Mpo& m)
{
    size_t b = 1;
    for (const DevCore& c : m.tt.cores) b = std::max(b, c.r);
    return b;
}

// copies of the parents, each masked by its projector: ONE mask launch for all of them
std::vector<std::unique_ptr<Mpo>> project_copies(const std::vector<Mpo*>& parents, const std::vector<LegProjector>& projs, const SiteDims& sd)
{
    std::vector<std::unique_ptr<Mpo>> out;
    for (Mpo* m : parents) out.push_back(std::make_unique<Mpo>(m->tt.cores, m->tt.eng.stream(), sd));
    if (out.empty()) return out;
    std::vector<std::vector<DevCore>*> chains;
    std::vector<const LegProjector*> pp;
    for (size_t k = 0; k < out.size(); ++k) {
        chains.push_back(&out[k]->tt.cores);
        pp.push_back(&projs[k]);
    }
    pmpo_mask_chains(out[0]->tt.eng, chains, pp, sd);
    return out;
}

BtRule budget_rule(double budget, size_t cap)
{
    SvdPolicy pol; // Absolute / SquaredValue / DiscardedTailSum at the budget (truncate_subdomain_with_optional_max_bond_dim, :755-773)
    pol.threshold = budget, pol.scale = 1, pol.measure = 1, pol.rule = 1;
    return bt_rule(pol, cap);
}

void count(PatchingStats& st, const TruncateManyStats& t, bool ranks_only)
{
    ++(ranks_only ? st.ranks_only_calls : st.truncate_calls);
    st.launches += t.launches;
    st.syncs += t.syncs;
}

// patch_stats + the budgets + the drop + the truncation, in one batched call: the norms after its QR sweep, the SVD sweeps under the
// budgets.  Returns the survivors in order, masked, truncated, with their budgets.
std::vector<Work> budgeted_of(const std::vector<Mpo*>& parents, std::vector<LegProjector> projs, const SiteDims& sd, double rtol, size_t cap,
                              CompressRoute route, PatchingStats& st, double* ms5 = nullptr)
{
    std::vector<Work> out;
    if (parents.empty()) return out;
    std::vector<size_t> volumes;
    for (const LegProjector& q : projs) volumes.push_back(patch_volume(q, sd));
    // (the host arithmetic that can refuse runs before the device is touched)
    patch_budgets(volumes, std::vector<double>(parents.size(), 0.0), rtol);
    std::vector<std::unique_ptr<Mpo>> masked = project_copies(parents, projs, sd);
    std::vector<const std::vector<DevCore>*> in;
    for (auto& m : masked) in.push_back(&m->tt.cores);
    TruncateBatch tb(masked[0]->tt.eng, in, route, false, ms5 != nullptr);
    tb.canonicalize(true);
    const PatchBudgets b = patch_budgets(volumes, tb.norms2(), rtol);
    if (b.empty) return out;
    std::vector<BtRule> rules(parents.size());
    for (size_t k = 0; k < parents.size(); ++k) {
        rules[k] = budget_rule(b.budget[k], cap);
        rules[k].skip = b.drop[k];
    }
    std::vector<std::vector<size_t>> bonds;
    std::vector<std::vector<DevCore>> res = tb.truncate(rules, false, bonds);
    count(st, tb.stats, false);
    if (ms5) std::copy(tb.stats.ms, tb.stats.ms + 5, ms5);
    for (size_t k = 0; k < parents.size(); ++k) {
        if (b.drop[k]) continue;
        Work x;
        x.proj = std::move(projs[k]);
        x.mpo = std::make_unique<Mpo>(std::move(res[k]), sd);
        x.budget = b.budget[k];
        out.push_back(std::move(x));
    }
    return out;
}

std::vector<Work> budgeted(std::vector<Work>& w, const SiteDims& sd, double rtol, size_t cap, CompressRoute route, PatchingStats& st)
{
    std::vector<Mpo*> parents;
    std::vector<LegProjector> projs;
    for (Work& x : w) {
        parents.push_back(x.mpo.get());
        projs.push_back(x.proj);
    }
    return budgeted_of(parents, std::move(projs), sd, rtol, cap, route, st);
}

std::unique_ptr<PartitionedMpo> assemble(std::vector<Work>& w, const SiteDims& sd)
{
    auto out = std::make_unique<PartitionedMpo>(sd);
    for (Work& x : w) {
        PmpoPatch p{std::move(x.proj), std::move(x.mpo)};
        p.has_budget = true;
        p.budget_squared = x.budget;
        out->patches.push_back(std::move(p));
    }
    return out;
}

std::vector<Work> working_copy(PartitionedMpo& p)
{
    std::vector<Work> w;
    for (PmpoPatch& q : p.patches) {
        Work x;
        x.proj = q.proj;
        x.mpo = std::make_unique<Mpo>(q.mpo->tt.cores, q.mpo->tt.eng.stream(), p.sd);
        w.push_back(std::move(x));
    }
    return w;
}

LegProjector with_leg(const LegProjector& p, const PatchLeg& leg, size_t value)
{
    LegProjector q = p;
    q[leg] = value;
    return q;
}

// choose_exact_parameter_gain_split (:825-863) for every over-cap patch at once: all children of all candidates in ONE ranks-only call.
// over[k] indexes w, cands[k] are its candidates (not empty); returns the chosen leg per over-cap patch.
std::vector<PatchLeg> exact_parameter_gain(std::vector<Work>& w, const std::vector<size_t>& over, const std::vector<std::vector<PatchLeg>>& cands,
                                           const SiteDims& sd, size_t cap, CompressRoute route, PatchingStats& st)
{
    std::vector<Mpo*> parents;
    std::vector<LegProjector> projs;
    std::vector<double> budgets;
    for (size_t k = 0; k < over.size(); ++k)
        for (const PatchLeg& leg : cands[k]) {
            const size_t dim = sd[leg.first][leg.second];
            for (size_t v = 0; v < dim; ++v) {
                parents.push_back(w[over[k]].mpo.get());
                projs.push_back(with_leg(w[over[k]].proj, leg, v));
                budgets.push_back(w[over[k]].budget / (double)dim);
            }
        }
    std::vector<std::unique_ptr<Mpo>> children = project_copies(parents, projs, sd);
    std::vector<const std::vector<DevCore>*> in;
    for (auto& m : children) in.push_back(&m->tt.cores);
    TruncateBatch tb(children[0]->tt.eng, in, route);
    tb.canonicalize(true);
    std::vector<BtRule> rules(children.size());
    for (size_t c = 0; c < children.size(); ++c) {
        rules[c] = budget_rule(budgets[c], cap);
        rules[c].skip = tb.norms2()[c] <= budgets[c];
    }
    std::vector<std::vector<size_t>> bonds;
    tb.truncate(rules, true, bonds);
    count(st, tb.stats, true);
    std::vector<PatchLeg> chosen;
    size_t c = 0;
    for (size_t k = 0; k < over.size(); ++k) {
        bool have = false;
        size_t best = 0;
        PatchLeg best_leg{};
        for (const PatchLeg& leg : cands[k]) {
            size_t total = 0;
            for (size_t v = 0; v < sd[leg.first][leg.second]; ++v, ++c) {
                if (rules[c].skip) continue;
                for (size_t i = 0; i < sd.size(); ++i) total += bonds[c][i] * sd[i][0] * sd[i][1] * bonds[c][i + 1];
            }
            if (!have || total < best) { // ties keep the first candidate
                have = true;
                best = total;
                best_leg = leg;
            }
        }
        chosen.push_back(best_leg);
    }
    return chosen;
}

// ---- contract_adaptive (:282-412)
struct Operand { // a patch of either operand; shared between the pairs of a group and the projection cache
    LegProjector proj;
    std::shared_ptr<Mpo> mpo;
};
using OperandPair = std::pair<Operand, Operand>;

struct ContractCtx {
    const SiteDims& sda;
    const SiteDims& sdb;
    SiteDims rsd;
    MpoAlgorithm alg;
    MpoContractionOptions copt;
    const PatchingOptions& po;
    CompressRoute route;
    PatchingStats& st;
};

// SubDomainTT::contract (subdomain_tt.rs:388-443) of one pair through the partitioned contraction of two one-patch operands: both are
// projected onto their own projectors inside its product launch.  False when the shared legs disagree.
bool contract_pair(ContractCtx& c, const Operand& a, const Operand& b, Work& out)
{
    PartitionedMpo pa(c.sda), pb(c.sdb);
    pa.patches.push_back({a.proj, std::make_unique<Mpo>(a.mpo->tt.cores, a.mpo->tt.eng.stream(), c.sda)});
    pb.patches.push_back({b.proj, std::make_unique<Mpo>(b.mpo->tt.cores, b.mpo->tt.eng.stream(), c.sdb)});
    std::unique_ptr<PartitionedMpo> r = pa.contract(pb, c.alg, true, c.copt, CompressRoute::Serial);
    if (r->patches.empty()) return false;
    out.proj = std::move(r->patches[0].proj);
    out.mpo = std::move(r->patches[0].mpo);
    return true;
}

// project_if_present (:466-495).  A leg of the result is A's leg 0 or B's leg 1 of the same site: the other operand does not have it and
// is handed on as it is.  The projected operand is truncated with Relative / Value / PerValue at 64 eps.  False: no overlap.
bool project_if_present(ContractCtx& c, const Operand& x, bool is_left, const PatchLeg& leg, size_t value, Operand& out)
{
    if ((leg.second == 0) != is_left) {
        out = x;
        return true;
    }
    auto it = x.proj.find(leg);
    if (it != x.proj.end() && it->second != value) return false;
    const SiteDims& sd = is_left ? c.sda : c.sdb;
    std::vector<std::unique_ptr<Mpo>> masked = project_copies({x.mpo.get()}, {with_leg(x.proj, leg, value)}, sd);
    SvdPolicy pol;
    pol.threshold = 64.0 * std::numeric_limits<double>::epsilon(), pol.scale = 0, pol.measure = 0, pol.rule = 0;
    std::vector<std::vector<size_t>> bonds;
    TruncateManyStats ts;
    std::vector<std::unique_ptr<Mpo>> res = mpo_truncate_many({masked[0].get()}, {bt_rule(pol, 0)}, c.route, false, bonds, &ts, nullptr);
    count(c.st, ts, false);
    out.proj = with_leg(x.proj, leg, value);
    out.mpo = std::move(res[0]);
    return true;
}

// contract_group_project_first (:332-412)
std::vector<Work> contract_group(ContractCtx& c, const std::vector<OperandPair>& pairs, std::vector<Work>* precomputed)
{
    std::vector<Work> contributions;
    if (precomputed) {
        contributions = std::move(*precomputed);
    } else {
        for (const OperandPair& pr : pairs) {
            Work w;
            if (contract_pair(c, pr.first, pr.second, w)) contributions.push_back(std::move(w));
        }
    }
    std::vector<Work> out;
    if (contributions.empty()) return out;
    Work probe;
    probe.proj = contributions[0].proj;
    probe.mpo = std::make_unique<Mpo>(contributions[0].mpo->tt.cores, contributions[0].mpo->tt.eng.stream(), c.rsd);
    const bool trunc = c.copt.tolerance != 0.0 || c.copt.max_bond_dim != 0;
    for (size_t k = 1; k < contributions.size(); ++k) { // add_reindexed_like_self + truncate, as PartitionedMpo::add
        std::unique_ptr<TensorTrain> s = probe.mpo->tt.add(contributions[k].mpo->tt, false);
        std::vector<DevCore> cores = std::move(s->cores);
        if (trunc) mpo_compress_cores(probe.mpo->tt.eng, cores, c.copt);
        probe.mpo->tt.eng.sync();
        probe.mpo = std::make_unique<Mpo>(std::move(cores), c.rsd);
    }
    auto single = [&](Work& w) {
        std::vector<Work> v;
        v.push_back(std::move(w));
        return v;
    };
    if (!c.po.has_max_bond_dim) return single(probe);
    const size_t cap = c.po.max_bond_dim;
    bool saturated = max_bond(*probe.mpo) >= cap;
    for (const Work& w : contributions) saturated = saturated || max_bond(*w.mpo) >= cap;
    if (!saturated) return single(probe);
    // assign_volume_budgets of the probe alone: masked by its projector, its budget the whole rtol^2 |probe|^2
    std::vector<std::unique_ptr<Mpo>> masked = project_copies({probe.mpo.get()}, {probe.proj}, c.rsd);
    const PatchBudgets b = patch_budgets({patch_volume(probe.proj, c.rsd)}, {masked[0]->tt.norm2()}, c.po.rtol);
    if (b.empty) invalid("Partitioned tensor train is empty");
    probe.mpo = std::move(masked[0]);
    probe.budget = b.budget[0];
    const std::vector<PatchLeg> cands = split_candidates(probe.proj, c.rsd, c.po);
    if (cands.empty()) return single(probe);
    PatchLeg leg = cands.front();
    if (c.po.split_strategy == PatchSplitStrategy::ExactParameterGain) {
        std::vector<Work> w = single(probe);
        leg = exact_parameter_gain(w, {0}, {cands}, c.rsd, cap, c.route, c.st)[0];
    }
    ++c.st.splits;
    for (size_t value = 0; value < c.rsd[leg.first][leg.second]; ++value) {
        // each operand is projected once per projector and value; an operand left without an overlap drops its pairs
        std::map<LegProjector, std::pair<bool, Operand>> left, right;
        std::vector<OperandPair> child_pairs;
        for (const OperandPair& pr : pairs) {
            auto l = left.find(pr.first.proj);
            if (l == left.end()) {
                Operand o;
                const bool ok = project_if_present(c, pr.first, true, leg, value, o);
                l = left.emplace(pr.first.proj, std::make_pair(ok, std::move(o))).first;
            }
            auto r = right.find(pr.second.proj);
            if (r == right.end()) {
                Operand o;
                const bool ok = project_if_present(c, pr.second, false, leg, value, o);
                r = right.emplace(pr.second.proj, std::make_pair(ok, std::move(o))).first;
            }
            if (l->second.first && r->second.first) child_pairs.push_back({l->second.second, r->second.second});
        }
        std::vector<Work> children = contract_group(c, child_pairs, nullptr);
        for (Work& w : children) out.push_back(std::move(w));
    }
    return out;
}

} // namespace

void validate_truncation_options(double rtol, bool has_max_bond_dim, size_t max_bond_dim)
{
    if (!std::isfinite(rtol) || rtol < 0.0) invalid("rtol must be finite and non-negative");
    if (has_max_bond_dim && max_bond_dim == 0) invalid("max_bond_dim must be at least 1");
}

void validate_patching_options(const PatchingOptions& o, const SiteDims& sd)
{
    validate_truncation_options(o.rtol, o.has_max_bond_dim, o.max_bond_dim);
    if ((int)o.split_strategy < 0 || (int)o.split_strategy > 1) invalid("unknown patch split strategy");
    for (const PatchLeg& leg : o.patch_order) {
        if (leg.first >= sd.size() || leg.second > 1)
            invalid("patch_order: leg (" + std::to_string(leg.first) + ", " + std::to_string(leg.second) + ") is outside the chain of " +
                    std::to_string(sd.size()) + " sites");
        if (sd[leg.first][leg.second] == 0) invalid("patch_order cannot contain zero-dimensional indices");
    }
}

size_t patch_volume(const LegProjector& p, const SiteDims& sd)
{
    size_t volume = 1;
    for (size_t i = 0; i < sd.size(); ++i)
        for (size_t leg = 0; leg < 2; ++leg) {
            const size_t factor = p.count({i, leg}) ? 1 : sd[i][leg];
            if (factor != 0 && volume > std::numeric_limits<size_t>::max() / factor) invalid("subdomain volume overflowed usize");
            volume *= factor;
        }
    return volume;
}

PatchBudgets patch_budgets(const std::vector<size_t>& volumes, const std::vector<double>& norm2, double rtol)
{
    if (volumes.size() != norm2.size()) invalid("patch budgets: " + std::to_string(volumes.size()) + " volumes but " + std::to_string(norm2.size()) + " norms");
    PatchBudgets b;
    size_t total_volume = 0;
    for (size_t v : volumes) {
        if (v > std::numeric_limits<size_t>::max() - total_volume) invalid("partition volume overflowed usize");
        total_volume += v;
    }
    if (volumes.empty() || total_volume == 0) {
        b.empty = true;
        return b;
    }
    double total_norm2 = 0.0;
    for (double v : norm2) total_norm2 += v;
    if (!std::isfinite(total_norm2)) invalid("partitioned norm is not finite");
    const double global = rtol * rtol * total_norm2;
    if (!std::isfinite(global)) invalid("rtol produced a non-finite truncation budget");
    for (size_t k = 0; k < volumes.size(); ++k) {
        const double budget = global * ((double)volumes[k] / (double)total_volume);
        b.budget.push_back(budget);
        b.drop.push_back(norm2[k] <= budget ? 1 : 0);
    }
    return b;
}

std::vector<PatchLeg> split_candidates(const LegProjector& p, const SiteDims& sd, const PatchingOptions& o)
{
    std::vector<PatchLeg> raw = o.patch_order;
    if (raw.empty())
        for (size_t i = 0; i < sd.size(); ++i)
            for (size_t leg = 0; leg < 2; ++leg)
                if (sd[i][leg] != 1) raw.push_back({i, leg}); // a leg of dimension 1 is no index of the reference's train (s2 = 1)
    std::vector<PatchLeg> out;
    for (const PatchLeg& leg : raw) {
        if (p.count(leg)) continue;
        if (leg.first >= sd.size() || leg.second > 1) continue;
        if (std::find(out.begin(), out.end(), leg) != out.end()) continue;
        out.push_back(leg);
    }
    return out;
}

std::unique_ptr<PartitionedMpo> truncate_adaptive(PartitionedMpo& p, double rtol, bool has_max_bond_dim, size_t max_bond_dim, CompressRoute route,
                                                  PatchingStats* stats, double* ms5)
{
    validate_truncation_options(rtol, has_max_bond_dim, max_bond_dim);
    PatchingStats st;
    std::vector<Mpo*> parents; // the masked copies of the batched call are the only copies: the operands are read where they are
    std::vector<LegProjector> projs;
    for (PmpoPatch& q : p.patches) {
        q.mpo->tt.eng.sync();
        parents.push_back(q.mpo.get());
        projs.push_back(q.proj);
    }
    std::vector<Work> kept = budgeted_of(parents, std::move(projs), p.sd, rtol, has_max_bond_dim ? max_bond_dim : 0, route, st, ms5);
    if (stats) *stats = st;
    return assemble(kept, p.sd);
}

std::unique_ptr<PartitionedMpo> add_with_patching(PartitionedMpo& p, const PatchingOptions& o, CompressRoute route, PatchingStats* stats,
                                                  std::vector<PatchLeg>* chosen)
{
    validate_patching_options(o, p.sd);
    const SiteDims& sd = p.sd;
    const size_t cap = o.has_max_bond_dim ? o.max_bond_dim : 0;
    PatchingStats st;
    std::vector<Work> working = working_copy(p);
    for (;;) {
        ++st.rounds;
        // assign_volume_budgets + budget_truncate_for_split_decision: the budget alone, no cap
        working = budgeted(working, sd, o.rtol, 0, route, st);
        std::vector<size_t> over;
        std::vector<std::vector<PatchLeg>> cands;
        if (cap != 0)
            for (size_t k = 0; k < working.size(); ++k) {
                if (max_bond(*working[k].mpo) <= cap) continue;
                std::vector<PatchLeg> c = split_candidates(working[k].proj, sd, o);
                if (c.empty()) continue; // it stays as it is
                over.push_back(k);
                cands.push_back(std::move(c));
            }
        if (over.empty()) break; // nothing above the cap, or nothing that can be split
        std::vector<PatchLeg> legs;
        if (o.split_strategy == PatchSplitStrategy::Sequential)
            for (const auto& c : cands) legs.push_back(c.front());
        else
            legs = exact_parameter_gain(working, over, cands, sd, cap, route, st);
        // split_subdomain (:886-910) of every over-cap patch: one mask launch for all the children
        std::vector<Mpo*> parents;
        std::vector<LegProjector> projs;
        std::vector<size_t> owner;
        for (size_t k = 0; k < over.size(); ++k) {
            if (chosen) chosen->push_back(legs[k]);
            for (size_t v = 0; v < sd[legs[k].first][legs[k].second]; ++v) {
                parents.push_back(working[over[k]].mpo.get());
                projs.push_back(with_leg(working[over[k]].proj, legs[k], v));
                owner.push_back(over[k]);
            }
        }
        std::vector<std::unique_ptr<Mpo>> children = project_copies(parents, projs, sd);
        std::vector<Work> next;
        size_t c = 0, o_at = 0;
        for (size_t k = 0; k < working.size(); ++k) {
            if (o_at < over.size() && over[o_at] == k) {
                for (; c < owner.size() && owner[c] == k; ++c) {
                    Work x;
                    x.proj = projs[c];
                    x.mpo = std::move(children[c]);
                    next.push_back(std::move(x));
                }
                ++o_at;
                ++st.splits;
            } else {
                next.push_back(std::move(working[k]));
            }
        }
        working = std::move(next);
    }
    // truncate_adaptive over what is left
    std::vector<Work> kept = budgeted(working, sd, o.rtol, cap, route, st);
    if (stats) *stats = st;
    return assemble(kept, sd);
}

std::unique_ptr<PartitionedMpo> contract_adaptive(PartitionedMpo& a, PartitionedMpo& b, MpoAlgorithm alg, const MpoContractionOptions& copt,
                                                  const PatchingOptions& po, CompressRoute route, PatchingStats* stats)
{
    if (a.sd.size() != b.sd.size())
        invalid("MPO length mismatch: expected " + std::to_string(a.sd.size()) + ", got " + std::to_string(b.sd.size()));
    SiteDims rsd(a.sd.size());
    for (size_t i = 0; i < a.sd.size(); ++i) {
        if (a.sd[i][1] != b.sd[i][0])
            invalid("Shared shape mismatch at site " + std::to_string(i) + ": MPO A has site_dim_2=" + std::to_string(a.sd[i][1]) +
                    ", MPO B has site_dim_1=" + std::to_string(b.sd[i][0]));
        rsd[i] = {a.sd[i][0], b.sd[i][1]};
    }
    validate_patching_options(po, rsd);
    PatchingStats st;
    ContractCtx c{a.sd, b.sd, rsd, alg, copt, po, route, st};
    // both sides in the order of projector_compare; the tasks a-major over them, grouped by result projector
    auto sorted = [](PartitionedMpo& p) {
        std::vector<Operand> v;
        for (PmpoPatch& q : p.patches) v.push_back({q.proj, std::make_shared<Mpo>(q.mpo->tt.cores, q.mpo->tt.eng.stream(), p.sd)});
        std::stable_sort(v.begin(), v.end(), [](const Operand& x, const Operand& y) { return projector_compare(x.proj, y.proj) < 0; });
        return v;
    };
    const std::vector<Operand> left = sorted(a), right = sorted(b);
    std::vector<LegProjector> pl, pr;
    for (const Operand& o : left) pl.push_back(o.proj);
    for (const Operand& o : right) pr.push_back(o.proj);
    const PmpoPlan plan = pmpo_contract_plan(pl, pr);
    std::vector<std::vector<OperandPair>> pairs(plan.results.size());
    std::vector<std::vector<Work>> contributions(plan.results.size());
    for (const PmpoTask& t : plan.tasks) {
        Work w;
        if (!contract_pair(c, left[t.a], right[t.b], w)) continue;
        pairs[t.result].push_back({left[t.a], right[t.b]});
        contributions[t.result].push_back(std::move(w));
    }
    std::vector<size_t> order(plan.results.size());
    for (size_t g = 0; g < order.size(); ++g) order[g] = g;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return projector_compare(plan.results[x], plan.results[y]) < 0; });
    std::vector<Work> subdomains;
    for (size_t g : order) {
        std::vector<Work> part = contract_group(c, pairs[g], &contributions[g]);
        for (Work& w : part) subdomains.push_back(std::move(w));
    }
    // from_subdomains (partitioned_tt.rs:104-110)
    for (size_t i = 0; i < subdomains.size(); ++i)
        for (size_t j = i + 1; j < subdomains.size(); ++j)
            if (projector_compatible(subdomains[i].proj, subdomains[j].proj))
                invalid("Projectors overlap: results " + std::to_string(i) + " and " + std::to_string(j) + " of the contraction are not disjoint");
    std::vector<Work> kept = budgeted(subdomains, rsd, po.rtol, po.has_max_bond_dim ? po.max_bond_dim : 0, route, st);
    if (stats) *stats = st;
    return assemble(kept, rsd);
}

} // namespace t4a
