// restructure.hpp — fuse_to and split_to (tensor4all-treetn, treetn/transform.rs: fuse_to, contract_node_group, split_to,
// split_tensor_for_targets) and restructure_to (treetn/restructure/mod.rs: build_plan, execute_plan,
// build_path_swap_then_fuse_assignment, apply_final_truncation; options.rs: SplitOptions, RestructureOptions) on a chain, for f64 and
// by position.  With swap_site_indices (swap.hpp) they are the structural family: swap decides which site holds which leg, these
// change the number of sites.
//
// THE TARGET is an ordered list of groups of leg keys; group j is site j of the result, the target topology is the path in list
// order (the reference's SiteIndexNetwork has no positions).  The order of the keys inside a group is the leg order of the result
// site, first leg fastest: this project's rule for these operations (swap steps keep their ascending-key rule).  Refused in the plan,
// before the device is touched: an empty group, a key in two groups, a key set that differs from the train's.
//
// FUSE_TO is exact.  Every site's legs lie in one group, the sites of a group are contiguous, groups ascend along the chain.  Sites
// without legs are absorbed as the reference does, iterated to a fixed point: one between two members of a group joins that group
// (step 4), a dangling one joins the unique neighbouring group and, between two groups, the one of the smaller target index (step 4b).
// All groups are contracted in lock step, left to right inside a group: round t multiplies the accumulated core of every group that
// still has a member left by that member — one fuse_round launch (kernels_restructure.hip) per round for all groups, k_max - 1
// launches for a largest group of k_max sites.  Intermediate rounds write the legs in chain order, a group's last round writes them
// in the target's order.  A group of one site whose order differs goes through legtrain_reorder (one more launch, counted).
// Left-to-right association is this project's fixed choice (the reference contracts from the leaves to the smallest node name).  A
// centre maps to the group that contains it: products of isometries stay isometries.
//
// SPLIT_TO.  Every group's legs lie on one site, the groups of a site are consecutive in the list, sites ascend.  Phase 1 is exact:
// one legtrain_reorder launch makes the legs of every site fragment-major in target order, then fragment after fragment is peeled
// from the left with the thin Householder QR of the engine: the (l |frag|) x (|rest| r) matricisation, Q the fragment, R the
// remainder, the rank by qr_retained_rank at rtol 0; the last fragment is the remainder.  (The reference picks the root fragment from
// a hash-map iteration; peeling left to right is this project's rule.)  The result has no centre.  Phase 2 (final_sweep) is the serial
// truncation stage of batch_truncate.hpp — TensorTrain::truncate — on the one chain with the policy and cap of the options.
//
// RESTRUCTURE_TO plans first (host only), kinds and precedence as build_plan: FuseOnly; SwapThenFuse (every site maps to one group
// but the blocks are not contiguous or not in order: groups in target order take consecutive blocks of as many sites as contribute to
// them, a group's keys in ascending order go to block[min(position, len - 1)]); SplitOnly; SwapOnly (as many groups as sites, group j
// <-> site j); SplitThenFuse (every site split into its fragments in ascending target index, then fused: on a chain this works
// whenever the concatenation over the sites of each site's ascending list of target indices is non-decreasing — wider than the
// reference, which gives up when one site holds two fragments shared with neighbours; by position the fragment order is determined).
// Everything else: NOT_IMPLEMENTED with the reference's placeholder message.
#pragma once

#include "swap.hpp"
#include "tensorops.hpp"

namespace t4a {

using RestructureTarget = std::vector<std::vector<int64_t>>; // group j = site j of the result, first key fastest

enum class RestructureKind : int { FuseOnly = 0, SwapThenFuse = 1, SplitOnly = 2, SwapOnly = 3, SplitThenFuse = 4 };

constexpr size_t RESTRUCTURE_DIM_MAX = 65535; // the tensor train's limit on a (fused) site dimension
constexpr size_t NO_CENTER = (size_t)-1;

struct FusePlan {
    std::vector<std::vector<size_t>> members; // per group its sites, ascending and contiguous; every site is in one group
    SiteLegs legs;                            // of the result
    std::vector<size_t> reorder;              // groups of one site whose leg order differs from the target's
    size_t rounds = 0;                        // k_max - 1
    size_t launches = 0;                      // rounds + (reorder.empty() ? 0 : 1)
};
// Host only.  INVALID_ARGUMENT with the reference's messages ("fuse_to: ambiguous mapping", "fuse_to: missing target for current
// node", "Nodes to contract do not form a connected subtree"), this project's message for contiguous groups that are not in chain
// order, a group of more than FUSE_MAX_LEGS legs, a fused site dimension above 65535 and — with link_dims (n - 1 bonds) — a result
// core above INT_MAX elements.
FusePlan fuse_plan(const SiteLegs& legs, const RestructureTarget& target, const std::vector<size_t>* link_dims);

struct SplitPlan {
    std::vector<std::vector<size_t>> groups; // per site the target groups it is split into, consecutive and ascending
    SiteLegs legs;                           // of the result
    size_t n_qr = 0;                         // sum over the sites of (fragments - 1)
    size_t launches = 0;                     // 1 when a site's legs have to be reordered first
};
// Host only.  INVALID_ARGUMENT with the reference's messages ("split_to: target node .. spans multiple current nodes; use
// restructure_to for mixed regrouping", "..has no corresponding target node").  keep_legless: a site without legs stays a site of its own
// (the split phase of SplitThenFuse; the fuse phase absorbs it) instead of being refused.
SplitPlan split_plan(const SiteLegs& legs, const RestructureTarget& target, bool keep_legless = false);

struct SplitOptions { // SplitOptions::default(): unitary, no truncation, no final sweep
    int form = 0;     // 0 Unitary; 1 LU, 2 CI: NOT_IMPLEMENTED
    bool has_policy = false;
    SvdPolicy policy;
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    bool final_sweep = false;
    void validate() const;
};
struct RestructureOptions {
    SplitOptions split;
    SwapOptions swap;
    bool has_final_truncation = false;
    SvdPolicy final_policy;
    size_t final_max_bond_dim = 0; // 0: no cap
    void validate() const;
};

struct RestructurePlan {
    RestructureKind kind = RestructureKind::FuseOnly;
    SiteLegs legs;                  // of the result
    size_t fuse_rounds = 0;         // of the fuse phase (0: none)
    size_t fuse_launches = 0;
    size_t n_qr = 0;                // of the split phase
    SwapAssignment swap_target;     // the swap kinds
    RestructureTarget split_target; // SplitThenFuse: the fragments in chain order
};
// Host only; link_dims may be null.  INVALID_ARGUMENT "restructure_to: site index .. appears in both target nodes .. and ..",
// "restructure_to: current and target must contain the same site indices"; NOT_IMPLEMENTED with the planner's placeholder message.
RestructurePlan restructure_plan(const SiteLegs& legs, const RestructureTarget& target, const std::vector<size_t>* link_dims);

struct RestructureResult {
    size_t center = NO_CENTER;
    size_t launches = 0; // fuse rounds and reorder launches of the call
    size_t n_qr = 0;
    size_t n_swap_steps = 0;
};
// In place on `cores` (owned by `eng`'s stream) and `legs`; `center` is the train's centre or NO_CENTER.  Each ends synced.
RestructureResult fuse_to(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const RestructureTarget& target, size_t center = NO_CENTER);
RestructureResult split_to(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const RestructureTarget& target, const SplitOptions& opt,
                           bool keep_legless = false);
RestructureResult restructure_to(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const RestructureTarget& target,
                                 const RestructureOptions& opt, size_t center = NO_CENTER, RestructureKind* kind = nullptr);
// TensorTrain::truncate by the serial stage of batch_truncate.hpp on the one chain, in place.
void truncate_chain_serial(Engine& eng, std::vector<DevCore>& cores, const SvdPolicy& policy, size_t max_bond_dim);

// Test hook, the counterpart of swap_theta: host cores A[l, X, m], B[m, Y, r] of several jobs through ONE fuse_round launch.  Per job the
// dims of the result's legs in chain order and, per leg of the result in its new order, its position in chain order (both empty: chain
// order).  Returns the outputs [l, X Y, r] and the route bits (FUSE_ROUTE_*) per job.
struct FuseRoundHostJob {
    const double* A;
    const double* B;
    size_t l, X, m, Y, r;
    std::vector<size_t> leg_dims, order;
};
std::vector<std::vector<double>> fuse_round(const std::vector<FuseRoundHostJob>& jobs, std::vector<int>& routes);
// Timing hook of tools/probe_restructure.py: device ms, per repetition behind a warm-up, of fusing n_groups pairs of binary-leg sites
// with every bond equal to `bond` — the one lock-step fuse_round launch, and the composition a train without it has: one swap_theta
// launch per pair with every leg sent left, issued group by group (constant operands: the time does not depend on the values).
void fuse_time(size_t n_groups, size_t bond, int reps, double* round_ms, double* per_pair_ms);

} // namespace t4a
