// pmpo_patching.hpp — adaptive patching of partitioned MPOs: crates/tensor4all-partitionedtt/src/patching.rs (the method of "Adaptive
// Patching for Tensor Train Computations", arXiv:2602.22372) on this project's slice: f64, chains, legs (site, leg) in place of index
// objects, MPO patches (a train is the case s2 = 1).
//   truncate_adaptive  (:566-615)  every patch gets an absolute squared-error budget rtol^2 |F|^2 volume_p / sum volume, patches whose
//                                   squared norm is at or below their budget are dropped, the rest are truncated with
//                                   Absolute / SquaredValue / DiscardedTailSum at the budget and the cap
//   add_with_patching  (:154-198)  while a budget-truncated patch stays above the cap it is replaced by its children along a leg
//                                   chosen by the strategy; ends with truncate_adaptive
//   contract_adaptive  (:282-412)  the pairwise products grouped by result projector (projector_compare order); per group the
//                                   contributions are summed by direct sum and truncated after each addition with the rank rule of
//                                   mpo.contract; when the sum or a contribution reaches the cap the group is split along a leg, both
//                                   operands projected per value (once per projector and value, then truncated with Relative / Value /
//                                   PerValue at 64 eps) and the group recurses; ends with truncate_adaptive
// The norms of all patches come from the QR sweep of ONE batched call (batch_truncate.hpp), whose SVD sweeps then run under the budgets:
// two host synchronisations per truncation.  ExactParameterGain puts all children of all candidates of all over-cap patches of a
// round into one ranks-only call.  Deviation as elsewhere in pmpo.hpp: patches keep their insertion order (the reference iterates a hash
// map).  Out of scope: partitionedtreetn, trees, complex scalars, autodiff metadata.
#pragma once

#include "batch_truncate.hpp"
#include "pmpo.hpp"

namespace t4a {

enum class PatchSplitStrategy : int { Sequential = 0, ExactParameterGain = 1 };

using PatchLeg = std::pair<size_t, size_t>; // (site, leg)

struct PatchingOptions { // PatchingOptions::default() (:98-107)
    double rtol = 1e-12;
    bool has_max_bond_dim = true;
    size_t max_bond_dim = 100;
    std::vector<PatchLeg> patch_order;
    PatchSplitStrategy split_strategy = PatchSplitStrategy::ExactParameterGain;
};

// ---- host only: no device is touched
// validate_truncation_options (:684-696): "rtol must be finite and non-negative", "max_bond_dim must be at least 1"
void validate_truncation_options(double rtol, bool has_max_bond_dim, size_t max_bond_dim);
// validate_patching_options (:617-627) on a chain: the above, then per leg of patch_order INVALID_ARGUMENT for a leg outside the chain and
// "patch_order cannot contain zero-dimensional indices"
void validate_patching_options(const PatchingOptions& o, const SiteDims& sd);
// subdomain_volume (:724-738): the product of the dims of the unprojected legs; "subdomain volume overflowed usize"
size_t patch_volume(const LegProjector& p, const SiteDims& sd);
// The budget arithmetic of truncate_adaptive / assign_volume_budgets: budget_p = rtol^2 sum norm2 * (volume_p / sum volume), drop_p =
// norm2_p <= budget_p.  "partition volume overflowed usize", "partitioned norm is not finite", "rtol produced a non-finite truncation
// budget".  A zero total volume (or no patch) gives `empty`.
struct PatchBudgets {
    bool empty = false;
    std::vector<double> budget;
    std::vector<int> drop;
};
PatchBudgets patch_budgets(const std::vector<size_t>& volumes, const std::vector<double>& norm2, double rtol);
// split_candidates (:801-823): the unprojected legs of patch_order, or all legs in chain order when it is empty; duplicates removed.
// With an empty order a leg of dimension 1 is left out: it is the absent s2 of a train, and a split along it changes nothing.
std::vector<PatchLeg> split_candidates(const LegProjector& p, const SiteDims& sd, const PatchingOptions& o);

// what a call did, counted where it is issued
struct PatchingStats {
    size_t rounds = 0;            // rounds of the split loop
    size_t truncate_calls = 0;    // batched calls that hand tensors back
    size_t ranks_only_calls = 0;  // batched calls of ExactParameterGain
    size_t launches = 0, syncs = 0; // of the batched parts of all those calls
    size_t splits = 0;            // patches replaced by their children
};

// The result's patches carry budget_squared.  `route` is that of truncate_many.  ms5 (a probe hook, else null) receives the wall
// milliseconds of the batched part's QR sweep, first synchronisation, leftward sweep, rightward sweep and last synchronisation; the
// stream is then drained after every sweep, which a call without the hook does not do.
std::unique_ptr<PartitionedMpo> truncate_adaptive(PartitionedMpo& p, double rtol, bool has_max_bond_dim, size_t max_bond_dim, CompressRoute route,
                                                  PatchingStats* stats, double* ms5 = nullptr);
// `p` holds the subdomains (its constructor made the checks of from_subdomains).  chosen (optional) receives the leg of every split in
// the order the splits happen.
std::unique_ptr<PartitionedMpo> add_with_patching(PartitionedMpo& p, const PatchingOptions& o, CompressRoute route, PatchingStats* stats,
                                                  std::vector<PatchLeg>* chosen);

// `alg` and `copt` are those of PartitionedMpo::contract (compress on); the legs of `po.patch_order` are legs of the result: (i, 0) is A's
// s1 leg of site i, (i, 1) B's s2 leg.  A host driver over contract, the direct sum, the mask launch and truncate_many.
std::unique_ptr<PartitionedMpo> contract_adaptive(PartitionedMpo& a, PartitionedMpo& b, MpoAlgorithm alg, const MpoContractionOptions& copt,
                                                  const PatchingOptions& po, CompressRoute route, PatchingStats* stats);

} // namespace t4a
