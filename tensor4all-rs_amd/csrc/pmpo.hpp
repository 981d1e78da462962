// pmpo.hpp — partitioned MPOs: the algebra of tensor4all-partitionedtt on device-resident MPOs
// (crates/tensor4all-partitionedtt/src/: projector.rs:39-268, subdomain_tt.rs:171-443 project / contract, partitioned_tt.rs:104-480
//  from_subdomains / insert / norm / contract / add / contraction_tasks / to_tensor_train, contract.rs:41-110, error.rs).
// This project's slice: f64 on a chain, sites identified by position, every site an MPO site [left, s1, s2, right] (a train is the
// case s2 = 1).  The reference's index objects are legs here: the key of a projector is (site, leg), leg 0 = s1, leg 1 = s2, and the
// shared index of a contraction A·B is A.(i, 1) == B.(i, 0).  Deviations: the task order of a contraction is fixed (a-major, insertion
// order; the reference iterates a hash map), patches keep their insertion order, and to_mpo sorts by keys then values with a shorter
// prefix first.  A patch may carry budget_squared, the absolute squared-error budget adaptive patching gave it (pmpo_patching.hpp, which
// restates patching.rs); partitionedtreetn, trees, complex scalars and autodiff metadata are out of scope.
#pragma once

#include <map>
#include <utility>

#include "batch_compress.hpp"

namespace t4a {

// (site, leg) -> value; std::map keeps the keys in the canonical order of projector.rs:227-268
using LegProjector = std::map<std::pair<size_t, size_t>, size_t>;
using SiteDims = std::vector<std::array<size_t, 2>>;

// ---- projector.rs on the host (no device call) ----
// from_pairs (projector.rs:57-63): `count` triples (site, leg, value); a key given twice keeps its last value.  leg > 1 is INVALID_ARGUMENT.
LegProjector projector_from_triples(const size_t* triples, size_t count);
// validate_invariants (error.rs ProjectorIndexNotFound / ProjectorCoordinateOutOfBounds): a key outside the chain, a value >= the dim
// of its leg.  INVALID_ARGUMENT with the site, leg, value and dim in the message.
void projector_validate(const LegProjector& p, const SiteDims& sd);
bool projector_compatible(const LegProjector& a, const LegProjector& b);                     // :172-174
bool projector_intersection(const LegProjector& a, const LegProjector& b, LegProjector& out); // :130-145, false on a conflict
LegProjector projector_common_restriction(const LegProjector& a, const LegProjector& b);     // :157-167
bool projector_is_subset_of(const LegProjector& a, const LegProjector& b);                   // :183-194
bool projectors_disjoint(const std::vector<LegProjector>& ps);                               // :199-208
LegProjector projector_filter(const LegProjector& p, const std::vector<std::pair<size_t, size_t>>& keys); // :214-224
// total order of to_mpo: entries ascending by (site, leg) then value, compared in turn, a proper prefix first.  -1 / 0 / 1.
int projector_compare(const LegProjector& a, const LegProjector& b);

// ---- contraction_tasks (partitioned_tt.rs:401-445) on the host ----
struct PmpoTask {
    size_t a, b;   // patch of each operand
    size_t result; // position of the result projector in PmpoPlan::results
};
struct PmpoPlan {
    std::vector<PmpoTask> tasks;       // a-major, insertion order
    std::vector<LegProjector> results; // distinct result projectors in order of first appearance
};
// A's leg-1 entries and B's leg-0 entries name the shared index: a pair is a task when they agree wherever both project.  The result
// projector is A's leg-0 entries plus B's leg-1 entries.
PmpoPlan pmpo_contract_plan(const std::vector<LegProjector>& pa, const std::vector<LegProjector>& pb);

struct PmpoPatch {
    LegProjector proj;
    std::unique_ptr<Mpo> mpo;
    bool has_budget = false; // with_budget_squared (subdomain_tt.rs): set by adaptive patching, not carried through the other operations
    double budget_squared = 0.0;
};

class PartitionedTT; // patching.hpp

class PartitionedMpo {
public:
    explicit PartitionedMpo(SiteDims d) : sd(std::move(d)) {}
    // from_subdomains (partitioned_tt.rs:104-110, insert :196-210).  Every check runs before the device is touched: a patch of another
    // length or other site dims, a projector key or value out of range, projectors that are not pairwise disjoint ("Projectors
    // overlap").  Device copies of the patches are taken; they are not masked (as in the reference) and keep their order.
    static std::unique_ptr<PartitionedMpo> from_patches(const std::vector<Mpo*>& patches, const std::vector<LegProjector>& projectors,
                                                        const SiteDims* site_dims);
    // a PartitionedTT of fused site indices as a partitioned MPO: site i splits into site_dims[2 i] x site_dims[2 i + 1] (NULL: d x 1),
    // every projected fused index into its two legs; the patches are copied
    static std::unique_ptr<PartitionedMpo> from_ptt(PartitionedTT& src, const size_t* site_dims);
    // the host half of from_patches, usable with no patch at hand
    static void validate(const SiteDims& sd, const std::vector<SiteDims>& patch_dims, const std::vector<LegProjector>& projectors);

    size_t len() const { return patches.size(); }
    double norm();                                                    // :286-295, sqrt(sum of the trains' norm2, which is the squared norm)
    std::vector<double> evaluate(const uint32_t* idx, size_t n_pts);  // layout of Mpo::evaluate, summed over the patches
    // SubDomainTT::project (subdomain_tt.rs:171-260) patch by patch: incompatible patches are dropped, the others are copied, masked
    // (all sites of all patches in ONE launch of pmpo_mask_kernel) and carry the intersection of the two projectors
    std::unique_ptr<PartitionedMpo> project(const LegProjector& p);
    // add (:356-398): the union of the projectors must be pairwise disjoint; patches on both sides are added by direct sum and
    // truncated with mpo_compress_cores, the others cloned (self's first, then other's)
    std::unique_ptr<PartitionedMpo> add(PartitionedMpo& other, const MpoContractionOptions& opt);
    // to_tensor_train (:460-480): direct sum in the order of projector_compare.  No patch: "Partitioned tensor train is empty".
    // route 1: the reference's chain of G - 1 pairwise TensorTrain::add; route 2: every site of the result in ONE launch
    // (pmpo_direct_sum_kernel; the same bits: both copy); route 0: the measured rule, which is route 2 from two sites
    // and two patches up.
    std::unique_ptr<Mpo> to_mpo(int route = 0);
    // contract (:305-340), arguments and rank rule of mpo_contract.  compress_route (batch_compress.hpp): Serial compresses the task
    // products one after the other with mpo_compress_cores; Batched and Auto hand all of them to compress_many_cores in one call (Naive
    // with compress only: ZipUp refuses Batched, its SVDs interleave with its products).  The add_truncate of results that share a
    // projector stays serial on every route.
    std::unique_ptr<PartitionedMpo> contract(PartitionedMpo& other, MpoAlgorithm alg, bool compress, const MpoContractionOptions& opt,
                                             CompressRoute compress_route = CompressRoute::Serial);

    SiteDims sd;
    std::vector<PmpoPatch> patches;
};

// Probe hook (tools/probe_pmpo.py): milliseconds per repetition of [0] the fused product launch of every task of a·b, [1] the
// composition "mask launch on copies plus one mpo_site_contract launch per task", [2] the compress stage of every task (tolerance and
// cap of `opt`) on copies of the products.
void pmpo_time_contract(PartitionedMpo& a, PartitionedMpo& b, const MpoContractionOptions& opt, size_t reps, double ms[3]);
// Probe hook (tools/probe_compress_many.py): milliseconds per repetition of the compress stage of every task product of a·b, [0] task by
// task on the serial stage, [1] all tasks in one compress_many_cores call on the batched route; copies of the same products, alternating.
void pmpo_time_compress(PartitionedMpo& a, PartitionedMpo& b, const MpoContractionOptions& opt, size_t reps, double ms[2]);

// Test hook: the product launch of `n_jobs` sites exactly as contract() issues it, host arrays in and out.  dims is 7 x n_jobs
// (la, s1, k, ra, lb, t, rb), sel 4 x n_jobs (k0, k1, sm, tm; sm / tm < 0 = no mask), A / B / C the sites concatenated.
void pmpo_pair_products(const size_t* dims, const long long* sel, size_t n_jobs, const double* A, const double* B, double* C);
// project every listed chain onto its projector: one job per site that carries a projected leg, ONE launch of pmpo_mask_kernel for all
// of them on `eng`'s stream; ends synced
void pmpo_mask_chains(Engine& eng, const std::vector<std::vector<DevCore>*>& chains, const std::vector<const LegProjector*>& projs,
                      const SiteDims& sd);
// Test hook: the mask launch on host arrays.  dims is 4 x n_jobs (l, s1, s2, r), sel 2 x n_jobs (m1, m2; < 0 = none), X in place.
void pmpo_mask_sites(const size_t* dims, const long long* sel, size_t n_jobs, double* X);

} // namespace t4a
