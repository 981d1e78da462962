// swap.hpp — swap_site_indices of tensor4all-treetn on a chain, for f64 and by position (treetn/swap.rs: SwapOptions,
// ScheduledSwapStep, SwapSchedule::build; treetn/mod.rs: swap_on_edge, swap_site_indices): the operation that decides which site
// holds which site index.
//
// A leg train is a chain of device cores over fused site indices plus, per site, an ordered list of legs (key, dim).  Keys are
// unique across the train, the first leg of a site is the fastest in its fused index (s1 + S1 s2 of an Mpo, the groups of the partial
// contraction), a site may hold no leg (s = 1) or several.  An MPO enters with the keys (i, 0), (i, 1) and a tensor train with (i, 0);
// this layer sees a key as one int64 whose order is the order of the keys.
//
// The schedule is host work and follows the reference literally on a chain: the base sweep is for_each_bond_from(root, n, ..) (for
// root 0 the edges (i, i+1) rightwards, then (i+1, i) leftwards), at most n - 1 passes (the diameter), a step only where a targeted
// leg crosses; a leg with a target goes to the side of the edge its target lies on, a leg without one stays; the transport path is
// empty when the centre is on the edge and [centre .. node_a] otherwise; the centre after a step is node_b.  The side sets are sets
// (the reference iterates a hash map); here they are kept in ascending key order.
//
// LEG ORDER WRITTEN BY A STEP (this project's rule: the reference has index objects and no positional order): on both sites of a
// step the legs are stored in ascending key order.  Sites that no step touches keep their order.  legtrain_reorder applies any
// other order.
//
// The driver: an empty target or an empty schedule leaves the train as it is (no canonicalisation, as in the reference); otherwise
// QrSweep::canonicalize(cores, root = 0), then per step the transport of the centre by exact QR steps, the step kernel
// (kernels_swap.hip: the contraction of the two sites written as the matrix the SVD reads, legs redistributed), the truncated SVD
// (threshold = rtol or 0 — never a global default —, Relative / Value / PerValue, max_bond_dim when given) and split_two_site such
// that node_a's site is the isometry and node_b's carries S.  A step at the end of the chain whose one side holds only the
// dimension-1 boundary bond is an ordinary 1 x N or M x 1 SVD (the reference's factorize_or_trivial differs by a sign at most).
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "tt_chain.hpp"

namespace t4a {

struct SwapLeg {
    int64_t key;
    size_t dim;
};
using SiteLegs = std::vector<std::vector<SwapLeg>>;      // per site, first leg fastest
using SwapAssignment = std::vector<std::pair<int64_t, size_t>>; // (key, site)

struct SwapOptions { // SwapOptions::default(): no truncation
    bool has_max_bond_dim = false;
    size_t max_bond_dim = 0;
    bool has_rtol = false;
    double rtol = 0.0;
    void validate() const; // INVALID_ARGUMENT: max_bond_dim == 0 when given, rtol negative or not finite
};

struct ScheduledSwapStep {
    std::vector<size_t> transport_path; // empty, or [centre .. node_a]
    size_t node_a = 0, node_b = 0;
    std::vector<int64_t> a_side, b_side; // ascending
};
struct SwapSchedule {
    size_t root = 0;
    std::vector<ScheduledSwapStep> steps;
};
constexpr size_t SWAP_PASSES_DIAMETER = (size_t)-1;
// Host only.  INVALID_ARGUMENT with the reference's messages: root / a current node / a target node not in the topology, a target key
// "which is not in the network", "did not converge within {n} passes" (max_passes: the diameter n - 1 unless given); and a key that
// occurs twice.
SwapSchedule swap_schedule_build(size_t n_sites, const SwapAssignment& current, const SwapAssignment& target, size_t root,
                                 size_t max_passes = SWAP_PASSES_DIAMETER);
// Host only, before the device is touched: INVALID_ARGUMENT for a step whose merged pair holds more than SWAP_MAX_LEGS (8) legs, a step
// either of whose sides exceeds the train's fused-dimension limit of 65535, and — when link_dims (n - 1 bonds) is given — a work
// matrix above INT_MAX elements (bonds bounded by min(M, N) of the steps before, and by max_bond_dim when non-zero).
void swap_plan_check(const SwapSchedule& sched, const SiteLegs& legs, const std::vector<size_t>* link_dims, size_t max_bond_dim);

struct SwapTimings { // device time per part in ms (tools/probe_swap.py); filled only when asked for
    double kernel_ms = 0.0, svd_ms = 0.0, qr_ms = 0.0;
};
struct SwapResult {
    bool moved = false; // false: nothing was done, no centre
    size_t center = 0;  // node_b of the last step
    size_t n_steps = 0;
};
// swap_on_edge (treetn/mod.rs): one step on the edge (node_a, node_b) of the chain, in place — the two sites contracted by the step
// kernel, factorised by the truncated SVD and split such that a_side lives on node_a (the isometry) and b_side on node_b (with S); the
// centre must be on the edge.  INVALID_ARGUMENT with the reference's messages: "no edge between nodes", "a_side_sites and b_side_sites
// overlap", "scheduled site partition does not match current edge sites".  Ends synced.
struct SwapWork { // buffers reused from step to step
    DevBuf<double> theta, u, s, vt;
    std::vector<double> hs;
};
void swap_on_edge(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, size_t node_a, size_t node_b, const std::vector<int64_t>& a_side,
                  const std::vector<int64_t>& b_side, const SwapOptions& opt, SwapWork& work, SwapTimings* timings = nullptr);
// swap_site_indices: in place on `cores` (owned by `eng`'s stream) and `legs`; ends synced.
SwapResult swap_site_indices(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const SwapAssignment& target, const SwapOptions& opt,
                             SwapTimings* timings = nullptr);

// The launch descriptor of a step on the cores `left` and `right` (chain order) whose legs end as new_left / new_right (each a
// permutation-free split of the merged legs); pointers are filled by the caller.
struct SwapStepPlan {
    std::vector<SwapLeg> new_left, new_right;
    size_t Ra = 1, Cb = 1;
    // per merged leg (left's, then right's): dim, source stride, side and stride of the destination
    std::vector<size_t> dim, src, dst;
    std::vector<bool> from_right, to_col;
};
SwapStepPlan swap_step_plan(const std::vector<SwapLeg>& left, const std::vector<SwapLeg>& right, const std::vector<int64_t>& to_left,
                            const std::vector<int64_t>& to_right);
// Test hook, the counterpart of mpo_partial_half: host cores A[l, X, m], B[m, Y, r] -> Theta' (M x N column-major) exactly as a step
// launches it, with the route bits (SWAP_ROUTE_*).
std::vector<double> swap_theta(const double* left, size_t l, size_t m, const double* right, size_t r, const std::vector<SwapLeg>& legs_left,
                               const std::vector<SwapLeg>& legs_right, const std::vector<int64_t>& to_left, const std::vector<int64_t>& to_right,
                               size_t& M, size_t& N, int& route);
// Timing hook of tools/probe_swap.py: device ms per launch, over `reps` launches behind a warm-up, of the step kernel and of the
// composition GEMM + one permutation launch, for binary legs exchanged at l = m = r = bond (constant operands: the time does not
// depend on the values).
void swap_theta_time(size_t bond, int reps, double* kernel_ms, double* composed_ms);

// The legs of the named sites in another order (a permutation of the site's keys), one gather launch over all of them.
void legtrain_reorder(Engine& eng, std::vector<DevCore>& cores, SiteLegs& legs, const std::vector<std::pair<size_t, std::vector<int64_t>>>& orders);

} // namespace t4a
