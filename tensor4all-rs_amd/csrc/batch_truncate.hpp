// batch_truncate.hpp — TensorTrain::truncate (itensorlike/src/tensortrain.rs:1180, treetn/truncate.rs:129-198) with an SvdPolicy and a cap
// PER ITEM for MANY chains in lock step: canonicalise onto the last site, then the two-site Euler tour from that site, which truncates
// every bond twice with the same rule — once on the way from n - 1 down to 0, once on the way back.  On a canonical chain the two-site
// SVD and the SVD of the centre matrix have the same singular values, so per item the sequence is
//   1. QR to the right   (bt_qr_step_kernel; its last step writes the item's squared norm, the Frobenius norm of the centre site),
//   2. SVD sweep to the left  (bt_svd_step_kernel<true>),
//   3. SVD sweep to the right (bt_svd_step_kernel<false>),
// one workgroup per item, one launch per site and sweep for the whole list: 3 (n - 1) launches.  The two directions of the SVD step are
// MIRRORED INSTANTIATIONS of one kernel (the matricisation is read and the factors are written through the direction's index map); there
// is no reversal launch and no transposed copy of a chain.  Every dimension that an earlier SVD step decided is read from the device rank
// array, so nothing inside a call waits for the host.
//
// The properties of batch_compress.hpp hold: every sum has a fixed order per output element, two runs give the same bits, an item's
// bits do not depend on the batch, a non-finite entry sets the item's flag, a matrix outside 2^-200 .. 2^200 is scaled exactly by a power
// of two, and an item is batched when, after the bound the shapes alone give (k_0 = 1, k_{i+1} = min(k_i s_i, r_{i+1}) from the left),
// every bond is at most BATCH_COMPRESS_BMAX = 64.  Every other item takes the serial stage (QrSweep, Engine::svd, svd_retained_rank:
// the same sequence with the same rule) inside the same call; the results keep the order of the operands.
//
// The rank rule on the device is svd_retained_rank (tensorops.hpp) statement by statement on the singular values the kernel computed,
// for all eight combinations of scale, measure and rule, followed by the cap and the floor of one.
//
// A call with given rules has ONE host synchronisation of the batched part; a caller that derives the rules from the norms
// (pmpo_patching.hpp: volume budgets) reads them after the QR sweep, which is a second one.
#pragma once

#include "batch_compress.hpp"
#include "tensorops.hpp"

namespace t4a {

// the rule of one item: SvdPolicy, the cap (0 = none), and `skip` for an item whose SVD sweeps are not wanted (a dropped patch)
struct BtRule {
    double threshold = 1e-12;
    int scale = 0, measure = 0, rule = 0;
    int cap = 0;
    int skip = 0;
};
inline BtRule bt_rule(const SvdPolicy& p, size_t cap)
{
    BtRule r;
    r.threshold = p.threshold, r.scale = p.scale, r.measure = p.measure, r.rule = p.rule;
    r.cap = (int)std::min<size_t>(cap, 1u << 30);
    return r;
}

// ---- device job tables (one entry per item and step; kernels_batch_truncate.hip)
// QR step of site i: T is the site as the ls x r matrix it is in memory, Nx the right neighbour as the r x rest matrix.  Q receives the
// thin Q (ls x k, k = min(ls, r)), Y receives R Nx (k x rest).  norm2 (the last step only, else null) receives sum Y^2.
struct BtQrJob {
    const double* T;
    const double* Nx;
    double* Q;
    double* Y;
    double* scratch; // ls * r + ls * k + 3 * k doubles
    double* norm2;
    int ls, r, rest, k;
};
// SVD step of the centre site C with site dim s.  `outer` is the bond that stays, `trunc` the bond that is truncated, `far` the other bond
// of the neighbour Nb (site dim nb_s) that takes diag(S) Vt; each is ranks[*_idx], or the host value *_dim where the index is negative
// (the *_dim are bounds otherwise).  Rightward: C is (outer s) x trunc, Nb is trunc x (nb_s far), U the site (outer, s, rank), Nout
// (rank, nb_s, far).  Leftward: C is trunc x (s outer), Nb is (far nb_s) x trunc, U the site (rank, s, outer), Nout (far, nb_s, rank).
// ranks[cur] receives the rank; sv (a test hook, else null) 64 doubles: the singular values, non-increasing, unscaled, zero-filled.
struct BtSvdJob {
    const double* C;
    const double* Nb;
    double* U;
    double* Nout;
    double* scratch; // 2 M N + 64 * 64 + 3 * 64 doubles at the bounds M = outer_dim * s, N = trunc_dim
    double* sv;
    int s, nb_s;
    int outer_dim, trunc_dim, far_dim;
    int outer_idx, trunc_idx, far_idx;
    int cur;
};
// grid = n_items workgroups; flags[item] != 0 or rules[item].skip makes the item's step return at once
void bt_qr_step_launch(const BtQrJob* d_jobs, int n_items, int* d_flags, hipStream_t stream);
void bt_svd_step_launch(bool leftward, const BtSvdJob* d_jobs, int n_items, const BtRule* d_rules, int* d_ranks, int* d_flags, hipStream_t stream);

// ---- the plan: host only
struct TruncateManyPlan {
    std::vector<int> batched;                  // per item: 1 = the kernels, 0 = the serial stage
    std::vector<std::vector<size_t>> bonds;    // per item the n + 1 bounds of the result's bonds
    std::vector<std::vector<size_t>> qr_bonds; // per item the n + 1 bonds after the QR sweep (exact)
    size_t launches = 0;                       // 3 (n - 1) when an item is batched
    size_t syncs = 0;                          // 1 with given rules, 2 when the rules wait for the norms; 0 when no item is batched
    size_t n_batched = 0;
};
// shapes[item][site] = (l, s1, s2, r); caps[item] (0 = none).  INVALID_ARGUMENT as compress_many_plan, with "truncate_many: " in front.
TruncateManyPlan truncate_many_plan(const std::vector<std::vector<std::array<size_t, 4>>>& shapes, const std::vector<size_t>& caps,
                                    CompressRoute route, bool rules_from_norms);

struct TruncateManyStats {
    size_t launches = 0, syncs = 0, n_batched = 0, n_serial = 0;
    double ms[5] = {0, 0, 0, 0, 0}; // with timing on: QR sweep, first sync, leftward sweep, rightward sweep, last sync (wall clock, each drained)
};

// What the test hook records per batched item: norm2, and per SVD step (2 (n - 1) of them, in the order they run) the rank and 64 values.
struct TruncateManyTrace {
    std::vector<double> norm2;              // per item (serial items too)
    std::vector<std::vector<int>> ranks;    // per item, 2 (n - 1)
    std::vector<std::vector<double>> sv;    // per item, 2 (n - 1) * 64
};

// The two phases of a call.  The operands are only read; every chain is owned by `eng`'s stream.
class TruncateBatch {
public:
    TruncateBatch(Engine& eng, std::vector<const std::vector<DevCore>*> in, CompressRoute route, bool trace = false, bool timing = false);
    ~TruncateBatch();
    // phase 1: queues the QR sweep of the batched items and canonicalises the serial ones.  With read_norms it ends synced and norms2() is
    // valid; a non-finite item then throws here.
    void canonicalize(bool read_norms);
    const std::vector<double>& norms2() const { return norm2_; }
    // phase 2: both SVD sweeps under rules[item]; result[item] is empty for a skipped item and, with ranks_only, for every item.
    // bonds[item] receives the n + 1 bonds of the result (empty for a skipped item).  Ends synced.
    std::vector<std::vector<DevCore>> truncate(const std::vector<BtRule>& rules, bool ranks_only, std::vector<std::vector<size_t>>& bonds);
    TruncateManyStats stats;
    TruncateManyTrace trace;

private:
    struct Impl;
    std::unique_ptr<Impl> p_;
    std::vector<double> norm2_;
};

// One call: the rules are given, one synchronisation of the batched part.  Throws INVALID_ARGUMENT
// "truncate_many: item <k>: SVD computation failed: non-finite input" (the lowest such k).
std::vector<std::unique_ptr<Mpo>> mpo_truncate_many(const std::vector<Mpo*>& items, const std::vector<BtRule>& rules, CompressRoute route,
                                                    bool ranks_only, std::vector<std::vector<size_t>>& bonds, TruncateManyStats* stats,
                                                    TruncateManyTrace* trace);

} // namespace t4a
