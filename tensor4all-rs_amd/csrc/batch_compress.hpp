// batch_compress.hpp — the compress stage of mpo.hpp (compress_mpo: right-canonicalise by thin QR, then the left-to-right SVD sweep with
// the rank rule of factorize) for MANY chains in lock step: one workgroup per chain, one launch per site of either sweep for the whole
// batch, one host synchronisation per call (kernels_batch_compress.hip; driver batch_compress.hip).
//
// The slice.  All items of a call have the same number of sites n; site dims and bonds may differ per item.  An item is BATCHED when,
// after the bound the shapes alone give (k_n = 1, k_i = min(l_i, s_i k_{i+1}) from the right), every bond k_i is at most
// BATCH_COMPRESS_BMAX = 64: the Jacobi iteration of a step then works on a square factor of at most 64 x 64 in the LDS.  The longer
// side of a step is bounded only by 64 * s and the MPO layer's own limits.  Every other item of the call (and every item of a call
// routed `Serial`) takes mpo_compress_cores, unchanged; the order of the results is that of the operands.  n <= 1 is a copy.
// Zip-up (whose SVDs interleave with its products) and the add_truncate of partitioned results that share a projector stay serial.
#pragma once

#include <array>
#include <memory>
#include <vector>

#include "mpo.hpp"

namespace t4a {

constexpr int BATCH_COMPRESS_BMAX = 64;
// `Auto` sends the items inside the envelope to the batched kernels when none of their bonds (after the right sweep) is above
// BATCH_COMPRESS_AUTO_SMALL_BOND, or when there are at least BATCH_COMPRESS_AUTO_MIN_ITEMS of them; else every item takes the serial
// stage.  From the measured table: up to bond 16 one batched call beats the serial stage even for a single chain; at
// bond 64 a call costs 25 - 30 ms whatever the number of chains against 9 ms per chain on the serial stage — slower for one chain,
// 4.7 times faster for 16, the smallest count above one that was measured.
constexpr size_t BATCH_COMPRESS_AUTO_MIN_ITEMS = 16;
constexpr size_t BATCH_COMPRESS_AUTO_SMALL_BOND = 16;

enum class CompressRoute : int { Auto = 0, Batched = 1, Serial = 2 };

// ---- device job tables (one entry per item and step; kernels_batch_compress.hip)
// Right step of site i: T is site i as the l x sr matrix it is in memory (sr = s * k_{i+1}), P the left neighbour as the pl x l matrix
// (pl = l' s').  Z receives Q^T (k x sr, k = min(l, sr)) of the thin Householder QR T^T = Q R, Y receives P R^T (pl x k).
struct BcRightJob {
    const double* T;
    const double* P;
    double* Z;
    double* Y;
    double* scratch; // sr * l + sr * k + 3 * k doubles
    int l, sr, pl, k;
};
// Left step of site i: C is the site as the (l s) x r matrix with the ACTUAL l = ranks[prev] (1 for prev < 0; lb bounds it), Nx the right
// neighbour as the r x rest matrix.  U receives U[:, :rank] ((l s) x rank, compact), Nout diag(S) Vt Nx (rank x rest, compact), and
// ranks[cur] the rank.
struct BcLeftJob {
    const double* C;
    const double* Nx;
    double* U;
    double* Nout;
    double* scratch; // max(lb * s, r) * min(lb * s, r) + 64 * 64 + 3 * 64 doubles
    int s, r, rest, lb;
    int prev, cur; // indices into `ranks`
};
// grid = n_items workgroups, job blockIdx.x belongs to item blockIdx.x; flags[item] != 0 (an Inf or NaN was met) makes every later step of the item return at once
void bc_right_step_launch(const BcRightJob* d_jobs, int n_items, int* d_flags, hipStream_t stream);
void bc_left_step_launch(const BcLeftJob* d_jobs, int n_items, int* d_ranks, int* d_flags, double tolerance, int cap, hipStream_t stream);

// ---- the plan: host only, no device is touched
struct CompressManyPlan {
    std::vector<int> batched;               // per item: 1 = the batched kernels, 0 = the serial stage
    std::vector<std::vector<size_t>> bonds; // per item the n + 1 bounds of the result's bonds (1 at both ends)
    std::vector<std::vector<size_t>> qr_bonds; // per item the n + 1 bonds after the right sweep (exact: they follow from the shapes)
    size_t launches = 0;                    // kernel launches of the batched part: 2 (n - 1), whatever the number of items
    size_t syncs = 0;                       // host synchronisations of the batched part: 1 (0 when no item is batched)
    size_t n_batched = 0;
};
// shapes[item][site] = (l, s1, s2, r).  INVALID_ARGUMENT for an empty list, items of different length, a shape mpo_validate_dims refuses
// (with "compress_many: item <k>: " in front); NOT_IMPLEMENTED for RSVD (as the serial stage).
CompressManyPlan compress_many_plan(const std::vector<std::vector<std::array<size_t, 4>>>& shapes, const MpoContractionOptions& opt,
                                    CompressRoute route);

// what a call did: the driver counts the kernel launches and the stream synchronisations of the BATCHED PART, where it issues them.
// Outside the count: mpo_compress_many synchronises every operand's own stream before it reads it, items on the serial stage
// synchronise as that stage always did, and a call with serial items or short chains ends with one more synchronisation.
struct CompressManyStats {
    size_t launches = 0, syncs = 0, n_batched = 0, n_serial = 0;
};

// Compress chains in place.  Every chain is owned by `eng`'s stream (its producer has been synchronised); ends synced.  Throws
// INVALID_ARGUMENT "compress_many: item <k>: SVD computation failed: non-finite input" (the lowest such k); the chains are then
// unspecified and the caller drops them.
void compress_many_cores(Engine& eng, const std::vector<std::vector<DevCore>*>& chains, const MpoContractionOptions& opt, CompressRoute route,
                         CompressManyStats* stats);
// The operands stay untouched; one result per operand, in order.
std::vector<std::unique_ptr<Mpo>> mpo_compress_many(const std::vector<Mpo*>& items, const MpoContractionOptions& opt, CompressRoute route,
                                                    CompressManyStats* stats);
// Edge cases that differ from the serial stage: RSVD is refused up front on every route, also for chains of fewer than two sites (which
// the serial stage copies without reaching its factorisation); an INVALID_ARGUMENT of an item's serial stage carries
// "compress_many: item <k>: " in front, also when the partitioned contraction hands its task products over (k is then the task).
// The serial stage made public: a compressed copy.
std::unique_ptr<Mpo> mpo_compress(Mpo& a, const MpoContractionOptions& opt);
// Timing hook: milliseconds per repetition of the serial and of the batched compress on copies of the same chains, alternating; the
// copies are outside the clock, one warm-up round of each first.
void compress_many_time(Engine& eng, const std::vector<std::vector<DevCore>>& chains, const MpoContractionOptions& opt, size_t reps, double ms[2]);

} // namespace t4a
