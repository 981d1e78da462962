"""Soak of adaptive patching (kernels_batch_truncate.hip: the batched QR and SVD site steps under a rule per item; batch_truncate.hip,
pmpo_patching.hip: the drivers) on random partitioned operands against the numpy restatement tests/patching_np.py.
  per seed: 3 - 6 sites with leg dims from {(2,1), (3,1), (2,2), (2,3)}, 1 - 4 patches on the values of one leg, each a low-rank chain
  plus a small full-bond perturbation (bonds up to 17), now and then a tiny or an all-zero patch; rtol from {1e-2, 1e-4, 1e-6, 0}, a cap
  of 2 or 3 or none; route "batched".  A seed whose restatement has a compared quantity within a relative 1e-6 of its budget is
  redrawn (counted); at rtol = 0, where only exact zeros are cut, no bonds are compared.  Checked: truncate_adaptive — the surviving projectors, the bonds, the budgets, the dense error within the derived
  bound (no cap) or the restatement's (cap), the same bonds on the serial route, the counters; on chains of at most 4 sites
  add_with_patching on the first patch with both strategies — the chosen legs, the projectors and the bonds.
Stops at the first failure.
usage: python3 tests/soak/soak_patching.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from t4a_amd import MPO  # noqa: E402
from t4a_amd import partitioned as P  # noqa: E402
import patching_np as R  # noqa: E402
import patching_cases_np as C  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
DIMS = [C.T2, C.T3, (2, 2), C.M23]
MARGIN = 1e-6


def draw(rng):
    n = int(rng.integers(3, 7))
    sd = [DIMS[int(rng.integers(0, len(DIMS)))] for _ in range(n)]
    ranks = [1] + [int(rng.integers(1, 4)) for _ in range(n - 1)] + [1]
    bonds = [1] + [r + int(rng.integers(1, 15)) for r in ranks[1:-1]] + [1]
    legs = [(i, leg) for i in range(n) for leg in (0, 1) if sd[i][leg] > 1]
    leg = legs[int(rng.integers(0, len(legs)))]
    projs = C.halves(sd, leg)[:int(rng.integers(1, 5))]
    patches = []
    for _ in projs:
        t = C.low_rank_plus(rng, sd, bonds, ranks, 10.0 ** -int(rng.integers(2, 9)))
        u = rng.random()
        t[0] = t[0] * (0.0 if u < 0.05 else 1e-7 if u < 0.15 else float(rng.uniform(0.5, 2.0)))
        patches.append(t)
    rtol = [1e-2, 1e-4, 1e-6, 0.0][int(rng.integers(0, 4))]
    cap = [None, None, 2, 3][int(rng.integers(0, 4))]
    return sd, patches, projs, rtol, cap


def main():
    t0 = time.time()
    redrawn = n_patches = 0
    for case in range(N):
        seed = seed0 + case
        rng = np.random.default_rng(seed)
        while True:
            sd, patches, projs, rtol, cap = draw(rng)
            log, log2 = [], []
            want = R.truncate_adaptive(patches, projs, sd, rtol, cap, log)
            split = []
            for s in (0, 1) if len(sd) <= 4 else ():  # (the restatement of ExactParameterGain on long chains is what a seed costs)
                chosen = []
                split.append((R.add_with_patching(patches[:1], projs[:1], sd, rtol, 2, (), s, log2, chosen=chosen), chosen))
            if min([s[2] for s in log + log2] + [np.inf]) > MARGIN:
                break
            redrawn += 1
        ctx = f"seed {seed} (n={len(sd)}, dims {sd}, {len(patches)} patches, rtol={rtol}, cap={cap})"
        pm = P.PartitionedMPO([MPO(t) for t in patches], projs)
        got, counts = P._truncate_adaptive(pm, rtol, cap, "batched")
        ser, _ = P._truncate_adaptive(pm, rtol, cap, "serial")
        gp = [dict(q.items()) for q in got.projectors()]
        if gp != [p for p, _, _ in want] or gp != [dict(q.items()) for q in ser.projectors()]:
            sys.exit(f"FAIL {ctx}: projectors {gp} against {[p for p, _, _ in want]}")
        # at rtol = 0 the rule cuts exact zeros only: whether a rank-deficient unfolding shows them is a matter of rounding (the two
        # routes differ there too, and the restatement's two-site SVD has min(M, N) values where the centre matrix has the bond), so the
        # bonds are not compared; the projectors and the dense error are
        pinned = rtol != 0.0
        if pinned and (got.link_dims() != [R.link_dims(t) for _, t, _ in want] or got.link_dims() != ser.link_dims()):
            sys.exit(f"FAIL {ctx}: bonds {got.link_dims()} / serial {ser.link_dims()} against {[R.link_dims(t) for _, t, _ in want]}")
        if any(abs(got.budget_squared(k) - b) > 1e-12 * b for k, (_, _, b) in enumerate(want)):
            sys.exit(f"FAIL {ctx}: budgets")
        if (counts["launches"], counts["syncs"]) != (3 * (len(sd) - 1), 2):
            sys.exit(f"FAIL {ctx}: counters {counts}")
        F = sum(R.dense(R.project(t, p)) for t, p in zip(patches, projs))
        norm = float(np.linalg.norm(F))
        if want:
            err, err_np = float(np.linalg.norm(got.full_tensor() - F)), float(np.linalg.norm(R.dense_sum(want, sd) - F))
            bound = C.error_bound(len(sd), rtol, norm) if cap is None else err_np * (1 + 1e-6) + 1e-10 * norm
            if not err <= bound:
                sys.exit(f"FAIL {ctx}: error {err:.3e}, bound {bound:.3e}, the restatement's {err_np:.3e}")
        for strategy, (ref, chosen) in enumerate(split if pinned else ()):
            res, _, legs = P._add_with_patching([MPO(patches[0])], projs[:1], P.PatchingOptions(rtol, 2, [], strategy), "batched")
            if legs != chosen or [dict(q.items()) for q in res.projectors()] != [p for p, _, _ in ref] or \
                    res.link_dims() != [R.link_dims(t) for _, t, _ in ref]:
                sys.exit(f"FAIL {ctx}: add_with_patching strategy {strategy}: legs {legs} against {chosen}, bonds {res.link_dims()}")
        n_patches += len(patches)
    print(f"{N} seeds from {seed0}, {n_patches} patches, {redrawn} redrawn for a margin below {MARGIN}, 0 failures, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
