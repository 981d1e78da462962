"""Soak of the partitioned-MPO layer (kernels_pmpo.hip: the mask launch and the fused pair-product launch; pmpo.hip: tasks, sums,
to_mpo, add) on integer-valued operands against the numpy restatement tests/pmpo_np.py, every comparison EXACT — the assertions of
tests/test_gpu_pmpo_exact.py over random partitions: 1 - 4 sites, site dims (s1, k, s2) per site with s1, s2 in 2 - 3 and k in 1 - 3, A split on an x
leg and inside one x value on a y leg, B split on a z leg and inside one z value on the same y leg (pmpo_np.split_projectors at random
sites: the contracted leg projected by A only, B only, both, neither), every inner bond of every patch drawn from {1, 2, 3, 5, 17},
entries from {-1, 0, 1}.  Bonds are lowered until the exact bound stays below 2^53 and no site product holds more than 2.4 million
elements.
  per case: contract(Naive, compress=False) — projectors, bonds and every site tensor against the restatement, the dense sum against
  the int64 dense product; project onto a random projector; to_mpo; add(tolerance=0) with a shuffled subset of the partition.
usage: python3 tests/soak/soak_pmpo.py N [seed0]     (test infrastructure: numpy int64 is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
from t4a_amd.partitioned import PartitionedMPO  # noqa: E402
import pmpo_np as P  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
BONDS = [1, 2, 3, 5, 17]
SITE_MAX = 2400000
fails = 0
counts = {}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def count(key, by=1):
    counts[key] = counts.get(key, 0) + by


def mismatch(got, want):
    got, want = np.asarray(got), np.rint(np.asarray(want)).astype(np.int64)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    if not np.array_equal(got, np.rint(got)):
        return "values that are no integers"
    bad = np.argwhere(got.astype(np.int64) != want)
    return None if len(bad) == 0 else f"{len(bad)} of {want.size} entries differ, first at {tuple(int(v) for v in bad[0])}"


def patch(rng, n, sd, cap):
    bonds = [1] + [min(cap, BONDS[int(rng.integers(0, len(BONDS)))]) for _ in range(n - 1)] + [1]
    return [rng.integers(-1, 2, size=(bonds[i], sd[i][0], sd[i][1], bonds[i + 1])).astype(np.float64) for i in range(n)]


def compare_patches(ctx, what, dev, want_p, want_t):
    if [p.as_dict() for p in dev.projectors()] != want_p:
        fail(ctx, f"{what}: projectors {dev.projectors()} against {want_p}")
        return
    for k, w in enumerate(want_t):
        for s, (g, ws) in enumerate(zip(dev.patch(k).site_tensors(), w)):
            bad = mismatch(g, ws)
            if bad:
                fail(ctx, f"{what} patch {k} site {s}: {bad}")


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n = int(rng.integers(1, 5))
    dims = [[int(rng.integers(2, 4)), int(rng.integers(1, 4)), int(rng.integers(2, 4))] for _ in range(n)]
    sda, sdb = [(d[0], d[1]) for d in dims], [(d[1], d[2]) for d in dims]
    ys, xs, zs = (int(rng.integers(0, n)) for _ in range(3))
    pa, pb = P.split_projectors(sda, sdb, ys, xs, zs)
    # the dense values are bounded by prod(k) * prod(bond_a * bond_b): cap the bonds so that the bound stays exact and the sites small
    cap = 17
    while np.prod([d[1] for d in dims]) * float(cap) ** (4 * (n - 1)) >= 2 ** 53 / len(pa) / len(pb) or cap ** 4 * 9 > SITE_MAX:
        cap = BONDS[BONDS.index(cap) - 1]
    ta, tb = [patch(rng, n, sda, cap) for _ in pa], [patch(rng, n, sdb, cap) for _ in pb]
    ctx = f"seed {seed0 + case} n {n} dims {dims} ys {ys} xs {xs} zs {zs} cap {cap}"
    try:
        a = PartitionedMPO([t4a.MPO(t) for t in ta], pa)
        b = PartitionedMPO([t4a.MPO(t) for t in tb], pb)
        tasks, _ = P.contraction_tasks(pa, pb)
        count("tasks", len(tasks))
        r = a.contract(b, compress=False)
        want_p, want_t = P.contract(pa, ta, pb, tb, do_compress=False)
        compare_patches(ctx, "contract", r, want_p, want_t)
        fa = P.full_sum([[np.rint(x).astype(np.int64) for x in P.mask(t, p)] for t, p in zip(ta, pa)])
        fb = P.full_sum([[np.rint(x).astype(np.int64) for x in P.mask(t, p)] for t, p in zip(tb, pb)])
        bad = mismatch(r.full_tensor(), P.dense_product(fa, fb))
        if bad:
            fail(ctx, f"dense product: {bad}")
        proj = {(int(rng.integers(0, n)), int(rng.integers(0, 2))): 0}
        compare_patches(ctx, f"project {proj}", a.project(proj), *P.project(pa, ta, proj))
        for s, (g, w) in enumerate(zip(a.to_mpo().site_tensors(), P.to_mpo(pa, ta))):
            bad = mismatch(g, w)
            if bad:
                fail(ctx, f"to_mpo site {s}: {bad}")
        pick = [int(k) for k in rng.permutation(len(pa))[:int(rng.integers(1, len(pa) + 1))]]
        qa, ua = [pa[k] for k in pick], [patch(rng, n, sda, min(cap, 5)) for _ in pick]
        compare_patches(ctx, "add", a.add(PartitionedMPO([t4a.MPO(t) for t in ua], qa), tolerance=0.0), *P.add(pa, ta, qa, ua, tol=0.0))
        count("patches", len(pa) + len(pb))
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
