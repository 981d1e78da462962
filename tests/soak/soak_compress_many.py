"""Soak of compress_many (kernels_batch_compress.hip: the batched right and left site steps; batch_compress.hip: the driver) on random
ragged batches against the numpy restatement tests/pmpo_np.py, with the items of tests/compress_many_np.py (sums of orthogonal product
operators on rotated bonds: the spectrum of every cut has a gap, which the soak checks per item before it uses it).
  per batch: 2 - 6 sites, 1 - 40 items, site dims from {(1,1), (2,2), (2,3), (3,1), (8,8)} and bonds from {1, 2, 3, 5, 8, 15, 16, 17, 33,
  64, 65} drawn per site and per item, 1 - 4 terms, now and then an all-zero item or a site scaled by 1e+-120, tolerance 1e-8 with no cap
  or a cap of 2; route "batched".  Checked per item: link dims equal to the restatement's, the error against the exact dense operator at
  most the restatement's plus 1e-10 * max(1, |exact|max), the orthogonality defect of the sites 0 .. n-2 at most that of MPO.compress plus
  1e-10; per batch: the driver's counters against the plan's, the same bits on a second call, the operands unchanged.
Stops at the first failure.
usage: python3 tests/soak/soak_compress_many.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from t4a_amd import MPO, ContractionOptions  # noqa: E402
from t4a_amd import mpo as M  # noqa: E402
import compress_many_np as H  # noqa: E402
import pmpo_np as P  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
SITE_DIMS = [H.A, H.B, H.C, H.D, H.E8]
BONDS = [1, 2, 3, 5, 8, 15, 16, 17, 33, 64, 65]
MARGIN = 1e-10


def bits(ts):
    return [t.view(np.uint64) for t in ts]


def orth_defect(ts):
    worst = 0.0
    for t in ts[:-1]:
        u = t.reshape((-1, t.shape[3]), order="F")
        worst = max(worst, float(np.abs(u.T @ u - np.eye(u.shape[1])).max()))
    return worst


def main():
    t0 = time.time()
    n_items = n_batched = 0
    for case in range(N):
        seed = seed0 + case
        rng = np.random.default_rng(seed)
        n = int(rng.integers(2, 7))
        tol, cap = H.OPTIONS[int(rng.integers(0, len(H.OPTIONS)))]
        items, count = [], int(rng.integers(1, 41))
        while len(items) < count:
            sd = [SITE_DIMS[int(rng.integers(0, len(SITE_DIMS)))] for _ in range(n)]
            if np.prod([a * b for a, b in sd]) > 200000:  # the dense operator is the checker
                continue
            bonds = [1] + [BONDS[int(rng.integers(0, len(BONDS)))] for _ in range(n - 1)] + [1]
            kw = {"terms": int(rng.integers(1, 5)), "zero": rng.random() < 0.05}
            if rng.random() < 0.1:
                kw["scale"] = (int(rng.integers(0, n)), 1e120 if rng.random() < 0.5 else 1e-120)
            item = H.make_item(int(rng.integers(0, 2**31)), sd, bonds, **kw)
            if all(H.gap_ok(c) for c in H.cut_report(item, tol, cap)):
                items.append(item)
        opt = ContractionOptions(tol, cap)
        ops = [MPO(t) for t in items]
        res, counts = M._compress_many(ops, opt, "batched")
        plan = M.compress_many_plan([H.shapes_of(t) for t in items], opt, "batched")
        ctx = f"seed {seed} (n={n}, {len(items)} items, tol={tol}, cap={cap})"
        if (counts["launches"], counts["syncs"], counts["n_batched"]) != (plan["launches"], plan["syncs"], plan["n_batched"]):
            sys.exit(f"FAIL {ctx}: counters {counts} against the plan {plan['launches']}, {plan['syncs']}, {plan['n_batched']}")
        again = M.compress_many(ops, opt, "batched")
        for k, (item, op, r) in enumerate(zip(items, ops, res)):
            got = r.site_tensors()
            want = P.compress(item, tol, cap)
            dense = P.full(item)
            scale = max(1.0, float(np.abs(dense).max()))
            if r.link_dims() != [t.shape[0] for t in want[1:]]:
                sys.exit(f"FAIL {ctx} item {k}: link dims {r.link_dims()} against {[t.shape[0] for t in want[1:]]}")
            err, err_np = float(np.abs(P.full(got) - dense).max()), float(np.abs(P.full(want) - dense).max())
            if not err <= err_np + MARGIN * scale:
                sys.exit(f"FAIL {ctx} item {k}: error {err:.3e}, the restatement's {err_np:.3e}, scale {scale:.3e}")
            mine, serial = orth_defect(got), orth_defect(op.compress(opt).site_tensors())
            if not mine <= serial + MARGIN:
                sys.exit(f"FAIL {ctx} item {k}: orthogonality defect {mine:.3e}, the serial route's {serial:.3e}")
            if not all(np.array_equal(a, b) for a, b in zip(bits(got), bits(again[k].site_tensors()))):
                sys.exit(f"FAIL {ctx} item {k}: a second call gave other bits")
            if not all(np.array_equal(a, b) for a, b in zip(bits(op.site_tensors()), bits(item))):
                sys.exit(f"FAIL {ctx} item {k}: the operand changed")
        n_items += len(items)
        n_batched += counts["n_batched"]
    print(f"{N} batches, {n_items} items ({n_batched} on the kernels), 0 failures, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
