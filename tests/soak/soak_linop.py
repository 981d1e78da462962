"""Soak of apply_linear_operator (csrc/linop.hip, kernels_apply.hip, the fused drivers in csrc/mpo.hip) on random small problems against
the numpy restatement (tests/apply_np.py): 1 - 8 state sites of dimension 2 or 3, state bonds 1 - 5, a random subset of 1 - n sites
for the operator, operator bonds 1 - 3, an output dimension of 2 or 3 per operator site.  Per case: (a) naive on both routes equals the
restated site product within 1e-13 of the scale, with equal link dims, and the fused bits twice; (b) zip-up and fit (two sweeps) on both
routes follow the restatement, equal link dims and a dense result within 1e-10 of the scale, without a cap and with a random one —
unless the restatement's singular values violate the gap condition at a cut (a condition on the inputs: skipped); (c) the half of a
random gap site equals int64 arithmetic on both mirrors.
usage: python3 tests/soak/soak_linop.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
from t4a_amd.linop import _gap_half  # noqa: E402
import apply_np as A  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
counts = {"cases": 0, "skipped_gap": 0, "halves": 0}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def dense(tt):
    return tt.full_tensor().reshape(tt.site_dims(), order="F")


def follows(ctx, got, want, rel):
    if got.link_dims() != [c.shape[0] for c in want[1:]]:
        return fail(ctx, f"link dims {got.link_dims()} != {[c.shape[0] for c in want[1:]]}")
    w = A.np_dense_state(want)
    if np.abs(dense(got) - w).max() > rel * max(np.abs(w).max(), 1e-300):
        fail(ctx, f"dense deviation {np.abs(dense(got) - w).max() / max(np.abs(w).max(), 1e-300):.3e}")


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n = int(rng.integers(1, 9))
    dims = [int(rng.integers(2, 4)) for _ in range(n)]
    bonds = [1] + [int(rng.integers(1, 6)) for _ in range(n - 1)] + [1]
    k = int(rng.integers(1, n + 1))
    sites = tuple(sorted(int(s) for s in rng.choice(n, size=k, replace=False)))
    ob = [1] + [int(rng.integers(1, 4)) for _ in range(k - 1)] + [1]
    x = [rng.uniform(-0.5, 0.5, (bonds[i], dims[i], bonds[i + 1])) for i in range(n)]
    op = [rng.uniform(-0.5, 0.5, (ob[j], int(rng.integers(2, 4)), dims[sites[j]], ob[j + 1])) for j in range(k)]
    ctx = f"case {seed0 + case} n={n} sites={sites}"
    lin, state = t4a.LinearOperator(t4a.MPO(op), sites), t4a.SimpleTensorTrain(x)
    counts["cases"] += 1
    naive = A.np_naive(op, sites, x)
    for route in ("fused", "composed"):
        got = t4a.apply_linear_operator(lin, state, t4a.ApplyOptions.naive(), route=route)
        follows(f"{ctx} naive {route}", got, naive, 1e-13)
    again = t4a.apply_linear_operator(lin, state, t4a.ApplyOptions.naive(), route="fused")
    first = t4a.apply_linear_operator(lin, state, t4a.ApplyOptions.naive(), route="fused")
    if any(a.tobytes() != b.tobytes() for a, b in zip(again.site_tensors(), first.site_tensors())):
        fail(ctx, "naive fused: other bits on the second run")
    exact = max(c.shape[2] for c in naive)
    for cap in (None, int(rng.integers(1, max(exact, 2)))):
        o = A.options_for(cap)
        (zip_want, log_z) = A.record(lambda: A.np_zipup(op, sites, x, o))
        ((fit_want, fit_info), log_f) = A.record(lambda: A.np_fit(op, sites, x, o))
        if A.gap_violations(log_z) or A.gap_violations(log_f):
            counts["skipped_gap"] += 1
            continue
        dev = t4a.ApplyOptions.zipup().with_svd_policy(t4a.SvdTruncationPolicy(A.TOLERANCE)).with_nfullsweeps(2)
        dev = dev if cap is None else dev.with_max_bond_dim(cap)
        for route in ("fused", "composed"):
            follows(f"{ctx} zipup {route} cap={cap}", t4a.apply_linear_operator(lin, state, dev, route=route), zip_want, 1e-10)
            fo = t4a.ApplyOptions(method=2, max_bond_dim=dev.max_bond_dim, svd_policy=dev.svd_policy, nfullsweeps=2)
            got, info = t4a.apply_linear_operator(lin, state, fo, route=route, return_info=True)
            follows(f"{ctx} fit {route} cap={cap}", got, fit_want, 1e-10)
            if info["n_sweeps"] != fit_info["n_sweeps"]:
                fail(ctx, f"fit {route}: {info['n_sweeps']} sweeps, the restatement {fit_info['n_sweeps']}")
    # one gap half, integers
    nn, m, lb, d, rb = (int(rng.integers(1, 40)), int(rng.integers(1, 4)), int(rng.integers(1, 40)), int(rng.integers(2, 4)), int(rng.integers(1, 40)))
    xs = rng.integers(-1, 2, (lb, d, rb)).astype(np.float64)
    for right in (False, True):
        env = rng.integers(-3, 4, (m, rb, nn) if right else (nn, m, lb)).astype(np.float64)
        res, guard = _gap_half(env, xs, right, fill=-7.5)
        counts["halves"] += 1
        if not np.array_equal(res, A.np_gap_half(env.astype(np.int64), xs.astype(np.int64), right).astype(np.float64)) or not np.all(guard == -7.5):
            fail(ctx, f"gap half right={right} shape n={nn} m={m} lb={lb} d={d} rb={rb}")

print(f"soak_linop: {counts} fails={fails} in {time.perf_counter() - t0:.1f}s", flush=True)
sys.exit(1 if fails else 0)
