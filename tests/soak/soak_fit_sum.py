"""Soak of fit_sum (csrc/fit_sum.hip, kernels_fit_sum.hip) on random small problems against the numpy restatement (tests/fit_sum_np.py)
and dense sums: 1 - 7 sites, one site dimension of 2 or 3 per case, 1 - 6 targets of ragged bonds 1 - 5, random coefficients for
half of the cases, a random centre, a random route.  Per case: (a) from an initial with full bonds one sweep returns
sum_k w_k T_k within 1e-12 of sum_k |w_k| |T_k|_F; (b) from a random initial of bonds 1 - 3 with a cap, two sweeps follow the
restatement — equal link dims and a dense result within 1e-10 of the scale — unless the restatement's singular values at a cut are
closer than 1e-6 (a condition on the inputs: skipped); (c) a second run gives the same bits.  The half kernel is compared with int64
arithmetic on a random ragged launch per case, on both routes.
usage: python3 tests/soak/soak_fit_sum.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
from t4a_amd.fitsum import _half  # noqa: E402
import fit_sum_np as F  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
counts = {"cases": 0, "skipped_gap": 0, "halves": 0}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def train(rng, n, site, bond):
    bonds = [1] + [min(int(rng.integers(1, bond + 1)), site ** min(i, n - i)) for i in range(1, n)] + [1]
    return [rng.uniform(-0.5, 0.5, (bonds[i], site, bonds[i + 1])) for i in range(n)]


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n, site, K = int(rng.integers(1, 8)), int(rng.integers(2, 4)), int(rng.integers(1, 7))
    if site ** n > 2200:
        site = 2
    center, route = int(rng.integers(0, n)), ("fused", "gemm", "auto")[int(rng.integers(0, 3))]
    targets = [train(rng, n, site, 5) for _ in range(K)]
    w = [float(x) for x in rng.uniform(-2, 2, K)] if rng.integers(0, 2) else None
    ctx = f"seed {seed0 + case} n {n} S {site} K {K} center {center} route {route}"
    try:
        dev = [t4a.SimpleTensorTrain(t) for t in targets]
        exact, scale = F.np_sum(targets, w), F.scale_of(targets, w)
        full = [rng.uniform(-0.5, 0.5, (a, site, b)) for a, b in zip(F.full_bonds(n, site)[:-1], F.full_bonds(n, site)[1:])]
        got = F.np_full(t4a.fit_sum(dev, t4a.SimpleTensorTrain(full), center, None, w, route).site_tensors())
        if np.linalg.norm(got - exact) > 1e-12 * scale:
            fail(ctx, f"full bonds: deviation {np.linalg.norm(got - exact) / scale}")
        if n >= 2:
            init, cap = train(rng, n, site, 3), int(rng.integers(1, 5))
            log = []
            want, info = F.np_fit_sum(targets, init, center, F.Options(nfullsweeps=2, max_bond_dim=cap), w, log=log)
            g = F.gaps(log)
            if g and min(min(x) for x in g) < F.GAP:
                counts["skipped_gap"] += 1
            else:
                o = t4a.FitSumOptions(nfullsweeps=2, max_bond_dim=cap)
                r = t4a.fit_sum(dev, t4a.SimpleTensorTrain(init), center, o, w, route, return_info=True)
                cores = r.state.site_tensors()
                if r.link_dims != info["link_dims"]:
                    fail(ctx, f"link dims {r.link_dims}, restatement {info['link_dims']}")
                elif np.linalg.norm(F.np_full(cores) - F.np_full(want)) > 1e-10 * scale:
                    fail(ctx, f"capped: deviation {np.linalg.norm(F.np_full(cores) - F.np_full(want)) / scale}")
                again = t4a.fit_sum(dev, t4a.SimpleTensorTrain(init), center, o, w, route).site_tensors()
                if any(p.tobytes() != q.tobytes() for p, q in zip(cores, again)):
                    fail(ctx, "a second run gave other bits")
        bonds = [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(int(rng.integers(1, 12)))]
        chi, S, right = int(rng.integers(1, 40)), int(rng.integers(1, 4)), bool(rng.integers(0, 2))
        A, B = sum(a for a, _ in bonds), sum(b for _, b in bonds)
        env = rng.integers(-3, 4, (B, chi) if right else (chi, A)).astype(np.float64)
        cores = [rng.integers(-1, 2, (a, S, b)).astype(np.float64) for a, b in bonds]
        out, oa, ob = [], 0, 0
        for t in cores:
            a, _, b = t.shape
            out.append(np.einsum("asb,bc->asc", t, env[ob:ob + b]) if right else np.einsum("ca,asb->csb", env[:, oa:oa + a], t))
            oa, ob = oa + a, ob + b
        ref = np.concatenate(out, axis=0 if right else 2)
        for rt in ("fused", "gemm"):
            if not np.array_equal(_half(env, cores, right, rt), ref):
                fail(ctx, f"half {rt} right={right} chi {chi} S {S} bonds {bonds}")
        counts["halves"] += 1
        counts["cases"] += 1
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
