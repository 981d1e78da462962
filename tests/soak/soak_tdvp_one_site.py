"""Soak of one-site TDVP (csrc/tdvp.hip, kernels_tdvp.hip) on random small problems against the numpy restatement
(tests/tdvp_one_site_np.py): 2 - 6 sites, site dimensions 2 or 3 drawn per site, operator bonds 1 - 4 with site tensors symmetrised in
(s1, s2), a random start whose bonds are full or capped at 2 - 4, order 1, 2 or 4, ANY site as the centre, 1 or 2 sweeps, tau in
[-0.1, 0.1], the bond-centre apply on the route of the rule or forced to one of the two.  Per case: the dense state is within
max(100 spread, 1e-12) of the restatement's (spread: the restatement on three starts perturbed in their last bits,
tdvp_np.spread_tolerance), with full bonds also within 1e-9 of exp(nsweeps tau H) psi_0, the bond dimensions are those of the
canonicalised start, the counters equal the restatement's, and a second run gives the same bits.
usage: python3 tests/soak/soak_tdvp_one_site.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import tdvp_np as tn  # noqa: E402
import tdvp_one_site_np as t1  # noqa: E402
from t4a_amd.tdvp import _set_bond_apply_route, BOND_AUTO  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
counts = {"cases": 0, "krylov_steps": 0, "fused_applies": 0, "gemm_applies": 0}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n = int(rng.integers(2, 7))
    dims = [int(rng.integers(2, 4)) for _ in range(n)]
    if int(np.prod(dims)) > 300:
        dims = [2] * n
    w, order, nsweeps = int(rng.integers(1, 5)), int(rng.choice([1, 2, 4])), int(rng.integers(1, 3))
    center = int(rng.integers(0, n))
    tau = float(rng.uniform(-0.1, 0.1))
    route = int(rng.integers(0, 3))
    ops = []
    for k, d in enumerate(dims):
        t = rng.uniform(-0.5, 0.5, (1 if k == 0 else w, d, d, 1 if k == n - 1 else w))
        ops.append(0.5 * (t + t.transpose(0, 2, 1, 3)))
    bonds = tn.full_bonds(dims)
    full = rng.integers(0, 2) == 0
    if not full:
        cap = int(rng.integers(2, 5))
        bonds = [min(b, cap) for b in bonds]
        full = bonds == tn.full_bonds(dims)
    init = [rng.uniform(-0.5, 0.5, (bonds[k], d, bonds[k + 1])) for k, d in enumerate(dims)]
    ctx = f"seed {seed0 + case} dims {dims} bonds {bonds} W {w} order {order} center {center} nsweeps {nsweeps} tau {tau} route {route}"
    try:
        op, x0 = t4a.MPO(ops), t4a.SimpleTensorTrain(init)
        o = t4a.TdvpOptions(nsite=1, nsweeps=nsweeps, order=order, exponent_step=tau)
        no = tn.Options(nsweeps=nsweeps, order=order, exponent_step=tau, cgs2=True)
        _set_bond_apply_route(route)
        r = t4a.tdvp_one_site(op, x0, center, o)
        cores = r.state.site_tensors()
        psi = tn.np_state_full(cores)
        restated = t1.np_tdvp_one_site(ops, init, center, no)
        tol, spread = tn.spread_tolerance(lambda start: tn.np_state_full(t1.np_tdvp_one_site(ops, start, center, no)["state"]), init)
        dist = tn.relative_distance(psi, tn.np_state_full(restated["state"]))
        if dist > tol:
            fail(ctx, f"distance to the restatement {dist}, tolerance {tol} (spread {spread})")
        if full:
            want = t1.dense_exponential(ops, init, nsweeps * tau)
            if tn.relative_distance(psi, want) > 1e-9:
                fail(ctx, f"distance to the dense exponential {tn.relative_distance(psi, want)}")
        if r.state.link_dims() != [t.shape[2] for t in tn.np_canonicalize(init, center)[:-1]]:
            fail(ctx, f"bond dimensions {r.state.link_dims()}")
        got = (r.sweeps_completed, r.local_updates, r.stats["one_site_steps"], r.stats["bond_corrections"])
        want_counts = (restated["sweeps_completed"], restated["local_updates"], restated["one_site_steps"], restated["bond_corrections"])
        if got != want_counts:
            fail(ctx, f"counters {got}, restatement {want_counts}")
        r2 = t4a.tdvp_one_site(op, x0, center, o)
        if any(p.tobytes() != s.tobytes() for p, s in zip(cores, r2.state.site_tensors())):
            fail(ctx, "a second run gave other bits")
        counts["cases"] += 1
        for key in ("krylov_steps", "fused_applies", "gemm_applies"):
            counts[key] += r.stats[key]
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
    finally:
        _set_bond_apply_route(BOND_AUTO)
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
