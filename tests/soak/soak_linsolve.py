"""Soak of square_linsolve (csrc/linsolve.hip, kernels_linsolve.hip) on random small problems against the numpy restatement
(tests/linsolve_np.py) and the dense solve: 3 - 7 sites, site dimension 2 or 3, operator bonds 1 - 4, rhs bonds 1 - 5, guess bonds
1 - 3, a random centre, a1 = +-1 and a0 = (1.5 .. 3) ||A||_2 (every projected problem then has its numerical range at least
||A||_2 / 2 away from zero), no bond cap below the exact bonds.  Per case: the device converges to convergence_tol = 1e-8 in at most one
sweep more than the restatement, its reported residual agrees with the dense recomputation from the downloaded cores to 1e-10, the
solution agrees with np.linalg.solve to 1e-6 relative, and a second run gives the same bits.
usage: python3 tests/soak/soak_linsolve.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import linsolve_np as ln  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
counts = {"sweeps": 0, "arnoldi_steps": 0}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n, d = int(rng.integers(3, 8)), int(rng.integers(2, 4))
    if d ** n > 2200:
        d = 2
    w, rb, ib = int(rng.integers(1, 5)), int(rng.integers(1, 6)), int(rng.integers(1, 4))
    center = int(rng.integers(0, n))
    ops = [rng.uniform(-0.5, 0.5, (1 if k == 0 else w, d, d, 1 if k == n - 1 else w)) for k in range(n)]
    rhs = [rng.uniform(-0.5, 0.5, (1 if k == 0 else rb, d, 1 if k == n - 1 else rb)) for k in range(n)]
    init = [rng.uniform(-0.5, 0.5, (1 if k == 0 else ib, d, 1 if k == n - 1 else ib)) for k in range(n)]
    am = ln.np_operator_full(ops)
    a1 = float(rng.choice([-1.0, 1.0]))
    a0 = float(rng.uniform(1.5, 3.0)) * float(np.linalg.norm(am, 2))
    ctx = f"seed {seed0 + case} n {n} d {d} W {w} rhs {rb} init {ib} center {center} a0 {a0:.4g} a1 {a1}"
    try:
        kw = dict(a0=a0, a1=a1, gmres_tol=1e-10, gmres_restart_dim=10, gmres_max_restarts=30, convergence_tol=1e-8)
        want = ln.np_square_linsolve(ops, rhs, init, center, ln.Options(**kw))
        op, b, x0 = t4a.MPO(ops), t4a.SimpleTensorTrain(rhs), t4a.SimpleTensorTrain(init)
        r = t4a.square_linsolve(op, b, x0, center, t4a.LinsolveOptions(**kw))
        cores = r.solution.site_tensors()
        if not (r.converged and r.residual < 1e-8):
            fail(ctx, f"not converged: residual {r.residual} after {r.sweeps} sweeps (restatement: {want[2]} after {want[1]})")
        if r.sweeps > want[1] + 1:
            fail(ctx, f"{r.sweeps} sweeps, the restatement took {want[1]}")
        again = ln.np_residual(ops, cores, rhs, a0, a1)
        if abs(again - r.residual) > 1e-10:
            fail(ctx, f"reported residual {r.residual}, recomputed {again}")
        exact = np.linalg.solve(a0 * np.eye(am.shape[0]) + a1 * am, ln.np_state_full(rhs))
        err = np.linalg.norm(ln.np_state_full(cores) - exact) / np.linalg.norm(exact)
        if err > 1e-6:
            fail(ctx, f"solution differs from the dense solve by {err}")
        r2 = t4a.square_linsolve(op, b, x0, center, t4a.LinsolveOptions(**kw))
        if any(p.tobytes() != q.tobytes() for p, q in zip(cores, r2.solution.site_tensors())) or r2.residual != r.residual:
            fail(ctx, "a second run gave other bits")
        counts["sweeps"] += r.sweeps
        counts["arnoldi_steps"] += r.stats["arnoldi_steps"]
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
