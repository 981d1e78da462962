"""Soak of two-site DMRG (csrc/dmrg.hip, kernels_dmrg.hip) on random small problems against the dense eigensolve and the numpy
restatement (tests/dmrg_np.py): 2 - 7 sites, site dimensions 2 or 3 drawn per site, operator bonds 1 - 4 with site tensors
symmetrised in (s1, s2), start bonds 1 - 3, a random centre, no bond cap.  Cases whose ground state is not unique to 1e-3 ||H||_2 are
skipped (a condition on the inputs).  Per case, after 3 sweeps with default options: the energy is within 1e-10 max(1, ||H||_2) of
the dense ground energy — or, where the restatement itself stays in a local minimum of the two-site sweeps (product operators, W = 1),
of the restatement's energy —, it agrees with the Rayleigh quotient recomputed in numpy from the downloaded cores and with dmrg_energy to
1e-12 ||H||_2, the overlap with the dense ground vector is at least 1 - 1e-8 (outside a local minimum), the largest residual is below the largest threshold of
the restatement's local solves (+ 1e-12 ||H||_2), and a second run gives the same bits.
usage: python3 tests/soak/soak_dmrg.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import dmrg_np as dn  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
counts = {"cases": 0, "skipped": 0, "local_minima": 0, "lanczos_steps": 0}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n = int(rng.integers(2, 8))
    dims = [int(rng.integers(2, 4)) for _ in range(n)]
    if int(np.prod(dims)) > 2200:
        dims = [2] * n
    w, ib, center = int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.integers(0, n))
    ops = []
    for k, d in enumerate(dims):
        t = rng.uniform(-0.5, 0.5, (1 if k == 0 else w, d, d, 1 if k == n - 1 else w))
        ops.append(0.5 * (t + t.transpose(0, 2, 1, 3)))
    init = [rng.uniform(-0.5, 0.5, (1 if k == 0 else ib, d, 1 if k == n - 1 else ib)) for k, d in enumerate(dims)]
    h = dn.full(ops)
    lams, vecs = np.linalg.eigh(0.5 * (h + h.T))
    norm = float(max(abs(lams[0]), abs(lams[-1])))
    ctx = f"seed {seed0 + case} dims {dims} W {w} init {ib} center {center}"
    if (lams[1] - lams[0]) < 1e-3 * norm:
        counts["skipped"] += 1
        continue
    try:
        op, x0 = t4a.MPO(ops), t4a.SimpleTensorTrain(init)
        o = t4a.DmrgOptions(nsweeps=3)
        r = t4a.dmrg(op, x0, center, o)
        cores = r.state.site_tensors()
        restated = dn.np_dmrg(ops, init, center, dn.Options(nsweeps=3))
        bound = 1e-10 * max(1.0, norm)
        if abs(restated["energy"] - lams[0]) > bound:
            # two-site sweeps can stay in a local minimum (a product operator, W = 1, is the usual case: the signs of the local factors
            # do not combine to the global minimum); then the device has to sit where the restatement sits
            counts["local_minima"] += 1
            if abs(r.energy - restated["energy"]) > bound:
                fail(ctx, f"energy {r.energy}, restatement {restated['energy']} (a local minimum; dense {lams[0]})")
        else:
            if abs(r.energy - lams[0]) > bound:
                fail(ctx, f"energy {r.energy}, dense {lams[0]}, restatement {restated['energy']}")
            psi = dn.np_state_full(cores)
            if abs(psi @ vecs[:, 0]) / np.linalg.norm(psi) < 1 - 1e-8:
                fail(ctx, f"overlap {abs(psi @ vecs[:, 0]) / np.linalg.norm(psi)}")
        if abs(r.energy - dn.np_energy(ops, cores, center)) > 1e-12 * norm or abs(r.energy - t4a.dmrg_energy(op, r.state, center)) > 1e-12 * norm:
            fail(ctx, f"reported energy {r.energy}, recomputed {dn.np_energy(ops, cores, center)}, dmrg_energy {t4a.dmrg_energy(op, r.state, center)}")
        if r.max_residual_norm > restated["max_threshold"] + 1e-12 * norm:
            fail(ctx, f"max residual {r.max_residual_norm}, the restatement's largest threshold {restated['max_threshold']}")
        if r.local_updates != 3 * 2 * (n - 1):
            fail(ctx, f"{r.local_updates} local updates")
        r2 = t4a.dmrg(op, x0, center, o)
        if any(p.tobytes() != q.tobytes() for p, q in zip(cores, r2.state.site_tensors())) or r2.energy != r.energy:
            fail(ctx, "a second run gave other bits")
        counts["cases"] += 1
        counts["lanczos_steps"] += r.stats["lanczos_steps"]
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
