"""Times the pieces of square_linsolve (t4a_amd.linsolve) at the shapes of the reference's projected-apply benchmark: a chain of 38
sites of dimension 2, state and operator bonds `chi` = `W` (32 and 64), the region at the middle bond.

  * warm ProjectedOperator.apply (environments cached, half operators built): the host call with its two copies and the stream
    synchronisation inside the window, next to the device time of its two products alone (HIP events) and to the numpy restatement
    (linsolve_np.np_projected_apply_steps, the four-step order of a CPU implementation) on ONE thread of the same box;
  * one Arnoldi step at j = 1 and j = 29, split into the two products and the three orthogonalisation launches (HIP events);
  * one full sweep of the 64 / 64 problem: 74 bond steps of exactly one GMRES cycle of 30 steps each (gmres_tol = 0, one restart), the
    SVD capped at the bond, no residual evaluation.

Every figure is the median of `reps` measurements behind one warm-up.  The operator's sites are scaled so that its norm stays O(1);
the state is QR-canonical around the region.

    python tools/probe_linsolve.py [reps] [--out FILE.json] [--no-sweep]
"""
import json
import os
import sys
import time

for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[var] = "1"  # the CPU figure is one thread; set before numpy loads its BLAS

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
import linsolve_np as ln  # noqa: E402

N_SITES, D = 38, 2
REFERENCE_MS = {32: 6.0, 64: 68.2}  # benchmarks/results/2026-05-18-projected-apply.md of the reference: another machine, context only


def median_ms(call, reps):
    call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def problem(chi, rng):
    scale = 1.0 / (0.29 * D * np.sqrt(chi))
    ops = [rng.uniform(-0.5, 0.5, (1 if k == 0 else chi, D, D, 1 if k == N_SITES - 1 else chi)) * scale for k in range(N_SITES)]
    bonds = [min(chi, D ** min(k, N_SITES - k)) for k in range(N_SITES + 1)]
    x = [rng.uniform(-0.5, 0.5, (bonds[k], D, bonds[k + 1])) for k in range(N_SITES)]
    return ops, x, bonds


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args and args[0].isdigit() else 5
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    site = N_SITES // 2 - 1
    results = {"n_sites": N_SITES, "site_dim": D, "region": [site, site + 1], "reps": reps, "apply": [], "arnoldi_step": [], "sweep": None}
    for chi in (32, 64):
        rng = np.random.default_rng(chi)
        ops, x, _ = problem(chi, rng)
        x = ln.np_canonicalize(x, site)
        op, state = t4a_amd.MPO(ops), t4a_amd.SimpleTensorTrain(x)
        po = t4a_amd.ProjectedOperator(op, state)
        shape = po.local_dimension(site)
        v = rng.standard_normal(shape)
        y = po.apply(site, v)
        left, right = po.environment("left", site), po.environment("right", site + 2)
        want = ln.np_projected_apply_steps(left, right, ops[site], ops[site + 1], v)
        err = float(np.linalg.norm(y - want) / np.linalg.norm(want))
        host_ms = median_ms(lambda: po.apply(site, v), reps)
        cpu_ms = median_ms(lambda: ln.np_projected_apply_steps(left, right, ops[site], ops[site + 1], v), reps)
        steps = {}
        for j in (1, 29):
            runs = [po.time_step(site, j + 1) for _ in range(reps + 1)][1:]
            steps[j] = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        dev_ms = steps[1]["product_left"] + steps[1]["product_right"]
        m, n = shape[0] * shape[1], shape[2] * shape[3]
        row = {"chi": chi, "W": chi, "M": m, "N": n, "apply_host_call_ms": round(host_ms, 4), "apply_device_ms": round(dev_ms, 4),
               "numpy_one_thread_ms": round(cpu_ms, 4), "reference_published_ms_other_machine": REFERENCE_MS[chi],
               "gflops_device": round(2.0 * chi * m * n * (m + n) / dev_ms / 1e6, 1), "rel_error_vs_numpy": err,
               "slower_than_one_cpu_thread": bool(host_ms > cpu_ms)}
        results["apply"].append(row)
        print(json.dumps(row), flush=True)
        for j in (1, 29):
            srow = {"chi": chi, "j": j, **{k: round(val, 4) for k, val in steps[j].items()}}
            srow["products_ms"] = round(steps[j]["product_left"] + steps[j]["product_right"], 4)
            srow["orthogonalisation_ms"] = round(2 * (steps[j]["gs_dots"] + steps[j]["gs_update"]) + steps[j]["gs_normalize"], 4)
            results["arnoldi_step"].append(srow)
            print(json.dumps(srow), flush=True)
    if "--no-sweep" not in sys.argv:
        chi = 64
        rng = np.random.default_rng(7)
        ops, x, bonds = problem(chi, rng)
        rb = [min(16, b) for b in bonds]
        rhs = [rng.uniform(-0.5, 0.5, (rb[k], D, rb[k + 1])) for k in range(N_SITES)]
        op, b, x0 = t4a_amd.MPO(ops), t4a_amd.SimpleTensorTrain(rhs), t4a_amd.SimpleTensorTrain(x)
        o = t4a_amd.LinsolveOptions(nfullsweeps=1, max_bond_dim=chi, gmres_tol=0.0, gmres_restart_dim=30, gmres_max_restarts=1, a0=1.0, a1=1.0,
                                    check_residual=False)
        last = {}

        def sweep():
            last["r"] = t4a_amd.square_linsolve(op, b, x0, 0, o)

        ms = median_ms(sweep, reps)
        r = last["r"]
        results["sweep"] = {"chi": chi, "W": chi, "rhs_bond": 16, "sweep_ms": round(ms, 2), **r.stats, "max_bond": max(r.solution.link_dims())}
        print(json.dumps(results["sweep"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
