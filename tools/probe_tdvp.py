"""Times what two-site TDVP (t4a_amd.tdvp) adds to the launches of the linear solver and of DMRG:

  * the projections of a Gram-Schmidt pass, the serial gs_dots against gs_dots_wide (a second grid dimension over the basis vectors),
    at len in {2048, 8192, 16384, 65536} x nb in {8, 16, 30}; `selected` says which of the two krylov_dots_route picks for the row;
  * the three launches of the one-site projected apply (HL = L A, T = HL V, Y = T R^T) at the middle site of a transverse-field Ising
    chain whose operator bonds are padded to W, for chi / W = 32 / 32 and 64 / 64;
  * one full second-order sweep (tau = -0.05, max_bond_dim = chi) of an Ising chain of n sites from a start with bonds chi, as wall time
    with its counters.

Device times are HIP events around `reps` launches behind a warm-up launch; every figure is the median of `repeats` such measurements,
`range` is the distance between the largest and the smallest of them (the run-to-run spread of the probe).

    python tools/probe_tdvp.py [--n 20] [--chi 64] [--reps 20] [--repeats 5] [--out profiles/tdvp_probe.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
import tdvp_np as tn  # noqa: E402
from t4a_amd.tdvp import _time_dots, _time_one_site, _dots_route, ROUTE_WIDE  # noqa: E402

LENGTHS, NBS = (2048, 8192, 16384, 65536), (8, 16, 30)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def padded_tfim(n, w, rng):
    """the Ising chain with its operator bonds padded from 3 to w by zero blocks (the same operator, the launches of a bond-w MPO)"""
    ops = []
    for k, t in enumerate(tn.tfim(n, 1.0)):
        wl, wr = (1 if k == 0 else w), (1 if k == n - 1 else w)
        p = np.zeros((wl, 2, 2, wr))
        p[:t.shape[0], :, :, :t.shape[3]] = t
        ops.append(p)
    return ops


def main():
    n, chi, reps, repeats = int(arg("--n", 20)), int(arg("--chi", 64)), int(arg("--reps", 20)), int(arg("--repeats", 5))
    out_path = arg("--out", None)
    results = {"reps": reps, "repeats": repeats, "gs_dots": [], "one_site_apply": []}
    for length in LENGTHS:
        for nb in NBS:
            runs = [_time_dots(length, nb, reps) for _ in range(repeats + 1)][1:]
            row = {"len": length, "nb": nb, "selected": "wide" if _dots_route(length, nb) == ROUTE_WIDE else "serial"}
            for k in ("serial", "wide"):
                vals = [r[k] for r in runs]
                row[k + "_ms"] = round(float(np.median(vals)), 5)
                row[k + "_range_ms"] = round(float(max(vals) - min(vals)), 5)
            results["gs_dots"].append(row)
            print(json.dumps(row), flush=True)
    rng = np.random.default_rng(chi)
    for c, w in ((32, 32), (64, 64)):
        m = 14
        bonds = [min(c, 2 ** min(k, m - k)) for k in range(m + 1)]
        site = m // 2
        x = tn.np_canonicalize([rng.uniform(-0.5, 0.5, (bonds[k], 2, bonds[k + 1])) for k in range(m)], site)
        po = t4a_amd.ProjectedOperator(t4a_amd.MPO(padded_tfim(m, w, rng)), t4a_amd.SimpleTensorTrain(x))
        runs = [_time_one_site(po, site, reps) for _ in range(repeats + 1)][1:]
        row = {"chi": c, "W": w, "site_shape": list(x[site].shape)}
        for k in runs[0]:
            vals = [r[k] for r in runs]
            row[k + "_ms"] = round(float(np.median(vals)), 5)
            row[k + "_range_ms"] = round(float(max(vals) - min(vals)), 5)
        results["one_site_apply"].append(row)
        print(json.dumps(row), flush=True)
    ops = tn.tfim(n, 1.0)
    bonds = [min(chi, 2 ** min(k, n - k)) for k in range(n + 1)]
    init = t4a_amd.SimpleTensorTrain([rng.uniform(-0.5, 0.5, (bonds[k], 2, bonds[k + 1])) for k in range(n)])
    op = t4a_amd.MPO(ops)
    o = t4a_amd.TdvpOptions(nsweeps=1, order=2, exponent_step=-0.05, max_bond_dim=chi)
    times = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        r = t4a_amd.tdvp(op, init, 0, o)
        times.append((time.perf_counter() - t0) * 1e3)
    results["sweep"] = {"n_sites": n, "chi": chi, "order": 2, "wall_ms": round(float(np.median(times[1:])), 2),
                        "wall_range_ms": round(float(max(times[1:]) - min(times[1:])), 2), "max_bond": max(r.state.link_dims()),
                        "local_updates": r.local_updates, "max_krylov_iterations": r.max_krylov_iterations, "max_error_estimate": r.max_error_estimate, **r.stats}
    print(json.dumps(results["sweep"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
