"""Times the two launches of an edge of the global subspace expansion (t4a_amd.gse) against the same products composed from the GEMM:

  * project, N_j = R_j - (R_j B^T) B over K references with the trace: one fused ragged launch against, per reference, a copy and two
    gemm_launch calls, and one launch for the trace;
  * absorb, parent_j (C_j B'^T) over the K + 1 trains: one fused ragged launch against two gemm_launch calls per train

at bonds chi in {64, 128, 256} with site dimension d = 2 and K = 2 references of bond chi + 1 (q = d chi, parents of d chi rows); and
one whole expansion (global_subspace_expand with one Krylov reference) of an Ising chain of n sites with bonds chi, as wall time.

Device times are HIP events around `reps` launches behind a warm-up launch; every figure is the median of `repeats` such measurements,
`range` is the distance between the largest and the smallest of them.  `route` says which of the two the driver takes at the shape
(gse_use_fused in csrc/gse.hip).

    python tools/probe_gse.py [--n 12] [--reps 20] [--repeats 5] [--out profiles/gse_probe.json]
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
from t4a_amd.gse import _time_routes, _route, ROUTE_FUSED  # noqa: E402

BONDS, D, K = (64, 128, 256), 2, 2


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    n, reps, repeats = int(arg("--n", 12)), int(arg("--reps", 20)), int(arg("--repeats", 5))
    out_path = arg("--out", None)
    results = {"reps": reps, "repeats": repeats, "d": D, "n_refs": K, "launches": [], "expansion": []}
    for chi in BONDS:
        runs = [_time_routes(chi, D, K, reps) for _ in range(repeats + 1)][1:]
        row = {"chi": chi, "q": D * chi, "route": "fused" if _route(D * chi, chi) == ROUTE_FUSED else "gemm"}
        for k in runs[0]:
            vals = [r[k] for r in runs]
            row[k + "_ms"] = round(float(np.median(vals)), 5)
            row[k + "_range_ms"] = round(float(max(vals) - min(vals)), 5)
        results["launches"].append(row)
        print(json.dumps(row), flush=True)
    rng = np.random.default_rng(n)
    ops = tn.tfim(n, 1.0)
    op = t4a_amd.MPO(ops)
    for chi in (16, 64):
        bonds = [min(chi, 2 ** min(k, n - k)) for k in range(n + 1)]
        init = t4a_amd.SimpleTensorTrain([rng.uniform(-0.5, 0.5, (bonds[k], 2, bonds[k + 1])) for k in range(n)])
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            r = t4a_amd.global_subspace_expand(op, init, 0, t4a_amd.GseOptions(krylov_dim=1))
            times.append((time.perf_counter() - t0) * 1e3)
        row = {"n_sites": n, "chi": chi, "wall_ms": round(float(np.median(times[1:])), 2), "wall_range_ms": round(float(max(times[1:]) - min(times[1:])), 2),
               "links": r.state.link_dims(), "edges_processed": r.edges_processed, "bonds_expanded": r.bonds_expanded, "max_added_basis": r.max_added_basis}
        results["expansion"].append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
