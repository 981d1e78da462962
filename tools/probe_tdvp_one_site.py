"""Times the bond-centre apply of one-site TDVP (t4a_amd.tdvp_one_site) and a whole sweep:

  * bond apply, Y[b, b'] = sum La[b, w, a] C[a, a'] Rb[b', w, a']: the fused launch (tdvp_bond_apply_kernel) against the two-GEMM
    composition on gemm_launch, at k_a = k_b in {8, 16, 32, 64, 128, 256} and W in {4, 16}; outside the envelope of the fused launch
    (W k_b <= 512) only the GEMMs are timed;
  * one second-order tdvp_one_site sweep against one second-order two-site tdvp sweep on the same operator and state: an Ising chain of
    n sites, d = 2, bonds 16 and 64, max_bond_dim of the two-site sweep equal to the bond; wall milliseconds ending synced.

Device times are HIP events around `reps` launches behind a warm-up launch, the two routes one after the other in every measurement;
every figure is the median of `repeats` such measurements, min and max beside it.  `route` says which of the two the driver takes at
the shape (tdvp_bond_apply_route in csrc/tdvp.hip).

    python tools/probe_tdvp_one_site.py [--n 12] [--reps 50] [--repeats 7] [--out profiles/tdvp_one_site_probe.json]
"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
import tdvp_np as tn  # noqa: E402
from t4a_amd.tdvp import _time_bond_apply, _bond_apply_route, BOND_FUSED  # noqa: E402

BONDS, WS = (8, 16, 32, 64, 128, 256), (4, 16)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(vals):
    vals = [v for v in vals if not math.isnan(v)]
    if not vals:
        return None
    return {"median": round(float(np.median(vals)), 5), "min": round(float(min(vals)), 5), "max": round(float(max(vals)), 5)}


def main():
    n, reps, repeats = int(arg("--n", 12)), int(arg("--reps", 50)), int(arg("--repeats", 7))
    out_path = arg("--out", None)
    results = {"reps": reps, "repeats": repeats, "bond_apply": [], "sweep": []}
    for w in WS:
        for k in BONDS:
            runs = [_time_bond_apply(k, k, w, reps) for _ in range(repeats + 1)][1:]
            row = {"k": k, "W": w, "route": "fused" if _bond_apply_route(k, k, w) == BOND_FUSED else "gemm",
                   "fused_ms": summary([r["fused"] for r in runs]), "gemm_ms": summary([r["gemm"] for r in runs])}
            results["bond_apply"].append(row)
            print(json.dumps(row), flush=True)
    rng = np.random.default_rng(n)
    ops = tn.tfim(n, 1.0)
    op = t4a_amd.MPO(ops)
    for chi in (16, 64):
        bonds = [min(chi, 2 ** min(k, n - k)) for k in range(n + 1)]
        init = t4a_amd.SimpleTensorTrain([rng.uniform(-0.5, 0.5, (bonds[k], 2, bonds[k + 1])) for k in range(n)])
        one, two = [], []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            r1 = t4a_amd.tdvp_one_site(op, init, 0, t4a_amd.TdvpOptions(nsite=1, order=2, exponent_step=-0.05))
            one.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            r2 = t4a_amd.tdvp(op, init, 0, t4a_amd.TdvpOptions(order=2, exponent_step=-0.05, max_bond_dim=chi))
            two.append((time.perf_counter() - t0) * 1e3)
        row = {"n_sites": n, "chi": chi, "one_site_wall_ms": summary(one[1:]), "two_site_wall_ms": summary(two[1:]), "one_site_links": r1.state.link_dims(),
               "two_site_links": r2.state.link_dims(), "one_site_stats": r1.stats, "one_site_local_updates": r1.local_updates,
               "two_site_stats": r2.stats, "two_site_local_updates": r2.local_updates}
        results["sweep"].append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
