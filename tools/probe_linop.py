"""Times apply_linear_operator (t4a_amd.linop) on the routes fused and composed in the same process, and one half launch of a
bridge site on both kernels.

Protocol: the interleaved layout x1 y1 x2 y2 ... of 2 R binary sites, a one-variable operator of R sites on the x bits
(sites = 0, 2, 4, ...: every second site is a bridge, the last one lies outside), a random state of bond `bond` (bonds min(2^i, bond)
towards the ends), operator bond 2 (shift_operator(R, 1, Periodic)) or a random MPO of bond `m`.  Zip-up and fit with ONE sweep,
tolerance 1e-12, max_bond_dim = bond.  The composed route runs only kernels the MPO-MPO contraction has, so it is the speed a tree
without kernels_apply.hip has.  Per configuration and method the two routes alternate: one warm-up call each, then `reps` timed calls
each (a call returns after its stream is synchronised, so the window holds all device work); median, minimum and spread
(max - min) per route.  `fused_wins` is true where fused_median + max(spread) < composed_median.
  half   device ms of the left half of a bridge site with environment rows = bond, state bonds bond x bond, through
         linop._time_half (HIP events around 20 launches): apply_gap_half_kernel against mpo_partial_half_kernel on the
         materialised bridge site, median and spread of `reps` runs.
Every row is printed as one JSON line; with `--out FILE` the rows are also collected in FILE ({"drivers": [...], "half": [...]}).

    python tools/probe_linop.py [--R 8 16] [--bonds 16 64 128] [--op-bonds 2 8] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python")]

import t4a_amd  # noqa: E402
from t4a_amd import ApplyOptions, LinearOperator, MPO, SimpleTensorTrain  # noqa: E402
from t4a_amd import linop  # noqa: E402


def random_state(rng, n, bond):
    bonds = [min(2 ** min(i, n - i), bond) for i in range(n + 1)]
    return SimpleTensorTrain([rng.uniform(-0.5, 0.5, (bonds[i], 2, bonds[i + 1])) for i in range(n)])


def operator(rng, r, m):
    if m == 2:
        return t4a_amd.shift_operator(r, 1, t4a_amd.BoundaryCondition.Periodic)
    bonds = [1] + [m] * (r - 1) + [1]
    return MPO([rng.uniform(-0.5, 0.5, (bonds[j], 2, 2, bonds[j + 1])) for j in range(r)])


def stats(times):
    return {"ms_median": round(float(np.median(times)), 3), "ms_min": round(min(times), 3), "ms_spread": round(max(times) - min(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--bonds", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--op-bonds", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = {"drivers": [], "half": []}

    def emit(kind, row):
        rows[kind].append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)

    rng = np.random.default_rng(0)
    for m in a.op_bonds:
        for bond in a.bonds:
            runs = [linop._time_half(bond, m, bond, 2, bond, 20) for _ in range(a.reps + 1)][1:]
            f, c = [r["fused"] for r in runs], [r["composed"] for r in runs]
            emit("half", {"n_env": bond, "op_bond": m, "state_bond": bond, "site_dim": 2,
                          "fused_ms_median": round(float(np.median(f)), 4), "fused_ms_spread": round(max(f) - min(f), 4),
                          "composed_ms_median": round(float(np.median(c)), 4), "composed_ms_spread": round(max(c) - min(c), 4)})
    for r in a.R:
        n = 2 * r
        sites = tuple(range(0, n, 2))
        for m in a.op_bonds:
            lin = LinearOperator(operator(rng, r, m), sites)
            lin.mpo()
            for bond in a.bonds:
                state = random_state(rng, n, bond)
                for method, base in ((1, ApplyOptions.zipup()), (2, ApplyOptions.fit())):
                    o = base.with_max_bond_dim(bond).with_nfullsweeps(1)
                    times = {"fused": [], "composed": []}
                    out = {}
                    for rep in range(a.reps + 1):
                        for route in ("fused", "composed"):  # alternating; rep 0 is the warm-up
                            t0 = time.perf_counter()
                            out[route] = t4a_amd.apply_linear_operator(lin, state, o, route=route)
                            if rep:
                                times[route].append((time.perf_counter() - t0) * 1e3)
                    idx = rng.integers(0, 2, (2048, n))
                    vf, vc = out["fused"].evaluate(idx), out["composed"].evaluate(idx)
                    sf, sc = stats(times["fused"]), stats(times["composed"])
                    emit("drivers", {"method": method, "n_sites": n, "n_gap_sites": n - r, "state_bond": bond, "op_bond": m,
                                     "fused": sf, "composed": sc, "link_dims_equal": out["fused"].link_dims() == out["composed"].link_dims(),
                                     "rel_l2_difference": float(np.linalg.norm(vf - vc) / max(np.linalg.norm(vc), 1e-300)),
                                     "fused_wins": bool(sf["ms_median"] + max(sf["ms_spread"], sc["ms_spread"]) < sc["ms_median"]),
                                     "auto": t4a_amd.apply_route(method, n, n - r, bond, m)})


if __name__ == "__main__":
    main()
