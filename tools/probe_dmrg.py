"""Times the launches of one Lanczos step and of a finalise of two-site DMRG (t4a_amd.dmrg) at a given bond and basis size: a
transverse-field Ising chain of `n` sites, the state QR-canonical around the middle bond with bonds `chi`.

  * one Lanczos step with nb basis vectors: the two products of the projected apply and the orthogonalisation launches (gs_dots and
    gs_update run twice per step, gs_normalize once), from ProjectedOperator.time_step;
  * one finalise: krylov_combine over nb vectors, eig_residual and the finishing launch (its apply is the two products above);
  * one full dmrg call (2 sweeps, default options, max_bond_dim = chi) as wall time, with its counters.

Device times are HIP events around `reps` launches behind a warm-up launch; every figure is the median of `repeats` such measurements.

    python tools/probe_dmrg.py [--n 16] [--chi 32] [--nb 8,64] [--reps 20] [--repeats 5] [--out FILE.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
import dmrg_np as dn  # noqa: E402
from t4a_amd.dmrg import _time_finalise  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    n, chi, reps, repeats = int(arg("--n", 16)), int(arg("--chi", 32)), int(arg("--reps", 20)), int(arg("--repeats", 5))
    nbs = [int(x) for x in str(arg("--nb", "8,64")).split(",")]
    out_path = arg("--out", None)
    ops = dn.tfim(n, 1.0)
    rng = np.random.default_rng(chi)
    bonds = [min(chi, 2 ** min(k, n - k)) for k in range(n + 1)]
    site = n // 2 - 1
    x = dn.np_canonicalize([rng.uniform(-0.5, 0.5, (bonds[k], 2, bonds[k + 1])) for k in range(n)], site)
    op, state = t4a_amd.MPO(ops), t4a_amd.SimpleTensorTrain(x)
    po = t4a_amd.ProjectedOperator(op, state)
    shape = po.local_dimension(site)
    length = int(np.prod(shape))
    results = {"n_sites": n, "chi": chi, "region": [site, site + 1], "local_shape": list(shape), "len": length, "reps": reps, "steps": []}
    for nb in nbs:
        step = [po.time_step(site, nb, reps) for _ in range(repeats + 1)][1:]
        fin = [_time_finalise(length, nb, reps) for _ in range(repeats + 1)][1:]
        row = {"nb": nb}
        row.update({k: round(float(np.median([r[k] for r in step])), 5) for k in step[0]})
        row.update({k: round(float(np.median([r[k] for r in fin])), 5) for k in fin[0]})
        row["step_ms"] = round(row["product_left"] + row["product_right"] + 2 * (row["gs_dots"] + row["gs_update"]) + row["gs_normalize"], 5)
        row["finalise_ms"] = round(row["product_left"] + row["product_right"] + row["krylov_combine"] + row["eig_residual"] + row["krylov_finish"], 5)
        results["steps"].append(row)
        print(json.dumps(row), flush=True)
    o = t4a_amd.DmrgOptions(nsweeps=2, max_bond_dim=chi)
    init = t4a_amd.SimpleTensorTrain(dn.random_state((2,) * n, [1] + [2] * (n - 1) + [1], dn.SEED ^ n))
    times = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        r = t4a_amd.dmrg(op, init, 0, o)
        times.append((time.perf_counter() - t0) * 1e3)
    results["dmrg"] = {"nsweeps": 2, "wall_ms": round(float(np.median(times[1:])), 2), "energy": r.energy, "max_bond": max(r.state.link_dims()),
                       "max_residual_norm": r.max_residual_norm, **r.stats}
    print(json.dumps(results["dmrg"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
