"""Times the stages of a patch-wise contraction of two partitioned MPOs (t4a_amd.partitioned, Naive route):

  * fused: the ONE launch of pmpo_pair_contract_kernel that forms the site products of every task and every site with the projection
    folded in (job upload and final sync included, as contract() pays them);
  * composed: the same products as "copy the operands, one mask launch per operand, then one mpo_site_contract launch per task"
    (mpo.contract_naive without compression on the masked copies);
  * compress: the compress stage of every task (right-canonicalise by QR, SVD sweep) on copies of the products.

Operands: random patches of bond `bond` over n sites of dims (2, 2).  "outer": A split on the x legs of its first `bits` sites, B on
the z legs of the same sites: 2^bits x 2^bits tasks with as many results.  "shared": both split on the y legs of those sites:
2^bits tasks (the diagonal) that sum into one result.

For the "outer" operands it also times ``to_mpo`` of A from Python: the reference's chain of G - 1 pairwise train additions against the
one direct-sum launch (each call ends synced and returns a new handle).

Times are wall milliseconds per repetition, each repetition ending with a stream sync; every figure is the median of `repeats`
measurements behind a warm-up, `range` the distance between the largest and the smallest.

    python tools/probe_pmpo.py [--reps 3] [--repeats 5] [--out profiles/pmpo_probe.json]
"""
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

from t4a_amd import MPO  # noqa: E402
from t4a_amd.partitioned import PartitionedMPO, contract_plan, _time_contract  # noqa: E402

# (n, bond, bits, kind)
SIZES = ((12, 8, 4, "outer"), (12, 8, 4, "shared"), (8, 16, 2, "outer"), (8, 16, 2, "shared"))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def partitioned(rng, n, bond, bits, leg):
    projs = [{(s, leg): v for s, v in enumerate(vals)} for vals in itertools.product(range(2), repeat=bits)]
    bonds = [1] + [bond] * (n - 1) + [1]
    patches = [MPO([rng.uniform(-1, 1, size=(bonds[i], 2, 2, bonds[i + 1])) for i in range(n)]) for _ in projs]
    return PartitionedMPO(patches, projs), projs


def main():
    reps, repeats = int(arg("--reps", 3)), int(arg("--repeats", 5))
    out_path = arg("--out", None)
    results = {"reps": reps, "repeats": repeats, "rows": []}
    rng = np.random.default_rng(0)
    for n, bond, bits, kind in SIZES:
        a, pa = partitioned(rng, n, bond, bits, 0 if kind == "outer" else 1)
        b, pb = partitioned(rng, n, bond, bits, 1 if kind == "outer" else 0)
        tasks, slots = contract_plan(pa, pb)
        runs = [_time_contract(a, b, tolerance=1e-12, reps=reps) for _ in range(repeats + 1)][1:]
        row = {"n_sites": n, "patch_bond": bond, "patches": [len(pa), len(pb)], "kind": kind, "tasks": len(tasks), "results": len(slots),
               "launches_fused": 1, "launches_composed": 2 + len(tasks)}
        for k, name in enumerate(("fused", "composed", "compress")):
            vals = [r[k] for r in runs]
            row[name + "_ms"] = round(float(np.median(vals)), 4)
            row[name + "_range_ms"] = round(float(max(vals) - min(vals)), 4)
        if kind == "outer":  # to_mpo of A: the chain of G - 1 pairwise additions against the one direct-sum launch (wall ms per call)
            for name, route in (("to_mpo_chain", 1), ("to_mpo_launch", 2)):
                vals = []
                for _ in range(repeats + 1):
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        a._to_mpo_route(route)
                    vals.append((time.perf_counter() - t0) * 1e3 / reps)
                row[name + "_ms"] = round(float(np.median(vals[1:])), 4)
                row[name + "_range_ms"] = round(float(max(vals[1:]) - min(vals[1:])), 4)
        results["rows"].append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
