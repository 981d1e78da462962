"""Times the compress stage (right-canonicalise by QR, left SVD sweep) of many chains on its two routes, in one process:

  * serial: chain by chain through mpo_compress_cores — the route PartitionedMPO.contract takes by default, whose code the batched
    route does not touch (the parent's behaviour);
  * batched: all chains in one compress_many call — one workgroup per chain, 2 (n - 1) launches and one host synchronisation.

Both run on copies of the same chains and alternate inside the timing hook (t4a_gpu_pmpo_time_compress, t4a_gpu_mpo_time_compress_many);
the copies are outside the clock, every repetition ends synced, and every call of the hook warms both routes up first.

Operands, all on 12 sites of dims (2, 2):
  "pmpo": the task products of two partitioned MPOs with random patches of bond b x b (b = 2, 4, 8: product bonds 4, 16, 64), A split on
          the x legs of its first `bits` sites and B on the z legs of the same sites: 4^bits = 1, 16, 64, 256 tasks;
  "list": plain random MPOs of the product's bonds, 1, 16, 64 and 256 of them, through compress_many's hook.

Every figure is the median of `repeats` calls of the hook (wall milliseconds per repetition), `range` the distance between the largest
and the smallest of them.

    python tools/probe_compress_many.py [--repeats 5] [--out profiles/compress_many_probe.json]
"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

from t4a_amd import MPO, ContractionOptions  # noqa: E402
from t4a_amd.mpo import _time_compress_many, compress_many_plan  # noqa: E402
from t4a_amd.partitioned import PartitionedMPO, contract_plan, _time_compress  # noqa: E402

N_SITES = 12
BONDS = (2, 4, 8)
BITS = (0, 2, 3, 4)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def partitioned(rng, bond, bits, leg):
    projs = [{(s, leg): v for s, v in enumerate(vals)} for vals in itertools.product(range(2), repeat=bits)]
    bonds = [1] + [bond] * (N_SITES - 1) + [1]
    patches = [MPO([rng.uniform(-1, 1, size=(bonds[i], 2, 2, bonds[i + 1])) for i in range(N_SITES)]) for _ in projs]
    return PartitionedMPO(patches, projs), projs


def summary(row, runs):
    for k, name in enumerate(("serial", "batched")):
        vals = [r[k] for r in runs]
        row[name + "_ms"] = round(float(np.median(vals)), 4)
        row[name + "_range_ms"] = round(float(max(vals) - min(vals)), 4)
    row["serial_over_batched"] = round(row["serial_ms"] / row["batched_ms"], 2)
    # faster by more than the spread: the slowest batched repetition under the fastest serial one
    row["batched_faster_beyond_spread"] = bool(max(r[1] for r in runs) < min(r[0] for r in runs))
    return row


def main():
    repeats = int(arg("--repeats", 5))
    out_path = arg("--out", None)
    results = {"repeats": repeats, "n_sites": N_SITES, "rows": []}
    rng = np.random.default_rng(0)
    for bond in BONDS:
        for bits in BITS:
            a, pa = partitioned(rng, bond, bits, 0)
            b, pb = partitioned(rng, bond, bits, 1)
            tasks, _ = contract_plan(pa, pb)
            runs = [_time_compress(a, b, tolerance=1e-12, reps=1) for _ in range(repeats)]
            row = summary({"kind": "pmpo", "patch_bond": bond, "product_bond": bond * bond, "chains": len(tasks)}, runs)
            results["rows"].append(row)
            print(json.dumps(row), flush=True)
            del a, b
    for bond in BONDS:
        pb = bond * bond
        bonds = [1] + [pb] * (N_SITES - 1) + [1]
        shapes = [(bonds[i], 2, 2, bonds[i + 1]) for i in range(N_SITES)]
        plan = compress_many_plan([shapes], ContractionOptions(1e-12, None), "batched")
        for count in (1, 16, 64, 256):
            ops = [MPO([rng.uniform(-1, 1, size=s) for s in shapes]) for _ in range(count)]
            runs = [_time_compress_many(ops, ContractionOptions(1e-12, None), reps=1) for _ in range(repeats)]
            row = summary({"kind": "list", "product_bond": pb, "chains": count, "launches": plan["launches"], "syncs": plan["syncs"],
                           "bounded_bonds": plan["bonds"][0]}, runs)
            results["rows"].append(row)
            print(json.dumps(row), flush=True)
            del ops
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
