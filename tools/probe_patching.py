"""Times adaptive patching on its two routes, in one process, on 12 sites of dims (2, 2):

  * truncate_adaptive over 16, 64 and 256 patches (the s1 legs of the first 4, 6, 8 sites projected) of bonds 16 and 64:
    route "batched" (one truncate_many call: 3 (n - 1) launches, two host synchronisations) against route "serial" (the same sequence
    chain by chain through QrSweep, Engine::svd and svd_retained_rank — the machinery MPO.compress runs on, with a policy) on the same
    PartitionedMPO, alternating, one warm-up call of each outside the clock.  Both routes make their masked copies inside the clock.
  * one ExactParameterGain decision on one patch of bond 16: the 2 children of each of the 24 candidate legs, all 48 in one ranks-only
    truncate_many call against candidate by candidate (24 calls of 2); the children are formed outside the clock.
  * the split of one batched truncate_adaptive call between its three sweeps and its two synchronisations (the stream drained after
    every sweep, which a plain call does not do).

Every figure is the median of `repeats` wall-clock calls in milliseconds, `range` the distance between the largest and the smallest.

    python tools/probe_patching.py [--repeats 5] [--out profiles/patching_probe.json]
"""
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

from t4a_amd import MPO, SvdTruncationPolicy  # noqa: E402
from t4a_amd import mpo as M  # noqa: E402
from t4a_amd import partitioned as P  # noqa: E402

N_SITES = 12
RTOL = 1e-6


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def random_mpo(rng, bond):
    bonds = [1] + [bond] * (N_SITES - 1) + [1]
    return MPO([rng.uniform(-1, 1, size=(bonds[i], 2, 2, bonds[i + 1])) for i in range(N_SITES)])


def partitioned(rng, bond, bits):
    projs = [{(s, 0): v for s, v in enumerate(vals)} for vals in itertools.product(range(2), repeat=bits)]
    return P.PartitionedMPO([random_mpo(rng, bond) for _ in projs], projs)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(row, runs, names):
    for k, name in enumerate(names):
        vals = [r[k] for r in runs]
        row[name + "_ms"] = round(float(np.median(vals)), 4)
        row[name + "_range_ms"] = round(float(max(vals) - min(vals)), 4)
    row["%s_over_%s" % names] = round(row[names[0] + "_ms"] / row[names[1] + "_ms"], 2)
    row["%s_faster_beyond_spread" % names[1]] = bool(max(r[1] for r in runs) < min(r[0] for r in runs))
    return row


def main():
    repeats = int(arg("--repeats", 5))
    out_path = arg("--out", None)
    results = {"repeats": repeats, "n_sites": N_SITES, "rtol": RTOL, "rows": []}
    rng = np.random.default_rng(0)
    for bond in (16, 64):
        for bits in (4, 6, 8):
            p = partitioned(rng, bond, bits)
            for route in ("serial", "batched"):
                P.truncate_adaptive(p, RTOL, None, route)
            runs = [(clock(lambda: P.truncate_adaptive(p, RTOL, None, "serial")), clock(lambda: P.truncate_adaptive(p, RTOL, None, "batched")))
                    for _ in range(repeats)]
            row = summary({"kind": "truncate_adaptive", "bond": bond, "patches": len(p)}, runs, ("serial", "batched"))
            split = np.median([P._time_truncate_adaptive(p, RTOL) for _ in range(repeats)], axis=0)
            row["split_ms"] = dict(zip(("qr_sweep", "sync_norms", "svd_left", "svd_right", "sync_ranks"), (round(float(v), 4) for v in split)))
            results["rows"].append(row)
            print(json.dumps(row), flush=True)
            del p
    # one ExactParameterGain decision
    parent = P.PartitionedMPO([random_mpo(rng, 16)], [{}])
    legs = [(s, leg) for s in range(N_SITES) for leg in (0, 1)]
    children = [[P.PartitionedMPO.project(parent, {leg: v}).patch(0) for v in (0, 1)] for leg in legs]
    flat = [c for pair in children for c in pair]
    pol = SvdTruncationPolicy(1e-8, 1, 1, 1)
    for route in ("batched", "serial"):
        def one_call():
            return M.truncate_many(flat, pol, 8, route, ranks_only=True)

        def by_candidate():
            return [M.truncate_many(pair, pol, 8, route, ranks_only=True) for pair in children]
        assert one_call() == [b for pair in by_candidate() for b in pair]
        runs = [(clock(by_candidate), clock(one_call)) for _ in range(repeats)]
        row = summary({"kind": "exact_parameter_gain", "bond": 16, "candidates": len(legs), "children": len(flat), "route": route}, runs,
                      ("by_candidate", "one_call"))
        results["rows"].append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
