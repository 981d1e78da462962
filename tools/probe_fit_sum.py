"""Times fit_sum (t4a_amd.fit_sum) at one stated protocol next to the only route a tree without it has, in the same process.

Protocol: `n` binary sites, K targets of bond `bond` (the LCG fixtures of tests/fit_sum_np.py), cap `cap`, ONE sweep from
initial = targets[0] (its bonds are below the cap already), centre 0, on the routes auto, fused and gemm.  Median and minimum of `reps`
calls after a warm-up call; a call returns after its stream is synchronised, so the window holds all device work.
Baselines:
  add_compress      the pairwise chain: acc = acc.add(T_k) followed by acc.compress(SVD, max_bond_dim=cap), target after target
  add_all_compress  every add first (bond K * bond), one compress at the end; only for K * bond <= 256
  half              device ms of one half of the middle bond (result bond `cap`), the fused launch against the GEMM composition,
                    through fitsum._time_half (HIP events around 20 launches), left and right
The errors are relative l2 deviations on 4096 random points against the sum of the targets' evaluations.

    python tools/probe_fit_sum.py [n] [bond] [cap] [reps] [K ...]          (defaults: 16 8 32 5, K = 2 16 256)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
from t4a_amd import fitsum  # noqa: E402
from fit_sum_np import random_train, SEED  # noqa: E402


def timed(call, reps):
    r = call()  # warm-up (allocations, first launches)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        times.append((time.perf_counter() - t0) * 1e3)
    return r, times


def main():
    a = [int(x) for x in sys.argv[1:]]
    n, bond, cap, reps = (a[:4] + [16, 8, 32, 5][len(a[:4]):])
    ks = a[4:] or [2, 16, 256]
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 2, (4096, n))
    for K in ks:
        targets = [t4a_amd.SimpleTensorTrain(random_train([1] + [bond] * (n - 1) + [1], 2, SEED ^ (0x9D * (k + 1)))) for k in range(K)]
        exact = sum(t.evaluate(idx) for t in targets)
        opts = t4a_amd.FitSumOptions(nfullsweeps=1, max_bond_dim=cap)

        def chain():
            acc = targets[0].clone()
            for t in targets[1:]:
                acc = acc.add(t)
                acc.compress(method=t4a_amd.COMPRESS_SVD, max_bond_dim=cap)
            return acc

        def all_first():
            acc = targets[0].clone()
            for t in targets[1:]:
                acc = acc.add(t)
            acc.compress(method=t4a_amd.COMPRESS_SVD, max_bond_dim=cap)
            return acc

        calls = [(f"fit_sum_{route}", lambda route=route: t4a_amd.fit_sum(targets, None, 0, opts, route=route)) for route in ("auto", "fused", "gemm")]
        calls.append(("add_compress", chain))
        if K * bond <= 256:
            calls.append(("add_all_compress", all_first))
        for name, call in calls:
            r, times = timed(call, reps)
            got = r.evaluate(idx)
            print(json.dumps({"route": name, "n": n, "K": K, "bond": bond, "cap": cap, "link_dims": r.link_dims(),
                              "ms_median": round(float(np.median(times)), 3), "ms_min": round(min(times), 3),
                              "rel_l2_error": float(np.linalg.norm(got - exact) / np.linalg.norm(exact))}), flush=True)
        for right in (False, True):
            runs = [fitsum._time_half(K, bond, 2, cap, right, 20) for _ in range(reps + 1)][1:]
            print(json.dumps({"route": "half", "side": "right" if right else "left", "K": K, "bond": bond, "chi": cap, "auto": t4a_amd.fit_sum_route(K, bond, cap, 2),
                              "fused_ms_median": round(float(np.median([r["fused"] for r in runs])), 4),
                              "fused_ms_min": round(min(r["fused"] for r in runs), 4),
                              "gemm_ms_median": round(float(np.median([r["gemm"] for r in runs])), 4),
                              "gemm_ms_min": round(min(r["gemm"] for r in runs), 4)}), flush=True)


if __name__ == "__main__":
    main()
