"""Times the step of swap_site_indices and one whole regrouping of a quantics train.

1. The step kernel (swap_theta_kernel, csrc/kernels_swap.hip: contraction of two sites written with the legs redistributed, as the
   matrix the SVD reads) against the composition from existing pieces — the f64-MFMA GEMM, then one permutation launch — for binary
   legs exchanged at l = m = r = bond.  Both are timed with device events around `reps` launches behind a warm-up launch
   (t4a_gpu_swap_theta_time), in the same process and alternating, `rounds` times; medians with min and max are printed.
2. regroup_quantics of 2 variables with R bits at a bond cap: host wall ms of the call (it ends synced) and the device ms of its
   parts — step kernel, SVD with the split, QR (canonicalisation and transport) — from events around each part.

    python tools/probe_swap.py [rounds=7] [R=8] [cap=64] [bond ...=8 32 64 128 256]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python")]

import t4a_amd  # noqa: E402
from t4a_amd import swap as swap_mod  # noqa: E402


def stats(v):
    return {"median": round(float(np.median(v)), 5), "min": round(float(min(v)), 5), "max": round(float(max(v)), 5)}


def main():
    nums = [int(x) for x in sys.argv[1:]]
    rounds, r_bits, cap = (nums + [7, 8, 64][len(nums):])[:3]
    bonds = nums[3:] or [8, 32, 64, 128, 256]
    t4a_amd.set_device(0)
    for bond in bonds:
        reps = 400 if bond <= 64 else 100
        swap_mod.swap_theta_time(bond, 5)  # warm both routes up at this shape
        kernel, composed = [], []
        for _ in range(rounds):
            k, c = swap_mod.swap_theta_time(bond, reps)
            kernel.append(k)
            composed.append(c)
        print(json.dumps({"step": True, "bond": bond, "reps": reps, "rounds": rounds, "swap_theta_kernel_ms": stats(kernel),
                          "gemm_plus_permute_ms": stats(composed), "ratio_of_medians": round(float(np.median(composed) / np.median(kernel)), 3)}),
              flush=True)
    n = 2 * r_bits
    rng = np.random.default_rng(0)
    link = [min(2 ** (b + 1), 2 ** (n - b - 1), cap) for b in range(n - 1)]
    cores = [rng.standard_normal((1 if s == 0 else link[s - 1], 2, link[s] if s < n - 1 else 1)) / np.sqrt(2.0) for s in range(n)]
    tt = t4a_amd.SimpleTensorTrain(cores)
    target = swap_mod.quantics_target(n, 2, "sequential")
    opts = t4a_amd.SwapOptions(max_bond_dim=cap)
    wall, parts = [], {"kernel_ms": [], "svd_ms": [], "qr_ms": []}
    for rep in range(rounds + 1):  # rep 0 warms up
        t0 = time.perf_counter()
        out = t4a_amd.swap_site_indices_legs(tt, target, opts)
        dt = (time.perf_counter() - t0) * 1e3
        _, ms = t4a_amd.swap_site_indices_legs(tt, target, opts, timings=True)
        if rep:
            wall.append(dt)
            for k in parts:
                parts[k].append(ms[k])
    print(json.dumps({"regroup_quantics": True, "R": r_bits, "max_bond_dim": cap, "n_steps": len(t4a_amd.SwapSchedule.build(n, {k: k[0] for k in target}, target)),
                      "link_dims_max": max(out.link_dims()), "wall_ms": stats(wall), **{k: stats(v) for k, v in parts.items()}}), flush=True)


if __name__ == "__main__":
    main()
