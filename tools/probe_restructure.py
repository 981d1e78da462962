"""Times fuse_to of an interleaved 2-variable quantics train and unfuse_quantics with its QR share.

1. The fuse: R groups of two binary-leg sites with every bond equal to `bond` (t4a_gpu_fuse_time) — the one lock-step launch of
   fuse_round_kernel (csrc/kernels_restructure.hip) over all R groups against the composition a train has without it: one
   swap_theta launch per pair with every leg sent left, issued group by group.  Both are timed with device events around `reps`
   repetitions behind a warm-up, in the same process and alternating, `rounds` times; medians with min and max are reported.
2. fuse_quantics and unfuse_quantics of a random train with R bits per variable at a bond cap: host wall ms of each call (each ends
   synced) and the number of QR factorisations of the split.

    python tools/probe_restructure.py [rounds=5] [cap=64] [out.json]     (bits R = 8 and 16, bonds 8 .. 256)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python")]

import t4a_amd  # noqa: E402
from t4a_amd import restructure as rmod  # noqa: E402


def stats(v):
    return {"median": round(float(np.median(v)), 5), "min": round(float(min(v)), 5), "max": round(float(max(v)), 5)}


def main():
    nums = [int(x) for x in sys.argv[1:] if x.isdigit()]
    paths = [x for x in sys.argv[1:] if not x.isdigit()]
    rounds, cap = (nums + [5, 64][len(nums):])[:2]
    rows = []
    t4a_amd.set_device(0)
    for r_bits in (8, 16):
        for bond in (8, 16, 32, 64, 128, 256):
            reps = 200 if bond <= 64 else 40
            rmod.fuse_time(r_bits, bond, 3)  # warm both routes up at this shape
            one, per_pair = [], []
            for _ in range(rounds):
                a, b = rmod.fuse_time(r_bits, bond, reps)
                one.append(a)
                per_pair.append(b)
            rows.append({"fuse": True, "R": r_bits, "bond": bond, "reps": reps, "rounds": rounds, "lock_step_round_ms": stats(one),
                         "swap_theta_per_pair_ms": stats(per_pair), "ratio_of_medians": round(float(np.median(per_pair) / np.median(one)), 3)})
            print(json.dumps(rows[-1]), flush=True)
    for r_bits in (8, 16):
        n = 2 * r_bits
        rng = np.random.default_rng(0)
        link = [min(2 ** (b + 1), 2 ** (n - b - 1), cap) for b in range(n - 1)]
        cores = [rng.standard_normal((1 if s == 0 else link[s - 1], 2, link[s] if s < n - 1 else 1)) / np.sqrt(2.0) for s in range(n)]
        tt = t4a_amd.SimpleTensorTrain(cores)
        fuse_ms, unfuse_ms = [], []
        for rep in range(rounds + 1):  # rep 0 warms up
            t0 = time.perf_counter()
            fused = t4a_amd.fuse_quantics(tt, 2)
            t1 = time.perf_counter()
            back = t4a_amd.unfuse_quantics(fused, 2)
            t2 = time.perf_counter()
            if rep:
                fuse_ms.append((t1 - t0) * 1e3)
                unfuse_ms.append((t2 - t1) * 1e3)
        rows.append({"quantics": True, "R": r_bits, "max_bond_dim": cap, "fused_link_dims_max": max(fused.link_dims()),
                     "unfused_link_dims_max": max(back.link_dims()), "n_qr": r_bits, "fuse_quantics_wall_ms": stats(fuse_ms),
                     "unfuse_quantics_wall_ms": stats(unfuse_ms), "unfuse_ms_per_qr": round(float(np.median(unfuse_ms)) / r_bits, 4)})
        print(json.dumps(rows[-1]), flush=True)
    for p in paths:
        with open(p, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
