"""Times the Hadamard product of two tensor trains through the partial contraction (t4a_amd.hadamard, zip-up: one launch of the half
product of csrc/kernels_partial.hip per site) next to the two routes that existed before it, in the same process and alternating:
  (a) the copy-tensor composition: A's site multiplied by delta(s, s', s'') on the host, then contract_zipup (two GEMMs, three
      permutations per site, a summed index larger by the site dimension);
  (b) ACI: elementwise_batched(ACI_PRODUCT) at the same cap (a cross interpolation: it samples, its error is not SVD-controlled).
Operands: two random trains of d binary sites at bond chi (standard normal entries / sqrt 2), tolerance 1e-12, caps chi and 2 chi.
A call returns after its stream is synchronised, so the host clock around it holds all device work.  The error is the relative l2
deviation on 4096 random points against the product of the two trains' own values (the uncompressed product).

    python tools/probe_partial.py [d=12] [reps=5] [chi ...=8 16 32 64] [--half-only CHI]

--half-only CHI launches only the half product of the middle site at bond CHI (one warm-up, `reps` calls through the test seam
t4a_gpu_mpo_partial_half) for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/probe_partial.py ...): the seam's host
time holds two copies, the kernel time is read from the trace.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python")]

import t4a_amd  # noqa: E402
from t4a_amd import MPO, ContractionOptions, ContractionAlgorithm, PartialContractionSpec  # noqa: E402
from t4a_amd.partial import _partial_half  # noqa: E402


def rand_tt(d, chi, seed):
    rng = np.random.default_rng(seed)
    link = [min(2 ** (b + 1), 2 ** (d - b - 1), chi) for b in range(d - 1)]
    return [rng.standard_normal((1 if s == 0 else link[s - 1], 2, link[s] if s < d - 1 else 1)) / np.sqrt(2.0) for s in range(d)]


def copy_composed(cores):
    """A'[a, s, s', c] = A[a, s, c] delta(s, s'): the operator whose matrix product with a state is the Hadamard product"""
    out = []
    for c in cores:
        t = np.zeros((c.shape[0], c.shape[1], c.shape[1], c.shape[2]))
        for s in range(c.shape[1]):
            t[:, s, s, :] = c[:, s, :]
        out.append(t)
    return out


def main():
    args = [x for x in sys.argv[1:]]
    half_only = None
    if "--half-only" in args:
        k = args.index("--half-only")
        half_only = int(args[k + 1])
        del args[k:k + 2]
    nums = [int(x) for x in args]
    d, reps = (nums + [12, 5][len(nums):])[:2]
    chis = nums[2:] or [8, 16, 32, 64]
    t4a_amd.set_device(0)
    if half_only is not None:
        chi = half_only
        a, b = rand_tt(d, chi, 1), rand_tt(d, chi, 2)
        ma, mb = MPO([c[:, :, None, :] for c in a]), MPO([c[:, :, None, :] for c in b])
        site = d // 2
        la, lb = a[site].shape[0], b[site].shape[0]
        for n_env in (chi, 2 * chi):
            env = np.random.default_rng(3).standard_normal((n_env, la, lb))
            for _ in range(reps + 1):
                _partial_half(env, 0, ma, mb, PartialContractionSpec.hadamard(d), site)
            print(json.dumps({"half_only": True, "chi": chi, "n_env": n_env, "site": site, "calls": reps + 1}), flush=True)
        return
    rng = np.random.default_rng(0)
    pts = rng.integers(0, 2, size=(4096, d))
    for chi in chis:
        a, b = rand_tt(d, chi, 1), rand_tt(d, chi, 2)
        ta, tb = t4a_amd.SimpleTensorTrain(a), t4a_amd.SimpleTensorTrain(b)
        exact = ta.evaluate(pts) * tb.evaluate(pts)
        op, state = MPO(copy_composed(a)), MPO.from_tensor_train(tb)
        for cap in (chi, 2 * chi):
            o = ContractionOptions(tolerance=1e-12, max_bond_dim=cap)
            ao = t4a_amd.AciOptions(tolerance=1e-12, max_bond_dim=cap, max_iters=8)
            routes = [("partial_zipup", lambda: t4a_amd.hadamard(ta, tb, ContractionAlgorithm.ZipUp, o)),
                      ("copy_tensor_zipup", lambda: t4a_amd.contract_zipup(op, state, o).to_tensor_train()),
                      ("aci", lambda: t4a_amd.elementwise_batched(t4a_amd.ACI_PRODUCT, [ta, tb], ao).tensor_train)]
            times = {name: [] for name, _ in routes}
            last = {}
            for rep in range(reps + 1):  # rep 0 warms every route up; the routes alternate inside a repetition
                for name, call in routes:
                    t0 = time.perf_counter()
                    last[name] = call()
                    if rep:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            for name, _ in routes:
                got = last[name].evaluate(pts)
                print(json.dumps({"route": name, "d": d, "chi": chi, "max_bond_dim": cap, "link_dims_max": max(last[name].link_dims()),
                                  "ms_median": round(float(np.median(times[name])), 3), "ms_min": round(min(times[name]), 3),
                                  "rel_l2_error": float(np.linalg.norm(got - exact) / np.linalg.norm(exact))}), flush=True)


if __name__ == "__main__":
    main()
