"""Times MPO-MPO contraction (t4a_amd.mpo.contract, Naive and ZipUp) at one stated shape and prints each next to a one-thread numpy
run of the same algorithm (the restatement in tests/test_gpu_mpo.py).

Shape: an operator of `n` sites, site dims (2, 2), bond `chi_op`, applied to a state of `n` sites, site dims (2, 1), bond
`chi_tt` (the LCG fixtures of the tests), truncated to `max_bond_dim` with tolerance 1e-12.

    python tools/probe_mpo.py [n] [chi_op] [chi_tt] [max_bond_dim] [reps]
"""
import os

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the numpy side runs on one thread
    os.environ[v] = "1"

import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
from t4a_amd import mpo  # noqa: E402
from test_gpu_mpo import random_tensors, np_naive, np_zipup, np_eval, SEED  # noqa: E402


def main():
    a = [int(x) for x in sys.argv[1:]]
    n, chi_op, chi_tt, cap, reps = (a + [16, 8, 48, 48, 5][len(a):])[:5]
    op = random_tensors([1] + [chi_op] * (n - 1) + [1], 2, 2, SEED)
    bonds = [min(chi_tt, 2 ** min(i, n - i)) for i in range(n + 1)]
    st = random_tensors(bonds, 2, 1, SEED ^ 0xFF)
    opts = t4a_amd.ContractionOptions(tolerance=1e-12, max_bond_dim=cap)
    A, B = t4a_amd.MPO(op), t4a_amd.MPO(st)
    rng = np.random.default_rng(0)
    idx = np.zeros((256, 2 * n), dtype=np.int64)
    idx[:, 0::2] = rng.integers(0, 2, (256, n))
    for name, alg, ref in (("naive", t4a_amd.ContractionAlgorithm.Naive, np_naive), ("zipup", t4a_amd.ContractionAlgorithm.ZipUp, np_zipup)):
        r = mpo.contract(A, B, alg, opts)  # warm-up (allocations, first launches)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = mpo.contract(A, B, alg, opts)
            times.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = ref(op, st, opts)
        np_ms = (time.perf_counter() - t0) * 1e3
        got, exp = r.evaluate(idx), np_eval(want, idx)
        print(json.dumps({"algorithm": name, "n": n, "chi_op": chi_op, "chi_tt": chi_tt, "max_bond_dim": cap,
                          "link_dims": r.link_dims(), "links_match": r.link_dims() == [t.shape[0] for t in want[1:]],
                          "gpu_ms_median": round(float(np.median(times)), 3), "gpu_ms_min": round(min(times), 3),
                          "numpy_1thread_ms": round(np_ms, 1),
                          "max_rel_dev": float(np.abs(got - exp).max() / max(1.0, np.abs(exp).max()))}), flush=True)


if __name__ == "__main__":
    main()
