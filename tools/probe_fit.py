"""Times the variational (fit) contraction of two MPOs (t4a_amd.contract_fit) at one stated shape next to contract_zipup, the
other truncated route, in the same process, and prints the error of both against the exact lazy product.

Shape: two operators of `n` sites, site dims (2, 2), bonds `chi_a` and `chi_b` (the LCG fixtures of the tests), truncated to
`max_bond_dim` with tolerance 1e-12; the fit starts from its own zip-up and runs exactly `sweeps` sweeps (convergence_tol = 0).
A call returns after its stream is synchronised, so the window holds all device work.  The error is the relative l2 deviation on
4096 random points against Contraction.evaluate_many.

    python tools/probe_fit.py [n] [chi_a] [chi_b] [max_bond_dim] [sweeps] [reps] [--fit-only]

--fit-only skips the zip-up timing (for a kernel trace of the fit alone: one warm-up call and `reps` timed calls).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
from fit_np import random_tensors, SEED  # noqa: E402


def timed(call, reps):
    r = call()  # warm-up (allocations, first launches)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        times.append((time.perf_counter() - t0) * 1e3)
    return r, times


def main():
    fit_only = "--fit-only" in sys.argv
    a = [int(x) for x in sys.argv[1:] if not x.startswith("--")]
    n, chi_a, chi_b, cap, sweeps, reps = (a + [16, 32, 24, 64, 2, 5][len(a):])[:6]
    ta = random_tensors([1] + [chi_a] * (n - 1) + [1], 2, 2, SEED)
    tb = random_tensors([1] + [chi_b] * (n - 1) + [1], 2, 2, SEED ^ 0xFF)
    A, B = t4a_amd.MPO(ta), t4a_amd.MPO(tb)
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 2, (4096, n, 2))
    exact, _ = t4a_amd.Contraction(A, B).evaluate_many(idx)
    flat = idx.reshape(4096, 2 * n)
    fit_opts = t4a_amd.FitOptions(tolerance=1e-12, max_bond_dim=cap, max_sweeps=sweeps, convergence_tol=0.0)
    zip_opts = t4a_amd.ContractionOptions(tolerance=1e-12, max_bond_dim=cap)
    routes = [("fit", lambda: t4a_amd.contract_fit(A, B, fit_opts))]
    if not fit_only:
        routes.append(("zipup", lambda: t4a_amd.contract_zipup(A, B, zip_opts)))
    for name, call in routes:
        r, times = timed(call, reps)
        got = r.evaluate(flat)
        print(json.dumps({"route": name, "n": n, "chi_a": chi_a, "chi_b": chi_b, "max_bond_dim": cap,
                          "sweeps": sweeps if name == "fit" else None, "link_dims": r.link_dims(),
                          "gpu_ms_median": round(float(np.median(times)), 3), "gpu_ms_min": round(min(times), 3),
                          "rel_l2_error": float(np.linalg.norm(got - exact) / np.linalg.norm(exact))}), flush=True)


if __name__ == "__main__":
    main()
