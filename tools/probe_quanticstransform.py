"""Times the quantics transform operators (t4a_amd.quanticstransform) at one stated shape and prints each next to a one-thread
numpy run of the same algorithm (the restatements in tests/test_gpu_mpo.py and tests/test_gpu_quanticstransform.py).

Shape: `r` binary sites, a state of bond `chi` (the LCG fixtures of the tests), a kernel train `f` of bond `chi_f`:
  shift_naive / shift_zipup   apply(shift_operator(r, 12345, Periodic), state) compressed at tolerance 1e-12
  difference_kernel           difference_kernel_mpo(f, Periodic)
  convolution                 apply(difference_kernel_mpo(f), state) by ZipUp with max_bond_dim = chi
Every timing is the median of `reps` calls after one warm-up, with a device synchronisation inside the timed window; the deviation
is the largest difference from the numpy result on 256 random points, relative to max(1, max|value|).

    python tools/probe_quanticstransform.py [r] [chi] [chi_f] [reps]
"""
import os

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the numpy side runs on one thread
    os.environ[v] = "1"

import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

import t4a_amd  # noqa: E402
from t4a_amd import quanticstransform as qt  # noqa: E402
from test_gpu_mpo import random_tensors, np_naive, np_zipup, np_eval, SEED  # noqa: E402
from test_gpu_quanticstransform import np_difference_kernel  # noqa: E402


def timed(call, reps):
    call()  # warm-up (allocations, first launches)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def numpy_timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    a = [int(x) for x in sys.argv[1:]]
    r, chi, chi_f, reps = (a + [20, 64, 16, 5][len(a):])[:4]
    P = qt.BoundaryCondition.Periodic
    state4 = random_tensors([min(chi, 2 ** min(i, r - i)) for i in range(r + 1)], 2, 1, SEED)
    f4 = random_tensors([min(chi_f, 2 ** min(i, r - i)) for i in range(r + 1)], 2, 1, SEED ^ 0xFF)
    state = t4a_amd.SimpleTensorTrain([t[:, :, 0, :] for t in state4])
    f = t4a_amd.SimpleTensorTrain([t[:, :, 0, :] for t in f4])
    rng = np.random.default_rng(0)
    pts = rng.integers(0, 2, (256, r))
    idx = np.zeros((256, 2 * r), dtype=np.int64)
    idx[:, 0::2] = pts

    def report(name, ms, np_ms, got, exp, links, extra=None):
        row = {"step": name, "r": r, "chi": chi, "chi_f": chi_f, "link_dims_max": max(links),
               "gpu_ms_median": round(float(np.median(ms)), 3), "gpu_ms_min": round(min(ms), 3), "numpy_1thread_ms": round(np_ms, 1),
               "max_rel_dev": float(np.abs(got - exp).max() / max(1.0, np.abs(exp).max()))}
        row.update(extra or {})
        print(json.dumps(row), flush=True)

    shift = qt.shift_operator(r, 12345, P)
    shift.mpo()  # the upload is not part of apply's timing
    shift_np = shift.site_tensors()
    opts = t4a_amd.ContractionOptions(tolerance=1e-12)
    for name, alg, ref in (("shift_naive", t4a_amd.ContractionAlgorithm.Naive, np_naive), ("shift_zipup", t4a_amd.ContractionAlgorithm.ZipUp, np_zipup)):
        out, ms = timed(lambda: qt.apply(shift, state, alg, opts), reps)
        want, np_ms = numpy_timed(lambda: ref(shift_np, state4, opts))
        report(name, ms, np_ms, out.evaluate(pts), np_eval(want, idx), out.link_dims())

    kernel, ms = timed(lambda: qt.difference_kernel_mpo(f, P), reps)
    want, np_ms = numpy_timed(lambda: np_difference_kernel([t[:, :, 0, :] for t in f4], P))
    kidx = np.zeros((256, 2 * r), dtype=np.int64)
    kidx[:, 0::2], kidx[:, 1::2] = pts, rng.integers(0, 2, (256, r))
    report("difference_kernel", ms, np_ms, kernel.evaluate(kidx), np_eval(want, kidx), kernel.link_dims())

    cap = t4a_amd.ContractionOptions(tolerance=1e-12, max_bond_dim=chi)
    out, ms = timed(lambda: qt.apply(kernel, state, t4a_amd.ContractionAlgorithm.ZipUp, cap), reps)
    conv, np_ms = numpy_timed(lambda: np_zipup(want, state4, cap))
    report("convolution", ms, np_ms, out.evaluate(pts), np_eval(conv, idx), out.link_dims(), {"max_bond_dim": chi})


if __name__ == "__main__":
    main()
