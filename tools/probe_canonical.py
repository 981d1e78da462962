"""Times SiteTensorTrain.from_tensor_train and VidalTensorTrain.from_tensor_train (t4a_amd.canonical) at one stated shape and prints each
next to a one-thread numpy run of the same algorithm (the restatement in tests/canonical_np.py, rrLU through the CPU oracle).

Shape: a train of `n` sites of dimension `d` with bond min(chi, d^i, d^(n-i)), standard normal cores; the site form is built at the
middle centre.  Median of `reps` runs after a warm-up.

    python tools/probe_canonical.py [n] [chi] [d] [reps]
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
import canonical_np as cn  # noqa: E402


def median_ms(f, reps):
    f()  # warm-up (allocations, first launches)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 3), round(min(times), 3)


def main():
    a = [int(x) for x in sys.argv[1:]]
    n, chi, d, reps = (a + [16, 48, 2, 5][len(a):])[:4]
    bonds = [min(chi, d ** min(i, n - i)) for i in range(n + 1)]
    cores = cn.random_train([d] * n, bonds, cn.SEED)
    tt = t4a_amd.SimpleTensorTrain(cores)
    pts = cn.lcg_points(256, [d] * n, 3)
    ref = tt.evaluate(pts)
    scale = max(1.0, float(np.abs(ref).max()))
    center = n // 2
    rows = (("site", lambda: t4a_amd.SiteTensorTrain.from_tensor_train(tt, center), lambda: cn.site_form(cores, center)),
            ("vidal", lambda: t4a_amd.VidalTensorTrain.from_tensor_train(tt), lambda: cn.vidal_form(cores)))
    for name, dev, host in rows:
        med, best = median_ms(dev, reps)
        np_med, _ = median_ms(host, reps)
        form = dev()
        want = host()
        want_links = [t.shape[0] for t in (want if name == "site" else want[0])[1:]]
        print(json.dumps({"form": name, "n": n, "chi": chi, "d": d, "link_dims": form.link_dims(), "links_match": form.link_dims() == want_links,
                          "gpu_ms_median": med, "gpu_ms_min": best, "numpy_1thread_ms_median": np_med,
                          "max_rel_dev": float(np.abs(form.to_tensor_train().evaluate(pts) - ref).max() / scale)}), flush=True)


if __name__ == "__main__":
    main()
