"""Soak of the gauge forms (t4a_amd.canonical: SiteTensorTrain / center_canonicalize, VidalTensorTrain, InverseTensorTrain;
tensor4all-simplett/src/canonical.rs:118-544, vidal.rs:215-767) against the numpy restatement of tests/canonical_np.py on random trains:
2 - 8 sites of dimension 1 - 4, bond dimensions 1 - 24 (also wider than the sites allow), gaussian cores / one bond index zeroed on both
neighbours / cores scaled by up to 1e+-20 / n each.  The same checks as tests/test_gpu_canonical.py:
  bit for bit: every re-gauged core of a gauge step taken from the device's own state, the bond dimensions, the Vidal / inverse arithmetic
  of new / to_tensor_train / from_vidal with random vectors (shorter and longer than their bonds, guard values mixed in);
  componentwise gamma_k (|F| |core|): the core that absorbed the other factor;
  1e-10 of the largest value: to_tensor_train of every form; 1e-12 lambda_max: the Vidal values; 1e-11: orthonormal rows of Gamma lambda.
usage: python3 tests/soak/soak_canonical.py N [seed0]     (test infrastructure: the oracle is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import canonical_np as cn  # noqa: E402
from luci_exact_np import gamma, _ratio_to_product_bound  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
counts = {}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def in_bound(dev, a, b):
    k = a.shape[1]
    return _ratio_to_product_bound(np.ascontiguousarray(dev), np.ascontiguousarray(a), np.ascontiguousarray(b)) * 2 * gamma(k + 2) / gamma(k) <= 1.0


def make_train(rng):
    n = int(rng.integers(2, 9))
    dims = [int(rng.integers(1, 5)) for _ in range(n)]
    chi = int(rng.integers(1, 25))
    kind = int(rng.integers(0, 3))
    links = [1] + [int(rng.integers(1, chi + 1)) for _ in range(n - 1)] + [1]
    cores = [rng.standard_normal((links[i], dims[i], links[i + 1])) for i in range(n)]
    if kind == 1:
        b = int(rng.integers(1, n))
        j = int(rng.integers(0, links[b]))
        cores[b - 1][:, :, j] = 0.0
        cores[b][j, :, :] = 0.0
    elif kind == 2:
        cores = [c * 10.0 ** float(rng.integers(-20, 21) / n) for c in cores]
    return dims, cores, kind


def random_vector(rng, bond):
    k = max(0, bond + int(rng.integers(-2, 3)))
    v = rng.standard_normal(k)
    for i in range(k):
        if rng.random() < 0.3:
            v[i] = cn.G_VALUES[int(rng.integers(0, len(cn.G_VALUES)))]
    return v


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    dims, cores, kind = make_train(rng)
    n = len(dims)
    ctx = f"seed {seed0 + case} dims {dims} links {[c.shape[2] for c in cores[:-1]]} kind {kind}"
    try:
        full = cn.dense(cores)
        scale = float(np.abs(full).max())
        pts = cn.lcg_points(64, dims, seed0 + case)
        want = full[tuple(pts.T)]
        tt = t4a.SimpleTensorTrain(cores)
        try:
            ref0 = cn.site_form(cores, 0)
        except Exception:  # noqa: BLE001
            ref0 = None
        try:
            s = t4a.SiteTensorTrain.from_tensor_train(tt, 0)
        except t4a.T4aError as exc:
            # a bond matrix that is exactly zero: the device refuses rank 0, the restatement carries a bond of 0
            if "rank 0" in str(exc) and (ref0 is None or any(0 in c.shape for c in ref0)):
                counts["rank0_refused"] = counts.get("rank0_refused", 0) + 1
                continue
            raise
        if s.link_dims() != [c.shape[0] for c in ref0[1:]]:
            fail(ctx, f"link dims at centre 0: {s.link_dims()} vs {[c.shape[0] for c in ref0[1:]]}")
            continue
        for i in range(n - 1):
            a, b = s.site_tensor(i), s.site_tensor(i + 1)
            s.move_center_right()
            na, nb = s.site_tensor(i), s.site_tensor(i + 1)
            wa, wb = cn.left_step(a, b)
            if not bits(na, wa) or nb.shape != wb.shape:
                fail(ctx, f"left step at site {i}: the gauged core differs")
            elif not in_bound(cn.right_matrix(nb), cn.step_factors(a, True)[1], cn.right_matrix(b)):
                fail(ctx, f"left step at site {i}: the absorbing core is outside the product bound")
        for i in range(n - 1, 0, -1):
            a, b = s.site_tensor(i - 1), s.site_tensor(i)
            s.move_center_left()
            na, nb = s.site_tensor(i - 1), s.site_tensor(i)
            wa, wb = cn.right_step(a, b)
            if not bits(nb, wb) or na.shape != wa.shape:
                fail(ctx, f"right step at site {i}: the gauged core differs")
            elif not in_bound(cn.left_matrix(na), cn.left_matrix(a), cn.step_factors(b, False)[1].T):
                fail(ctx, f"right step at site {i}: the absorbing core is outside the product bound")
        counts["steps"] = counts.get("steps", 0) + 2 * (n - 1)
        if scale > 0 and not np.abs(s.to_tensor_train().evaluate(pts) - want).max() <= 1e-10 * scale:
            fail(ctx, "site form: values differ")
        c = int(rng.integers(0, n))
        plain = tt.clone()
        t4a.center_canonicalize(plain, c)
        if not all(bits(g, w) for g, w in zip(plain.site_tensors(), t4a.SiteTensorTrain.from_tensor_train(tt, c).site_tensors())):
            fail(ctx, f"center_canonicalize differs from the site form at centre {c}")
        # ---- Vidal and inverse forms
        start = int(rng.integers(0, n))
        end = int(rng.integers(start, n + 1)) if rng.random() < 0.5 else n
        if rng.random() < 0.5:
            start, end = 0, n
        v = t4a.VidalTensorTrain.from_tensor_train_with_partition(tt, range(start, end))
        ref_t, ref_sv = cn.vidal_form(cores, start, end)
        sv = v.all_singular_values()
        if [len(x) for x in sv] != [len(x) for x in ref_sv]:
            fail(ctx, f"vidal {start}..{end}: bond dimensions differ")
            continue
        for b, (x, y) in enumerate(zip(sv, ref_sv)):
            if len(y) and not (np.abs(x - y).max() <= 1e-12 * y.max() and np.all(np.diff(x) <= 0) and np.all(x >= 0)):
                fail(ctx, f"vidal {start}..{end}: singular values of bond {b} differ by {np.abs(x - y).max() / y.max():.2e}")
        # a singular value at the reference's guard (<= 1e-15: divided by 1.0, multiplied back by itself) loses the tensor in the reference
        # as well, and a value near it may fall on either side of the guard on two correct implementations: only the counts are compared
        at_guard = any(len(y) and y.min() <= 1e-14 for y in ref_sv)
        if at_guard:
            counts["vidal_at_guard"] = counts.get("vidal_at_guard", 0) + 1
            if [int(np.sum(x > 1e-12 * x.max())) for x in sv if len(x)] != [int(np.sum(y > 1e-12 * y.max())) for y in ref_sv if len(y)]:
                fail(ctx, f"vidal {start}..{end}: the number of values above 1e-12 lambda_max differs")
        elif scale > 0 and not np.abs(v.to_tensor_train().evaluate(pts) - want).max() <= 1e-10 * scale:
            fail(ctx, f"vidal {start}..{end}: values differ")
        if kind == 0 and all(len(x) == 0 or x.min() > 1e-10 * x.max() for x in sv):
            d = cn.rows_orthonormal_defect(v.site_tensors(), sv, start, end)
            if not d <= 1e-11:
                fail(ctx, f"vidal {start}..{end}: rows of Gamma lambda are off orthonormal by {d:.2e}")
        counts["vidal"] = counts.get("vidal", 0) + 1
        # ---- the scale kernel alone, bit for bit
        vecs = [random_vector(rng, cores[i].shape[2]) for i in range(n - 1)]
        with np.errstate(all="ignore"):
            vv = t4a.VidalTensorTrain.new(cores, vecs)
            if not all(bits(g, w) for g, w in zip(vv.to_tensor_train().site_tensors(), cn.vidal_to_tt(cores, vecs))):
                fail(ctx, "VidalTensorTrain.to_tensor_train differs from numpy")
            inv = t4a.InverseTensorTrain.from_vidal(vv)
            wt, wi = cn.inverse_from_vidal(cores, vecs)
            if not all(bits(g, w) for g, w in zip(inv.site_tensors(), wt)) or not all(bits(g, w) for g, w in zip(inv.all_inverse_singular_values(), wi)):
                fail(ctx, "InverseTensorTrain.from_vidal differs from numpy")
            if not all(bits(g, w) for g, w in zip(inv.to_tensor_train().site_tensors(), cn.inverse_to_tt(wt, wi))):
                fail(ctx, "InverseTensorTrain.to_tensor_train differs from numpy")
    except Exception as exc:  # noqa: BLE001 (a soak reports and goes on)
        fail(ctx, f"exception {type(exc).__name__}: {exc}")
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
