"""Soak of swap_site_indices (csrc/kernels_swap.hip, csrc/swap.hip) over random cases — the assertions of
tests/test_gpu_swap_exact.py and tests/test_gpu_swap.py:
  step kernel: cores with entries from {-1, 0, 1}, bonds l, m, r drawn from {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33} (both sides of the
    16 x 16 matrix-core tile, of the chunk of four and of the trip of four chunks), 0 - 3 legs of dim 2 or 3 per site, a random
    split of the merged legs, right- or left-moving: swap_theta must EQUAL the int64 einsum and report the route of its shape;
  driver: a random leg train of 2 - 6 sites with 0 - 2 legs of dim 2 or 3 per site (at most 4096 dense elements), gaussian cores, a
    random partial target: the result against the exact axis permutation within C_DENSE * n_steps * eps * |T|_F (tests/swap_np.py),
    every leg on its target, the legs of touched sites in ascending key order, the centre as the restatement reports it.
usage: python3 tests/soak/soak_swap.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import swap_np as sn  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
BONDS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33]
fails = 0
counts = {}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def count(key, by=1):
    counts[key] = counts.get(key, 0) + by


def step_case(rng, ctx):
    l, m, r = (BONDS[int(rng.integers(0, len(BONDS)))] for _ in range(3))
    n_left, n_right = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    keys = [int(k) for k in rng.permutation(n_left + n_right)]
    legs = [(k, int(rng.integers(2, 4))) for k in keys]
    legs_left, legs_right = legs[:n_left], legs[n_left:]
    to_a = {k for k in keys if rng.random() < 0.5}
    to_b = set(keys) - to_a
    left_moving = bool(rng.integers(0, 2))
    x = int(np.prod([d for _, d in legs_left], dtype=np.int64))
    y = int(np.prod([d for _, d in legs_right], dtype=np.int64))
    a, b = rng.integers(-1, 2, size=(l, x, m)), rng.integers(-1, 2, size=(m, y, r))
    to_left, to_right = (to_b, to_a) if left_moving else (to_a, to_b)
    want, _, _ = sn.theta_np(a, b, legs_left, legs_right, to_left, to_right)
    got, route = t4a.swap_theta(a, b, legs_left, legs_right, to_a, to_b, left_moving=left_moving)
    ctx = f"{ctx} step l {l} m {m} r {r} legs {legs_left} | {legs_right} to_a {sorted(to_a)} left_moving {left_moving}"
    if got.shape != want.shape or not np.array_equal(got, want.astype(np.float64)):
        fail(ctx, f"swap_theta differs from the integer einsum (shape {got.shape} against {want.shape})")
    if route != ((2 if l >= 16 and r >= 16 else 0) | (1 if l % 16 or r % 16 else 0)):
        fail(ctx, f"route {route}")
    count(f"route_{route}")


def driver_case(rng, ctx):
    n = int(rng.integers(2, 7))
    while True:
        legs, key = [], 0
        for _ in range(n):
            site = []
            for _ in range(int(rng.integers(0, 3))):
                site.append((key, int(rng.integers(2, 4))))
                key += 1
            legs.append(site)
        total = int(np.prod([d for s in legs for _, d in s], dtype=np.int64))
        if key and total <= 4096:
            break
    sd = [int(np.prod([d for _, d in s], dtype=np.int64)) for s in legs]
    bonds = [int(min(rng.integers(1, 18), np.prod(sd[:i + 1]) * 2, np.prod(sd[i + 1:]) * 2)) for i in range(n - 1)]
    cores = sn.random_train(rng, legs, bonds)
    target = {k: int(rng.integers(0, n)) for k in range(key) if rng.random() < 0.5}
    ctx = f"{ctx} driver n {n} legs {legs} bonds {bonds} target {target}"
    dense = sn.to_dense(cores, legs)
    _, ref_legs, ref_center, info = sn.swap(cores, legs, target)
    lt = t4a.LegTrain(t4a.SimpleTensorTrain(cores), legs)
    try:
        out = t4a.swap_site_indices_legs(lt, target)
    except t4a.T4aError as exc:
        if "at most 8" not in str(exc):  # a merged pair of more than eight legs is refused at plan time
            raise
        count("refused_more_than_8_legs")
        return
    if info["n_steps"] == 0:
        if out is not lt:
            fail(ctx, "an empty schedule did not return the input")
        count("no_op")
        return
    if out.legs != ref_legs or out.center != ref_center:
        fail(ctx, f"legs {out.legs} centre {out.center} against {ref_legs} / {ref_center}")
        return
    err = np.linalg.norm(out.to_dense() - sn.permuted(dense, sn.keys_of(legs), out.keys()))
    tol = sn.C_DENSE * info["n_steps"] * sn.EPS * np.linalg.norm(dense)
    if not err <= tol:
        fail(ctx, f"dense deviation {err:.3e} above {tol:.3e}")
    count("steps", info["n_steps"])


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    ctx = f"seed {seed0 + case}"
    try:
        step_case(rng, ctx)
        driver_case(rng, ctx)
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
