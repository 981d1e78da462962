"""Soak of fuse_to, split_to and restructure_to (csrc/kernels_restructure.hip, csrc/restructure.hip) over random cases — the
assertions of tests/test_gpu_restructure_exact.py and tests/test_gpu_restructure.py:
  fuse kernel: 1 - 6 jobs in one launch, cores with entries from {-2 .. 2}, bonds l, m, r drawn from {1, 2, 3, 4, 5, 15, 16, 17, 31,
    32, 33} (both sides of the 16 x 16 matrix-core tile, of the chunk of four and of the trip of four chunks), 0 - 3 legs of dim 2 or 3
    in a random order: fuse_round must EQUAL the int64 einsum and report the route of every job's shape;
  drivers: a random leg train of 2 - 7 sites with 0 - 2 legs of dim 2 or 3 per site (at most 4096 dense elements), gaussian cores,
    and a random target (the keys shuffled and cut into groups): the plan must be the restatement's (kind, legs, counts, or the same
    refusal) and the result the regrouped dense tensor within the tolerance of tests/test_gpu_restructure.py.
usage: python3 tests/soak/soak_restructure.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import swap_np as sn  # noqa: E402
import restructure_np as rn  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
BONDS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33]
U = 2.0 ** -53
fails = 0
counts = {}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def count(key, by=1):
    counts[key] = counts.get(key, 0) + by


def kernel_case(rng, ctx):
    jobs, want = [], []
    for _ in range(int(rng.integers(1, 7))):
        l, m, r = (BONDS[int(rng.integers(0, len(BONDS)))] for _ in range(3))
        n_left, n_right = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        dims = [int(rng.integers(2, 4)) for _ in range(n_left + n_right)]
        x, y = int(np.prod(dims[:n_left], dtype=np.int64)), int(np.prod(dims[n_left:], dtype=np.int64))
        a, b = rng.integers(-2, 3, size=(l, x, m)), rng.integers(-2, 3, size=(m, y, r))
        order = [int(p) for p in rng.permutation(len(dims))]
        t = np.einsum("lxm,myr->lxyr", a, b).reshape([l] + dims + [r], order="F")
        t = np.transpose(t, [0] + [1 + p for p in order] + [len(dims) + 1]).reshape(l, x * y, r, order="F")
        jobs.append((a, b, dims, order) if dims else (a, b))
        want.append((t, (2 if l >= 16 and r >= 16 else 0) | (1 if l % 16 or r % 16 else 0)))
    got = t4a.fuse_round(jobs)
    for k, ((res, route), (t, rt)) in enumerate(zip(got, want)):
        if res.shape != t.shape or not np.array_equal(res, t.astype(np.float64)):
            fail(f"{ctx} kernel job {k} of {len(jobs)} shapes {jobs[k][0].shape} {jobs[k][1].shape}", "fuse_round differs from the integer einsum")
        if route != rt:
            fail(f"{ctx} kernel job {k}", f"route {route} against {rt}")
        count(f"route_{route}")


def driver_case(rng, ctx):
    n = int(rng.integers(2, 8))
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
    keys = list(range(key))
    if rng.random() < 0.4:  # the other targets keep the chain order of the keys: fuse, split and split-then-fuse
        keys = [int(k) for k in rng.permutation(key)]
    cuts = sorted({int(c) for c in rng.integers(1, key, size=int(rng.integers(0, key)))}) if key > 1 else []
    target = [keys[a:b] for a, b in zip([0] + cuts, cuts + [key])]
    ctx = f"{ctx} driver legs {legs} bonds {bonds} target {target}"
    try:
        ref = rn.plan(legs, target, bonds)
    except (ValueError, NotImplementedError) as exc:
        try:
            t4a.restructure_plan(legs, target, bonds)
            fail(ctx, f"the restatement refuses ({exc}) and the library does not")
        except t4a.T4aError as lib:
            if str(exc) not in str(lib):
                fail(ctx, f"refusals differ: {exc} | {lib}")
        count("refused")
        return
    p = t4a.restructure_plan(legs, target, bonds)
    if any(p[k] != ref[k] for k in ("kind", "legs", "fuse_rounds", "fuse_launches", "n_qr", "swap_target")):
        fail(ctx, f"plan {p} against {ref}")
        return
    try:
        out = t4a.restructure_to(t4a.LegTrain(t4a.SimpleTensorTrain(cores), legs), target, as_legs=True)
    except t4a.T4aError as exc:
        if "at most 8" not in str(exc) and "more than 8" not in str(exc):  # the swap and reorder launches hold eight legs
            raise
        count("refused_more_than_8_legs")
        return
    dense = sn.to_dense(cores, legs)
    ref_cores, ref_legs, info = rn.restructure(cores, legs, target)
    if out.legs != ref_legs:
        fail(ctx, f"legs {out.legs} against {ref_legs}")
        return
    share = (sum(bonds) * 4 + 2 * n + len(target)) * U * float(np.linalg.norm(sn.to_dense([np.abs(c) for c in ref_cores], ref_legs)))
    tol = (sn.C_DENSE * info["n_steps"] + rn.C_SPLIT * info["n_qr"]) * rn.EPS * np.linalg.norm(dense) + share
    err = np.linalg.norm(out.to_dense() - sn.permuted(dense, sn.keys_of(legs), out.keys()))
    if not err <= tol:
        fail(ctx, f"{ref['kind']}: dense deviation {err:.3e} above {tol:.3e}")
    count(ref["kind"])


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    ctx = f"seed {seed0 + case}"
    try:
        kernel_case(rng, ctx)
        driver_case(rng, ctx)
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
