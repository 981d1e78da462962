"""Soak of the two kernels of the partial contraction (kernels_partial.hip: the site product of the naive route and the half product
of zip-up and fit) on integer-valued operands against int64 einsums, every comparison EXACT — the assertions of
tests/test_gpu_partial_exact.py over random operands: 1 - 5 sites, leg dims 1 - 3 per leg and site, a random valid spec per site
(each leg of A is contracted with, identified with or kept apart from a leg of B of the same dimension), every inner bond of A and
of B drawn independently from {1, 2, 3, 5, 15, 16, 17, 20, 31, 32, 33} (both sides of the 16 x 16 matrix-core threshold, summed
dimensions that are no multiple of 4, ragged last tiles), entries from {-1, 0, 1}: the largest sum is 33 * 33 * 9 < 2^53.  Bonds are
lowered one at a time until no site of the naive product and no half product holds more than 2.4 million elements.
  per case: every site tensor of partial_contract (Naive, uncompressed) against np_site, and at one random site both half products
  with an environment index of 1 - 40 against np_half_left / np_half_right.
usage: python3 tests/soak/soak_partial.py N [seed0]     (test infrastructure: numpy int64 is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
from t4a_amd.partial import _partial_half  # noqa: E402
import partial_np as pn  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
BONDS = [1, 2, 3, 5, 15, 16, 17, 20, 31, 32, 33]
SITE_MAX = 2400000
N_ENV_MAX = 40
fails = 0
counts = {}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def count(key, by=1):
    counts[key] = counts.get(key, 0) + by


def mismatch(got, want):
    """None when the device's f64 values are integers equal to the int64 reference, else what differs"""
    got = np.asarray(got)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    if not np.array_equal(got, np.rint(got)):
        return "values that are no integers"
    as_int = got.astype(np.int64)
    if np.array_equal(as_int, want):
        return None
    bad = np.argwhere(as_int != want)
    first = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {want.size} entries differ, first at {first}: device {got[first]!r}, reference {int(want[first])}"


def make_case(rng):
    n = int(rng.integers(1, 6))
    da = [tuple(int(x) for x in rng.integers(1, 4, 2)) for _ in range(n)]
    db = [tuple(int(x) for x in rng.integers(1, 4, 2)) for _ in range(n)]
    contract, diagonal = [], []
    for i in range(n):
        free_b = [0, 1]
        for la in (int(x) for x in rng.permutation(2)):
            kind = int(rng.integers(0, 3))  # 0 contract, 1 diagonal, 2 keep
            match = [lb for lb in free_b if db[i][lb] == da[i][la]]
            if kind == 2 or not match:
                continue
            lb = match[int(rng.integers(0, len(match)))]
            free_b.remove(lb)
            (contract if kind == 0 else diagonal).append(((i, la), (i, lb)))
    plan = pn.np_plan(da, db, contract, diagonal)
    ba = [1] + [BONDS[int(rng.integers(0, len(BONDS)))] for _ in range(n - 1)] + [1]
    bb = [1] + [BONDS[int(rng.integers(0, len(BONDS)))] for _ in range(n - 1)] + [1]

    def too_big():
        return any(max(ba[s] * bb[s], N_ENV_MAX) * plan[s].S * plan[s].T * max(ba[s + 1] * bb[s + 1], N_ENV_MAX) > SITE_MAX for s in range(n))

    while too_big():  # lower one bond to the next smaller value of the list
        which = ba if rng.integers(0, 2) else bb
        s = int(rng.integers(1, n))
        which[s] = BONDS[max(0, BONDS.index(which[s]) - 1)]
    a = [np.asarray(rng.integers(-1, 2, size=(ba[s], da[s][0], da[s][1], ba[s + 1])), dtype=np.float64) for s in range(n)]
    b = [np.asarray(rng.integers(-1, 2, size=(bb[s], db[s][0], db[s][1], bb[s + 1])), dtype=np.float64) for s in range(n)]
    return n, da, db, contract, diagonal, plan, ba, bb, a, b


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n, da, db, contract, diagonal, plan, ba, bb, a, b = make_case(rng)
    ctx = f"seed {seed0 + case} n {n} dims A {da} B {db} contract {contract} diagonal {diagonal} bonds A {ba} B {bb}"
    try:
        ma, mb = t4a.MPO(a), t4a.MPO(b)
        spec = t4a.PartialContractionSpec(contract, diagonal)
        ia, ib = [x.astype(np.int64) for x in a], [x.astype(np.int64) for x in b]
        prod = t4a.partial_contract(ma, mb, spec)
        if prod.site_dims() != [(p.S, p.T) for p in plan]:
            fail(ctx, f"site dims {prod.site_dims()}")
        for s in range(n):
            bad = mismatch(prod.site_tensor(s), pn.np_site(ia[s], ib[s], plan[s]))
            if bad:
                fail(ctx, f"naive site {s}: {bad}")
            count("naive_elements", prod.site_tensor(s).size)
        site = int(rng.integers(0, n))
        n_env = int(rng.integers(1, N_ENV_MAX + 1))
        env_l = rng.integers(-1, 2, size=(n_env, ba[site], bb[site])).astype(np.float64)
        env_r = rng.integers(-1, 2, size=(ba[site + 1], bb[site + 1], n_env)).astype(np.float64)
        bad = mismatch(_partial_half(env_l, 0, ma, mb, spec, site), pn.np_half_left(env_l.astype(np.int64), ia[site], ib[site], plan[site]))
        if bad:
            fail(ctx, f"left half product at site {site}, n_env {n_env}: {bad}")
        bad = mismatch(_partial_half(env_r, 1, ma, mb, spec, site), pn.np_half_right(env_r.astype(np.int64), ia[site], ib[site], plan[site]))
        if bad:
            fail(ctx, f"right half product at site {site}, n_env {n_env}: {bad}")
        count("core_rows" if n_env >= 16 else "scalar_rows")
        count("diagonal_pairs", len(diagonal))
        count("contract_pairs", len(contract))
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
