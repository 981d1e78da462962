"""Soak of the MPO layer's kernels (kernels_contraction.hip: the environment walks and the pairing kernel; kernels_mpo.hip: the site
contraction of the naive product; tt_env_dot of evaluate_many) on integer-valued operands against int64 arithmetic, every comparison
EXACT — the assertions of tests/test_gpu_mpo_exact.py over random operands: 1 - 7 sites, site dims (s1, k, s2) of 1 - 3 each and per
site, every inner bond of A and of B drawn independently from {1, 2, 3, 5, 15, 16, 17, 20, 31, 32, 33} (both sides of the 16 x 16
matrix-core threshold of wg_product, summed dimensions that are no multiple of 4, more tiles than wavefronts), entries from
{-1, 0, 1}.  With bonds up to 33 a working set is at most 5 * 33 * 33 = 5445 doubles: every walk here is on the LDS route, the
scratch route is pinned by tests/test_gpu_mpo_exact.py alone.  Bonds are lowered one at a time until cnp.exact_bound < 2^53 (every
partial sum is then exact in f64 in any order) and until no site of the naive product holds more than 2.4 million elements; site
dims are lowered until the dense product has at most 2e5 entries.
  per case, np.array_equal against cnp.ContractionNP(exact=True) / np_site on int64 after checking that the device's values are
  integers: evaluate on 1 - 300 points, evaluate_left and evaluate_right at a random cut, evaluate_many at a random split (or the
  heuristic's), evaluate_matrix at a random cut with 1 - 130 rows and columns (up to three 64-wide tiles each way), and every site
  tensor of contract_naive without options.
usage: python3 tests/soak/soak_mpo.py N [seed0]     (test infrastructure: numpy int64 is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import contraction_np as cnp  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
BONDS = [1, 2, 3, 5, 15, 16, 17, 20, 31, 32, 33]
SITE_MAX = 2400000
DENSE_MAX = 200000
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


def bound_of(n, dims, ba, bb):
    total = 1
    for s in range(n):
        total *= dims[s][1]
    for s in range(1, n):
        total *= ba[s] * bb[s]
    return total


def make_operands(rng):
    n = int(rng.integers(1, 8))
    dims = [[int(rng.integers(1, 4)) for _ in range(3)] for _ in range(n)]
    while np.prod([d[0] * d[2] for d in dims]) > DENSE_MAX:
        d = dims[int(rng.integers(0, n))]
        d[0], d[2] = max(1, d[0] - 1), max(1, d[2] - 1)
    ba = [1] + [BONDS[int(rng.integers(0, len(BONDS)))] for _ in range(n - 1)] + [1]
    bb = [1] + [BONDS[int(rng.integers(0, len(BONDS)))] for _ in range(n - 1)] + [1]

    def too_big():
        if bound_of(n, dims, ba, bb) >= 2 ** 53:
            return True
        return any(ba[s] * bb[s] * dims[s][0] * dims[s][2] * ba[s + 1] * bb[s + 1] > SITE_MAX for s in range(n))

    while too_big():  # lower one bond to the next smaller value of the list
        which = ba if rng.integers(0, 2) else bb
        s = int(rng.integers(1, n))
        which[s] = BONDS[max(0, BONDS.index(which[s]) - 1)]
    a = [np.asarray(rng.integers(-1, 2, size=(ba[s], dims[s][0], dims[s][1], ba[s + 1])), dtype=np.float64) for s in range(n)]
    b = [np.asarray(rng.integers(-1, 2, size=(bb[s], dims[s][1], dims[s][2], bb[s + 1])), dtype=np.float64) for s in range(n)]
    return n, dims, ba, bb, a, b


def random_pairs(rng, n_pts, site_dims):
    """(n_pts, len(site_dims), 2) index pairs below the (s1, s2) of every site"""
    out = np.zeros((n_pts, len(site_dims), 2), dtype=np.int64)
    for s, (s1, s2) in enumerate(site_dims):
        out[:, s, 0] = rng.integers(0, s1, size=n_pts)
        out[:, s, 1] = rng.integers(0, s2, size=n_pts)
    return out


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n, dims, ba, bb, a, b = make_operands(rng)
    ctx = f"seed {seed0 + case} n {n} dims {dims} bonds A {ba} B {bb}"
    try:
        bound = cnp.exact_bound(a, b)
        if bound != bound_of(n, dims, ba, bb) or bound >= 2 ** 53:
            fail(ctx, f"the generator left exact_bound at {bound}")
            continue
        for s in range(n):
            la, ra, lb, rb = ba[s], ba[s + 1], bb[s], bb[s + 1]
            for m, k in ((ra, lb), (ra, rb), (la, rb), (la, lb)):
                count("core_products" if m >= 16 and k >= 16 else "scalar_products")
        ma, mb = t4a.MPO(a), t4a.MPO(b)
        c = t4a.Contraction(ma, mb)
        ref = cnp.ContractionNP(a, b, exact=True)
        site_dims = ref.site_dims
        pts = random_pairs(rng, int(rng.integers(1, 301)), site_dims)
        pts[-1] = pts[0]
        bad = mismatch(c.evaluate(pts), ref.evaluate(pts))
        if bad:
            fail(ctx, f"evaluate: {bad}")
        cut = int(rng.integers(0, n + 1))
        bad = mismatch(c.evaluate_left(cut, pts), ref.evaluate_left(cut, pts))
        if bad:
            fail(ctx, f"evaluate_left({cut}): {bad}")
        bad = mismatch(c.evaluate_right(cut, pts), ref.evaluate_right(cut, pts))
        if bad:
            fail(ctx, f"evaluate_right({cut}): {bad}")
        split = None if rng.integers(0, 4) == 0 else int(rng.integers(1, n + 1))
        vals, used = c.evaluate_many(pts, split=split)
        want_split = cnp.find_split(pts) if split is None else split
        if used != want_split:
            fail(ctx, f"evaluate_many used split {used}, expected {want_split}")
        bad = mismatch(vals, ref.evaluate_many(pts, used))
        if bad:
            fail(ctx, f"evaluate_many(split={split}): {bad}")
        mcut = int(rng.integers(0, n + 1))
        rows = random_pairs(rng, int(rng.integers(1, 131)), site_dims[:mcut])
        cols = random_pairs(rng, int(rng.integers(1, 131)), site_dims[mcut:])
        bad = mismatch(c.evaluate_matrix(mcut, rows, cols), ref.evaluate_matrix(mcut, rows, cols))
        if bad:
            fail(ctx, f"evaluate_matrix(cut={mcut}, {len(rows)} x {len(cols)}): {bad}")
        count("matrix_entries", len(rows) * len(cols))
        prod = t4a.contract_naive(ma, mb)
        total = 0
        for s in range(n):
            want = cnp.np_site(ref.a[s], ref.b[s])
            total += want.size
            bad = mismatch(prod.site_tensor(s), want)
            if bad:
                fail(ctx, f"contract_naive site {s}: {bad}")
        count("naive_elements", total)
        if total > 8192 * 256:
            count("naive_second_trip")
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
