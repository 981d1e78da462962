"""Seeded items for the tests of compress_many (tests/test_cpu_compress_many.py, tests/test_gpu_compress_many.py, the soak) with a
prescribed singular spectrum at every cut, and the report that checks it.  The restatement is tests/pmpo_np.py: ``compress`` is the
right QR sweep and the left SVD sweep, ``factorize`` the rank rule, ``full`` the dense operator.

An item is a sum of R <= 4 product operators  T = sum_a c_a  O_0^(a) x O_1^(a) x ... x O_{n-1}^(a)  with c = COEFFS[:R].  At site i
the factors are columns of one random orthogonal matrix of the fused site index, O_i^(a) = Q_i[:, a mod s_i]: two factors of a site
are equal or orthogonal, so at a cut the left parts (and the right parts) of two terms are equal or orthogonal, and the cut matrix is,
in orthonormal bases, the matrix C[class left, class right] = sum of the c_a of that pair of classes.  Terms 0 and 1 share a class on
one side only when that side has a single class (then the cut has exact rank 1), so every singular value of a cut is within 3e-4 of
1 or 0.5 (up to the factor sqrt(1.25) when both sit in one row), or at most 3e-4, or exactly zero: tolerance 1e-8 keeps the former
two kinds and drops only exact zeros, a cap of 2 cuts between 0.5 and 3e-4.  The MPO carries these terms on bonds D_i >= R rotated by
random orthogonal gauges, so the site tensors are dense and the bonds above R hold exact rank deficiency.  ``same_first`` makes all
factors of site 0 equal: the first cut then has rank 1 although its matrix has R columns — the tolerance binds there.
"""
import functools

import numpy as np

from pmpo_np import compress, factorize, full

BMAX = 64
COEFFS = (1.0, -0.5, 2e-4, -1e-4)
GAP = 1e3


def _orth(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def make_item(seed, site_dims, bonds, terms=4, scale=None, same_first=False, zero=False, coeffs=COEFFS):
    """site tensors [l, s1, s2, r] with bonds [1, D_1, .., D_{n-1}, 1]; ``scale = (site, factor)`` multiplies one site; ``coeffs``: the
    coefficients of the terms"""
    n = len(site_dims)
    assert len(bonds) == n + 1 and bonds[0] == 1 and bonds[-1] == 1
    rng = np.random.default_rng(seed)
    R = max(1, min([terms, len(coeffs)] + list(bonds[1:-1])))
    c = np.array(coeffs[:R])
    sites = []
    gauges = [np.ones((1, 1))] + [_orth(rng, d) for d in bonds[1:-1]] + [np.ones((1, 1))]
    for i, (s1, s2) in enumerate(site_dims):
        s = s1 * s2
        q = _orth(rng, s)
        core = np.zeros((R if i > 0 else 1, s, R if i < n - 1 else 1))
        for a in range(R):
            f = q[:, 0 if (same_first and i == 0) else a % s] * (c[a] if i == 0 else 1.0)
            core[a if i > 0 else 0, :, a if i < n - 1 else 0] += f
        gl = gauges[i][:core.shape[0], :] if i > 0 else gauges[i]
        gr = gauges[i + 1][:core.shape[2], :] if i < n - 1 else gauges[i + 1]
        t = np.einsum("ax,asb,by->xsy", gl, core, gr)
        if scale is not None and scale[0] == i:
            t = t * scale[1]
        if zero:
            t = np.zeros_like(t)
        sites.append(np.ascontiguousarray(t.reshape((t.shape[0], s1, s2, t.shape[2]), order="F")))
    return sites


def shapes_of(item):
    return [tuple(int(x) for x in t.shape) for t in item]


def qr_bonds(shapes):
    """the bonds after the right sweep: k_n = 1, k_i = min(l_i, s_i k_{i+1})"""
    n = len(shapes)
    k = [1] * (n + 1)
    for i in range(n - 1, 0, -1):
        k[i] = min(shapes[i][0], shapes[i][1] * shapes[i][2] * k[i + 1])
    return k


def bound_bonds(shapes, cap):
    k = qr_bonds(shapes)
    b = [1] * (len(shapes) + 1)
    for i in range(len(shapes) - 1):
        b[i + 1] = min(k[i + 1], b[i] * shapes[i][1] * shapes[i][2])
        if cap is not None:
            b[i + 1] = min(b[i + 1], cap)
    return b


def inside(shapes):
    return len(shapes) >= 2 and max(qr_bonds(shapes)[1:-1]) <= BMAX


def cut_report(item, tol, cap):
    """The left sweep of ``compress`` cut by cut: a list of dicts {rows, cols, rank, by_cap, s_max, kept_min, dropped_max, cutoff} —
    the values relative to nothing, the cutoff tol * s_max; dropped_max is 0.0 where nothing is dropped."""
    ts = [t.copy() for t in item]
    out = []
    if len(ts) <= 1:
        return out
    for i in range(len(ts) - 1, 0, -1):
        l, s1, s2, r = ts[i].shape
        q, rr = np.linalg.qr(ts[i].reshape((l, s1 * s2 * r), order="F").T)
        ts[i] = q.T.reshape((q.shape[1], s1, s2, r), order="F")
        ts[i - 1] = np.einsum("ausl,lk->ausk", ts[i - 1], rr.T)
    for i in range(len(ts) - 1):
        l, s1, s2, r = ts[i].shape
        mat = ts[i].reshape((l * s1 * s2, r), order="F")
        s = np.linalg.svd(mat, compute_uv=False)
        left, right, rank = factorize(mat, tol, cap)
        s_max = float(s.max())
        out.append({"rows": l * s1 * s2, "cols": r, "rank": rank, "by_cap": cap is not None and rank == cap and rank < len(s),
                    "s_max": s_max, "kept_min": float(s[rank - 1]), "dropped_max": float(s[rank]) if rank < len(s) else 0.0,
                    "cutoff": tol * s_max})
        ts[i] = left.reshape((l, s1, s2, rank), order="F")
        ts[i + 1] = np.einsum("lk,ksqr->lsqr", right, ts[i + 1])
    return out


def gap_ok(cut):
    """kept >= 1e3 * cutoff and dropped <= 1e-3 * cutoff, or a cut made by the cap between values a factor >= 1e3 apart"""
    by_tolerance = cut["kept_min"] >= GAP * cut["cutoff"] and cut["dropped_max"] <= cut["cutoff"] / GAP
    by_cap = cut["by_cap"] and cut["kept_min"] >= GAP * cut["dropped_max"]
    return by_tolerance or by_cap


def orientations(item, tol, cap):
    return ["tall" if c["rows"] > c["cols"] else "square" if c["rows"] == c["cols"] else "wide" for c in cut_report(item, tol, cap)]


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
OPTIONS = [(1e-8, None), (1e-8, 2)]
A, B, C, D, E8, E9 = (1, 1), (2, 2), (2, 3), (3, 1), (8, 8), (8, 9)

# name -> (site dims, bonds, keyword arguments of make_item) per number of sites
KINDS = {
    2: {
        "tall": ([C, B], [1, 3, 1], {}),
        "square": ([B, B], [1, 5, 1], {}),       # the QR bounds the bond by 4: a 4 x 4 step
        "wide": ([D, C], [1, 5, 1], {}),
        "bond1": ([B, C], [1, 1, 1], {}),
        "zero": ([C, B], [1, 3, 1], {"zero": True}),
        "rank1": ([C, C], [1, 5, 1], {"terms": 1}),
        "tol_and_cap": ([B, C], [1, 5, 1], {}),  # one bond only: the cap binds there, the tolerance drops the exact zeros without a cap
        "bmax": ([E8, E8], [1, 64, 1], {}),
        "bmax_plus_1": ([E9, E9], [1, 65, 1], {}),
        "big": ([C, B], [1, 3, 1], {"scale": (0, 1e120)}),
        "small": ([B, C], [1, 2, 1], {"scale": (1, 1e-120)}),
    },
    3: {
        "tall": ([C, B, D], [1, 3, 2, 1], {}),
        "square": ([C, D, B], [1, 8, 2, 1], {}),  # the QR bounds the first bond by 3 * 2: a 6 x 6 step
        "wide": ([D, C, B], [1, 17, 3, 1], {}),
        "bond1": ([B, A, C], [1, 1, 1, 1], {}),
        "zero": ([C, B, D], [1, 8, 3, 1], {"zero": True}),
        "rank1": ([C, D, C], [1, 5, 15, 1], {"terms": 1}),
        "tol_and_cap": ([B, C, B], [1, 8, 5, 1], {"same_first": True}),
        "bmax": ([E8, B, E8], [1, 64, 33, 1], {}),
        "bmax_plus_1": ([E9, B, E9], [1, 65, 33, 1], {}),
        "big": ([C, B, C], [1, 5, 3, 1], {"scale": (1, 1e120)}),
        "small": ([B, C, D], [1, 3, 2, 1], {"scale": (2, 1e-120)}),
    },
    5: {
        "tall": ([C, B, A, D, B], [1, 2, 8, 5, 3, 1], {}),
        "square": ([C, D, B, C, B], [1, 8, 2, 5, 3, 1], {}),  # as at three sites: a 6 x 6 first step
        "wide": ([D, C, B, C, B], [1, 17, 33, 16, 3, 1], {}),
        "bond1": ([B, A, C, D, B], [1, 1, 1, 1, 1, 1], {}),
        "zero": ([C, B, D, A, C], [1, 8, 3, 2, 2, 1], {"zero": True}),
        "rank1": ([C, D, C, B, B], [1, 5, 15, 8, 3, 1], {"terms": 1}),
        "tol_and_cap": ([B, C, B, D, C], [1, 8, 5, 17, 5, 1], {"same_first": True}),
        "bmax": ([C, C, C, C, C], [1, 5, 64, 33, 5, 1], {}),
        "bmax_plus_1": ([C, C, C, C, C], [1, 5, 65, 33, 5, 1], {}),
        "big": ([C, B, C, D, B], [1, 5, 3, 2, 2, 1], {"scale": (3, 1e120)}),
        "small": ([B, C, D, C, B], [1, 3, 2, 3, 3, 1], {"scale": (0, 1e-120)}),
    },
}
KIND_ORDER = ["tall", "square", "wide", "bond1", "zero", "rank1", "tol_and_cap", "bmax", "bmax_plus_1", "big", "small"]
LENGTHS = (2, 3, 5)
SIZES = (1, 3, 11, 300)


def kind_of(k):
    return KIND_ORDER[k % len(KIND_ORDER)]


@functools.lru_cache(maxsize=None)
def batch(n, size):
    """``size`` items of ``n`` sites: item k is of kind KIND_ORDER[k % 11] with seed 1000 n + k, so a batch of 300 holds every kind 27
    times with different values and a batch of 11 every kind once; the batches of 1 and 3 are the kinds (wide,) and (tall, square, wide)."""
    picks = {1: ["wide"], 3: ["tall", "square", "wide"]}.get(size)
    names = picks if picks is not None else [kind_of(k) for k in range(size)]
    items = []
    for k, name in enumerate(names):
        sd, bonds, kw = KINDS[n][name]
        items.append(make_item(1000 * n + (KIND_ORDER.index(name) if picks is not None else k), sd, bonds, **kw))
    return names, items


@functools.lru_cache(maxsize=None)
def reference(n, size, tol, cap):
    """per item of batch(n, size): (restatement site tensors, exact dense operator, restatement error against it)"""
    out = []
    for item in batch(n, size)[1]:
        want = compress(item, tol, cap)
        dense = full(item)
        out.append((want, dense, float(np.abs(full(want) - dense).max())))
    return out


# ------------------------------------------------------------------------------------------------ the partitioned cases
# Site dims (pmpo_np.SD3 / SD4), projector splits (pmpo_np.split_projectors), partitions and options are those of tests/test_gpu_pmpo.py;
# the VALUES are designed, because a product of random patches has no gap where a cap falls.  Every patch of A is ONE product operator
# (bonds 2 - 3, rotated), every patch of B a sum of four (bonds 4 - 5) with the coefficients PMPO_COEFFS[cap]: a task product is then a
# sum of four product operators whose factors the projection and the matrix product with A's factor leave generic, so its singular
# values at a cut are the coefficients times geometry factors of order 1e-2 .. 1.  Without a cap and with a cap of 4 all four are large:
# the tolerance drops exact zeros only and a cap of 4 cuts against exact zeros.  With a cap of 3 the fourth coefficient is 1e-6: the cap
# cuts between a value of order 1e-2 .. 1 and one of order 1e-8 .. 1e-6 (observed ratio at least 1.9e3), which tolerance 1e-12 alone
# would have kept.  PMPO_SEED was picked on the CPU so that every cut of every task meets gap_ok (tests/test_cpu_compress_many.py).
PMPO_CASES = [(3, 0, 1, 2), (3, 1, 0, 0), (4, 3, 1, 1), (4, 2, 0, 3)]
PMPO_OPTIONS = [(1e-12, None), (1e-12, 3), (1e-8, 4)]
PMPO_COEFFS = {None: (1.0, -0.8, 0.6, -0.5), 3: (1.0, -0.8, 0.6, 1e-6), 4: (1.0, -0.8, 0.6, -0.5)}
PMPO_SEED = 0


def pmpo_operands(n, ys, xs, zs, cap, seed=PMPO_SEED):
    import pmpo_np as P
    sda, sdb = P.SD3 if n == 3 else P.SD4
    pa, pb = P.split_projectors(sda, sdb, ys, xs, zs)
    rng = np.random.default_rng(seed)
    ta = [make_item(int(rng.integers(0, 2**31)), list(sda), P.random_bonds(rng, n, 2, 3), terms=1) for _ in pa]
    tb = [make_item(int(rng.integers(0, 2**31)), list(sdb), P.random_bonds(rng, n, 4, 5), terms=4, coeffs=PMPO_COEFFS[cap]) for _ in pb]
    return sda, sdb, pa, ta, pb, tb


def pmpo_task_products(n, ys, xs, zs, cap):
    """the exact site products of every task of a case, as the compress stage receives them"""
    import pmpo_np as P
    sda, sdb, pa, ta, pb, tb = pmpo_operands(n, ys, xs, zs, cap)
    tasks, _ = P.contraction_tasks(pa, pb)
    return [[P.site_product(u, v) for u, v in zip(P.mask(ta[i], pa[i]), P.mask(tb[j], pb[j]))] for i, j, _ in tasks]
