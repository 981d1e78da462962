"""The cases of tests/test_gpu_patching_exact.py and tests/test_gpu_patching.py, built once and checked on the CPU by
tests/test_cpu_patching.py.  No device, no library.

EXACT ITEMS.  A chain of 2 or 3 sites whose tensor is F = sum_j (+-2^-k_j) e_x(j) (x) e_y(j) (x) e_z(j) with x and z injective: every
core is a signed partial permutation, the first one times diag(2^-k_j); term j runs over bond index j of every bond, and the bonds may
be wider than the number of terms (zero columns).  At every bond the singular values are exactly the 2^-k_j of the terms that survived
the truncations before it; exponents come in groups of three equal ones from 0 to 21, so every sum of squares is a multiple of 2^-42
below 2^7 and exact in any order.  ``model`` follows the surviving terms through the 2 (n - 1) truncations."""
import numpy as np

import patching_np as R

POLICIES = [(scale, measure, rule) for scale in (0, 1) for measure in (0, 1) for rule in (0, 1)]


def exponents(count):
    return [j // 3 for j in range(count)]


def exact_item(site_dims, bonds, n_terms, seed):
    """site tensors (l, s1, s2, r) of the chain with bonds [1, b1, (b2,) 1] and n_terms <= min(fused dims of the end sites, bonds)"""
    rng = np.random.default_rng(seed)
    n = len(site_dims)
    fused = [a * b for a, b in site_dims]
    assert n in (2, 3) and n_terms <= min(fused[0], fused[-1], *bonds[1:-1])
    ks = exponents(n_terms)
    cores = [np.zeros((bonds[i], fused[i], bonds[i + 1])) for i in range(n)]
    x = rng.permutation(fused[0])[:n_terms]
    z = rng.permutation(fused[-1])[:n_terms]
    order = rng.permutation(n_terms)  # which bond index carries which exponent: the values arrive unsorted
    for j in range(n_terms):
        cores[0][0, x[j], j] = rng.choice([-1.0, 1.0]) * 2.0 ** -ks[order[j]]
        if n == 3:
            cores[1][j, rng.integers(fused[1]), j] = rng.choice([-1.0, 1.0])
        cores[-1][j, z[j], 0] = rng.choice([-1.0, 1.0])
    return [R.unfuse(c, sd) for c, sd in zip(cores, site_dims)], sorted((2.0 ** -k for k in ks), reverse=True)


def model(values, n, policy, cap):
    """(norm2, [(singular values before the cut, rank, margin)] for the 2 (n - 1) truncations) of an exact item with the given terms"""
    alive = list(values)
    steps = []
    for _ in range(2 * (n - 1)):
        s = np.array(alive if alive else [0.0])
        keep = R.svd_retained_rank(s, policy)
        if cap is not None:
            keep = min(keep, cap)
        keep = max(min(keep, len(s)), 1)
        steps.append((s, keep, R.margin(s, policy)))
        alive = alive[:keep]
    return float(sum(v * v for v in values)), steps


def threshold_between(values, scale_measure_rule, cut):
    """the threshold halfway, on a log scale, between the two quantities the rule compares around keeping `cut` values"""
    scale, measure, rule = scale_measure_rule
    m = np.array(values) if measure == 0 else np.array(values) ** 2
    if rule == 0:
        x = m / m.max() if scale == 0 else m
        lo, hi = x[cut], x[cut - 1]  # kept while x > thr
    else:
        tails = np.cumsum(m[::-1])[::-1]  # tails[i] = sum m[i:]
        x = tails / m.sum() if scale == 0 else tails
        lo, hi = x[cut], x[cut - 1]  # discarded while tail <= thr: tail[cut] <= thr < tail[cut - 1]
    assert 0.0 < lo < hi
    return float(np.sqrt(lo * hi))


E8, E9, T2, T3, M23 = (8, 8), (9, 9), (2, 1), (3, 1), (2, 3)

# (name, site dims, bonds, terms, cut, cap): `cut` = values the threshold keeps at the first truncation (a group boundary: a multiple of
# 3 or all), cap = None or a cap (a group boundary too).  Bonds 1, 2, 15, 16, 17, 33, 64 and, on the serial stage, 65.
EXACT_2 = [
    ("bond1", [T2, T3], [1, 1, 1], 1, 1, None),
    ("bond2_dims23", [T2, T3], [1, 2, 1], 2, 2, None),
    ("wide_qr", [T3, E8], [1, 5, 1], 3, 3, None),
    ("bond15", [E8, E8], [1, 15, 1], 15, 9, None),
    ("bond16", [E8, E8], [1, 16, 1], 16, 12, 6),
    ("bond17", [E8, E8], [1, 17, 1], 17, 6, None),
    ("bond33", [E8, E8], [1, 33, 1], 33, 30, 21),
    ("bond64_square", [E8, E8], [1, 64, 1], 64, 48, None),
    ("bond65_serial", [E9, E9], [1, 65, 1], 65, 33, None),
    ("zero", [E8, E8], [1, 16, 1], 0, 0, None),
]
EXACT_3 = [
    ("bond1", [T2, T3, T2], [1, 1, 1, 1], 1, 1, None),
    ("dims23", [T3, M23, T3], [1, 3, 3, 1], 3, 3, None),
    ("wide_step", [E8, T2, E8], [1, 16, 16, 1], 16, 12, 3),
    ("bond17_33", [E8, M23, E8], [1, 17, 33, 1], 17, 15, None),
    ("bond64", [E8, E8, E8], [1, 64, 64, 1], 64, 63, 60),
    ("bond65_serial", [E9, T2, E9], [1, 65, 65, 1], 65, 33, None),
    ("zero", [E8, T3, E8], [1, 4, 4, 1], 0, 0, None),
]


def exact_batch(n, smr):
    """[(name, tensors, values, policy, cap)] for the policy combination smr = (scale, measure, rule)"""
    out = []
    for k, (name, sd, bonds, terms, cut, cap) in enumerate(EXACT_2 if n == 2 else EXACT_3):
        tensors, values = exact_item(sd, bonds, terms, 100 * n + k)
        thr = threshold_between(values, smr, cut) if 0 < cut < terms else 0.0  # (0 keeps every value under every rule)
        out.append((name, tensors, values, (thr,) + tuple(smr), cap))
    return out


# ---------------------------------------------------------------------------------------------- random partitioned operands
def random_chain(rng, site_dims, bonds, decay=1.0):
    return [rng.standard_normal((bonds[i], sd[0], sd[1], bonds[i + 1])) * decay for i, sd in enumerate(site_dims)]


def low_rank_plus(rng, site_dims, bonds, ranks, eps):
    """a chain of bonds `bonds` whose dense tensor is a chain of bonds `ranks` plus eps times a full-bond perturbation"""
    a = random_chain(rng, site_dims, ranks)
    b = random_chain(rng, site_dims, [x - y if 0 < i < len(bonds) - 1 else 1 for i, (x, y) in enumerate(zip(bonds, ranks))])
    out = []
    n = len(site_dims)
    for i in range(n):
        x, y = a[i], b[i] * (eps if i == 0 else 1.0)
        l = 1 if i == 0 else x.shape[0] + y.shape[0]
        r = 1 if i == n - 1 else x.shape[3] + y.shape[3]
        t = np.zeros((l, x.shape[1], x.shape[2], r))
        if i == 0:
            t[:, :, :, :x.shape[3]], t[:, :, :, x.shape[3]:] = x, y
        elif i == n - 1:
            t[:x.shape[0]], t[x.shape[0]:] = x, y
        else:
            t[:x.shape[0], :, :, :x.shape[3]], t[x.shape[0]:, :, :, x.shape[3]:] = x, y
        out.append(t)
    return out


def halves(site_dims, leg):
    """the projectors that fix `leg` to each of its values"""
    return [{leg: v} for v in range(site_dims[leg[0]][leg[1]])]


# (name, site dims, input bonds, underlying ranks, eps, partition leg, scales per patch, rtol, cap, seed)
ADAPTIVE = [
    ("train3", [T2, T3, T2], [1, 2, 2, 1], [1, 1, 1, 1], 1e-3, (0, 0), [1.0, 1.0], 1e-2, None, 3),
    ("train5_drop", [T2, T3, T2, T3, T2], [1, 2, 6, 6, 2, 1], [1, 1, 2, 2, 1, 1], 1e-4, (2, 0), [1.0, 1e-7], 1e-3, None, 5),
    ("mpo4_cap", [M23, (2, 2), (3, 2), M23], [1, 6, 17, 6, 1], [1, 2, 3, 2, 1], 1e-5, (1, 1), [1.0, 0.5], 1e-4, 2, 7),
    ("train6_bond17", [T3, T3, T3, T3, T3, T3], [1, 3, 9, 17, 9, 3, 1], [1, 2, 3, 4, 3, 2, 1], 1e-6, (5, 0), [1.0, 2.0, 1e-3], 1e-5, 3, 11),
]


def adaptive_case(name):
    """(site dims, patches, projectors, rtol, cap)"""
    for nm, sd, bonds, ranks, eps, leg, scales, rtol, cap, seed in ADAPTIVE:
        if nm == name:
            rng = np.random.default_rng(seed)
            projs = halves(sd, leg)[:len(scales)]
            patches = []
            for s in scales:
                t = low_rank_plus(rng, sd, bonds, ranks, eps)
                t[0] = t[0] * s
                patches.append(t)
            return sd, patches, projs, rtol, cap
    raise KeyError(name)


# add_with_patching: (name, site dims, bonds, seed, rtol, cap, patch_order)
SPLIT = [
    ("train4", [T2, T3, T2, T2], [1, 2, 6, 2, 1], 1, 1e-6, 2, ()),
    ("mpo3", [(2, 2), M23, (2, 2)], [1, 4, 4, 1], 2, 1e-8, 2, ()),
    ("train4_order", [T2, T3, T2, T2], [1, 2, 6, 2, 1], 3, 1e-6, 2, ((2, 0), (1, 0), (0, 0), (3, 0))),
]


def split_case(name):
    """(site dims, tensors, rtol, cap, patch_order)"""
    for nm, sd, bonds, seed, rtol, cap, order in SPLIT:
        if nm == name:
            return sd, random_chain(np.random.default_rng(seed), sd, bonds), rtol, cap, list(order)
    raise KeyError(name)


def doc_add_example():
    """the doc example of add_with_patching (patching.rs:123-152): one patch of bond 3 over two binary sites, entries 1 .. 6"""
    t0 = np.arange(1.0, 7.0).reshape((2, 3), order="C").reshape((1, 2, 1, 3))  # from_dense is row-major over [s0, bond]
    t1 = np.arange(1.0, 7.0).reshape((3, 2), order="C").reshape((3, 2, 1, 1))
    return [T2, T2], [t0, t1]


def doc_truncate_example():
    """the doc example of truncate_adaptive (:533-565): two rank-one patches scaled 10 and 0.01 on the two values of s0"""
    def rank_one(scale):
        return [np.full((1, 2, 1, 1), scale), np.ones((1, 2, 1, 1))]
    return [T2, T2], [rank_one(10.0), rank_one(0.01)], [{(0, 0): 0}, {(0, 0): 1}]


def doc_contract_example():
    """the doc example of contract_adaptive (:231-281): two all-ones trains of bond 3 over the same three binary indices, so the product
    sums over every site index.  Here A has site dims (1, 2), B (2, 1): the result's legs have dimension 1, and the leg (0, 0) named in
    the order — s0 there — splits into one child."""
    bonds = [1, 3, 3, 1]
    a = [np.ones((bonds[i], 1, 2, bonds[i + 1])) for i in range(3)]
    b = [np.ones((bonds[i], 2, 1, bonds[i + 1])) for i in range(3)]
    return [(1, 2)] * 3, [(2, 1)] * 3, a, b


def conditioned_chain(rng, leg_first):
    """three sites of dims (2, 2), bond 2, block-diagonal in the bond: fixed to a value of its first site's leg `leg_first` (0: s1, 1: s2)
    the chain has rank 1"""
    u = rng.uniform(0.5, 1.5, size=(2, 2))
    t0 = np.zeros((1, 2, 2, 2))
    for v in range(2):
        if leg_first == 0:
            t0[0, v, :, v] = u[:, v]
        else:
            t0[0, :, v, v] = u[:, v]
    t1 = np.zeros((2, 2, 2, 2))
    t2 = np.zeros((2, 2, 2, 1))
    for v in range(2):
        t1[v, :, :, v] = rng.uniform(0.5, 1.5, size=(2, 2))
        t2[v, :, :, 0] = rng.uniform(0.5, 1.5, size=(2, 2))
    return [t0, t1, t2]


def saturating_product(seed=0):
    """A rank 1 given its x0, B rank 1 given its z0: the product has bond 4 >= the cap 2, the group splits along (0, 0), its children
    (bond 2, still at the cap) along (0, 1), and the four grandchildren have bond 1.  (site dims of A, of B, A, B, rtol, cap, order)"""
    rng = np.random.default_rng(seed)
    return [(2, 2)] * 3, [(2, 2)] * 3, conditioned_chain(rng, 0), conditioned_chain(rng, 1), 1e-8, 2, [(0, 0), (0, 1)]


def error_bound(n, rtol, norm):
    """|F - F~| <= 2 (n - 1) rtol |F| + 1e-13 |F|: each of the 2 (n - 1) truncations of a patch discards at most its budget in squared
    Frobenius norm on a canonical chain, the errors add by the triangle inequality, a dropped patch costs at most its budget, and the
    patches are disjoint, so their squared errors add to at most (2 (n - 1))^2 rtol^2 |F|^2"""
    return (2 * (n - 1) * rtol + 1e-13) * norm
