"""numpy restatement of swap_site_indices on a chain (tensor4all-treetn, treetn/swap.rs and swap_site_indices in treetn/mod.rs): the
schedule literally, and the driver with numpy's QR and LAPACK SVD and the rank rule of the device code (keep while
s / s_max > threshold, then max_bond_dim, at least 1).  Also the shared cases of tests/test_cpu_swap.py and tests/test_gpu_swap.py.

A leg train here is (cores, legs): cores[i] of shape (l, s, r), legs[i] the ordered list of (key, dim) of site i, first leg fastest
in the fused index s.  A step stores the legs of both its sites in ascending key order.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)

# The dense tolerance of the device tests is C_DENSE * n_steps * eps * |T|_F.  The restatement itself (numpy QR, LAPACK SVD) deviates
# from the exact axis permutation by at most RESTATEMENT_DEVIATION = 8.35 of these units over driver_cases() with seeds 0 .. 19 (3.6 at
# seed 0, the seed the tests use; tests/test_cpu_swap.py asserts it).  A Jacobi SVD and LAPACK's round differently, which is given a
# margin of 8: C_DENSE = 8 * 8.35 -> 67.  Neither number was taken from the device's output.
RESTATEMENT_DEVIATION = 8.35
C_DENSE = 67.0


# ------------------------------------------------------------------------------------------------ schedule
def sweep_edges(root, n):
    """for_each_bond_from(root, n): (a, b) of the Euler tour of a chain from root"""
    out = [(i, i + 1) for i in range(root, n - 1)]
    out += [(i + 1, i) for i in range(n - 2, -1, -1)]
    out += [(i, i + 1) for i in range(0, root)]
    return out


def on_a_side(a, b, target):
    return target <= a if a < b else target >= a


def schedule(n, current, target, root=0, max_passes=None):
    """SwapSchedule::build: a list of (transport_path, node_a, node_b, a_side set, b_side set); ValueError with the reference's text"""
    if not 0 <= root < n:
        raise ValueError(f"SwapSchedule::build: root {root} not in topology")
    for k, node in current.items():
        if not 0 <= node < n:
            raise ValueError(f"SwapSchedule::build: current node {node} for index {k!r} is not in the topology")
    for k, node in target.items():
        if k not in current:
            raise ValueError(f"SwapSchedule::build: target_assignment contains index {k!r} which is not in the network")
        if not 0 <= node < n:
            raise ValueError(f"SwapSchedule::build: target node {node} for index {k!r} is not in the topology")
    max_passes = n - 1 if max_passes is None else max_passes
    position = dict(current)
    center = root
    steps = []

    def done():
        return all(position[k] == v for k, v in target.items())

    for _ in range(max_passes):
        if done():
            break
        moved = False
        for a, b in sweep_edges(root, n):
            a_side, b_side, crossing = set(), set(), False
            for k, node in position.items():
                if node != a and node != b:
                    continue
                if k in target:
                    if on_a_side(a, b, target[k]):
                        a_side.add(k)
                        crossing |= node == b
                    else:
                        b_side.add(k)
                        crossing |= node == a
                elif node == a:
                    a_side.add(k)
                else:
                    b_side.add(k)
            if not crossing:
                continue
            if center in (a, b):
                path = []
            else:
                path = list(range(center, a + 1)) if center < a else list(range(center, a - 1, -1))
            steps.append((path, a, b, a_side, b_side))
            for k in a_side:
                position[k] = a
            for k in b_side:
                position[k] = b
            center = b
            moved = True
        if not moved:
            break
    if not done():
        raise ValueError(f"SwapSchedule::build: did not converge within {max_passes} passes")
    return steps


# ------------------------------------------------------------------------------------------------ dense
def keys_of(legs):
    return [k for site in legs for k, _ in site]


def to_dense(cores, legs):
    """one axis per leg in train order"""
    acc = cores[0].reshape(-1, cores[0].shape[2], order="F")
    for c in cores[1:]:
        acc = (acc @ c.reshape(c.shape[0], -1, order="F")).reshape(-1, c.shape[2], order="F")
    return acc.reshape([d for site in legs for _, d in site], order="F")


def permuted(dense, keys_in, keys_out):
    """the exact answer: the axes of `dense` (in the order keys_in) in the order keys_out"""
    return np.transpose(dense, [keys_in.index(k) for k in keys_out])


# ------------------------------------------------------------------------------------------------ driver
def retained_rank(s, threshold, max_bond_dim):
    smax = float(s.max()) if s.size else 0.0
    keep = 0
    while keep < len(s) and smax > 0.0 and s[keep] / smax > threshold:
        keep += 1
    if max_bond_dim is not None:
        keep = min(keep, max_bond_dim)
    return min(max(keep, 1), len(s))


def _left_step(cores, i):
    c = cores[i]
    l, s, r = c.shape
    q, rr = np.linalg.qr(c.reshape(l * s, r, order="F"))
    k = q.shape[1]
    cores[i] = q.reshape(l, s, k, order="F")
    nx = cores[i + 1]
    cores[i + 1] = (rr @ nx.reshape(nx.shape[0], -1, order="F")).reshape(k, nx.shape[1], nx.shape[2], order="F")


def _right_step(cores, i):
    c = cores[i]
    l, s, r = c.shape
    q, rr = np.linalg.qr(c.reshape(l, s * r, order="F").T)
    k = q.shape[1]
    cores[i] = q.T.reshape(k, s, r, order="F")
    p = cores[i - 1]
    cores[i - 1] = (p.reshape(-1, l, order="F") @ rr.T).reshape(p.shape[0], p.shape[1], k, order="F")


def theta_np(a, b, legs_left, legs_right, to_left, to_right):
    """The step: A[l, x, m], B[m, y, r] -> Theta'[(l, left'), (right', r)] with the legs in ascending key order on both sides.
    Returns (theta, new_left, new_right)."""
    l, m, r = a.shape[0], a.shape[2], b.shape[2]
    merged = list(legs_left) + list(legs_right)
    dims = dict(merged)
    t = np.einsum("lxm,myr->lxyr", a, b).reshape([l] + [d for _, d in merged] + [r], order="F")
    new_left = [(k, dims[k]) for k in sorted(to_left)]
    new_right = [(k, dims[k]) for k in sorted(to_right)]
    keys = [k for k, _ in merged]
    perm = [0] + [1 + keys.index(k) for k, _ in new_left + new_right] + [len(merged) + 1]
    t = np.transpose(t, perm)
    ra = int(np.prod([d for _, d in new_left], dtype=np.int64))
    cb = int(np.prod([d for _, d in new_right], dtype=np.int64))
    return t.reshape(l * ra, cb * r, order="F"), new_left, new_right


def swap(cores, legs, target, rtol=None, max_bond_dim=None):
    """swap_site_indices.  Returns (cores, legs, center, info); info = {"n_steps", "steps", "discarded": [sum of the squared singular
    values a step cut], "margin": the smallest factor by which a kept / cut singular value is away from the threshold (inf when
    nothing was decided by it)}.  center is None when nothing was done."""
    cores = [np.array(c, dtype=np.float64) for c in cores]
    legs = [list(s) for s in legs]
    n = len(cores)
    info = {"n_steps": 0, "steps": [], "discarded": [], "margin": np.inf}
    if not target:
        return cores, legs, None, info
    steps = schedule(n, {k: i for i, site in enumerate(legs) for k, _ in site}, dict(target), 0)
    if not steps:
        return cores, legs, None, info
    for i in range(n - 1, 0, -1):
        _right_step(cores, i)
    threshold = 0.0 if rtol is None else rtol
    center = 0
    for path, a, b, a_side, b_side in steps:
        for frm, to in zip(path[:-1], path[1:]):
            (_left_step if to == frm + 1 else _right_step)(cores, frm)
        right_moving = a < b
        i = min(a, b)
        th, nl, nr = theta_np(cores[i], cores[i + 1], legs[i], legs[i + 1], a_side if right_moving else b_side, b_side if right_moving else a_side)
        u, s, vt = np.linalg.svd(th, full_matrices=False)
        keep = retained_rank(s, threshold, max_bond_dim)
        if threshold > 0.0 and s[0] > 0.0:
            rel = s / s[0]
            by_rule = int(np.sum(rel > threshold))
            if by_rule >= 1:
                info["margin"] = min(info["margin"], rel[by_rule - 1] / threshold)
            if by_rule < len(s):
                info["margin"] = min(info["margin"], threshold / rel[by_rule] if rel[by_rule] > 0.0 else np.inf)
        info["discarded"].append(float(np.sum(s[keep:] ** 2)))
        l, r = cores[i].shape[0], cores[i + 1].shape[2]
        u, s, vt = u[:, :keep], s[:keep], vt[:keep]
        if right_moving:
            left, right = u, s[:, None] * vt
        else:
            left, right = u * s[None, :], vt
        cores[i] = left.reshape(l, -1, keep, order="F")
        cores[i + 1] = right.reshape(keep, -1, r, order="F")
        legs[i], legs[i + 1] = nl, nr
        center = b
    info["n_steps"] = len(steps)
    info["steps"] = steps
    return cores, legs, center, info


# ------------------------------------------------------------------------------------------------ shared cases
def random_train(rng, legs, bonds):
    """gaussian cores for the legs with the given bonds (len(legs) - 1 of them)"""
    b = [1] + list(bonds) + [1]
    return [rng.standard_normal((b[i], int(np.prod([d for _, d in site], dtype=np.int64)), b[i + 1])) for i, site in enumerate(legs)]


def train_legs(dims):
    return [[((i, 0), d)] for i, d in enumerate(dims)]


def mpo_legs(site_dims):
    return [[((i, 0), a), ((i, 1), b)] for i, (a, b) in enumerate(site_dims)]


def quantics_target(n, n_vars, to):
    r = n // n_vars
    if to == "sequential":
        return {(b * n_vars + v, 0): v * r + b for b in range(r) for v in range(n_vars)}
    return {(v * r + b, 0): b * n_vars + v for b in range(r) for v in range(n_vars)}


def driver_cases():
    """name -> (legs, bonds, target, kind): chains of 2 to 6 sites, leg dims 2 and 3, bonds up to 17, at most 4096 dense elements.
    kind: what swap_site_indices returns ("train", "mpo" or "legs")."""
    c = {}
    c["n5_4to0"] = (train_legs([2, 3, 2, 3, 2]), [2, 5, 6, 2], {(4, 0): 0}, "legs")
    c["n5_0to4"] = (train_legs([3, 2, 3, 2, 3]), [3, 6, 5, 3], {(0, 0): 4}, "legs")
    c["n3_exchange"] = (train_legs([3, 2, 3]), [3, 3], {(0, 0): 2, (2, 0): 0}, "train")
    c["quantics_r3"] = (train_legs([2] * 6), [2, 4, 7, 4, 2], quantics_target(6, 2, "sequential"), "train")
    c["reversal_6"] = (train_legs([2, 3, 2, 2, 3, 2]), [2, 5, 8, 5, 2], {(i, 0): 5 - i for i in range(6)}, "train")
    c["mpo_n4"] = (mpo_legs([(2, 3), (3, 2), (2, 3), (3, 2)]), [5, 17, 5], {(i, 1): 3 - i for i in range(4)}, "mpo")
    c["partial_target"] = (mpo_legs([(2, 3), (3, 2), (2, 2), (3, 2)]), [4, 17, 6], {(0, 1): 2}, "legs")
    c["n2"] = (train_legs([3, 2]), [3], {(0, 0): 1, (1, 0): 0}, "train")
    c["empty_site"] = ([[((0, 0), 2), ((0, 1), 3)], [], [((2, 0), 3)], [((3, 0), 2)]], [4, 4, 2], {(0, 1): 1, (3, 0): 2}, "legs")
    return c


def low_rank_train(rng, legs, chi):
    """cores with every bond min(chi, what the legs allow): after a swap the singular values are either of order one or rounding
    zeros, the gap the rank tests need (swap() reports it as info["margin"])"""
    n = len(legs)
    sd = [int(np.prod([d for _, d in site], dtype=np.int64)) for site in legs]
    bonds = []
    for i in range(n - 1):
        bonds.append(min(chi, int(np.prod(sd[:i + 1])), int(np.prod(sd[i + 1:]))))
    return random_train(rng, legs, bonds)
