"""A literal numpy restatement of the partitioned-MPO algebra (tensor4all-partitionedtt: projector.rs, subdomain_tt.rs project /
contract, partitioned_tt.rs contract / add / to_tensor_train) for the project's slice: site tensors are [left, s1, s2, right] numpy
arrays, a projector is a dict {(site, leg): value} with leg 0 = s1 and leg 1 = s2, a partitioned MPO is (projectors, patches) in
insertion order.  The truncation is the project's rank rule: s >= tol * s_max, at most cap, at least one."""
import functools

import numpy as np


# ------------------------------------------------------------------------------------------------ projectors
def compatible(p, q):
    return all(q.get(k, v) == v for k, v in p.items())


def intersection(p, q):
    if not compatible(p, q):
        return None
    out = dict(p)
    out.update(q)
    return out


def common_restriction(p, q):
    return {k: v for k, v in p.items() if q.get(k) == v}


def is_subset_of(p, q):
    return all(p.get(k) == v for k, v in q.items()) and len(p) >= len(q)


def are_disjoint(ps):
    return not any(compatible(ps[i], ps[j]) for i in range(len(ps)) for j in range(i + 1, len(ps)))


def compare(p, q):
    """entries ascending by (site, leg), then value, compared in turn; a proper prefix first"""
    a, b = sorted(p.items()), sorted(q.items())
    for x, y in zip(a, b):
        if x != y:
            return -1 if x < y else 1
    return (len(a) > len(b)) - (len(a) < len(b))


# ------------------------------------------------------------------------------------------------ masking and tasks
def mask(ts, proj):
    """SubDomainTT::project of one patch: zeros outside the subdomain, the values inside untouched"""
    out = [t.copy() for t in ts]
    for (site, leg), v in proj.items():
        keep = np.zeros(out[site].shape[1 + leg], dtype=bool)
        keep[v] = True
        if leg == 0:
            out[site][:, ~keep, :, :] = 0.0
        else:
            out[site][:, :, ~keep, :] = 0.0
    return out


def contraction_tasks(pa, pb):
    """[(i, j, slot)] a-major and the distinct result projectors in order of first appearance"""
    tasks, results = [], []
    for i, p in enumerate(pa):
        for j, q in enumerate(pb):
            if any(leg == 1 and q.get((site, 0), v) != v for (site, leg), v in p.items()):
                continue
            r = {k: v for k, v in p.items() if k[1] == 0}
            r.update({k: v for k, v in q.items() if k[1] == 1})
            if r not in results:
                results.append(r)
            tasks.append((i, j, results.index(r)))
    return tasks, results


# ------------------------------------------------------------------------------------------------ one product
def site_product(a, b):
    """C[(la*Lb+lb), s1, t, (ra*Rb+rb)] = sum_k A[la,s1,k,ra] B[lb,k,t,rb]"""
    la, s1, _, ra = a.shape
    lb, _, t, rb = b.shape
    return np.einsum("askr,bktq->bastqr", a, b).reshape((lb * la, s1, t, rb * ra), order="F")


def factorize(mat, tol, cap):
    u, s, vt = np.linalg.svd(mat, full_matrices=False)
    s_max = s.max() if s.size else 0.0
    rank = 0
    if s_max > 0:
        for v in s:
            if cap is not None and rank >= cap:
                break
            if v < tol * s_max:
                break
            rank += 1
    rank = max(rank, 1)
    return u[:, :rank], s[:rank, None] * vt[:rank], rank


def compress(ts, tol, cap):
    """compress_mpo: right-canonicalise by QR, then the left-to-right SVD sweep"""
    ts = [t.copy() for t in ts]
    if len(ts) <= 1:
        return ts
    for i in range(len(ts) - 1, 0, -1):
        l, s1, s2, r = ts[i].shape
        q, rr = np.linalg.qr(ts[i].reshape((l, s1 * s2 * r), order="F").T)
        ts[i] = q.T.reshape((q.shape[1], s1, s2, r), order="F")
        ts[i - 1] = np.einsum("ausl,lk->ausk", ts[i - 1], rr.T)
    for i in range(len(ts) - 1):
        l, s1, s2, r = ts[i].shape
        left, right, rank = factorize(ts[i].reshape((l * s1 * s2, r), order="F"), tol, cap)
        ts[i] = left.reshape((l, s1, s2, rank), order="F")
        ts[i + 1] = np.einsum("lk,ksqr->lsqr", right, ts[i + 1])
    return ts


def zipup(a, b, tol, cap):
    rem = np.ones((1, 1, 1))
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        c = np.einsum("nbskc,bktd->nstcd", np.einsum("nab,askc->nbskc", rem, x), y)
        n0, s1, t, ca, cb = c.shape
        if i == len(a) - 1:
            out.append(c.reshape((n0, s1, t, 1), order="F"))
            break
        left, right, rank = factorize(c.reshape((n0 * s1 * t, ca * cb), order="F"), tol, cap)
        out.append(left.reshape((n0, s1, t, rank), order="F"))
        rem = right.reshape((rank, ca, cb), order="F")
    return out


def direct_sum(x, y):
    """TensorTrain::add: block-diagonal inner sites, concatenation at the ends, a plain sum for one site"""
    n = len(x)
    if n == 1:
        return [x[0] + y[0]]
    out = []
    for i, (a, b) in enumerate(zip(x, y)):
        first, last = i == 0, i == n - 1
        t = np.zeros((1 if first else a.shape[0] + b.shape[0], a.shape[1], a.shape[2], 1 if last else a.shape[3] + b.shape[3]), dtype=a.dtype)
        t[:a.shape[0], :, :, :a.shape[3]] = a
        t[(0 if first else a.shape[0]):, :, :, (0 if last else a.shape[3]):] = b
        out.append(t)
    return out


def truncates(tol, cap):
    return tol != 0.0 or cap is not None


def add_truncate(x, y, trunc, tol, cap):
    s = direct_sum(x, y)
    return compress(s, tol, cap) if trunc else s


# ------------------------------------------------------------------------------------------------ the partitioned operations
def contract(pa, ta, pb, tb, zip_up=False, do_compress=True, tol=1e-12, cap=None):
    """(result projectors, result patches): every task with both operands masked, equal projectors summed and truncated"""
    tasks, results = contraction_tasks(pa, pb)
    if not are_disjoint(results):  # PartitionedTT::insert (partitioned_tt.rs:196-210) refuses a different overlapping projector
        raise ValueError("Projectors overlap")
    sums = [None] * len(results)
    trunc = (zip_up or do_compress) and truncates(tol, cap)
    for i, j, slot in tasks:
        x, y = mask(ta[i], pa[i]), mask(tb[j], pb[j])
        if zip_up:
            c = zipup(x, y, tol, cap)
        else:
            c = [site_product(u, v) for u, v in zip(x, y)]
            if do_compress:
                c = compress(c, tol, cap)
        sums[slot] = c if sums[slot] is None else add_truncate(sums[slot], c, trunc, tol, cap)
    return results, sums


def project(ps, ts, proj):
    out_p, out_t = [], []
    for p, t in zip(ps, ts):
        m = intersection(p, proj)
        if m is None:
            continue
        out_p.append(m)
        out_t.append(mask(t, m))
    return out_p, out_t


def add(pa, ta, pb, tb, tol=1e-12, cap=None):
    uni = list(pa) + [q for q in pb if q not in pa]
    if not are_disjoint(uni):
        raise ValueError("Incompatible projectors: Projectors must be pairwise disjoint for patch-wise addition")
    out_p, out_t = [], []
    for p, t in zip(pa, ta):
        out_p.append(p)
        out_t.append(add_truncate(t, tb[pb.index(p)], truncates(tol, cap), tol, cap) if p in pb else [x.copy() for x in t])
    for q, t in zip(pb, tb):
        if q not in pa:
            out_p.append(q)
            out_t.append([x.copy() for x in t])
    return out_p, out_t


def to_mpo(ps, ts):
    if not ps:
        raise ValueError("Partitioned tensor train is empty")
    order = sorted(range(len(ps)), key=functools.cmp_to_key(lambda x, y: compare(ps[x], ps[y])))
    acc = ts[order[0]]
    for k in order[1:]:
        acc = direct_sum(acc, ts[k])
    return acc


def norm(ts):
    return float(np.sqrt(sum(float(np.sum(full(t).astype(np.float64) ** 2)) for t in ts)))


def full(ts):
    """dense operator indexed [i1, j1, i2, j2, ...]"""
    acc = ts[0][0]
    for t in ts[1:]:
        acc = np.tensordot(acc, t, axes=([-1], [0]))
    return acc[..., 0]


def full_sum(ts_list, shape=None):
    out = None
    for ts in ts_list:
        f = full(ts)
        out = f if out is None else out + f
    return np.zeros(shape) if out is None else out


def dense_product(fa, fb):
    """C(x, z) = sum_y A(x, y) B(y, z) on dense operators indexed [i1, j1, i2, j2, ...]"""
    n = fa.ndim // 2
    letters = "abcdefghijklmnopqrstuvwxyz"
    x, y, z = letters[:n], letters[n:2 * n], letters[2 * n:3 * n]
    ia = "".join(x[k] + y[k] for k in range(n))
    ib = "".join(y[k] + z[k] for k in range(n))
    ic = "".join(x[k] + z[k] for k in range(n))
    return np.einsum(f"{ia},{ib}->{ic}", fa, fb)


# ------------------------------------------------------------------------------------------------ operands for the tests
SD3 = ([(2, 3), (3, 2), (2, 2)], [(3, 2), (2, 4), (2, 3)])
SD4 = ([(2, 2), (2, 3), (3, 2), (2, 2)], [(2, 3), (3, 2), (2, 2), (2, 3)])


def split_projectors(sda, sdb, ys, xs, zs):
    """A split on its x leg (xs, 0) and, inside x = 1, on the y leg (ys, 1); B split on its z leg (zs, 1) and, inside z = 0, on the same y
    leg (ys, 0).  Every result projector is {(xs, 0): u, (zs, 1): w}: two of them are equal or disjoint.  The pairs cover the contracted
    leg projected by A only, by B only, by both (agreeing: a task; differing: none) and by neither."""
    k, s, t = sda[ys][1], sda[xs][0], sdb[zs][1]
    assert sdb[ys][0] == k
    pa = [{(xs, 0): 0}] + [{(xs, 0): 1, (ys, 1): v} for v in range(k)] + [{(xs, 0): u} for u in range(2, s)]
    pb = [{(zs, 1): 0, (ys, 0): v} for v in range(k)] + [{(zs, 1): w} for w in range(1, t)]
    return pa, pb


def random_bonds(rng, n, lo=1, hi=5):
    return [1] + [int(v) for v in rng.integers(lo, hi + 1, size=n - 1)] + [1]
