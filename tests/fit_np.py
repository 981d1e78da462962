"""numpy restatement of the variational (fit) contraction of two MPOs (t4a_gpu_mpo_contract_fit): the two-site fit of
tensor4all-treetn (treetn/fit.rs) on a chain, with the SVD rank rule of factorize (factorize.rs:126-313) and the zip-up
(contract_zipup.rs:45-167) as initialiser.  random_tensors, np_factorize, np_zipup and np_full are copies of those of
tests/test_gpu_mpo.py.  Site tensors are [left, s1, s2, right]."""
import numpy as np

SEED = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


class Options:
    """FitOptions::default() (contract_fit.rs:36-46)"""

    def __init__(self, tolerance=1e-12, max_bond_dim=100, max_sweeps=10, convergence_tol=1e-10):
        self.tolerance = tolerance
        self.max_bond_dim = max_bond_dim
        self.max_sweeps = max_sweeps
        self.convergence_tol = convergence_tol


def random_tensors(bonds, s1, s2, seed):
    """random_mpo (test_support.rs:8-44): an LCG fills every site tensor column-major."""
    state = seed
    out = []
    for left, right in zip(bonds[:-1], bonds[1:]):
        vals = []
        for _ in range(left * s1 * s2 * right):
            state = (state * 6364136223846793005 + 1442695040888963407) & MASK
            vals.append((state >> 33) / float(1 << 31) - 0.5)
        out.append(np.array(vals).reshape((left, s1, s2, right), order="F"))
    return out


def np_factorize(mat, tol, max_bond_dim):
    u, s, vt = np.linalg.svd(mat, full_matrices=False)
    s_max = s.max() if s.size else 0.0
    rank = 0
    if s_max > 0:
        for v in s:
            if max_bond_dim is not None and rank >= max_bond_dim:
                break
            if v < tol * s_max:
                break
            rank += 1
    rank = max(rank, 1)
    return u[:, :rank], s[:rank], vt[:rank], rank


def np_zipup(a, b, options):
    rem = np.ones((1, 1, 1))
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        c = np.einsum("nbskc,bktd->nstcd", np.einsum("nab,askc->nbskc", rem, x), y)
        n0, s1, t, ca, cb = c.shape
        if i == len(a) - 1:
            out.append(c.reshape((n0, s1, t, 1), order="F"))
            break
        u, s, vt, rank = np_factorize(c.reshape((n0 * s1 * t, ca * cb), order="F"), options.tolerance, options.max_bond_dim)
        out.append(u.reshape((n0, s1, t, rank), order="F"))
        rem = (s[:, None] * vt).reshape((rank, ca, cb), order="F")
    return out


def np_full(ts):
    """dense operator indexed [i1, j1, i2, j2, ...]"""
    acc = ts[0][0]
    for t in ts[1:]:
        acc = np.tensordot(acc, t, axes=([-1], [0]))
    return acc[..., 0]


def np_product(a, b):
    """dense A·B indexed [i1, j1, i2, j2, ...] from the exact site-wise product"""
    ts = []
    for x, y in zip(a, b):
        la, s1, _, ra = x.shape
        lb, _, t, rb = y.shape
        ts.append(np.einsum("askr,bktq->bastqr", x, y).reshape((lb * la, s1, t, rb * ra), order="F"))
    return np_full(ts)


def links(ts):
    return [t.shape[0] for t in ts[1:]]


def rel_error(got, want):
    return float(np.linalg.norm(np.asarray(got) - want) / np.linalg.norm(want))


def np_half_left(env, x, y):
    """P[n, s, t, c, d] = sum_{a, b, k} L[n, a, b] A[a, s, k, c] B[b, k, t, d]"""
    return np.einsum("nab,askc,bktd->nstcd", env, x, y)


def np_half_right(env, x, y):
    """Q[a, b, s, t, n] = sum_{c, d, k} A[a, s, k, c] B[b, k, t, d] R[c, d, n]"""
    return np.einsum("askc,bktd,cdn->abstn", x, y, env)


def np_right_canonicalize(ts):
    ts = list(ts)
    for i in range(len(ts) - 1, 0, -1):
        l, s1, s2, r = ts[i].shape
        q, rr = np.linalg.qr(ts[i].reshape((l, s1 * s2 * r), order="F").T)
        k = q.shape[1]
        ts[i] = q.T.reshape((k, s1, s2, r), order="F")
        ts[i - 1] = np.einsum("ausl,lk->ausk", ts[i - 1], rr.T)
    return ts


def np_fit(a, b, options=None, initial=None):
    """-> (site tensors, {"n_sweeps", "norms"})"""
    o = Options() if options is None else options
    n = len(a)
    info = {"n_sweeps": 0, "norms": []}
    if n == 0:
        return [], info
    if n == 1:
        return [np.einsum("askc,bktd->abstcd", a[0], b[0]).reshape((1, a[0].shape[1], b[0].shape[2], 1))], info
    c = [t.copy() for t in initial] if initial is not None else np_zipup(a, b, o)
    if o.max_sweeps == 0:
        return c, info
    c = np_right_canonicalize(c)
    left = [None] * n
    right = [None] * (n + 1)
    left[0] = np.ones((1, 1, 1))
    right[n] = np.ones((1, 1, 1))
    for i in range(n - 1, 1, -1):
        right[i] = np.einsum("abstn,cstn->abc", np_half_right(right[i + 1], a[i], b[i]), c[i])
    norms = [float(np.linalg.norm(c[0]))]

    def bond_step(i, move_right):
        p = np_half_left(left[i], a[i], b[i])
        q = np_half_right(right[i + 2], a[i + 1], b[i + 1])
        ci, s, t = p.shape[:3]
        s2, t2, cn = q.shape[2:]
        ab = p.shape[3] * p.shape[4]
        pm = p.reshape((ci * s * t, ab), order="F")
        qm = q.reshape((ab, s2 * t2 * cn), order="F")
        u, sv, vt, rank = np_factorize(pm @ qm, o.tolerance, o.max_bond_dim)
        if move_right:
            c[i] = u.reshape((ci, s, t, rank), order="F")
            c[i + 1] = (sv[:, None] * vt).reshape((rank, s2, t2, cn), order="F")
            left[i + 1] = (u.T @ pm).reshape((rank,) + p.shape[3:], order="F")
        else:
            c[i] = (u * sv[None, :]).reshape((ci, s, t, rank), order="F")
            c[i + 1] = vt.reshape((rank, s2, t2, cn), order="F")
            right[i + 1] = (qm @ vt.T).reshape(q.shape[:2] + (rank,), order="F")
        return float(np.linalg.norm(sv))

    for sweep in range(1, o.max_sweeps + 1):
        nrm = 0.0
        for i in range(n - 1):
            nrm = bond_step(i, True)
        for i in range(n - 2, -1, -1):
            nrm = bond_step(i, False)
        norms.append(nrm)
        info["n_sweeps"] = sweep
        with np.errstate(divide="ignore", invalid="ignore"):
            converged = abs(np.float64(nrm) / np.float64(norms[-2]) - 1.0) < o.convergence_tol
        if converged:
            break
    info["norms"] = norms
    return c, info
