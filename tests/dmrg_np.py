"""numpy restatement of two-site DMRG (t4a_gpu_dmrg): the sweeps of tensor4all-treetn's dmrg (dmrg/mod.rs) on a chain with the
Hermitian Lanczos of tensor4all-core (krylov.rs:517-634) — two passes of MODIFIED Gram-Schmidt as the reference runs them, the
projected matrix from the full upper-Hessenberg columns, the Hermitian check per entry pair, the lowest eigenpair by numpy's eigh —,
and the cases the CPU and the device tests share.  Operator sites are [w_l, s1, s2, w_r], state sites [l, s, r].  The projected
operator, the canonicalisation, the sweep plan and the truncation rule are those of tests/linsolve_np.py."""
import numpy as np

from fit_np import SEED, random_tensors
from linsolve_np import (np_canonicalize, np_left_env, np_right_env, np_projected_apply_steps as np_projected_apply, np_truncated_svd, np_operator_full, np_state_full,  # noqa: F401
                         sweep_plan, lcg_matrix)


class LanczosOptions:
    """HermitianLanczosOptions::default()"""

    def __init__(self, max_iter=64, rtol=1e-10, atol=0.0, breakdown_tol=1e-14, hermitian_tol=1e-10):
        self.max_iter = max_iter
        self.rtol = rtol
        self.atol = atol
        self.breakdown_tol = breakdown_tol
        self.hermitian_tol = hermitian_tol

    def threshold(self, lam):
        return max(self.atol, self.rtol * max(1.0, abs(lam)))


class Options:
    """DmrgOptions::default(); svd_threshold is the default policy of tensor_svd (relative, per value)"""

    def __init__(self, nsweeps=5, max_bond_dim=None, lanczos=None, energy_tol=None, real_scalar_tol=1e-10, svd_threshold=1e-12):
        self.nsweeps = nsweeps
        self.max_bond_dim = max_bond_dim
        self.lanczos = LanczosOptions() if lanczos is None else lanczos
        self.energy_tol = energy_tol
        self.real_scalar_tol = real_scalar_tol
        self.svd_threshold = svd_threshold


def full(ops):
    """the operator as a dense matrix, first site fastest in rows and columns"""
    return np_operator_full(ops)


# ------------------------------------------------------------------------------------------------ Lanczos
def np_lanczos(apply, v0, options=None):
    """-> (eigenvalue, unit eigenvector, iterations, true residual norm, converged); apply(v) on flat vectors.  ValueError: a start
    of norm <= breakdown_tol, a projected matrix that is not Hermitian."""
    o = LanczosOptions() if options is None else options
    if o.max_iter == 0:
        raise ValueError("max_iter must be greater than zero")
    v0 = np.asarray(v0, dtype=np.float64).reshape(-1)
    n0 = float(np.linalg.norm(v0))
    if n0 <= o.breakdown_tol:
        raise ValueError("the initial vector is numerically zero")
    basis = [v0 * (1.0 / n0)]
    cols = []

    def finalise(dim, lam, c):
        vec = c[0] * basis[0]
        for ci, vi in zip(c[1:dim], basis[1:dim]):
            vec = vec + ci * vi
        res = float(np.linalg.norm(apply(vec) - lam * vec))
        return lam, vec, dim, res, res <= o.threshold(lam)

    last = None
    for j in range(o.max_iter):
        w = apply(basis[j])
        col = []
        for v in basis[:j + 1]:
            h = float(v @ w)
            col.append(h)
            w = w - h * v
        for i, v in enumerate(basis[:j + 1]):
            c = float(v @ w)
            col[i] += c
            w = w - c * v
        beta = float(np.linalg.norm(w))
        col.append(beta)
        cols.append(col)
        dim = j + 1
        a = np.zeros((dim, dim))
        for cc in range(dim):
            for r in range(min(dim, len(cols[cc]))):
                a[r, cc] = cols[cc][r]
        for r in range(dim):
            for cc in range(r + 1, dim):
                scale = max(1.0, abs(a[r, cc]), abs(a[cc, r]))
                if not abs(a[r, cc] - a[cc, r]) <= o.hermitian_tol * scale:
                    raise ValueError("projected operator is not Hermitian")
        a = 0.5 * (a + a.T)
        lams, vecs = np.linalg.eigh(a)
        lam, c = float(lams[0]), vecs[:, 0]
        estimate = beta * abs(c[dim - 1])
        last = (dim, lam, c)
        if estimate <= o.threshold(lam) or beta <= o.breakdown_tol:
            out = finalise(dim, lam, c)
            if out[4] or beta <= o.breakdown_tol:
                return out
        basis.append(w * (1.0 / beta))
    return finalise(*last)


# ------------------------------------------------------------------------------------------------ the sweeps
def _envs(ops, x, i):
    left = np.ones((1, 1, 1))
    for k in range(i):
        left = np_left_env(left, ops[k], x[k])
    right = np.ones((1, 1, 1))
    for k in range(len(ops) - 1, i + 1, -1):
        right = np_right_env(right, ops[k], x[k])
    return left, right


def _rayleigh(ops, x, center, real_scalar_tol=1e-10):
    """<theta|H theta> / <theta|theta> at the region of `center` of a state that is canonical there"""
    n = len(ops)
    i = center if center + 1 < n else center - 1
    left, right = _envs(ops, x, i)
    theta = np.einsum("lsm,mtr->lstr", x[i], x[i + 1])
    y = np_projected_apply(left, right, ops[i], ops[i + 1], theta)
    den = float(np.sum(theta * theta))
    if abs(den) <= real_scalar_tol:
        raise ValueError("DMRG Rayleigh quotient denominator is zero")
    return float(np.sum(theta * y)) / den


def np_energy(ops, x, center=0, real_scalar_tol=1e-10):
    """the Rayleigh quotient of t4a_gpu_dmrg_energy: a copy of x is canonicalised onto `center`"""
    return _rayleigh(ops, np_canonicalize(x, center), center, real_scalar_tol)


def np_dmrg(ops, init, center=0, options=None, exact_local=False):
    """-> dict(state, energy, sweeps_completed, local_updates, converged, max_residual_norm, max_threshold, history, lanczos_steps);
    history[k] is the Rayleigh quotient after sweep k + 1.  exact_local: the local problems by numpy's eigh."""
    o = Options() if options is None else options
    n = len(ops)
    if n < 2:
        raise ValueError("two-site DMRG requires at least one state edge")
    if o.nsweeps == 0:
        raise ValueError("nsweeps must be greater than zero")
    x = np_canonicalize(init, center)
    out = {"local_updates": 0, "max_residual_norm": 0.0, "max_threshold": 0.0, "history": [], "lanczos_steps": 0, "converged": False}
    last_energy = None

    def bond_step(i, move_right):
        nonlocal last_energy
        left, right = _envs(ops, x, i)
        theta0 = np.einsum("lsm,mtr->lstr", x[i], x[i + 1])
        shape = theta0.shape

        def apply(v):
            return np_projected_apply(left, right, ops[i], ops[i + 1], v.reshape(shape, order="F")).reshape(-1, order="F")
        if exact_local:
            dim = int(np.prod(shape))
            h = np.stack([apply(e) for e in np.eye(dim)], axis=1)
            lams, vecs = np.linalg.eigh(0.5 * (h + h.T))
            lam, theta, iters = float(lams[0]), vecs[:, 0], 0
            res = float(np.linalg.norm(h @ theta - lam * theta))
        else:
            lam, theta, iters, res, _ = np_lanczos(apply, theta0.reshape(-1, order="F"), o.lanczos)
        last_energy = lam
        out["lanczos_steps"] += iters
        out["max_residual_norm"] = max(out["max_residual_norm"], res)
        out["max_threshold"] = max(out["max_threshold"], o.lanczos.threshold(lam))
        u, s, vt = np_truncated_svd(theta.reshape((shape[0] * shape[1], shape[2] * shape[3]), order="F"), o.svd_threshold, o.max_bond_dim)
        k = len(s)
        if move_right:
            x[i] = u.reshape((shape[0], shape[1], k), order="F")
            x[i + 1] = (s[:, None] * vt).reshape((k, shape[2], shape[3]), order="F")
        else:
            x[i] = (u * s[None, :]).reshape((shape[0], shape[1], k), order="F")
            x[i + 1] = vt.reshape((k, shape[2], shape[3]), order="F")
        out["local_updates"] += 1

    previous = None
    sweeps = 0
    for sweep in range(o.nsweeps):
        for i, move_right in sweep_plan(n, center):
            bond_step(i, move_right)
        sweeps = sweep + 1
        out["history"].append(_rayleigh(ops, x, center, o.real_scalar_tol))
        if o.energy_tol is not None:
            if previous is not None and abs(last_energy - previous) <= o.energy_tol:
                out["converged"] = True
                break
            previous = last_energy
    out["state"] = x
    out["sweeps_completed"] = sweeps
    out["energy"] = out["history"][-1]
    return out


# ------------------------------------------------------------------------------------------------ operators
def _boundary(w):
    """the chain of bulk operator-valued matrices w[k] (W x W x d x d, lower-triangular form: the last row starts, the first column
    ends) as site tensors [w_l, s1, s2, w_r]"""
    sites = []
    n = len(w)
    for k, m in enumerate(w):
        t = m.transpose(0, 2, 3, 1)  # [w_l, s1, s2, w_r]
        if k == 0:
            t = t[-1:, :, :, :]
        if k == n - 1:
            t = t[:, :, :, :1]
        sites.append(np.ascontiguousarray(t))
    return sites


def heisenberg(n):
    """open spin-1/2 Heisenberg chain sum_i S_i . S_{i+1}, operator bond 5"""
    sp, sm, sz, one = np.array([[0.0, 1.0], [0.0, 0.0]]), np.array([[0.0, 0.0], [1.0, 0.0]]), np.diag([0.5, -0.5]), np.eye(2)
    m = np.zeros((5, 5, 2, 2))
    m[0, 0], m[1, 0], m[2, 0], m[3, 0] = one, sp, sm, sz
    m[4, 1], m[4, 2], m[4, 3], m[4, 4] = 0.5 * sm, 0.5 * sp, sz, one
    return _boundary([m] * n)


def tfim(n, g):
    """open transverse-field Ising chain -sum Z_i Z_{i+1} - g sum X_i, operator bond 3"""
    x, z, one = np.array([[0.0, 1.0], [1.0, 0.0]]), np.diag([1.0, -1.0]), np.eye(2)
    m = np.zeros((3, 3, 2, 2))
    m[0, 0], m[1, 0] = one, z
    m[2, 0], m[2, 1], m[2, 2] = -g * x, -z, one
    return _boundary([m] * n)


def symmetric_integer_operator(dims, w, seed):
    """site tensors with integer entries in {-3, ..., 3}, symmetric in (s1, s2) for every pair of operator bonds: every term of the
    operator is a Kronecker product of symmetric matrices"""
    n = len(dims)
    bonds = [1] + [w] * (n - 1) + [1]
    sites = []
    for k, d in enumerate(dims):
        t = random_tensors([bonds[k], bonds[k + 1]], d, d, seed ^ (0x51 * (k + 1)))[0]
        t = np.floor(t * 7.0 + 0.5).transpose(0, 3, 1, 2)  # (-0.5, 0.5) -> {-3, ..., 3}; [w_l, w_r, s1, s2]
        t = np.triu(t) + np.swapaxes(np.triu(t, 1), -1, -2)
        sites.append(np.ascontiguousarray(t.transpose(0, 2, 3, 1)))
    return sites


def random_state(dims, bonds, seed):
    """site tensors [l, d_k, r] from the LCG of tests/fit_np.py"""
    return [random_tensors([bonds[k], bonds[k + 1]], d, 1, seed ^ (0x77 * (k + 1)))[0][:, :, 0, :] for k, d in enumerate(dims)]


# ------------------------------------------------------------------------------------------------ the cases the CPU and the device tests share
CASES = {  # name: (site dimensions, start bond, max_bond_dim, center)
    "heis8": ((2,) * 8, 4, None, 0),
    "heis6_c3": ((2,) * 6, 2, None, 3),
    "tfim6": ((2,) * 6, 2, None, 5),
    "tfim8_cap4": ((2,) * 8, 3, 4, 0),
    "mixed5": ((2, 3, 2, 3, 2), 3, None, 2),
    "n2": ((3, 2), 2, None, 0),
}
UNTRUNCATED = tuple(sorted(k for k, v in CASES.items() if v[2] is None))

_CACHE = {}


def make_case(name):
    """-> (operator sites, start sites, center, max_bond_dim)"""
    dims, bond, cap, center = CASES[name]
    n = len(dims)
    if name.startswith("heis"):
        ops = heisenberg(n)
    elif name == "tfim6":
        ops = tfim(n, 0.7)
    elif name == "tfim8_cap4":
        ops = tfim(n, 1.0)
    else:
        ops = symmetric_integer_operator(dims, 3, SEED ^ 0xD3 ^ n)
    init = random_state(dims, [1] + [bond] * (n - 1) + [1], SEED ^ 0xD0 ^ n)
    return ops, init, center, cap


def dense_spectrum(name):
    """-> (H, eigenvalues ascending, ground vector, ||H||_2), computed once per case"""
    if name not in _CACHE:
        h = full(make_case(name)[0])
        lams, vecs = np.linalg.eigh(0.5 * (h + h.T))
        _CACHE[name] = (h, lams, vecs[:, 0], float(max(abs(lams[0]), abs(lams[-1]))))
    return _CACHE[name]


def restated(name, nsweeps):
    """np_dmrg of the case with default options and `nsweeps` sweeps, computed once"""
    key = (name, nsweeps)
    if key not in _CACHE:
        ops, init, center, cap = make_case(name)
        _CACHE[key] = np_dmrg(ops, init, center, Options(nsweeps=nsweeps, max_bond_dim=cap))
    return _CACHE[key]


def diag3_matrix(n=12):
    return np.diag(np.array([1.0, 2.0, 3.0])[np.arange(n) % 3])


def dense_cases():
    """name -> (H, v0, LanczosOptions, ends by breakdown): the matrices the device's lanczos_dense is run on as well"""
    n = 12
    v = lcg_matrix(n, SEED ^ 0xB)[:, 0].copy()
    big = lcg_matrix(40, SEED ^ 0x40)
    big = 0.5 * (big + big.T)
    sym = lcg_matrix(n, SEED ^ 0x6E)
    sym = 0.5 * (sym + sym.T)
    lams, vecs = np.linalg.eigh(sym)
    return {
        "identity": (np.eye(n), v, LanczosOptions(), True),
        "diag3": (diag3_matrix(n), v, LanczosOptions(), True),
        "eigenvector_start": (sym, 2.5 * vecs[:, 0], LanczosOptions(), True),
        "symmetric12": (sym, v, LanczosOptions(), False),
        "max_iter_2": (big, lcg_matrix(40, SEED ^ 0x41)[:, 0].copy(), LanczosOptions(max_iter=2), False),
        "symmetric40": (big, lcg_matrix(40, SEED ^ 0x41)[:, 0].copy(), LanczosOptions(), False),
    }


def nonsymmetric_case():
    n = 12
    return 3.0 * np.eye(n) + lcg_matrix(n, SEED ^ 0x6E), lcg_matrix(n, SEED ^ 0xB)[:, 0].copy()
