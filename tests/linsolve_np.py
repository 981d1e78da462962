"""numpy restatement of square_linsolve (t4a_gpu_square_linsolve): the two-site sweeps with a local GMRES of tensor4all-treetn
(linsolve/square/mod.rs:233-351, square/updater.rs, common/projected_operator.rs) on a chain, and gmres_affine_impl
(tensor4all-core/src/krylov.rs:1083-1490) with the reference's two passes of MODIFIED Gram-Schmidt and host Givens rotations.
Operator sites are [w_l, s, t, w_r], state and rhs sites [l, s, r]; environments L[beta, w, alpha], R[beta, w, alpha].
random_tensors and the LCG are those of tests/fit_np.py."""
import numpy as np

from fit_np import SEED, random_tensors  # noqa: F401

RELATIVE, ABSOLUTE = 0, 1


class Options:
    """LinsolveOptions::default()"""

    def __init__(self, nfullsweeps=5, max_bond_dim=None, gmres_tol=1e-10, gmres_tolerance_mode=RELATIVE, gmres_max_restarts=100,
                 gmres_restart_dim=30, a0=0.0, a1=1.0, convergence_tol=None, check_residual=True, svd_threshold=1e-12):
        self.nfullsweeps = nfullsweeps
        self.max_bond_dim = max_bond_dim
        self.gmres_tol = gmres_tol
        self.gmres_tolerance_mode = gmres_tolerance_mode
        self.gmres_max_restarts = gmres_max_restarts
        self.gmres_restart_dim = gmres_restart_dim
        self.a0 = a0
        self.a1 = a1
        self.convergence_tol = convergence_tol
        self.check_residual = check_residual
        self.svd_threshold = svd_threshold  # the default policy of tensor_svd: relative, per value


def random_state(bonds, d, seed):
    return [t[:, :, 0, :] for t in random_tensors(bonds, d, 1, seed)]


# ------------------------------------------------------------------------------------------------ GMRES
def _givens(a, b):
    aa, ba = abs(a), abs(b)
    r = np.sqrt(aa * aa + ba * ba)
    if r < 1e-15:
        return 1.0, 0.0
    if aa < 1e-15:
        return 0.0, b / r
    return aa / r, (a / aa) * b / r


def _rotate(c, s, x, y):
    return c * x + s * y, -(s * x) + c * y


def _solve_upper(h, g, n):
    y = np.zeros(n)
    for i in range(n - 1, -1, -1):
        acc = g[i]
        for j in range(i + 1, n):
            acc = acc - h[j][i] * y[j]
        if abs(h[i][i]) < 1e-15:
            raise ValueError("Near-singular upper triangular matrix in GMRES")
        y[i] = acc / h[i][i]
    return y


def np_gmres_affine(apply, b, x0, a0, a1, tol=1e-10, mode=RELATIVE, restart_dim=30, max_restarts=100):
    """-> (x, iterations, residual, converged); apply(v) is the unshifted operator on flat vectors."""
    b = np.asarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    b_norm = float(np.linalg.norm(b))

    def value(r):
        return r / b_norm if mode == RELATIVE else r

    if b_norm < 1e-15:
        return x, 0, 0.0, True
    if a0 == 0 and a1 == 0:
        raise ValueError("gmres: a0 and a1 are both zero")
    if a1 == 0:
        return b * (1.0 / a0), 0, 0.0, True

    def residual(x):
        return b - (a0 * x + a1 * apply(x))

    iters = 0
    for _ in range(max_restarts):
        r = residual(x)
        r_norm = float(np.linalg.norm(r))
        if value(r_norm) < tol:
            return x, iters, value(r_norm), True
        basis = [r * (1.0 / r_norm)]
        hm, cs, sn, g = [], [], [], [r_norm]
        updated = False
        for j in range(restart_dim):
            iters += 1
            w = apply(basis[j])
            ha = []
            for v in basis[:j + 1]:
                h = float(v @ w)
                ha.append(h)
                w = w - h * v
            for i, v in enumerate(basis[:j + 1]):
                c = float(v @ w)
                ha[i] += c
                w = w - c * v
            h_next = float(np.linalg.norm(w))
            ha.append(h_next)
            hc = [a1 * h for h in ha[:j]] + [a0 + a1 * ha[j], a1 * ha[j + 1]]
            for i in range(j):
                hc[i], hc[i + 1] = _rotate(cs[i], sn[i], hc[i], hc[i + 1])
            c, s = _givens(hc[j], hc[j + 1])
            cs.append(c)
            sn.append(s)
            hc[j], _ = _rotate(c, s, hc[j], hc[j + 1])
            hc[j + 1] = 0.0
            g[j], gn = _rotate(c, s, g[j], 0.0)
            g.append(gn)
            hm.append(hc)
            if value(abs(gn)) < tol:
                y = _solve_upper(hm, g, j + 1)
                x = x + sum(yi * v for yi, v in zip(y, basis))
                true_res = float(np.linalg.norm(residual(x)))  # check_true_residual
                if value(true_res) < tol:
                    return x, iters, value(true_res), True
                updated = True
                break
            if h_next > 1e-14:
                basis.append(w * (1.0 / h_next))
            else:
                y = _solve_upper(hm, g, j + 1)
                x = x + sum(yi * v for yi, v in zip(y, basis))
                final = float(np.linalg.norm(residual(x)))
                return x, iters, value(final), value(final) < tol
        if not updated:
            y = _solve_upper(hm, g, len(hm))
            x = x + sum(yi * v for yi, v in zip(y, basis))
    final = float(np.linalg.norm(residual(x)))
    return x, iters, value(final), value(final) < tol


# ------------------------------------------------------------------------------------------------ dense helpers
def np_state_full(ts):
    """dense vector indexed [s_1, s_2, ...], flattened with the FIRST site fastest"""
    acc = ts[0][0]
    for t in ts[1:]:
        acc = np.tensordot(acc, t, axes=([-1], [0]))
    return acc[..., 0].reshape(-1, order="F")


def np_operator_full(ops):
    """dense matrix [row = (s_1, s_2, ...), col = (t_1, t_2, ...)], first site fastest in both"""
    acc = ops[0][0]  # [s, t, w]
    for t in ops[1:]:
        acc = np.tensordot(acc, t, axes=([-1], [0]))
    acc = acc[..., 0]  # [s1, t1, s2, t2, ...]
    n = len(ops)
    acc = acc.transpose(list(range(0, 2 * n, 2)) + list(range(1, 2 * n, 2)))
    dim = int(np.prod(acc.shape[:n]))
    return acc.reshape((dim, dim), order="F")


def np_residual(ops, x, b, a0, a1):
    """||(a0 + a1 A) x - b|| / ||b|| (the absolute norm when ||b|| <= 1e-15) from the dense objects"""
    am, xv, bv = np_operator_full(ops), np_state_full(x), np_state_full(b)
    r = float(np.linalg.norm(a0 * xv + a1 * (am @ xv) - bv))
    bn = float(np.linalg.norm(bv))
    return r / bn if bn > 1e-15 else r


# ------------------------------------------------------------------------------------------------ environments and the local problem
def np_left_env(env, op, x):
    """L'[b', w', a'] = sum L[b, w, a] x[b, s, b'] A[w, s, t, w'] x[a, t, a']"""
    return np.einsum("bwa,bsc,wstv,atd->cvd", env, x, op, x)


def np_right_env(env, op, x):
    """R'[b, w, a] = sum x[b, s, b'] A[w, s, t, w'] x[a, t, a'] R[b', w', a']"""
    return np.einsum("bsc,wstv,atd,cvd->bwa", x, op, x, env)


def np_half_operators(left, right, op1, op2):
    """HL (W M) x M and HR (W N) x N in the layouts of csrc/linsolve.hpp"""
    chi_l, chi_r = left.shape[0], right.shape[0]
    d1, d2, w = op1.shape[1], op2.shape[1], op1.shape[3]
    hl = np.einsum("bla,lstw->bswat", left, op1).reshape((chi_l * d1 * w, chi_l * d1), order="F")
    hr = np.einsum("wstr,bra->wtasb", op2, right).reshape((w * d2 * chi_r, d2 * chi_r), order="F")
    return hl, hr


def np_projected_apply(left, right, op1, op2, v):
    """y[b_l, s1, s2, b_r] = sum L[b_l, w_l, a_l] A1[w_l, s1, t1, w] v[a_l, t1, t2, a_r] A2[w, s2, t2, w_r] R[b_r, w_r, a_r]"""
    return np.einsum("blp,lsuw,puvq,wtvr,crq->bstc", left, op1, v, op2, right)


def np_projected_apply_steps(left, right, op1, op2, v):
    """np_projected_apply in the usual four-step order (environment, site, site, environment), one tensordot each: what a CPU
    implementation runs, and not the order of the device"""
    t1 = np.tensordot(left, v, axes=([2], [0]))                 # [b, l, u, x, q]
    t2 = np.tensordot(t1, op1, axes=([1, 2], [0, 2]))           # [b, x, q, s, w]
    t3 = np.tensordot(t2, op2, axes=([4, 1], [0, 2]))           # [b, q, s, t, r]
    return np.tensordot(t3, right, axes=([4, 1], [1, 2]))       # [b, s, t, c]


def np_projected_dense(left, right, op1, op2):
    """the projected operator as a matrix over flattened (column-major) two-site vectors"""
    chi_l, chi_r, d1, d2 = left.shape[0], right.shape[0], op1.shape[1], op2.shape[1]
    h = np.einsum("blp,lsuw,wtvr,crq->bstcpuvq", left, op1, op2, right)
    dim = chi_l * d1 * d2 * chi_r
    return h.reshape((dim, dim), order="F")


def np_canonicalize(x, center):
    x = [t.copy() for t in x]
    for i in range(center):
        l, s, r = x[i].shape
        q, rr = np.linalg.qr(x[i].reshape((l * s, r), order="F"))
        x[i] = q.reshape((l, s, q.shape[1]), order="F")
        x[i + 1] = np.einsum("kr,rsq->ksq", rr, x[i + 1])
    for i in range(len(x) - 1, center, -1):
        l, s, r = x[i].shape
        q, rr = np.linalg.qr(x[i].reshape((l, s * r), order="F").T)
        x[i] = q.T.reshape((q.shape[1], s, r), order="F")
        x[i - 1] = np.einsum("lsr,kr->lsk", x[i - 1], rr)
    return x


def sweep_plan(n, center):
    """[(bond, move_right)]: the Euler tour from `center`, the second node of a step the new centre"""
    return ([(i, True) for i in range(center, n - 1)] + [(i, False) for i in range(n - 2, -1, -1)] + [(i, True) for i in range(center)])


def np_truncated_svd(mat, threshold, max_bond_dim):
    u, s, vt = np.linalg.svd(mat, full_matrices=False)
    keep = int(np.sum(s >= threshold * s[0])) if s[0] > 0 else 0
    if max_bond_dim is not None:
        keep = min(keep, max_bond_dim)
    keep = min(max(keep, 1), len(s))
    return u[:, :keep], s[:keep], vt[:keep]


def np_square_linsolve(ops, rhs, init, center=0, options=None, exact_local=False):
    """-> (site tensors, sweeps, residual or None, converged, stats).  exact_local: the local problems by np.linalg.solve."""
    o = Options() if options is None else options
    n = len(ops)
    stats = {"local_solves": 0, "arnoldi_steps": 0}
    wants = o.check_residual or o.convergence_tol is not None
    if o.a1 == 0 or np.linalg.norm(np_operator_full(ops)) <= 1e-15:
        if o.a0 == 0:
            raise ValueError("square_linsolve: a0 and effective operator term are both zero")
        sol = [t.copy() for t in rhs]
        sol[-1] = sol[-1] * (1.0 / o.a0)
        res = np_residual(ops, sol, rhs, o.a0, o.a1) if wants else None
        return sol, 0, res, o.convergence_tol is not None and res is not None and res < o.convergence_tol, stats
    x = np_canonicalize(init, center)

    def envs(i):
        left, lb = np.ones((1, 1, 1)), np.ones((1, 1))
        for k in range(i):
            left = np_left_env(left, ops[k], x[k])
            lb = np.einsum("bg,bsc,gsh->ch", lb, x[k], rhs[k])
        right, rb = np.ones((1, 1, 1)), np.ones((1, 1))
        for k in range(n - 1, i + 1, -1):
            right = np_right_env(right, ops[k], x[k])
            rb = np.einsum("bsc,gsh,ch->bg", x[k], rhs[k], rb)
        return left, right, lb, rb

    def bond_step(i, move_right):
        left, right, lb, rb = envs(i)
        theta0 = np.einsum("lsm,mtr->lstr", x[i], x[i + 1])
        shape = theta0.shape
        bt = np.einsum("bg,gsm,mth,ch->bstc", lb, rhs[i], rhs[i + 1], rb)
        if exact_local:
            h = np_projected_dense(left, right, ops[i], ops[i + 1])
            theta = np.linalg.solve(o.a0 * np.eye(h.shape[0]) + o.a1 * h, bt.reshape(-1, order="F"))
        else:
            def apply(v):
                return np_projected_apply(left, right, ops[i], ops[i + 1], v.reshape(shape, order="F")).reshape(-1, order="F")
            theta, iters, _, _ = np_gmres_affine(apply, bt.reshape(-1, order="F"), theta0.reshape(-1, order="F"), o.a0, o.a1, o.gmres_tol,
                                                 o.gmres_tolerance_mode, o.gmres_restart_dim, o.gmres_max_restarts)
            stats["arnoldi_steps"] += iters
        stats["local_solves"] += 1
        u, s, vt = np_truncated_svd(theta.reshape((shape[0] * shape[1], shape[2] * shape[3]), order="F"), o.svd_threshold, o.max_bond_dim)
        k = len(s)
        if move_right:
            x[i] = u.reshape((shape[0], shape[1], k), order="F")
            x[i + 1] = (s[:, None] * vt).reshape((k, shape[2], shape[3]), order="F")
        else:
            x[i] = (u * s[None, :]).reshape((shape[0], shape[1], k), order="F")
            x[i + 1] = vt.reshape((k, shape[2], shape[3]), order="F")

    sweeps, residual, converged = 0, None, False
    for sweep in range(o.nfullsweeps):
        sweeps = sweep + 1
        for i, move_right in sweep_plan(n, center):
            bond_step(i, move_right)
        if o.convergence_tol is not None:
            residual = np_residual(ops, x, rhs, o.a0, o.a1)
            if residual < o.convergence_tol:
                converged = True
                break
    if residual is None and o.check_residual:
        residual = np_residual(ops, x, rhs, o.a0, o.a1)
        converged = o.convergence_tol is not None and residual < o.convergence_tol
    return x, sweeps, residual, converged, stats


# ------------------------------------------------------------------------------------------------ the cases the CPU and the device tests share
CASES = {  # name: (n, d, W, rhs bond, init bond, cap, the solution's bonds)
    "n6": (6, 2, 3, 4, 2, 16, [2, 4, 8, 4, 2]),
    "n5": (5, 3, 2, 3, 1, 27, [3, 9, 9, 3]),
    "n8": (8, 2, 4, 5, 2, 16, [2, 4, 8, 16, 8, 4, 2]),
}


def make_case(name):
    """-> (operator sites, rhs sites, init sites, a0, cap): a1 = 1 and a0 = 2 ||A||_2, so that every projected problem (the sites are
    isometries) has its numerical range at least ||A||_2 away from zero."""
    n, d, w, rb, ib, cap, _ = CASES[name]
    ops = random_tensors([1] + [w] * (n - 1) + [1], d, d, SEED ^ n)
    rhs = random_state([1] + [rb] * (n - 1) + [1], d, SEED ^ 0xB0 ^ n)
    init = random_state([1] + [ib] * (n - 1) + [1], d, SEED ^ 0x1A17 ^ n)
    a0 = 2.0 * float(np.linalg.norm(np_operator_full(ops), 2))
    return ops, rhs, init, a0, cap


def lcg_matrix(n, seed):
    return random_tensors([n, n], 1, 1, seed)[0].reshape((n, n), order="F")


def three_eigenvalue_matrix(n=12):
    q, _ = np.linalg.qr(lcg_matrix(n, SEED ^ 0x3E))
    lam = np.array([1.0, 2.0, 3.0])[np.arange(n) % 3]
    return (q * lam[None, :]) @ q.T


def dense_cases():
    """name -> (H, b, x0, a0, a1, kwargs): the matrices the device's gmres_dense is run on as well"""
    n = 12
    b = lcg_matrix(n, SEED ^ 0xB)[:, 0].copy()
    z = np.zeros(n)
    gen = 3.0 * np.eye(n) + lcg_matrix(n, SEED ^ 0x6E)
    return {
        "identity": (np.eye(n), b, z, 0.0, 1.0, {}),
        "three_eigenvalues": (three_eigenvalue_matrix(n), b, z, 0.0, 1.0, {}),
        "restart": (gen, b, z, 0.5, 1.0, {"restart_dim": 2}),
        "zero_rhs": (gen, z, b, 0.5, 1.0, {}),
        "a1_zero": (gen, b, z, 4.0, 0.0, {}),
        "not_converged": (gen, b, z, 0.0, 1.0, {"restart_dim": 2, "max_restarts": 1}),
        "absolute": (gen, b, z, 0.5, 1.0, {"mode": ABSOLUTE, "tol": 1e-9}),
    }
