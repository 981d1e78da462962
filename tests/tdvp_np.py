"""numpy restatement of two-site TDVP (t4a_gpu_tdvp): the region plan of tensor4all-treetn's tdvp (tdvp/plan.rs:41-181) on a chain
rooted at an end, the sweeps of tdvp/mod.rs:1107-1217 (update_two_site :916-1042, the site correction :639-700, the full-rank centre
move :1318-1390) and the Krylov exponential of tensor4all-core (krylov.rs:707-926) for a real exponent — two passes of MODIFIED
Gram-Schmidt as the reference runs them, or the two classical passes of the device (cgs2=True), the projected matrix from the full
upper-Hessenberg columns, the Hermitian check per entry pair, exp(tau T) e_1 by numpy's eigh —, and the cases the CPU and the device
tests share.  Operator sites are [w_l, s1, s2, w_r], state sites [l, s, r]; the environments, the canonicalisation and the
truncation rule are those of tests/linsolve_np.py, the operators those of tests/dmrg_np.py."""
import numpy as np

from fit_np import SEED
from linsolve_np import np_canonicalize, np_left_env, np_right_env, np_projected_apply_steps, np_operator_full, np_state_full, lcg_matrix  # noqa: F401
from dmrg_np import heisenberg, tfim, symmetric_integer_operator, random_state, diag3_matrix

TWO, CORR = 0, 1  # the kinds of a plan step, as t4a_gpu_tdvp_plan reports them


class KrylovOptions:
    """HermitianKrylovExpmOptions::default() (krylov.rs:429-440)"""

    def __init__(self, max_iter=30, max_time_splits=100, tol=1e-12, breakdown_tol=1e-14, hermitian_tol=1e-10):
        self.max_iter = max_iter
        self.max_time_splits = max_time_splits
        self.tol = tol
        self.breakdown_tol = breakdown_tol
        self.hermitian_tol = hermitian_tol


class Options:
    """TdvpOptions::default() with this project's real exponent (-0.1 where the reference has -0.1i); svd_threshold is the default
    policy of tensor_svd (relative, per value)"""

    def __init__(self, nsweeps=1, order=2, exponent_step=-0.1, max_bond_dim=None, krylov=None, svd_threshold=1e-12, cgs2=False):
        self.nsweeps = nsweeps
        self.order = order
        self.exponent_step = exponent_step
        self.max_bond_dim = max_bond_dim
        self.krylov = KrylovOptions() if krylov is None else krylov
        self.svd_threshold = svd_threshold
        self.cgs2 = cgs2


# ------------------------------------------------------------------------------------------------ the plan
def applyexp_sub_steps(order):
    """plan.rs:76-86"""
    if order == 1:
        return [1.0]
    if order == 2:
        return [0.5, 0.5]
    if order == 4:
        s = 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))
        return [s / 2.0, s / 2.0, 0.5 - s, 0.5 - s, s / 2.0, s / 2.0]
    raise ValueError("TDVP applyexp order %d is not supported; supported orders are 1, 2, and 4" % order)


def tdvp_plan(n, center, order, tau):
    """-> [(kind, nodes, new_center, exponent)]: plan.rs:41-73 with the root-edge-first walk of :112-158 from an end of a chain (the
    edges (0,1), (1,2), ... from 0, their mirror images from n-1): the centre of a two-site step is the node shared with the next
    edge, the correction there carries -exponent, the last edge has none; every even substep (1-based) is the reversed list with
    the nodes reversed and the last node the new centre (:164-181)."""
    if n < 2:
        raise ValueError("two-site TDVP requires at least one state edge")
    if center not in (0, n - 1):
        raise ValueError("center must be an end of the chain")
    chain = list(range(n)) if center == 0 else list(range(n - 1, -1, -1))
    base = []
    for j in range(n - 1):
        a, b = chain[j], chain[j + 1]
        base.append((TWO, (a, b), b, 1.0))
        if j < n - 2:
            base.append((CORR, (b,), b, -1.0))
    steps = []
    for k, weight in enumerate(applyexp_sub_steps(order)):
        part = [(kind, nodes, nc, (tau * sign) * weight) for kind, nodes, nc, sign in base]
        if (k + 1) % 2 == 0:
            part = [(kind, nodes[::-1], nodes[::-1][-1], e) for kind, nodes, _, e in reversed(part)]
        steps.extend(part)
    return steps


# ------------------------------------------------------------------------------------------------ the Krylov exponential
def _expm_once(apply, tau, v0, o, cgs2):
    """hermitian_krylov_expm_multiply_once (krylov.rs:790-906) -> (out, iterations, estimate, converged)"""
    n0 = float(np.linalg.norm(v0))
    if n0 <= o.breakdown_tol:
        return v0.copy(), 0, 0.0, True
    basis = [v0 * (1.0 / n0)]
    cols = []
    threshold = o.tol * max(n0, 1.0)
    last = None

    def combine(c, dim):
        out = (n0 * c[0]) * basis[0]
        for ci, vi in zip(c[1:dim], basis[1:dim]):
            out = out + (n0 * ci) * vi
        return out

    for j in range(o.max_iter):
        w = apply(basis[j])
        col = [0.0] * (j + 1)
        for _ in range(2):
            if cgs2:
                hs = [float(v @ w) for v in basis[:j + 1]]
                for i, v in enumerate(basis[:j + 1]):
                    col[i] += hs[i]
                    w = w - hs[i] * v
            else:
                for i, v in enumerate(basis[:j + 1]):
                    h = float(v @ w)
                    col[i] += h
                    w = w - h * v
        beta = float(np.linalg.norm(w))
        col.append(beta)
        cols.append(col)
        dim = j + 1
        a = np.zeros((dim, dim))
        for cc in range(dim):
            rows = min(dim, len(cols[cc]))
            a[:rows, cc] = cols[cc][:rows]
        scale = np.maximum(1.0, np.maximum(np.abs(a), np.abs(a.T)))  # the check per entry pair
        if not np.all(np.abs(a - a.T) <= o.hermitian_tol * scale):
            raise ValueError("projected operator is not Hermitian")
        lams, q = np.linalg.eigh(0.5 * (a + a.T))
        c = q @ (np.exp(tau * lams) * q[0, :])
        estimate = 0.0 if beta <= o.breakdown_tol else n0 * beta * abs(c[dim - 1])
        if beta <= o.breakdown_tol or estimate <= threshold:
            return combine(c, dim), dim, estimate, True
        last = (c, dim, estimate)
        basis.append(w * (1.0 / beta))
    c, dim, estimate = last
    return combine(c, dim), dim, estimate, False


def np_krylov_expm(apply, tau, v0, options=None, cgs2=False):
    """exp(tau H) v0 -> (out, iterations, error_estimate, converged, time_splits); apply(v) on flat vectors (krylov.rs:707-788).
    ValueError: bad options, a projected matrix that is not Hermitian, no convergence at max_time_splits."""
    o = KrylovOptions() if options is None else options
    if o.max_iter == 0:
        raise ValueError("hermitian_krylov_expm_multiply: max_iter must be greater than zero")
    if o.max_time_splits == 0:
        raise ValueError("hermitian_krylov_expm_multiply: max_time_splits must be greater than zero")
    v0 = np.asarray(v0, dtype=np.float64).reshape(-1)
    if tau == 0.0 or float(np.linalg.norm(v0)) <= o.breakdown_tol:
        return v0.copy(), 0, 0.0, True, 1
    splits = 1
    while True:
        out, iters, err, conv = v0, 0, 0.0, True
        for _ in range(splits):
            out, it, e, ok = _expm_once(apply, tau / splits, out, o, cgs2)
            iters += it
            err = max(err, e)
            if not ok:
                conv = False
                break
        if conv:
            return out, iters, err, True, splits
        if splits >= o.max_time_splits:
            raise ValueError("hermitian_krylov_expm_multiply did not converge within max_time_splits=%d and max_iter=%d" % (o.max_time_splits, o.max_iter))
        splits = min(2 * splits, o.max_time_splits)


# ------------------------------------------------------------------------------------------------ the sweeps
def np_one_site_apply(left, right, op, v):
    """y[b, s, c] = sum L[b, w, a] A[w, s, t, v] x[a, t, d] R[c, v, d]"""
    t1 = np.tensordot(left, v, axes=([2], [0]))              # [b, w, t, d]
    t2 = np.tensordot(t1, op, axes=([1, 2], [0, 2]))         # [b, d, s, v]
    return np.tensordot(t2, right, axes=([3, 1], [1, 2]))    # [b, s, c]


def _left(ops, x, i):
    env = np.ones((1, 1, 1))
    for k in range(i):
        env = np_left_env(env, ops[k], x[k])
    return env


def _right(ops, x, i):
    """the environment of the sites >= i"""
    env = np.ones((1, 1, 1))
    for k in range(len(ops) - 1, i - 1, -1):
        env = np_right_env(env, ops[k], x[k])
    return env


def _move_center(x, cur, target):
    """move_center_to_region_full_rank (tdvp/mod.rs:1318-1390): thin QR steps along the path, no truncation"""
    while cur < target:
        l, s, r = x[cur].shape
        q, rr = np.linalg.qr(x[cur].reshape((l * s, r), order="F"))
        x[cur] = q.reshape((l, s, q.shape[1]), order="F")
        x[cur + 1] = np.einsum("kr,rsq->ksq", rr, x[cur + 1])
        cur += 1
    while cur > target:
        l, s, r = x[cur].shape
        q, rr = np.linalg.qr(x[cur].reshape((l, s * r), order="F").T)
        x[cur] = q.T.reshape((q.shape[1], s, r), order="F")
        x[cur - 1] = np.einsum("lsr,kr->lsk", x[cur - 1], rr)
        cur -= 1
    return cur


def np_tdvp(ops, init, center=0, options=None, exact_local=False):
    """-> dict(state, sweeps_completed, local_updates, max_error_estimate, max_krylov_iterations, two_site_steps, corrections,
    krylov_steps, max_time_splits, cut_ratios); cut_ratios holds sigma_k / sigma_{k+1} of every split that dropped a non-zero singular
    value.  exact_local: the local exponentials from numpy's eigh of the dense projected operator."""
    o = Options() if options is None else options
    n = len(ops)
    if o.nsweeps == 0:
        raise ValueError("invalid TDVP option nsweeps: must be greater than zero")
    plan = tdvp_plan(n, center, o.order, o.exponent_step)
    x = np_canonicalize(init, center)
    cur = center
    out = {"local_updates": 0, "max_error_estimate": 0.0, "max_krylov_iterations": 0, "two_site_steps": 0, "corrections": 0, "krylov_steps": 0,
           "max_time_splits": 1, "cut_ratios": []}

    def evolve(apply, v, exponent):
        if exact_local:
            h = np.stack([apply(e) for e in np.eye(v.size)], axis=1)
            lams, q = np.linalg.eigh(0.5 * (h + h.T))
            res = (q @ (np.exp(exponent * lams) * (q.T @ v)), 0, 0.0, True, 1)
        else:
            res = np_krylov_expm(apply, exponent, v, o.krylov, o.cgs2)
        out["local_updates"] += 1
        out["krylov_steps"] += res[1]
        out["max_error_estimate"] = max(out["max_error_estimate"], res[2])
        out["max_krylov_iterations"] = max(out["max_krylov_iterations"], res[1])
        out["max_time_splits"] = max(out["max_time_splits"], res[4])
        return res[0]

    sweeps = 0
    for sweep in range(o.nsweeps):
        for kind, nodes, new_center, exponent in plan:
            if cur not in nodes:
                cur = _move_center(x, cur, min(nodes, key=lambda k: abs(k - cur)))
            if kind == TWO:
                i = min(nodes)
                left, right = _left(ops, x, i), _right(ops, x, i + 2)
                theta0 = np.einsum("lsm,mtr->lstr", x[i], x[i + 1])
                shape = theta0.shape

                def apply(v):
                    return np_projected_apply_steps(left, right, ops[i], ops[i + 1], v.reshape(shape, order="F")).reshape(-1, order="F")
                theta = evolve(apply, theta0.reshape(-1, order="F"), exponent)
                u, s, vt = np.linalg.svd(theta.reshape((shape[0] * shape[1], shape[2] * shape[3]), order="F"), full_matrices=False)
                keep = int(np.sum(s >= o.svd_threshold * s[0])) if s[0] > 0 else 0
                if o.max_bond_dim is not None:
                    keep = min(keep, o.max_bond_dim)
                keep = min(max(keep, 1), len(s))
                if keep < len(s) and s[keep] > 0.0:
                    out["cut_ratios"].append(float(s[keep - 1] / s[keep]))
                u, s, vt = u[:, :keep], s[:keep], vt[:keep]
                if new_center == i + 1:
                    x[i] = u.reshape((shape[0], shape[1], keep), order="F")
                    x[i + 1] = (s[:, None] * vt).reshape((keep, shape[2], shape[3]), order="F")
                else:
                    x[i] = (u * s[None, :]).reshape((shape[0], shape[1], keep), order="F")
                    x[i + 1] = vt.reshape((keep, shape[2], shape[3]), order="F")
                out["two_site_steps"] += 1
            else:
                c = nodes[0]
                left, right = _left(ops, x, c), _right(ops, x, c + 1)
                shape = x[c].shape

                def apply1(v):
                    return np_one_site_apply(left, right, ops[c], v.reshape(shape, order="F")).reshape(-1, order="F")
                x[c] = evolve(apply1, x[c].reshape(-1, order="F"), exponent).reshape(shape, order="F")
                out["corrections"] += 1
            cur = new_center
        sweeps = sweep + 1
    out["state"] = x
    out["sweeps_completed"] = sweeps
    return out


# ------------------------------------------------------------------------------------------------ the cases the CPU and the device tests share
TAU = -0.05
CASES = {  # name: site dimensions
    "heis6": (2,) * 6,
    "tfim6": (2,) * 6,
    "mixed3": (2, 3, 2),
    "n2": (3, 2),
}
DENSE_CHECKED = ("heis6", "tfim6", "mixed3")  # the cases of the issue; n2 (one edge) runs on the device as well
RUNS = [(order, end, 1) for order in (1, 2, 4) for end in (0, 1)] + [(1, 0, 2), (1, 1, 2)]  # (order, which end, nsweeps)

_CACHE = {}


def full_bonds(dims):
    n = len(dims)
    return [1] + [int(min(np.prod(dims[:i]), np.prod(dims[i:]))) for i in range(1, n)] + [1]


def make_case(name):
    """-> (operator sites, full-bond random start)"""
    dims = CASES[name]
    n = len(dims)
    if name.startswith("heis"):
        ops = heisenberg(n)
    elif name.startswith("tfim"):
        ops = tfim(n, 0.7)
    else:
        ops = symmetric_integer_operator(dims, 3, SEED ^ 0x7D ^ n)
    return ops, random_state(dims, full_bonds(dims), SEED ^ 0x7D0 ^ n)


def dense_exponential(name, tau):
    """exp(tau H) psi_0 from numpy's eigh, once per (case, tau)"""
    key = ("dense", name, tau)
    if key not in _CACHE:
        ops, init = make_case(name)
        h = np_operator_full(ops)
        lams, q = np.linalg.eigh(0.5 * (h + h.T))
        _CACHE[key] = q @ (np.exp(tau * lams) * (q.T @ np_state_full(init)))
    return _CACHE[key]


def restated(name, order, end, nsweeps=1, cgs2=False):
    """np_tdvp of the case from the centre 0 (end == 0) or n - 1 with tau = TAU, once"""
    key = (name, order, end, nsweeps, cgs2)
    if key not in _CACHE:
        ops, init = make_case(name)
        _CACHE[key] = np_tdvp(ops, init, 0 if end == 0 else len(ops) - 1, Options(nsweeps=nsweeps, order=order, exponent_step=TAU, cgs2=cgs2))
    return _CACHE[key]


def perturbed(init, seed):
    """every entry multiplied by 1 + 2^-50 u, u uniform in [-1, 1]"""
    rng = np.random.default_rng(seed)
    return [t * (1.0 + 2.0 ** -50 * rng.uniform(-1.0, 1.0, t.shape)) for t in init]


def relative_distance(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def spread_tolerance(run, init):
    """The tolerance of "device against restatement": run(init) -> dense state; three more runs with the start perturbed in its last
    bits (seeds 1, 2, 3); 100 times the largest relative distance, floor 1e-12 -> (tol, spread)."""
    base = run(init)
    spread = max(relative_distance(run(perturbed(init, s)), base) for s in (1, 2, 3))
    return max(100.0 * spread, 1e-12), spread


# the capped case: TFIM n = 8, g = 1, max_bond_dim = 4, 3 sweeps
CAPPED = {"n": 8, "g": 1.0, "max_bond_dim": 4, "nsweeps": 3, "tau": -0.05, "order": 2, "bond": 2, "seed": SEED ^ 0xCA8}


def capped_case():
    ops = tfim(CAPPED["n"], CAPPED["g"])
    n = CAPPED["n"]
    init = random_state((2,) * n, [1] + [CAPPED["bond"]] * (n - 1) + [1], CAPPED["seed"])
    return ops, init, Options(nsweeps=CAPPED["nsweeps"], order=CAPPED["order"], exponent_step=CAPPED["tau"], max_bond_dim=CAPPED["max_bond_dim"])


def capped_restated():
    if "capped" not in _CACHE:
        ops, init, o = capped_case()
        _CACHE["capped"] = np_tdvp(ops, init, 0, o)
    return _CACHE["capped"]


def dense_cases():
    """name -> (H, v0, tau, KrylovOptions): the matrices the device's krylov_expm_dense is run on as well"""
    n = 12
    v = lcg_matrix(n, SEED ^ 0xB)[:, 0].copy()
    big = lcg_matrix(40, SEED ^ 0x40)
    big = 0.5 * (big + big.T)
    vb = lcg_matrix(40, SEED ^ 0x41)[:, 0].copy()
    sym = lcg_matrix(n, SEED ^ 0x6E)
    sym = 0.5 * (sym + sym.T)
    _, vecs = np.linalg.eigh(sym)
    return {
        "diag3": (diag3_matrix(n), v, -0.3, KrylovOptions()),
        "eigenvector_start": (sym, 2.5 * vecs[:, 0], -0.3, KrylovOptions()),
        "tau_zero": (sym, v, 0.0, KrylovOptions()),
        "zero_start": (sym, np.zeros(n), -0.3, KrylovOptions()),
        "symmetric12": (sym, v, -0.3, KrylovOptions()),
        "symmetric40": (big, vb, 0.7, KrylovOptions()),
        "forced_split": (big, vb, -0.02, KrylovOptions(max_iter=2, tol=1e-3)),
    }


def failing_case():
    """max_time_splits = 1 with max_iter = 1 on a 40 x 40 matrix: the error"""
    big = lcg_matrix(40, SEED ^ 0x40)
    return 0.5 * (big + big.T), lcg_matrix(40, SEED ^ 0x41)[:, 0].copy(), -0.3, KrylovOptions(max_iter=1, max_time_splits=1)


def nonsymmetric_case():
    n = 12
    return 3.0 * np.eye(n) + lcg_matrix(n, SEED ^ 0x6E), lcg_matrix(n, SEED ^ 0xB)[:, 0].copy()
