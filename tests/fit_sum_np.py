"""numpy restatement of fit_sum (tensor4all-treetn/src/treetn/fit.rs:1521-1644) on a chain, followed literally: validation in the
reference's order, the short-circuits, the forced QR canonicalisation onto `center`, one PRIVATE environment set per target
(SumFitEnvironment), the Euler tour of two-site steps from `center` (the second node of a step the new centre), the local optimum
accumulated target by target (SumFitUpdater::update), the Canonical::Left split with the bond cap of fit_two_site_update
(fit.rs:691-703) and the rank rule of svd_with, the invalidation of after_step and the stop test of run_fit_sweeps.  The project's two
extensions are restated as well: coefficients (site 0 of a target scaled once) and initial=None (a copy of targets[0]).
A train is a list of site tensors (l, s, r); an MPO (l, s1, s2, r) is fused to s1 + S1 s2 by fuse() and restored by unfuse().
The library keeps the environments of all targets concatenated in one matrix; this file does not, which is what makes it a check.
The case list of the truncating GPU tests lives here (CASES), with the gap condition tests/test_cpu_fit_sum.py asserts on it.
No device, no library."""
import numpy as np

from patching_np import svd_retained_rank, margin, DEFAULT_POLICY

SEED = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
SVD, QR, LU, CI = 0, 1, 2, 3


class Options:
    """FitOptions::new(1) with the builder names as keywords; svd_policy is (threshold, scale, measure, rule) or None"""

    def __init__(self, nfullsweeps=1, max_bond_dim=None, svd_policy=None, qr_rtol=None, factorize_alg=SVD, convergence_tol=None):
        self.nfullsweeps = nfullsweeps
        self.max_bond_dim = max_bond_dim
        self.svd_policy = svd_policy
        self.qr_rtol = qr_rtol
        self.factorize_alg = factorize_alg
        self.convergence_tol = convergence_tol


def _tol_ok(v):
    return np.isfinite(v) and v >= 0


def validate_options(o):
    """validate_fit_sum_options (fit.rs:1451-1473) and FactorizeOptions::validate (tensor_like.rs:397-436)"""
    if o.convergence_tol is not None and not _tol_ok(o.convergence_tol):
        raise ValueError("convergence tolerance must be finite and non-negative")
    if o.qr_rtol is not None and not _tol_ok(o.qr_rtol):
        raise ValueError("QR relative tolerance must be finite and non-negative")
    if o.max_bond_dim is not None and o.max_bond_dim == 0:
        raise ValueError("max_bond_dim must be at least 1")
    if o.svd_policy is not None and not _tol_ok(o.svd_policy[0]):
        raise ValueError("SVD truncation threshold must be finite and non-negative")
    if o.factorize_alg == SVD:
        if o.qr_rtol is not None:
            raise ValueError("SVD factorization does not accept qr_rtol")
    elif o.factorize_alg == QR:
        if o.svd_policy is not None:
            raise ValueError("QR factorization does not accept svd_policy")
    else:
        if o.svd_policy is not None:
            raise ValueError("LU/CI factorization does not accept svd_policy")
        if o.qr_rtol is not None:
            raise ValueError("LU/CI factorization does not accept qr_rtol")
    if o.factorize_alg != SVD:
        raise NotImplementedError("only the SVD factorization is restated")


def random_train(bonds, site, seed):
    """an LCG fills every site tensor column-major (random_mpo of test_support.rs:8-44 with one site leg); site: an int or one per site"""
    state = seed & MASK
    out = []
    sites = [site] * (len(bonds) - 1) if isinstance(site, int) else list(site)
    for left, right, s in zip(bonds[:-1], bonds[1:], sites):
        vals = []
        for _ in range(left * s * right):
            state = (state * 6364136223846793005 + 1442695040888963407) & MASK
            vals.append((state >> 33) / float(1 << 31) - 0.5)
        out.append(np.array(vals).reshape((left, s, right), order="F"))
    return out


def full_bonds(n, site):
    """min(S^i, S^(n-i)): the bonds at which a chain holds every tensor"""
    return [min(site ** i, site ** (n - i)) for i in range(n + 1)]


def fuse(mpo):
    return [t.reshape((t.shape[0], t.shape[1] * t.shape[2], t.shape[3]), order="F") for t in mpo]


def unfuse(train, site_dims):
    return [t.reshape((t.shape[0], s1, s2, t.shape[2]), order="F") for t, (s1, s2) in zip(train, site_dims)]


def np_full(ts):
    """dense tensor indexed [s_1, .., s_n]"""
    acc = ts[0][0]
    for t in ts[1:]:
        acc = np.tensordot(acc, t, axes=([-1], [0]))
    return acc[..., 0]


def np_sum(targets, coefficients=None):
    w = [1.0] * len(targets) if coefficients is None else list(coefficients)
    return sum(wk * np_full(t) for wk, t in zip(w, targets))


def scale_of(targets, coefficients=None):
    """sum_k |w_k| |T_k|_F: what the deviations of the exact cases are measured against"""
    w = [1.0] * len(targets) if coefficients is None else list(coefficients)
    return float(sum(abs(wk) * np.linalg.norm(np_full(t)) for wk, t in zip(w, targets)))


def links(ts):
    return [t.shape[0] for t in ts[1:]]


def np_canonicalize(x, center):
    """QrSweep::canonicalize: thin QR from the left up to `center`, then from the right down to it"""
    x = [t.copy() for t in x]
    for i in range(center):
        l, s, r = x[i].shape
        q, rr = np.linalg.qr(x[i].reshape((l * s, r), order="F"))
        x[i] = q.reshape((l, s, q.shape[1]), order="F")
        x[i + 1] = np.einsum("kl,lsr->ksr", rr, x[i + 1])
    for i in range(len(x) - 1, center, -1):
        l, s, r = x[i].shape
        q, rr = np.linalg.qr(x[i].reshape((l, s * r), order="F").T)
        x[i] = q.T.reshape((q.shape[1], s, r), order="F")
        x[i - 1] = np.einsum("lsr,kr->lsk", x[i - 1], rr)
    return x


def sweep_plan(n, center):
    """[(bond, move_right)]: LocalUpdateSweepPlan::from_treetn(psi, center, 2) on a chain"""
    return ([(i, True) for i in range(center, n - 1)] + [(i, False) for i in range(n - 2, -1, -1)] + [(i, True) for i in range(center)])


def check_shapes(targets, initial, center):
    """the shape answers of fit_sum in its order; dimension lists or tensors"""
    def dims(t):
        return [tuple(x.shape) if hasattr(x, "shape") else tuple(x) for x in t]
    if len(targets) == 0:
        raise ValueError("fit_sum: targets must not be empty")
    tds = [dims(t) for t in targets]
    init = tds[0] if initial is None else dims(initial)
    if len(init) == 0:
        raise ValueError("fit_sum: initial TreeTN must not be empty")
    if center >= len(init):
        raise ValueError("fit_sum: center node is not in initial TreeTN")
    for k, t in enumerate(tds):
        if len(t) == 0:
            raise ValueError(f"fit_sum: target {k} TreeTN must not be empty")
        if len(t) != len(init):
            raise ValueError(f"fit_sum: target {k} has an incompatible named topology")
        if any(a[1] != b[1] for a, b in zip(t, init)):
            raise ValueError(f"fit_sum: target {k} site-space validation failed")


def np_fit_sum(targets, initial=None, center=0, options=None, coefficients=None, log=None):
    """-> (site tensors, {"sweeps_completed", "local_updates", "converged", "link_dims", "norms"}).
    log (a list, optional) receives (bond, singular values, kept, policy or None, cap or None) of every split."""
    o = Options() if options is None else options
    validate_options(o)
    check_shapes(targets, initial, center)
    info = {"sweeps_completed": 0, "local_updates": 0, "converged": False, "norms": []}
    start = [t.copy() for t in (targets[0] if initial is None else initial)]
    n = len(start)

    def done(ts):
        info["link_dims"] = links(ts)
        return ts, info

    if o.nfullsweeps == 0:
        return done(start)
    tg = [[t.copy() for t in tk] for tk in targets]
    if coefficients is not None:
        for tk, w in zip(tg, coefficients):
            if w != 1.0:
                tk[0] = tk[0] * w
    if n == 1:
        acc = None
        for tk in tg:
            acc = tk[0].copy() if acc is None else 1.0 * acc + 1.0 * tk[0]
        return done([acc])
    psi = np_canonicalize(start, center)
    K = len(tg)
    # envs[k][("L", i)]: (c_i, a_i) of the sites < i; envs[k][("R", i)]: (a_i, c_i) of the sites >= i
    envs = [{("L", 0): np.ones((1, 1)), ("R", n): np.ones((1, 1))} for _ in range(K)]

    def left_env(k, i):
        e = envs[k]
        if ("L", i) not in e:
            e[("L", i)] = np.einsum("ca,csd,asb->db", left_env(k, i - 1), psi[i - 1], tg[k][i - 1])
        return e[("L", i)]

    def right_env(k, i):
        e = envs[k]
        if ("R", i) not in e:
            e[("R", i)] = np.einsum("asb,csd,bd->ac", tg[k][i], psi[i], right_env(k, i + 1))
        return e[("R", i)]

    for k in range(K):  # SumFitEnvironment::prepare: towards the centre
        for i in range(1, center + 1):
            left_env(k, i)
        for i in range(n - 1, center, -1):
            right_env(k, i)

    def step(i, move_right):
        theta = None
        for k in range(K):
            contribution = np.einsum("ca,asb,btd,de->cste", left_env(k, i), tg[k][i], tg[k][i + 1], right_env(k, i + 2))
            theta = contribution if theta is None else 1.0 * theta + 1.0 * contribution
        c, s1, s2, cn = theta.shape
        if o.max_bond_dim is not None:
            cap = o.max_bond_dim
        elif o.svd_policy is not None or o.qr_rtol is not None:
            cap = None
        else:
            cap = psi[i].shape[2]
        u, s, vt = np.linalg.svd(theta.reshape((c * s1, s2 * cn), order="F"), full_matrices=False)
        policy = DEFAULT_POLICY if o.svd_policy is None else tuple(o.svd_policy)
        keep = svd_retained_rank(s, policy)
        if cap is not None:
            keep = min(keep, cap)
        keep = max(min(keep, len(s)), 1)
        if log is not None:
            log.append((i, s.copy(), keep, policy, cap))
        u, s, vt = u[:, :keep], s[:keep], vt[:keep]
        if move_right:  # nodes (i, i + 1): the isometry on i, S Vt on the new centre i + 1
            psi[i] = u.reshape((c, s1, keep), order="F")
            psi[i + 1] = (s[:, None] * vt).reshape((keep, s2, cn), order="F")
        else:           # nodes (i + 1, i): the isometry on i + 1, U S on the new centre i
            psi[i] = (u * s[None, :]).reshape((c, s1, keep), order="F")
            psi[i + 1] = vt.reshape((keep, s2, cn), order="F")
        for e in envs:  # after_step: every environment that contains a node of the step
            for key in [kk for kk in e if (kk[0] == "L" and kk[1] > i) or (kk[0] == "R" and 1 <= kk[1] <= i + 1)]:
                del e[key]
        info["local_updates"] += 1

    def log_norm():
        with np.errstate(divide="ignore"):
            return float(np.log(np.linalg.norm(psi[center])))

    plan = sweep_plan(n, center)
    for _ in range(o.nfullsweeps):
        before = log_norm() if o.convergence_tol is not None else None
        for i, move_right in plan:
            step(i, move_right)
        info["sweeps_completed"] += 1
        info["norms"].append(float(np.linalg.norm(psi[center])))
        if o.convergence_tol is not None:
            with np.errstate(invalid="ignore"):
                change = abs(np.exp(log_norm() - before) - 1.0)
            info.setdefault("changes", []).append(float(change))
            if change < o.convergence_tol:
                info["converged"] = True
                break
    return done(psi)


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def exact_case(n, site, K, coefficients=None, cancel=False, seed=SEED):
    """targets of bond 3 (2 next to the ends), an initial with full bonds: one sweep returns the sum"""
    tb = [1] + [min(3, b) for b in full_bonds(n, site)[1:-1]] + [1]
    targets = [random_train(tb, site, seed ^ (0x51 * (k + 1))) for k in range(K)]
    if cancel:
        targets = [targets[0], [t.copy() for t in targets[0]]]
        coefficients = [1.0, -1.0]
    initial = random_train(full_bonds(n, site), site, seed ^ 0xABCDEF)
    return targets, initial, coefficients


EXACT = [(n, site, K) for n in (4, 5) for site in (2, 3) for K in (1, 3)]

# name -> (targets, initial, center, Options, coefficients): the truncating cases.  Each is checked for the gap condition.
def _cases():
    c = {}
    t = [random_train([1, 2, 3, 3, 3, 2, 1], 2, SEED ^ (0x77 * (k + 1))) for k in range(3)]
    c["cap"] = (t, random_train([1, 2, 2, 2, 2, 2, 1], 2, SEED ^ 0x1234), 2, Options(nfullsweeps=2, max_bond_dim=3), None)
    c["policy"] = (t, random_train([1] * 7, 2, SEED ^ 0x4321), 0, Options(nfullsweeps=2, svd_policy=(0.2, 0, 0, 0)), [1.0, 0.5, -2.0])
    c["stop"] = (t, random_train([1, 2, 2, 2, 2, 2, 1], 2, SEED ^ 0x1234), 3, Options(nfullsweeps=12, max_bond_dim=2, convergence_tol=1e-4), None)
    t40 = [random_train([1, 2, 2, 2, 2, 2, 2, 2, 1], 2, SEED ^ (0x3D * (k + 1))) for k in range(40)]
    c["k40"] = (t40, None, 4, Options(nfullsweeps=2, max_bond_dim=8), None)
    return c


CASES = _cases()
GAP = 1e-6


def gaps(log):
    """per split that cut something: the relative gap of the singular values at the cut and the margin of the policy's decision"""
    out = []
    for i, s, keep, policy, cap in log:
        if keep < len(s) and s[0] > 0:
            out.append(((s[keep - 1] - s[keep]) / s[0], margin(s, policy) if (cap is None or svd_retained_rank(s, policy) <= cap) else np.inf))
    return out
