"""numpy restatement of the partial contraction of two MPOs (t4a_gpu_mpo_partial_*): the plan, the site product by einsum, and the
three routes.  Factorize, right-canonicalisation, the zip-up recursion and the fit sweeps are those of tests/fit_np.py, used by
import; only the site product changes (np_partial_fit runs fit_np.np_fit itself with the two half products replaced).  Site tensors
are [left, leg 0, leg 1, right]; a pair is ((site, leg_a), (site, leg_b)).

The module also holds the operand sets the GPU tests compare ranks on (CASES, BIG): tests/test_cpu_partial.py asserts the gap
condition for exactly these, tests/test_gpu_partial.py runs them on the device."""
import contextlib
from unittest import mock

import numpy as np

import fit_np
from fit_np import SEED, Options, random_tensors, np_factorize, np_full, links  # noqa: F401  (re-exported)


class PlanError(ValueError):
    """INVALID_ARGUMENT of the plan; NotImplementedError stands for NOT_IMPLEMENTED"""


class SitePlan:
    """s_legs: the legs of A in no contract pair; diag: {leg of A: leg of B}; k_pairs: [(leg of A, leg of B)]; t_legs: free legs of B"""

    def __init__(self, a_dims, b_dims):
        self.a_dims, self.b_dims = tuple(a_dims), tuple(b_dims)
        self.s_legs, self.diag, self.k_pairs, self.t_legs = [], {}, [], []

    def finish(self, contract, diagonal):
        self.k_pairs = sorted(contract)
        self.diag = dict(diagonal)
        used_a = {la for la, _ in self.k_pairs}
        used_b = {lb for _, lb in self.k_pairs} | set(self.diag.values())
        self.s_legs = [leg for leg in (0, 1) if leg not in used_a]
        self.t_legs = [leg for leg in (0, 1) if leg not in used_b]
        self.S = int(np.prod([self.a_dims[leg] for leg in self.s_legs], dtype=np.int64))
        self.K = int(np.prod([self.a_dims[la] for la, _ in self.k_pairs], dtype=np.int64))
        self.T = int(np.prod([self.b_dims[leg] for leg in self.t_legs], dtype=np.int64))
        self.s_dims = [self.a_dims[leg] for leg in self.s_legs]
        self.t_dims = [self.b_dims[leg] for leg in self.t_legs]
        return self

    def letters(self):
        """einsum letters of the two legs of A and of B (a paired leg of B carries A's letter), and of the groups S and T"""
        la = ["p", "q"]
        lb = ["u", "v"]
        for x, y in self.k_pairs + list(self.diag.items()):
            lb[y] = la[x]
        return "".join(la), "".join(lb), "".join(la[x] for x in self.s_legs), "".join(lb[y] for y in self.t_legs)


def np_plan(a_dims, b_dims, contract_pairs=(), diagonal_pairs=(), output_order=None):
    """a_dims / b_dims: (leg 0, leg 1) per site -> [SitePlan]; the checks and their order are those of mpo_partial_plan"""
    if len(a_dims) != len(b_dims):
        raise PlanError(f"MPO length mismatch: expected {len(a_dims)}, got {len(b_dims)}")
    n = len(a_dims)
    seen_a, seen_b = set(), set()
    contract, diagonal = [[] for _ in range(n)], [[] for _ in range(n)]
    cross = None
    for kind, pairs, into in (("contract_pairs", contract_pairs, contract), ("diagonal_pairs", diagonal_pairs, diagonal)):
        for (sa, la), (sb, lb) in pairs:
            if sa >= n or la > 1:
                raise PlanError(f"partial_contract: (site {sa}, leg {la}) from {kind} not found in first MPO external indices")
            if sb >= n or lb > 1:
                raise PlanError(f"partial_contract: (site {sb}, leg {lb}) from {kind} not found in second MPO external indices")
            da, db = a_dims[sa][la], b_dims[sb][lb]
            if da != db:
                raise PlanError(f"partial_contract: {kind} index shape mismatch: {da} != {db}")
            if (sa, la) in seen_a:
                raise PlanError(f"partial_contract: first MPO index (site {sa}, leg {la}) appears in multiple pairs")
            if (sb, lb) in seen_b:
                raise PlanError(f"partial_contract: second MPO index (site {sb}, leg {lb}) appears in multiple pairs")
            seen_a.add((sa, la))
            seen_b.add((sb, lb))
            if sa != sb:
                cross = cross or ((sa, la), (sb, lb))
                continue
            into[sa].append((la, lb))
    if cross:
        raise NotImplementedError(f"partial_contract: the pair (site {cross[0][0]}, leg {cross[0][1]}) - (site {cross[1][0]}, leg "
                                  f"{cross[1][1]}) joins two sites; moving a site index (swap_site_indices) is not implemented")
    if output_order is not None:
        raise NotImplementedError("partial_contract: output_order is not implemented (it needs swap_site_indices)")
    plan = [SitePlan(a_dims[i], b_dims[i]).finish(contract[i], diagonal[i]) for i in range(n)]
    for i, p in enumerate(plan):
        if p.S * p.T > 65535:
            raise PlanError(f"partial_contract: site {i}: dimensions above 65535 are not supported")
    return plan


def plan_for(a, b, contract_pairs=(), diagonal_pairs=()):
    return np_plan([t.shape[1:3] for t in a], [t.shape[1:3] for t in b], contract_pairs, diagonal_pairs)


def matrix_product_pairs(n):
    return [((i, 1), (i, 0)) for i in range(n)]


def hadamard_pairs(n):
    return [((i, leg), (i, leg)) for i in range(n) for leg in (0, 1)]


def np_site(a, b, sp):
    """C[(la*Lb+lb), s, t, (ra*Rb+rb)] = sum_kappa A[la, x(s, kappa), ra] B[lb, y(s, kappa, t), rb]"""
    xa, xb, s, t = sp.letters()
    c = np.einsum(f"a{xa}r,b{xb}z->ba{s}{t}zr", a, b)
    return c.reshape((a.shape[0] * b.shape[0], sp.S, sp.T, a.shape[3] * b.shape[3]), order="F")


def np_half_left(env, x, y, sp):
    """P[n, s, t, c, d] = sum L[n, a, b] A[a, ., c] B[b, ., d]"""
    xa, xb, s, t = sp.letters()
    p = np.einsum(f"nab,a{xa}c,b{xb}d->n{s}{t}cd", env, x, y)
    return p.reshape((env.shape[0], sp.S, sp.T, x.shape[3], y.shape[3]), order="F")


def np_half_right(env, x, y, sp):
    """Q[a, b, s, t, n] = sum A[a, ., c] B[b, ., d] R[c, d, n]"""
    xa, xb, s, t = sp.letters()
    q = np.einsum(f"a{xa}c,b{xb}d,cdn->ab{s}{t}n", x, y, env)
    return q.reshape((x.shape[0], y.shape[0], sp.S, sp.T, env.shape[2]), order="F")


def np_partial_naive(a, b, plan, options=None):
    """the exact site-wise product, or (options given) compress_mpo of it: right-canonicalise, then the left-to-right SVD sweep"""
    ts = [np_site(x, y, sp) for x, y, sp in zip(a, b, plan)]
    if options is None or len(ts) <= 1:
        return ts
    ts = fit_np.np_right_canonicalize(ts)
    for i in range(len(ts) - 1):
        l, s1, s2, r = ts[i].shape
        u, s, vt, rank = fit_np.np_factorize(ts[i].reshape((l * s1 * s2, r), order="F"), options.tolerance, options.max_bond_dim)
        ts[i] = u.reshape((l, s1, s2, rank), order="F")
        ts[i + 1] = np.einsum("lk,ksqr->lsqr", s[:, None] * vt, ts[i + 1])
    return ts


def np_partial_zipup(a, b, plan, options):
    """fit_np.np_zipup with the site step replaced"""
    rem = np.ones((1, 1, 1))
    out = []
    for i, (x, y, sp) in enumerate(zip(a, b, plan)):
        c = np_half_left(rem, x, y, sp)
        n0, s1, t, ca, cb = c.shape
        if i == len(a) - 1:
            out.append(c.reshape((n0, s1, t, 1), order="F"))
            break
        u, s, vt, rank = fit_np.np_factorize(c.reshape((n0 * s1 * t, ca * cb), order="F"), options.tolerance, options.max_bond_dim)
        out.append(u.reshape((n0, s1, t, rank), order="F"))
        rem = (s[:, None] * vt).reshape((rank, ca, cb), order="F")
    return out


class _Planned:
    """a site of B together with its plan: what fit_np.np_fit hands to the half products as `b[i]`"""

    def __init__(self, y, sp):
        self.y, self.sp = y, sp


def np_partial_fit(a, b, plan, options=None, initial=None):
    """fit_np.np_fit, run as it is: its half products and its initialiser are replaced for the duration of the call"""
    o = Options() if options is None else options
    info = {"n_sweeps": 0, "norms": []}
    if len(a) == 0:
        return [], info
    if len(a) == 1:
        return [np_site(a[0], b[0], plan[0])], info
    pb = [_Planned(y, sp) for y, sp in zip(b, plan)]
    with contextlib.ExitStack() as stack:
        stack.enter_context(mock.patch.object(fit_np, "np_half_left", lambda env, x, y: np_half_left(env, x, y.y, y.sp)))
        stack.enter_context(mock.patch.object(fit_np, "np_half_right", lambda env, x, y: np_half_right(env, x, y.y, y.sp)))
        stack.enter_context(mock.patch.object(fit_np, "np_zipup", lambda x, y, opt: np_partial_zipup(x, [s.y for s in y], plan, opt)))
        return fit_np.np_fit(a, pb, o, initial)


# ------------------------------------------------------------------------------------------------ the gap condition
class GapLog:
    """Records every factorize of a restatement run.  ok(): at every split the singular values stay a factor 100 clear of
    tolerance * s_max on both sides, and no cap cuts inside a pair of values closer than a factor 1 + 1e-6."""

    def __init__(self):
        self.splits = []

    @contextlib.contextmanager
    def recording(self):
        inner = fit_np.np_factorize

        def logged(mat, tol, cap):
            self.splits.append((np.linalg.svd(mat, compute_uv=False), tol, cap))
            return inner(mat, tol, cap)

        with mock.patch.object(fit_np, "np_factorize", logged):
            yield self

    def violations(self):
        bad = []
        for k, (s, tol, cap) in enumerate(self.splits):
            if s.size == 0 or s.max() == 0.0:
                continue
            cut = tol * s.max()
            if tol > 0.0:
                # the rank rule stops at the cap before it looks at a value behind it: only the first `cap` values can decide
                for v in s if cap is None else s[:cap]:
                    if cut / 100.0 < v < cut * 100.0:
                        bad.append((k, "tolerance", float(v / cut)))
            kept = int((s >= cut).sum()) if tol > 0.0 else s.size
            if cap is not None and cap < kept and s[cap] > 0.0 and s[cap - 1] / s[cap] < 1.0 + 1e-6:
                bad.append((k, "cap", float(s[cap - 1] / s[cap])))
        return bad

    def ok(self):
        return not self.violations()


# ------------------------------------------------------------------------------------------------ the operand sets of the GPU tests
TOL_CAP = [(1e-12, None), (1e-6, None), (0.0, 3), (1e-3, 4)]


def _mixed(n):  # f(x, y) g(y, z) with y kept on even sites and summed on odd ones
    return {"contract_pairs": [((i, 1), (i, 0)) for i in range(n) if i % 2], "diagonal_pairs": [((i, 1), (i, 0)) for i in range(n) if i % 2 == 0]}


# The seeds were picked on the CPU so that the gap condition holds for every route and every (tolerance, cap) pair below.
# name -> (bonds of A, (leg dims of A), bonds of B, (leg dims of B), seeds, spec); 4 sites, site dims 2 and 3, bonds up to 6
CASES = {
    "hadamard": ([1, 3, 6, 3, 1], (2, 3), [1, 2, 4, 2, 1], (2, 3), (SEED ^ 0x101, SEED ^ 0x102), {"diagonal_pairs": hadamard_pairs(4)}),
    "mixed": ([1, 3, 5, 3, 1], (2, 3), [1, 2, 6, 2, 1], (3, 2), (SEED ^ 0x1, SEED ^ 0x2), _mixed(4)),
    "diag0_contract1": ([1, 2, 4, 3, 1], (3, 2), [1, 3, 3, 2, 1], (3, 2), (SEED ^ 0x1, SEED ^ 0x2),
                        {"contract_pairs": [((i, 1), (i, 1)) for i in range(4)], "diagonal_pairs": [((i, 0), (i, 0)) for i in range(4)]}),
}
# one case at bonds 17 x 18: MFMA tiles and ragged edges inside the drivers
BIG = ([1, 6, 17, 6, 1], (2, 3), [1, 6, 18, 6, 1], (2, 3), (SEED ^ 0x1, SEED ^ 0x2), {"diagonal_pairs": hadamard_pairs(4)})
BIG_OPTIONS = (1e-8, 40)


def case_operands(case):
    bonds_a, dims_a, bonds_b, dims_b, seeds, spec = case
    a = random_tensors(bonds_a, dims_a[0], dims_a[1], seeds[0])
    b = random_tensors(bonds_b, dims_b[0], dims_b[1], seeds[1])
    return a, b, spec, plan_for(a, b, spec.get("contract_pairs", ()), spec.get("diagonal_pairs", ()))


def fit_options(tol, cap):
    return Options(tolerance=tol, max_bond_dim=cap, max_sweeps=2, convergence_tol=0.0)
