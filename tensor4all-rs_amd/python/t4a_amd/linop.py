"""An operator applied to a state when it acts on a subset of the state's sites (tensor4all-treetn/src/operator/: apply.rs,
compose.rs, identity.rs), on a chain and by position.

``LinearOperator(mpo, sites)`` is an ``MPO`` (or a ``QuanticsOperator``) of ``k`` sites ``O_j[a, y, x, a']`` (leg 0 the output, leg 1
the input) together with its ``k`` strictly ascending state positions; ``sites=None`` is full coverage.  A state site the operator
does not act on is a *bridge* (between two operator sites: the operator bond passes through unchanged) or lies *outside* (operator
bond 1).  ``apply_linear_operator`` mirrors the reference's function with ``ApplyOptions.zipup() / fit() / naive()``; the result's
bonds are fused with the operator index slow and the state index fast.  ``route="fused"`` runs the kernels of
``csrc/kernels_apply.hip`` and never forms an identity; ``route="composed"`` builds the full-length operator
(``extend_operator_to_full_space``) and runs the MPO-MPO contraction; ``"auto"`` follows the measured table.
``are_exclusive_operators`` and ``compose_exclusive_linear_operators`` are compose.rs for a chain.

Not mirrored: an MPO as the state, several site indices per node, index rebinding (positions replace index objects), trees, complex
scalars.  ``quanticstransform.apply`` keeps its own code.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, NOT_IMPLEMENTED, SimpleTensorTrain, SvdTruncationPolicy, RELATIVE, VALUE, PER_VALUE,
               c_size_t, c_double, c_int32, c_void_p)
from .mpo import MPO
from .quanticstransform import QuanticsOperator

ROUTES = {"auto": 0, "fused": 1, "composed": 2}
KINDS = ("op", "bridge", "outside")


class ContractionMethod:
    """ContractionMethod of apply.rs as this layer numbers it"""
    Naive, Zipup, Fit = 0, 1, 2


class ApplyOptionsC(ctypes.Structure):
    """t4a_gpu_linop_options"""
    _fields_ = [("method", c_int32), ("tolerance", c_double), ("has_max_bond_dim", c_int32), ("max_bond_dim", c_size_t), ("nfullsweeps", c_size_t),
                ("has_convergence_tol", c_int32), ("convergence_tol", c_double)]


class ApplyOptions:
    """ApplyOptions (apply.rs:137-220); the defaults are ApplyOptions::default() (zip-up).  Mapped onto the options of the MPO
    contraction: ``svd_policy=None`` is the project's tolerance 1e-12, a relative per-value policy on the values with threshold ``t``
    becomes ``tolerance = t`` (the MPO rank rule holds where it differs from svd_retained_rank: a value equal to the cutoff is kept,
    and one value is always kept), every other policy answers NOT_IMPLEMENTED.  ``qr_rtol`` is validated and unused (zip-up and fit
    factorise by SVD only), ``nfullsweeps`` is the fit's ``max_sweeps``, ``convergence_tol=None`` runs every sweep."""

    def __init__(self, method=ContractionMethod.Zipup, max_bond_dim=None, svd_policy=None, qr_rtol=None, nfullsweeps=1, convergence_tol=None):
        self.method = method
        self.max_bond_dim = max_bond_dim
        self.svd_policy = svd_policy
        self.qr_rtol = qr_rtol
        self.nfullsweeps = nfullsweeps
        self.convergence_tol = convergence_tol

    @classmethod
    def zipup(cls):
        return cls()

    @classmethod
    def fit(cls):
        return cls(method=ContractionMethod.Fit)

    @classmethod
    def naive(cls):
        return cls(method=ContractionMethod.Naive)

    def _with(self, **kw):
        o = ApplyOptions(self.method, self.max_bond_dim, self.svd_policy, self.qr_rtol, self.nfullsweeps, self.convergence_tol)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def with_max_bond_dim(self, max_bond_dim):
        return self._with(max_bond_dim=max_bond_dim)

    def with_svd_policy(self, policy):
        return self._with(svd_policy=policy)

    def with_qr_rtol(self, rtol):
        return self._with(qr_rtol=rtol)

    def with_nfullsweeps(self, nfullsweeps):
        return self._with(nfullsweeps=nfullsweeps)

    def with_convergence_tol(self, tol):
        return self._with(convergence_tol=tol)

    def tolerance(self):
        """the tolerance of the MPO rank rule this svd_policy maps onto"""
        p = self.svd_policy
        if p is None:
            return 1e-12
        if not isinstance(p, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "ApplyOptions::svd_policy must be an SvdTruncationPolicy")
        if (p.scale, p.measure, p.rule) != (RELATIVE, VALUE, PER_VALUE):
            name = (f"SvdTruncationPolicy(scale={'Relative' if p.scale == RELATIVE else 'Absolute'}, "
                    f"measure={'Value' if p.measure == VALUE else 'SquaredValue'}, rule={'PerValue' if p.rule == PER_VALUE else 'DiscardedTailSum'})")
            raise T4aError(NOT_IMPLEMENTED, f"apply_linear_operator: the svd policy {name} is not implemented; only a relative per-value "
                                            "policy on the values maps onto the MPO rank rule")
        t = float(p.threshold)
        if not (np.isfinite(t) and t >= 0.0):
            raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: the svd policy's threshold must be finite and not negative")
        return t

    def to_c(self):
        if self.method not in (0, 1, 2):
            raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: unknown method")
        tol = self.tolerance()
        if self.max_bond_dim is not None and int(self.max_bond_dim) < 1:
            raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: max_bond_dim must be at least 1")
        if self.qr_rtol is not None and not (np.isfinite(float(self.qr_rtol)) and float(self.qr_rtol) >= 0.0):
            raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: qr_rtol must be finite and not negative")
        if int(self.nfullsweeps) < 0:
            raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: nfullsweeps must not be negative")
        ct = self.convergence_tol
        if ct is not None and not (np.isfinite(float(ct)) and float(ct) >= 0.0):
            raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: convergence_tol must be finite and not negative")
        return ApplyOptionsC(int(self.method), tol, 0 if self.max_bond_dim is None else 1, 0 if self.max_bond_dim is None else int(self.max_bond_dim),
                             int(self.nfullsweeps), 0 if ct is None else 1, 0.0 if ct is None else float(ct))


def _usz(values):
    a = np.asarray(list(values), dtype=np.int64).reshape(-1)
    if (a < 0).any():
        raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: positions and dimensions must not be negative")
    return np.ascontiguousarray(a.astype(np.uintp))


def _ptr(a):
    return _p(a) if a.size else None


class LinearOperator:
    """An operator and the state positions of its sites.  ``mpo``: an ``MPO`` or a ``QuanticsOperator``; ``sites=None``: site j acts on
    position j (full coverage when the lengths agree)."""

    def __init__(self, mpo, sites=None):
        if not isinstance(mpo, (MPO, QuanticsOperator)):
            raise T4aError(INVALID_ARGUMENT, "LinearOperator: the operator must be an MPO or a QuanticsOperator")
        self._op = mpo
        k = len(mpo)
        self.sites = tuple(range(k)) if sites is None else tuple(int(s) for s in sites)
        if any(s < 0 for s in self.sites):
            raise T4aError(INVALID_ARGUMENT, "LinearOperator: sites must not be negative")

    def mpo(self):
        return self._op.mpo() if isinstance(self._op, QuanticsOperator) else self._op

    def dims(self):
        return self._op.dims()

    def __len__(self):
        return len(self._op)


def _as_operator(operator):
    return operator if isinstance(operator, LinearOperator) else LinearOperator(operator)


def apply_plan(op_dims, sites, state_dims):
    """The plan of an apply on plain dimension lists (t4a_gpu_linop_plan), host only.  op_dims: (left, out, in, right) per operator
    site; sites: their state positions; state_dims: (left, site, right) per state site -> {"kinds": ["op" | "bridge" | "outside"],
    "bonds": [(operator bond left, right)], "result_dims": [(left, site, right)]}."""
    od = _usz(x for d in op_dims for x in d)
    sd = _usz(x for d in state_dims for x in d)
    st = _usz(sites)
    n = len(state_dims)
    kinds = np.zeros(max(n, 1), dtype=np.int32)
    bonds = np.zeros(max(2 * n, 1), dtype=np.uintp)
    res = np.zeros(max(3 * n, 1), dtype=np.uintp)
    _check(_lib.t4a_gpu_linop_plan(_ptr(od), c_size_t(len(op_dims)), _ptr(st), c_size_t(st.size), _ptr(sd), c_size_t(n),
                                   kinds.ctypes.data_as(ctypes.POINTER(c_int32)), _p(bonds), _p(res)))
    return {"kinds": [KINDS[k] for k in kinds[:n]], "bonds": [(int(a), int(b)) for a, b in bonds[:2 * n].reshape(-1, 2)],
            "result_dims": [tuple(int(x) for x in r) for r in res[:3 * n].reshape(-1, 3)]}


def apply_route(method, n_sites, n_gap_sites, state_bond, op_bond):
    """The route ``auto`` takes (t4a_gpu_linop_route), host only -> 'fused' or 'composed'."""
    r = c_int32(0)
    _check(_lib.t4a_gpu_linop_route(c_int32(int(method)), c_size_t(n_sites), c_size_t(n_gap_sites), c_size_t(state_bond), c_size_t(op_bond),
                                    ctypes.byref(r)))
    return {v: k for k, v in ROUTES.items()}[r.value]


def apply_linear_operator(operator, state, options=None, route="auto", initial=None, return_info=False):
    """apply_linear_operator (apply.rs:306): ``operator`` (a LinearOperator, an MPO or a QuanticsOperator) on the SimpleTensorTrain
    ``state`` -> SimpleTensorTrain.  ``options``: an ApplyOptions, default zip-up; ``initial``: the train the fit starts from (default
    the zip-up result).  ``return_info=True`` gives ``(train, info)`` with info ``{"route", "n_sweeps", "norms", "link_dims"}``: norms[0]
    belongs to the start of the fit, norms[k] to sweep k."""
    op = _as_operator(operator)
    if not isinstance(state, SimpleTensorTrain):
        raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: the state must be a SimpleTensorTrain")
    if initial is not None and not isinstance(initial, SimpleTensorTrain):
        raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: initial must be a SimpleTensorTrain")
    if route not in ROUTES:
        raise T4aError(INVALID_ARGUMENT, "apply_linear_operator: route must be 'auto', 'fused' or 'composed'")
    o = (ApplyOptions() if options is None else options).to_c()
    st = _usz(op.sites)
    h = c_void_p()
    n_sweeps, taken = c_size_t(0), c_int32(0)
    norms = np.full(int(o.nfullsweeps) + 1, np.nan)
    _check(_lib.t4a_gpu_linop_apply(op.mpo()._h, _ptr(st), c_size_t(st.size), state._h, ctypes.byref(o), c_int32(ROUTES[route]),
                                    None if initial is None else initial._h, ctypes.byref(h), ctypes.byref(n_sweeps), _p(norms), ctypes.byref(taken)))
    out = SimpleTensorTrain._adopt(h)
    if not return_info:
        return out
    k = n_sweeps.value
    return out, {"route": {v: q for q, v in ROUTES.items()}[taken.value], "n_sweeps": k, "norms": [float(v) for v in norms[:k + 1]] if k else [],
                 "link_dims": out.link_dims()}


def extend_operator_to_full_space(operator, state_site_dims):
    """The full-length ``MPO`` of ``operator`` on a state with these site dims (t4a_gpu_linop_extend): operator sites are device
    copies, bridge sites ``delta_{aa'} delta_{yx}`` of shape (m, d, d, m), outside sites (1, d, d, 1) identities."""
    op = _as_operator(operator)
    st, sd = _usz(op.sites), _usz(state_site_dims)
    h = c_void_p()
    _check(_lib.t4a_gpu_linop_extend(op.mpo()._h, _ptr(st), c_size_t(st.size), _ptr(sd), c_size_t(sd.size), ctypes.byref(h)))
    return MPO._adopt(h)


def _supports(operators):
    sites = [tuple(o.sites) if isinstance(o, LinearOperator) else tuple(int(s) for s in o) for o in operators]
    flat = _usz(s for t in sites for s in t)
    lens = _usz(len(t) for t in sites)
    return flat, lens


def are_exclusive_operators(n, operators):
    """are_exclusive_operators (compose.rs) on a chain of ``n`` sites, host only: the supports (LinearOperators or plain lists of
    positions) are disjoint and each is contiguous, so no path between two sites of one operator crosses another."""
    flat, lens = _supports(operators)
    r = c_int32(0)
    _check(_lib.t4a_gpu_linop_exclusive(c_size_t(int(n)), _ptr(flat), _ptr(lens), c_size_t(lens.size), ctypes.byref(r)))
    return bool(r.value)


def compose_exclusive_linear_operators(state_site_dims, operators):
    """compose_exclusive_linear_operators (compose.rs:190) -> a full-length LinearOperator, gaps identities with bond 1."""
    ops = [_as_operator(o) for o in operators]
    flat, lens = _supports(ops)
    sd = _usz(state_site_dims)
    mpos = [o.mpo() for o in ops]
    hs = (c_void_p * max(len(ops), 1))(*[m._h for m in mpos])
    h = c_void_p()
    _check(_lib.t4a_gpu_linop_compose(_ptr(sd), c_size_t(sd.size), hs, _ptr(flat), _ptr(lens), c_size_t(len(ops)), ctypes.byref(h)))
    return LinearOperator(MPO._adopt(h))


def _gap_half(env, x, right=False, fill=None):
    """Test hook (t4a_gpu_linop_gap_half).  x: the state's site (lb, d, rb).  right=False: env is L (n, m, lb) -> P (n, d, m, rb);
    right=True: env is R (m, rb, n) -> Q (m, lb, d, n).  With ``fill`` the output buffer and a guard of 64 doubles behind it hold that
    value before the launch -> (result, guard)."""
    env = np.asarray(env, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if env.ndim != 3 or x.ndim != 3:
        raise T4aError(INVALID_ARGUMENT, "linop_gap_half: the environment and the site have three legs")
    lb, d, rb = x.shape
    n, m = (env.shape[2], env.shape[0]) if right else (env.shape[0], env.shape[1])
    if env.shape != ((m, rb, n) if right else (n, m, lb)):
        raise T4aError(INVALID_ARGUMENT, f"linop_gap_half: the environment has shape {env.shape}")
    shape = (m, lb, d, n) if right else (n, d, m, rb)
    count = int(np.prod(shape))
    out = np.zeros(count + 64)
    _check(_lib.t4a_gpu_linop_gap_half(c_int32(1 if right else 0), _p(np.ascontiguousarray(env.reshape(-1, order="F"))), c_size_t(n), c_size_t(m),
                                       _p(np.ascontiguousarray(x.reshape(-1, order="F"))), c_size_t(lb), c_size_t(d), c_size_t(rb),
                                       c_int32(0 if fill is None else 1), c_double(0.0 if fill is None else float(fill)), _p(out)))
    res = out[:count].reshape(shape, order="F")
    return res if fill is None else (res, out[count:count + 64].copy())


def _time_half(n_env, m, lb, d, rb, reps=20):
    """Probe (t4a_gpu_linop_time_half): device milliseconds of the left half of a bridge site -> {"fused", "composed"}."""
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_linop_time_half(c_size_t(n_env), c_size_t(m), c_size_t(lb), c_size_t(d), c_size_t(rb), c_size_t(reps), _p(ms)))
    return {"fused": float(ms[0]), "composed": float(ms[1])}
