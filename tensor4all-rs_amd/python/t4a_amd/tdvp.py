"""Two-site TDVP: a tensor train evolved under an MPO on the device, exp(tau H) per sweep (tensor4all-treetn/src/tdvp/mod.rs).

Mirrors ``tdvp`` / ``tdvp_with_treetn_operator``, ``TdvpOptions``, ``TdvpResult`` and ``HermitianKrylovExpmOptions`` of the Rust crates,
restated for what ``square_linsolve`` and ``dmrg`` cover: a chain, f64, one site index per node, V_in = V_out.  The local solver is
``hermitian_krylov_expm_multiply`` (tensor4all-core/src/krylov.rs:693-926).

Deviations from the reference: the exponent is REAL — ``exponent_step`` defaults to -0.1 where the reference has -0.1i, a Python complex
is accepted and a non-zero imaginary part refused, because real-time evolution needs complex trains, which this project does not have
(u' = -H u: heat and diffusion flows, imaginary-time relaxation, is what a real exponent covers); ``center`` must be 0 or n - 1, because
the reference's two-site plan from an inner root of a chain applies a site correction at a leaf where the projector splitting needs it
at the root; ``tdvp`` refuses ``nsite = 1``: one-site TDVP has entry points of its own, ``tdvp_one_site_plan`` and ``tdvp_one_site``
below (fixed bond dimensions, any centre).  Trees, index mappings and ``verbose`` are not mirrored.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, SvdPolicyC, SvdTruncationPolicy, c_size_t, c_double, c_int32,
               c_void_p)
from .linsolve import _operands, _flat

ROUTE_SERIAL, ROUTE_WIDE, ROUTE_AUTO = 0, 1, 2  # KrylovDotsRoute
TWO_SITE, SITE_CORRECTION, ONE_SITE = 0, 1, 2    # the kinds of a plan step
BOND_FUSED, BOND_GEMM, BOND_AUTO = 0, 1, 2       # BondApplyRoute


class KrylovExpmOptionsC(ctypes.Structure):
    """t4a_gpu_krylov_expm_options"""
    _fields_ = [("max_iter", c_size_t), ("max_time_splits", c_size_t), ("tol", c_double), ("breakdown_tol", c_double), ("hermitian_tol", c_double)]


class TdvpOptionsC(ctypes.Structure):
    """t4a_gpu_tdvp_options"""
    _fields_ = [("nsite", c_size_t), ("nsweeps", c_size_t), ("order", c_size_t), ("exponent_step_re", c_double), ("exponent_step_im", c_double),
                ("has_max_bond_dim", c_int32), ("max_bond_dim", c_size_t), ("has_svd_policy", c_int32), ("svd_policy", SvdPolicyC),
                ("krylov", KrylovExpmOptionsC)]


class TdvpStatsC(ctypes.Structure):
    """t4a_gpu_tdvp_stats"""
    _fields_ = [("two_site_steps", c_size_t), ("corrections", c_size_t), ("krylov_steps", c_size_t), ("apply_calls", c_size_t),
                ("max_time_splits", c_size_t)]


class TdvpOneSiteStatsC(ctypes.Structure):
    """t4a_gpu_tdvp_one_site_stats"""
    _fields_ = [("one_site_steps", c_size_t), ("bond_corrections", c_size_t), ("qr_steps", c_size_t), ("krylov_steps", c_size_t),
                ("apply_calls", c_size_t), ("max_time_splits", c_size_t), ("fused_applies", c_size_t), ("gemm_applies", c_size_t)]


class HermitianKrylovExpmOptions:
    """HermitianKrylovExpmOptions (krylov.rs:413-440); the defaults are HermitianKrylovExpmOptions::default()."""

    def __init__(self, max_iter=30, max_time_splits=100, tol=1e-12, breakdown_tol=1e-14, hermitian_tol=1e-10):
        self.max_iter = max_iter
        self.max_time_splits = max_time_splits
        self.tol = tol
        self.breakdown_tol = breakdown_tol
        self.hermitian_tol = hermitian_tol

    def to_c(self):
        if int(self.max_iter) < 0 or int(self.max_time_splits) < 0:
            raise T4aError(INVALID_ARGUMENT, "HermitianKrylovExpmOptions: counts must not be negative")
        return KrylovExpmOptionsC(int(self.max_iter), int(self.max_time_splits), float(self.tol), float(self.breakdown_tol), float(self.hermitian_tol))


class TdvpOptions:
    """TdvpOptions (tdvp/mod.rs:311-330) with a real ``exponent_step`` (default -0.1; a complex with a zero imaginary part is accepted).
    ``max_bond_dim`` and ``svd_policy`` (an SvdTruncationPolicy) are None for "not set"; ``krylov`` is a HermitianKrylovExpmOptions."""

    def __init__(self, nsite=2, nsweeps=1, order=2, exponent_step=-0.1, max_bond_dim=None, svd_policy=None, krylov=None):
        self.nsite = nsite
        self.nsweeps = nsweeps
        self.order = order
        self.exponent_step = exponent_step
        self.max_bond_dim = max_bond_dim
        self.svd_policy = svd_policy
        self.krylov = HermitianKrylovExpmOptions() if krylov is None else krylov

    def to_c(self):
        if int(self.nsite) < 0 or int(self.nsweeps) < 0 or int(self.order) < 0:
            raise T4aError(INVALID_ARGUMENT, "TdvpOptions: counts must not be negative")
        if self.max_bond_dim is not None and int(self.max_bond_dim) < 1:
            raise T4aError(INVALID_ARGUMENT, "invalid TDVP option max_bond_dim: must be greater than zero when set")
        if self.svd_policy is not None and not isinstance(self.svd_policy, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "TdvpOptions::svd_policy must be an SvdTruncationPolicy")
        if not isinstance(self.krylov, HermitianKrylovExpmOptions):
            raise T4aError(INVALID_ARGUMENT, "TdvpOptions::krylov must be a HermitianKrylovExpmOptions")
        step = complex(self.exponent_step)
        if step.imag != 0.0:
            raise T4aError(INVALID_ARGUMENT, "tdvp: exponent_step must be real here: real-time evolution (a non-zero imaginary part) needs "
                                             "complex tensor trains, which this project does not have")
        pol = (self.svd_policy or SvdTruncationPolicy()).to_c()
        return TdvpOptionsC(int(self.nsite), int(self.nsweeps), int(self.order), step.real, step.imag, 0 if self.max_bond_dim is None else 1,
                            0 if self.max_bond_dim is None else int(self.max_bond_dim), 0 if self.svd_policy is None else 1, pol, self.krylov.to_c())


class TdvpResult:
    """TdvpResult (tdvp/mod.rs:434-449): ``local_updates`` counts the projected exponentials (two-site steps and site corrections),
    ``max_error_estimate`` and ``max_krylov_iterations`` are the largest over them; ``stats`` counts two-site steps, corrections, Krylov
    steps, projected applies and the largest number of time splits."""

    def __init__(self, state, sweeps_completed, local_updates, max_error_estimate, max_krylov_iterations, stats):
        self.state = state
        self.sweeps_completed = sweeps_completed
        self.local_updates = local_updates
        self.max_error_estimate = max_error_estimate
        self.max_krylov_iterations = max_krylov_iterations
        self.stats = stats


def _run(fn, stats_cls, who, default_nsite, operator, init, center, options):
    """The driver ``fn`` (t4a_gpu_tdvp or t4a_gpu_tdvp_one_site) with its stats struct -> TdvpResult"""
    _operands(operator, init)
    if int(center) < 0:
        raise T4aError(INVALID_ARGUMENT, who + ": center must not be negative")
    o = (TdvpOptions(nsite=default_nsite) if options is None else options).to_c()
    h = c_void_p()
    sweeps, updates, err, iters = c_size_t(0), c_size_t(0), c_double(0.0), c_size_t(0)
    stats = stats_cls()
    _check(fn(operator._h, init._h, c_size_t(int(center)), ctypes.byref(o), ctypes.byref(h), ctypes.byref(sweeps), ctypes.byref(updates), ctypes.byref(err),
              ctypes.byref(iters), ctypes.byref(stats)))
    return TdvpResult(SimpleTensorTrain._adopt(h), sweeps.value, updates.value, err.value, iters.value,
                      {name: getattr(stats, name) for name, _ in stats_cls._fields_})


def _plan(fn, n, center, order, tau):
    """The plan entry ``fn``: the count-only call, then the arrays -> [(kind, both nodes, new_center, exponent)]"""
    count = c_size_t(0)
    args = (c_size_t(int(n)), c_size_t(int(center)), c_size_t(int(order)), c_double(float(tau)))
    _check(fn(*args, c_size_t(0), None, None, None, None, ctypes.byref(count)))
    k = count.value
    kinds, nodes, centers, exps = np.zeros(max(k, 1), dtype=np.int32), np.zeros(2 * max(k, 1), dtype=np.uintp), np.zeros(max(k, 1), dtype=np.uintp), np.zeros(max(k, 1))
    _check(fn(*args, c_size_t(k), _p(kinds), _p(nodes), _p(centers), _p(exps), ctypes.byref(count)))
    return [(int(kinds[j]), (int(nodes[2 * j]), int(nodes[2 * j + 1])), int(centers[j]), float(exps[j])) for j in range(k)]


def tdvp(operator, init, center=0, options=None):
    """Two-site TDVP: ``nsweeps`` sweeps of exp(exponent_step * operator) on ``init`` from ``center`` (0 or n - 1) (tdvp/mod.rs:1107-1217)
    -> TdvpResult.  The state is not renormalised.  ``nsite = 1`` is refused here: see ``tdvp_one_site``."""
    return _run(_lib.t4a_gpu_tdvp, TdvpStatsC, "tdvp", 2, operator, init, center, options)


def tdvp_plan(n, center, order, tau):
    """The region plan of one sweep (t4a_gpu_tdvp_plan, host only) -> [(kind, nodes, new_center, exponent)], nodes a tuple of two sites
    for a two-site step (the other node, the new centre) and of one for a site correction."""
    return [(kind, nodes if kind == TWO_SITE else nodes[:1], new_center, exponent)
            for kind, nodes, new_center, exponent in _plan(_lib.t4a_gpu_tdvp_plan, n, center, order, tau)]


def tdvp_one_site(operator, init, center=0, options=None):
    """One-site TDVP (TdvpOptions::with_nsite(1), tdvp/mod.rs:639-914): ``nsweeps`` sweeps of exp(exponent_step * operator) on ``init``
    from any ``center`` with every bond dimension fixed -> TdvpResult, whose ``stats`` count one-site steps, bond corrections, QR steps,
    Krylov steps, applies, time splits and the bond-centre applies by route.  ``options`` defaults to ``TdvpOptions(nsite=1)``;
    ``max_bond_dim`` and ``svd_policy`` are refused (fixed ranks).  ``local_updates`` counts site and bond solves, w (2n - 1) per sweep."""
    return _run(_lib.t4a_gpu_tdvp_one_site, TdvpOneSiteStatsC, "tdvp_one_site", 1, operator, init, center, options)


def tdvp_one_site_plan(n, center, order, tau):
    """The one-site plan of one sweep (t4a_gpu_tdvp_one_site_plan, host only) -> [(ONE_SITE, (node,), node, exponent)]: post order from
    ``center``, the left arm leaf first, every even substep reversed."""
    return [(kind, nodes[:1], new_center, exponent) for kind, nodes, new_center, exponent in _plan(_lib.t4a_gpu_tdvp_one_site_plan, n, center, order, tau)]


def _apply_bond_center(left, right, c, route=BOND_AUTO):
    """Test hook (t4a_gpu_tdvp_bond_apply): left [ka, W, ka], right [kb, W, kb], c (ka, kb) -> (Y (ka, kb), the route taken)."""
    left, right, c = (np.asarray(a, dtype=np.float64) for a in (left, right, c))
    if left.ndim != 3 or right.ndim != 3 or c.ndim != 2 or left.shape[0] != left.shape[2] or right.shape[0] != right.shape[2] \
            or left.shape[1] != right.shape[1] or c.shape != (left.shape[0], right.shape[0]):
        raise T4aError(INVALID_ARGUMENT, "apply_bond_center: left [ka, W, ka], right [kb, W, kb] and c (ka, kb)")
    ka, kb, w = left.shape[0], right.shape[0], left.shape[1]
    out = np.zeros(max(c.size, 1))
    taken = c_int32(-1)
    _check(_lib.t4a_gpu_tdvp_bond_apply(_p(_flat(left)), _p(_flat(right)), _p(_flat(c)), c_size_t(ka), c_size_t(kb), c_size_t(w), c_int32(route), _p(out),
                                        ctypes.byref(taken)))
    return out[:c.size].reshape(c.shape, order="F"), taken.value


def _bond_apply_route(ka, kb, w):
    """tdvp_bond_apply_route(ka, kb, W) (host only) -> BOND_FUSED or BOND_GEMM"""
    r = c_int32(0)
    _check(_lib.t4a_gpu_tdvp_bond_apply_route(c_size_t(ka), c_size_t(kb), c_size_t(w), ctypes.byref(r)))
    return r.value


def _bond_apply_fused_admits(ka, kb, w):
    """whether the fused launch admits the shape (host only)"""
    r = c_int32(0)
    _check(_lib.t4a_gpu_tdvp_bond_apply_fused_admits(c_size_t(ka), c_size_t(kb), c_size_t(w), ctypes.byref(r)))
    return bool(r.value)


def _set_bond_apply_route(route):
    """Test hook: forces the route of the bond-centre applies of the drivers (BOND_FUSED where admitted, BOND_GEMM; BOND_AUTO: the rule)"""
    _check(_lib.t4a_gpu_tdvp_set_bond_apply_route(c_int32(route if route in (BOND_FUSED, BOND_GEMM) else -1)))


def _bond_center_env(po, site, toward_right):
    """Test hook (t4a_gpu_projected_operator_bond_center_env): the environment [k, W, k] of the bond-centre step next to ``site`` built
    with the present tensor of that site as Q."""
    dims = np.zeros(3, dtype=np.uintp)
    _check(_lib.t4a_gpu_projected_operator_bond_center_env(po._h, c_size_t(site), c_int32(1 if toward_right else 0), _p(dims), None))
    out = np.zeros(max(int(np.prod(dims)), 1))
    _check(_lib.t4a_gpu_projected_operator_bond_center_env(po._h, c_size_t(site), c_int32(1 if toward_right else 0), _p(dims), _p(out)))
    return out[:int(np.prod(dims))].reshape(tuple(int(d) for d in dims), order="F")


def _time_bond_apply(ka, kb, w, reps=20):
    """Probe (t4a_gpu_tdvp_bond_apply_time) -> {"fused", "gemm"} in device milliseconds (fused: nan outside the envelope)."""
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_tdvp_bond_apply_time(c_size_t(ka), c_size_t(kb), c_size_t(w), c_size_t(reps), _p(ms)))
    return {"fused": float(ms[0]), "gemm": float(ms[1])}


def _apply_one_site(po, site, v):
    """Test hook (t4a_gpu_projected_operator_apply_one_site) on a ProjectedOperator: v [chi_l, d, chi_r] -> (H v, whether the HL of an
    earlier two-site apply at (site, site + 1) was reused)."""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 3:
        raise T4aError(INVALID_ARGUMENT, "apply_one_site: v has three legs (left, site, right)")
    out = np.zeros(max(v.size, 1))
    reused = c_int32(0)
    _check(_lib.t4a_gpu_projected_operator_apply_one_site(po._h, c_size_t(site), _p(_flat(v)), _p(out), ctypes.byref(reused)))
    return out[:v.size].reshape(v.shape, order="F"), bool(reused.value)


def _krylov_orth(basis, w, route):
    """Test hook (t4a_gpu_krylov_orth): basis (len, nb), w (len), route ROUTE_SERIAL / ROUTE_WIDE / ROUTE_AUTO -> (w after both passes and
    the normalisation, pass-1 coefficients, pass-2 coefficients, norm before the normalisation)."""
    basis = np.asarray(basis, dtype=np.float64)
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1)).copy()
    ln, nb = basis.shape
    h = np.zeros(2 * max(nb, 1))
    nrm = c_double(0.0)
    _check(_lib.t4a_gpu_krylov_orth(_p(_flat(basis)), c_size_t(ln), c_size_t(nb), _p(w), c_int32(route), _p(h), ctypes.byref(nrm)))
    return w, h[:nb].copy(), h[nb:2 * nb].copy(), nrm.value


def _dots_route(length, nb):
    """krylov_dots_route(len, nb) (host only) -> ROUTE_SERIAL or ROUTE_WIDE"""
    r = c_int32(0)
    _check(_lib.t4a_gpu_krylov_dots_route(c_size_t(length), c_size_t(nb), ctypes.byref(r)))
    return r.value


def _krylov_expm_dense(h, v0, tau, options=None):
    """Test hook (t4a_gpu_krylov_expm_dense) -> (exp(tau H) v0, iterations, error_estimate, converged, time_splits)."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    if h.shape != (n, n) or np.asarray(v0).size != n:
        raise T4aError(INVALID_ARGUMENT, "krylov_expm_dense: H must be square and v0 of its order")
    o = (HermitianKrylovExpmOptions() if options is None else options).to_c()
    out = np.zeros(max(n, 1))
    it, err, conv, splits = c_size_t(0), c_double(0.0), c_int32(0), c_size_t(0)
    _check(_lib.t4a_gpu_krylov_expm_dense(_p(_flat(h)), c_size_t(n), _p(_flat(v0)), c_double(tau), ctypes.byref(o), _p(out), ctypes.byref(it),
                                          ctypes.byref(err), ctypes.byref(conv), ctypes.byref(splits)))
    return out[:n], it.value, err.value, bool(conv.value), splits.value


def _time_dots(length, nb, reps=20):
    """Probe (t4a_gpu_krylov_time_dots): device milliseconds of the serial and the wide launch of the projections -> {"serial", "wide"}."""
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_krylov_time_dots(c_size_t(length), c_size_t(nb), c_size_t(reps), _p(ms)))
    return {"serial": float(ms[0]), "wide": float(ms[1])}


def _time_one_site(po, site, reps=20):
    """Probe (t4a_gpu_projected_operator_time_one_site) -> {"linsolve_hl", "product_left", "product_right"} in device milliseconds."""
    ms = np.zeros(3)
    _check(_lib.t4a_gpu_projected_operator_time_one_site(po._h, c_size_t(site), c_size_t(reps), _p(ms)))
    return dict(zip(("linsolve_hl", "product_left", "product_right"), (float(x) for x in ms)))
