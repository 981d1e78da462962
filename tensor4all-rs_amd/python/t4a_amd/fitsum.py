"""Variational sum of many tensor trains or MPOs on the device (tensor4all-treetn/src/treetn/fit.rs: ``fit_sum``).

Mirrors ``fit_sum(targets, initial, center, FitOptions)`` restated for a chain, f64, by position: one result is swept two sites at a
time against the environments of every target, so the sum with its bond ``sum_k chi_k`` is never formed.  ``FitSumOptions`` carries
the reference's builder names as keywords.  Two extensions of this project: ``coefficients`` (one real per target) and
``initial=None`` (a clone of ``targets[0]``).  Trees, complex scalars and the QR, LU and CI factorisations are not mirrored.
``FitOptions`` of ``t4a_amd.mpo`` belongs to ``contract_fit`` and has nothing to do with this module.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, SvdPolicyC, SvdTruncationPolicy, c_size_t, c_double, c_int32,
               c_void_p)
from .mpo import MPO

ROUTES = {"auto": 0, "fused": 1, "gemm": 2}


class FactorizeAlg:
    """FactorizeAlg of tensor4all-core; only SVD is built"""
    SVD, QR, LU, CI = 0, 1, 2, 3


class FitSumOptionsC(ctypes.Structure):
    """t4a_gpu_fit_sum_options"""
    _fields_ = [("nfullsweeps", c_size_t), ("has_max_bond_dim", c_int32), ("max_bond_dim", c_size_t), ("has_svd_policy", c_int32),
                ("svd_policy", SvdPolicyC), ("has_qr_rtol", c_int32), ("qr_rtol", c_double), ("factorize_alg", c_int32),
                ("has_convergence_tol", c_int32), ("convergence_tol", c_double)]


class FitSumOptions:
    """FitOptions (fit.rs) as fit_sum reads it; the defaults are FitOptions::new(1).  ``max_bond_dim``, ``svd_policy`` (an
    SvdTruncationPolicy), ``qr_rtol`` and ``convergence_tol`` are None for "not set".  With none of the first three set, a bond step
    keeps at most the present dimension of its bond: the ranks are fixed."""

    def __init__(self, nfullsweeps=1, max_bond_dim=None, svd_policy=None, qr_rtol=None, factorize_alg=FactorizeAlg.SVD, convergence_tol=None):
        self.nfullsweeps = nfullsweeps
        self.max_bond_dim = max_bond_dim
        self.svd_policy = svd_policy
        self.qr_rtol = qr_rtol
        self.factorize_alg = factorize_alg
        self.convergence_tol = convergence_tol

    def to_c(self):
        if int(self.nfullsweeps) < 0:
            raise T4aError(INVALID_ARGUMENT, "FitSumOptions: nfullsweeps must not be negative")
        if self.max_bond_dim is not None and int(self.max_bond_dim) < 0:
            raise T4aError(INVALID_ARGUMENT, "FitSumOptions: max_bond_dim must not be negative")
        if self.svd_policy is not None and not isinstance(self.svd_policy, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "FitSumOptions::svd_policy must be an SvdTruncationPolicy")
        pol = (self.svd_policy or SvdTruncationPolicy()).to_c()
        return FitSumOptionsC(int(self.nfullsweeps), 0 if self.max_bond_dim is None else 1, 0 if self.max_bond_dim is None else int(self.max_bond_dim),
                              0 if self.svd_policy is None else 1, pol, 0 if self.qr_rtol is None else 1,
                              0.0 if self.qr_rtol is None else float(self.qr_rtol), int(self.factorize_alg),
                              0 if self.convergence_tol is None else 1, 0.0 if self.convergence_tol is None else float(self.convergence_tol))


class FitSumResult:
    """``state`` is the fitted train or MPO, ``norms`` its norm after each completed sweep."""

    def __init__(self, state, sweeps_completed, local_updates, converged, link_dims, norms):
        self.state = state
        self.sweeps_completed = sweeps_completed
        self.local_updates = local_updates
        self.converged = converged
        self.link_dims = link_dims
        self.norms = norms


def _route(route):
    if route not in ROUTES:
        raise T4aError(INVALID_ARGUMENT, "fit_sum: route must be 'auto', 'fused' or 'gemm'")
    return ROUTES[route]


def fit_sum(targets, initial=None, center=0, options=None, coefficients=None, route="auto", return_info=False):
    """The sum of ``targets`` (a list of SimpleTensorTrain or a list of MPO) fitted from ``initial`` by two-site sweeps from ``center``
    (fit.rs:1521-1644) -> the fitted train or MPO, or a FitSumResult with ``return_info``."""
    targets = list(targets)
    kinds = {type(t) for t in targets} | ({type(initial)} if initial is not None else set())
    if kinds - {SimpleTensorTrain, MPO}:
        raise T4aError(INVALID_ARGUMENT, "fit_sum: targets and initial must be SimpleTensorTrain or MPO")
    if len(kinds) > 1:
        raise T4aError(INVALID_ARGUMENT, "fit_sum: targets and initial must all be SimpleTensorTrain or all be MPO, not a mixture")
    if int(center) < 0:
        raise T4aError(INVALID_ARGUMENT, "fit_sum: center must not be negative")
    rt = _route(route)
    o = (FitSumOptions() if options is None else options).to_c()
    w = None
    if coefficients is not None:
        w = np.ascontiguousarray(np.asarray(coefficients, dtype=np.float64).reshape(-1))
        if w.size != len(targets):
            raise T4aError(INVALID_ARGUMENT, "fit_sum: one coefficient per target")
    is_mpo = MPO in kinds
    fn = _lib.t4a_gpu_mpo_fit_sum if is_mpo else _lib.t4a_gpu_tt_fit_sum
    hs = (c_void_p * max(len(targets), 1))(*[t._h for t in targets])
    h = c_void_p()
    sweeps, updates, conv = c_size_t(0), c_size_t(0), c_int32(0)
    norms = np.zeros(max(int(o.nfullsweeps), 1))
    _check(fn(hs, c_size_t(len(targets)), None if w is None or w.size == 0 else _p(w), None if initial is None else initial._h, c_size_t(int(center)),
              ctypes.byref(o), c_int32(rt), ctypes.byref(h), ctypes.byref(sweeps), ctypes.byref(updates), ctypes.byref(conv), _p(norms)))
    state = (MPO if is_mpo else SimpleTensorTrain)._adopt(h)
    if not return_info:
        return state
    return FitSumResult(state, sweeps.value, updates.value, bool(conv.value), state.link_dims(), [float(x) for x in norms[:sweeps.value]])


def fit_sum_check_shapes(target_dims, initial_dims=None, center=0, options=None):
    """The checks of fit_sum on plain dimension lists (t4a_gpu_fit_sum_check_shapes), host only: target_dims is a list of lists of
    (left, site, right), initial_dims one such list or None for "the first target"; options a FitSumOptions, a FitSumOptionsC or None."""
    lens = np.asarray([len(t) for t in target_dims], dtype=np.uintp)
    flat = np.asarray([x for t in target_dims for d in t for x in d], dtype=np.uintp)
    init = None if initial_dims is None else np.asarray([x for d in initial_dims for x in d], dtype=np.uintp)
    o = options.to_c() if isinstance(options, FitSumOptions) else options
    _check(_lib.t4a_gpu_fit_sum_check_shapes(_p(flat) if flat.size else None, _p(lens) if lens.size else None, c_size_t(len(target_dims)),
                                             c_int32(0 if initial_dims is None else 1), None if init is None or init.size == 0 else _p(init),
                                             c_size_t(0 if initial_dims is None else len(initial_dims)), c_size_t(int(center)),
                                             None if o is None else ctypes.byref(o)))


def fit_sum_plan(n_sites, center=0, n_targets=1, site_dim=2, route="fused"):
    """Launch counts of fit_sum (t4a_gpu_fit_sum_plan), host only -> dict."""
    out = np.zeros(6, dtype=np.uintp)
    _check(_lib.t4a_gpu_fit_sum_plan(c_size_t(n_sites), c_size_t(center), c_size_t(n_targets), c_size_t(site_dim), c_int32(_route(route)), _p(out)))
    keys = ("bond_steps_per_sweep", "half_launches_per_step", "gemms_per_step", "svds_per_step", "prepare_half_launches", "prepare_gemms")
    return dict(zip(keys, (int(x) for x in out)))


def fit_sum_route(n_targets, target_bond, result_bond=1, site_dim=2):
    """The route ``auto`` takes for a half (t4a_gpu_fit_sum_route), host only -> 'fused' or 'gemm'."""
    r = c_int32(0)
    _check(_lib.t4a_gpu_fit_sum_route(c_size_t(n_targets), c_size_t(target_bond), c_size_t(result_bond), c_size_t(site_dim), ctypes.byref(r)))
    return {v: k for k, v in ROUTES.items()}[r.value]


def _half(env, cores, right=False, route="fused", fill=None):
    """Test hook (t4a_gpu_fit_sum_half).  cores: a list of (a_k, S, b_k) arrays.  right=False: env is EL (chi, sum a_k) -> P as an array
    (chi, S, sum b_k); right=True: env is ER (sum b_k, chi) -> Q as an array (sum a_k, S, chi).  With ``fill`` the output buffer and a
    guard of 64 doubles behind it hold that value before the launch -> (result, guard)."""
    env = np.asarray(env, dtype=np.float64)
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    if env.ndim != 2 or not cores or any(c.ndim != 3 or c.shape[1] != cores[0].shape[1] for c in cores):
        raise T4aError(INVALID_ARGUMENT, "fit_sum_half: env must be a matrix and the cores (a, S, b) arrays of one site dimension")
    a = np.asarray([c.shape[0] for c in cores], dtype=np.uintp)
    b = np.asarray([c.shape[2] for c in cores], dtype=np.uintp)
    S = cores[0].shape[1]
    A, B = int(a.sum()), int(b.sum())
    chi = env.shape[1] if right else env.shape[0]
    if env.shape != ((B, chi) if right else (chi, A)):
        raise T4aError(INVALID_ARGUMENT, "fit_sum_half: the environment does not match the concatenated bonds of the cores")
    shape = (A, S, chi) if right else (chi, S, B)
    count = int(np.prod(shape))
    out = np.zeros(count + 64)
    flat = np.ascontiguousarray(np.concatenate([c.reshape(-1, order="F") for c in cores]))
    _check(_lib.t4a_gpu_fit_sum_half(c_int32(1 if right else 0), c_int32(_route(route)), _p(np.ascontiguousarray(env.reshape(-1, order="F"))), c_size_t(chi),
                                     c_size_t(S), _p(flat), _p(a), _p(b), c_size_t(len(cores)), c_int32(0 if fill is None else 1),
                                     c_double(0.0 if fill is None else float(fill)), _p(out)))
    res = out[:count].reshape(shape, order="F")
    return res if fill is None else (res, out[count:count + 64].copy())


def _time_half(n_targets, bond, site_dim, chi, right=False, reps=20):
    """Probe (t4a_gpu_fit_sum_time_half): device milliseconds of one half -> {"fused", "gemm"}."""
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_fit_sum_time_half(c_int32(1 if right else 0), c_size_t(n_targets), c_size_t(bond), c_size_t(site_dim), c_size_t(chi), c_size_t(reps),
                                          _p(ms)))
    return {"fused": float(ms[0]), "gemm": float(ms[1])}
