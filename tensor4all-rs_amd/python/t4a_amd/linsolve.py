"""square_linsolve: (a0 + a1 A) x = b for an MPO A and tensor trains x, b on the device (tensor4all-treetn/src/linsolve/).

Mirrors ``square_linsolve``, ``LinsolveOptions``, ``SquareLinsolveResult``, ``relative_linear_system_residual`` and
``ProjectedOperator`` of the Rust crate, restated for a chain, f64, V_in = V_out: every site of the operator has
s1 == s2 == the state's site dimension.  The algorithm is DMRG-style two-site sweeps with a local GMRES
(tensor4all-core/src/krylov.rs, ``gmres_affine_impl``); index mappings, tree topologies and complex scalars are not mirrored.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, SvdPolicyC, SvdTruncationPolicy, c_size_t, c_double, c_int32,
               c_void_p)
from .mpo import MPO


class GmresToleranceMode:
    """GmresTolerance (krylov.rs:240-264): the residual is compared relative to ||b|| or as it is."""
    Relative, Absolute = 0, 1


class LinsolveOptionsC(ctypes.Structure):
    """t4a_gpu_linsolve_options"""
    _fields_ = [("nfullsweeps", c_size_t), ("has_max_bond_dim", c_int32), ("max_bond_dim", c_size_t), ("has_svd_policy", c_int32),
                ("svd_policy", SvdPolicyC), ("gmres_tol", c_double), ("gmres_tolerance_mode", c_int32), ("gmres_max_restarts", c_size_t),
                ("gmres_restart_dim", c_size_t), ("a0", c_double), ("a1", c_double), ("has_convergence_tol", c_int32),
                ("convergence_tol", c_double), ("check_residual", c_int32)]


class LinsolveStatsC(ctypes.Structure):
    """t4a_gpu_linsolve_stats"""
    _fields_ = [("local_solves", c_size_t), ("arnoldi_steps", c_size_t), ("apply_calls", c_size_t)]


class LinsolveOptions:
    """LinsolveOptions (linsolve/common/options.rs); the defaults are LinsolveOptions::default().  ``max_bond_dim``, ``svd_policy``
    (an SvdTruncationPolicy) and ``convergence_tol`` are None for "not set"."""

    def __init__(self, nfullsweeps=5, max_bond_dim=None, svd_policy=None, gmres_tol=1e-10, gmres_tolerance_mode=GmresToleranceMode.Relative,
                 gmres_max_restarts=100, gmres_restart_dim=30, a0=0.0, a1=1.0, convergence_tol=None, check_residual=True):
        self.nfullsweeps = nfullsweeps
        self.max_bond_dim = max_bond_dim
        self.svd_policy = svd_policy
        self.gmres_tol = gmres_tol
        self.gmres_tolerance_mode = gmres_tolerance_mode
        self.gmres_max_restarts = gmres_max_restarts
        self.gmres_restart_dim = gmres_restart_dim
        self.a0 = a0
        self.a1 = a1
        self.convergence_tol = convergence_tol
        self.check_residual = check_residual

    def to_c(self):
        if int(self.nfullsweeps) < 0 or int(self.gmres_max_restarts) < 0 or int(self.gmres_restart_dim) < 0:
            raise T4aError(INVALID_ARGUMENT, "LinsolveOptions: counts must not be negative")
        if self.max_bond_dim is not None and int(self.max_bond_dim) < 1:
            raise T4aError(INVALID_ARGUMENT, "LinsolveOptions::max_bond_dim must be positive when specified")
        if self.svd_policy is not None and not isinstance(self.svd_policy, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "LinsolveOptions::svd_policy must be an SvdTruncationPolicy")
        pol = (self.svd_policy or SvdTruncationPolicy()).to_c()
        return LinsolveOptionsC(int(self.nfullsweeps), 0 if self.max_bond_dim is None else 1,
                                0 if self.max_bond_dim is None else int(self.max_bond_dim), 0 if self.svd_policy is None else 1, pol,
                                float(self.gmres_tol), int(self.gmres_tolerance_mode), int(self.gmres_max_restarts),
                                int(self.gmres_restart_dim), float(self.a0), float(self.a1), 0 if self.convergence_tol is None else 1,
                                0.0 if self.convergence_tol is None else float(self.convergence_tol), 1 if self.check_residual else 0)


class SquareLinsolveResult:
    """SquareLinsolveResult (square/mod.rs): ``residual`` is None when it was not asked for; ``stats`` counts local solves, Arnoldi
    steps and projected applies."""

    def __init__(self, solution, sweeps, residual, converged, stats):
        self.solution = solution
        self.sweeps = sweeps
        self.residual = residual
        self.converged = converged
        self.stats = stats


def _operands(operator, *states):
    if not isinstance(operator, MPO):
        raise T4aError(INVALID_ARGUMENT, "the operator must be an MPO")
    for s in states:
        if not isinstance(s, SimpleTensorTrain):
            raise T4aError(INVALID_ARGUMENT, "states must be SimpleTensorTrain objects")


def square_linsolve(operator, rhs, init, center=0, options=None):
    """Solve (a0 + a1 A) x = rhs from the guess ``init`` (square/mod.rs:233-351) -> SquareLinsolveResult."""
    _operands(operator, rhs, init)
    if int(center) < 0:
        raise T4aError(INVALID_ARGUMENT, "square_linsolve: center must not be negative")
    o = (LinsolveOptions() if options is None else options).to_c()
    h = c_void_p()
    sweeps, has_res, res, conv = c_size_t(0), c_int32(0), c_double(0.0), c_int32(0)
    stats = LinsolveStatsC()
    _check(_lib.t4a_gpu_square_linsolve(operator._h, rhs._h, init._h, c_size_t(int(center)), ctypes.byref(o), ctypes.byref(h),
                                        ctypes.byref(sweeps), ctypes.byref(has_res), ctypes.byref(res), ctypes.byref(conv),
                                        ctypes.byref(stats)))
    return SquareLinsolveResult(SimpleTensorTrain._adopt(h), sweeps.value, res.value if has_res.value else None, bool(conv.value),
                                {"local_solves": stats.local_solves, "arnoldi_steps": stats.arnoldi_steps, "apply_calls": stats.apply_calls})


def relative_linear_system_residual(operator, solution, rhs, a0, a1):
    """||(a0 + a1 A) x - b|| / ||b||, the absolute norm when ||b|| <= 1e-15 (square/mod.rs:432-)."""
    _operands(operator, solution, rhs)
    v = c_double(0.0)
    _check(_lib.t4a_gpu_relative_linear_system_residual(operator._h, solution._h, rhs._h, c_double(a0), c_double(a1), ctypes.byref(v)))
    return v.value


def _flat(a):
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a.reshape(-1, order="F")) if a.size else np.zeros(1)


class ProjectedOperator:
    """ProjectedOperator (common/projected_operator.rs) of <x|A|x> on a chain; the two-site region (site, site + 1).  Environments
    L[beta, w, alpha], R[beta, w, alpha] are computed lazily from the state and cached on the device."""

    def __init__(self, operator, state):
        _operands(operator, state)
        self._h = c_void_p()
        _check(_lib.t4a_gpu_projected_operator_new(operator._h, state._h, ctypes.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.t4a_gpu_projected_operator_release(h)
            self._h = None

    def local_dimension(self, site):
        """(chi_l, d_site, d_{site+1}, chi_r): the shape of a two-site vector of the region."""
        d = np.zeros(4, dtype=np.uintp)
        _check(_lib.t4a_gpu_projected_operator_local_dims(self._h, c_size_t(site), _p(d)))
        return tuple(int(x) for x in d)

    def apply(self, site, v):
        """H v for the region (site, site + 1); v has the shape local_dimension(site)."""
        shape = self.local_dimension(site)
        v = np.asarray(v, dtype=np.float64)
        if v.shape != shape:
            raise T4aError(INVALID_ARGUMENT, f"apply: v has shape {v.shape}, the region has {shape}")
        out = np.zeros(max(v.size, 1))
        _check(_lib.t4a_gpu_projected_operator_apply(self._h, c_size_t(site), _p(_flat(v)), _p(out)))
        return out[:v.size].reshape(shape, order="F")

    def environment(self, side, bond):
        """side "left" / 0: the environment of the sites < bond; "right" / 1: of the sites >= bond -> array [chi, W, chi]."""
        side = {"left": 0, "right": 1}.get(side, side)
        d = np.zeros(3, dtype=np.uintp)
        _check(_lib.t4a_gpu_projected_operator_environment(self._h, c_int32(side), c_size_t(bond), _p(d), None))
        shape = tuple(int(x) for x in d)
        out = np.zeros(max(int(np.prod(shape)), 1))
        _check(_lib.t4a_gpu_projected_operator_environment(self._h, c_int32(side), c_size_t(bond), _p(d), _p(out)))
        return out[:int(np.prod(shape))].reshape(shape, order="F")

    def time_step(self, site, nb, reps=20):
        """Probe (t4a_gpu_projected_operator_time_step): device milliseconds of the launches of one Arnoldi step with nb basis vectors
        -> {"product_left", "product_right", "gs_dots", "gs_update", "gs_normalize"}."""
        ms = np.zeros(5)
        _check(_lib.t4a_gpu_projected_operator_time_step(self._h, c_size_t(site), c_size_t(nb), c_size_t(reps), _p(ms)))
        return dict(zip(("product_left", "product_right", "gs_dots", "gs_update", "gs_normalize"), (float(v) for v in ms)))

    def invalidate(self, site):
        _check(_lib.t4a_gpu_projected_operator_invalidate(self._h, c_size_t(site)))

    def set_site_tensors(self, site, t_a, t_b):
        """Replace the state's sites (site, site + 1) (outer bonds and site dimensions kept) and invalidate the caches they are in."""
        t_a, t_b = np.asarray(t_a, dtype=np.float64), np.asarray(t_b, dtype=np.float64)
        if t_a.ndim != 3 or t_b.ndim != 3:
            raise T4aError(INVALID_ARGUMENT, "site tensors must have three legs (left, site, right)")
        da, db = np.array(t_a.shape, dtype=np.uintp), np.array(t_b.shape, dtype=np.uintp)
        _check(_lib.t4a_gpu_projected_operator_set_site_tensors(self._h, c_size_t(site), _p(da), _p(_flat(t_a)), _p(db), _p(_flat(t_b))))


def _apply_env(left, right, operator, site, v, return_half_operators=False):
    """Test hook (t4a_gpu_projected_operator_apply_env): the apply on caller-supplied environments L[chi_l, W_l, chi_l],
    R[chi_r, W_r, chi_r], launched as the sweeps launch it -> y, or (y, HL, HR) with the half operators as matrices."""
    left, right, v = (np.asarray(a, dtype=np.float64) for a in (left, right, v))
    dims4 = operator.dims()
    if left.ndim != 3 or right.ndim != 3 or v.ndim != 4 or not 0 <= site < len(dims4) - 1:
        raise T4aError(INVALID_ARGUMENT, "apply_env: environments have three legs, v four, and the region must exist")
    wl, d1, _, w = (int(x) for x in dims4[site])
    _, d2, _, wr = (int(x) for x in dims4[site + 1])
    chi_l, chi_r = left.shape[0], right.shape[0]
    if left.shape != (chi_l, wl, chi_l) or right.shape != (chi_r, wr, chi_r) or v.shape != (chi_l, d1, d2, chi_r):
        raise T4aError(INVALID_ARGUMENT, f"apply_env: shapes {left.shape}, {right.shape}, {v.shape} do not fit the operator")
    m, n = chi_l * d1, d2 * chi_r
    out = np.zeros(m * n)
    hl, hr = np.zeros(w * m * m), np.zeros(w * n * n)
    dims = np.array([chi_l, chi_r], dtype=np.uintp)
    _check(_lib.t4a_gpu_projected_operator_apply_env(_p(_flat(left)), _p(_flat(right)), _p(dims), operator._h, c_size_t(site), _p(_flat(v)),
                                                     _p(out), _p(hl) if return_half_operators else None,
                                                     _p(hr) if return_half_operators else None))
    y = out.reshape(v.shape, order="F")
    if not return_half_operators:
        return y
    return y, hl.reshape((w * m, m), order="F"), hr.reshape((w * n, n), order="F")


def _orth(basis, w):
    """Test hook (t4a_gpu_linsolve_orth): basis (len, nb), w (len) -> (w after both passes and the normalisation, pass-1
    coefficients, pass-2 coefficients, norm before the normalisation)."""
    basis = np.asarray(basis, dtype=np.float64)
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1)).copy()
    ln, nb = basis.shape
    h = np.zeros(2 * nb)
    nrm = c_double(0.0)
    _check(_lib.t4a_gpu_linsolve_orth(_p(_flat(basis)), c_size_t(ln), c_size_t(nb), _p(w), _p(h), ctypes.byref(nrm)))
    return w, h[:nb].copy(), h[nb:].copy(), nrm.value


def _gmres_dense(h, b, x0, a0, a1, tol=1e-10, mode=GmresToleranceMode.Relative, restart_dim=30, max_restarts=100):
    """Test hook (t4a_gpu_linsolve_gmres_dense) -> (x, iterations, residual, converged)."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    x = np.zeros(max(n, 1))
    it, res, conv = c_size_t(0), c_double(0.0), c_int32(0)
    _check(_lib.t4a_gpu_linsolve_gmres_dense(_p(_flat(h)), c_size_t(n), _p(_flat(b)), _p(_flat(x0)), c_double(a0), c_double(a1), c_double(tol),
                                             c_int32(mode), c_size_t(restart_dim), c_size_t(max_restarts), _p(x), ctypes.byref(it),
                                             ctypes.byref(res), ctypes.byref(conv)))
    return x[:n], it.value, res.value, bool(conv.value)
