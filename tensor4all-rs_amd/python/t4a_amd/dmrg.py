"""Two-site DMRG: the lowest eigenpair of an MPO over tensor trains on the device (tensor4all-treetn/src/dmrg/mod.rs).

Mirrors ``dmrg`` / ``dmrg_with_treetn_operator``, ``DmrgOptions``, ``DmrgResult`` and ``HermitianLanczosOptions`` of the Rust crates,
restated for what ``square_linsolve`` covers: a chain, f64, one site index per node, V_in = V_out (every site of the operator has
s1 == s2 == the state's site dimension).  The local solver is ``hermitian_lanczos_lowest_eigenpair`` (tensor4all-core/src/krylov.rs);
trees, index mappings, complex scalars and nsite != 2 are not mirrored.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, SvdPolicyC, SvdTruncationPolicy, c_size_t, c_double, c_int32,
               c_void_p)
from .linsolve import _operands, _flat


class LanczosOptionsC(ctypes.Structure):
    """t4a_gpu_lanczos_options"""
    _fields_ = [("max_iter", c_size_t), ("rtol", c_double), ("atol", c_double), ("breakdown_tol", c_double), ("hermitian_tol", c_double)]


class DmrgOptionsC(ctypes.Structure):
    """t4a_gpu_dmrg_options"""
    _fields_ = [("nsite", c_size_t), ("nsweeps", c_size_t), ("has_max_bond_dim", c_int32), ("max_bond_dim", c_size_t),
                ("has_svd_policy", c_int32), ("svd_policy", SvdPolicyC), ("lanczos", LanczosOptionsC), ("has_energy_tol", c_int32),
                ("energy_tol", c_double), ("real_scalar_tol", c_double)]


class DmrgStatsC(ctypes.Structure):
    """t4a_gpu_dmrg_stats"""
    _fields_ = [("local_solves", c_size_t), ("lanczos_steps", c_size_t), ("apply_calls", c_size_t)]


class HermitianLanczosOptions:
    """HermitianLanczosOptions (krylov.rs:311-360); the defaults are HermitianLanczosOptions::default()."""

    def __init__(self, max_iter=64, rtol=1e-10, atol=0.0, breakdown_tol=1e-14, hermitian_tol=1e-10):
        self.max_iter = max_iter
        self.rtol = rtol
        self.atol = atol
        self.breakdown_tol = breakdown_tol
        self.hermitian_tol = hermitian_tol

    def to_c(self):
        if int(self.max_iter) < 0:
            raise T4aError(INVALID_ARGUMENT, "HermitianLanczosOptions: max_iter must not be negative")
        return LanczosOptionsC(int(self.max_iter), float(self.rtol), float(self.atol), float(self.breakdown_tol), float(self.hermitian_tol))


class DmrgOptions:
    """DmrgOptions (dmrg/mod.rs); the defaults are DmrgOptions::default().  ``max_bond_dim``, ``svd_policy`` (an SvdTruncationPolicy)
    and ``energy_tol`` are None for "not set"; ``lanczos`` is a HermitianLanczosOptions."""

    def __init__(self, nsite=2, nsweeps=5, max_bond_dim=None, svd_policy=None, lanczos=None, energy_tol=None, real_scalar_tol=1e-10):
        self.nsite = nsite
        self.nsweeps = nsweeps
        self.max_bond_dim = max_bond_dim
        self.svd_policy = svd_policy
        self.lanczos = HermitianLanczosOptions() if lanczos is None else lanczos
        self.energy_tol = energy_tol
        self.real_scalar_tol = real_scalar_tol

    def to_c(self):
        if int(self.nsite) < 0 or int(self.nsweeps) < 0:
            raise T4aError(INVALID_ARGUMENT, "DmrgOptions: counts must not be negative")
        if self.max_bond_dim is not None and int(self.max_bond_dim) < 1:
            raise T4aError(INVALID_ARGUMENT, "invalid DMRG option max_bond_dim: must be greater than zero when set")
        if self.svd_policy is not None and not isinstance(self.svd_policy, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "DmrgOptions::svd_policy must be an SvdTruncationPolicy")
        if not isinstance(self.lanczos, HermitianLanczosOptions):
            raise T4aError(INVALID_ARGUMENT, "DmrgOptions::lanczos must be a HermitianLanczosOptions")
        pol = (self.svd_policy or SvdTruncationPolicy()).to_c()
        return DmrgOptionsC(int(self.nsite), int(self.nsweeps), 0 if self.max_bond_dim is None else 1,
                            0 if self.max_bond_dim is None else int(self.max_bond_dim), 0 if self.svd_policy is None else 1, pol,
                            self.lanczos.to_c(), 0 if self.energy_tol is None else 1,
                            0.0 if self.energy_tol is None else float(self.energy_tol), float(self.real_scalar_tol))


class DmrgResult:
    """DmrgResult (dmrg/mod.rs): ``energy`` is the final Rayleigh quotient, ``max_residual_norm`` the largest true residual of a local
    eigensolve; ``stats`` counts local solves, Lanczos steps and projected applies."""

    def __init__(self, state, energy, sweeps_completed, local_updates, converged, max_residual_norm, stats):
        self.state = state
        self.energy = energy
        self.sweeps_completed = sweeps_completed
        self.local_updates = local_updates
        self.converged = converged
        self.max_residual_norm = max_residual_norm
        self.stats = stats


def dmrg(operator, init, center=0, options=None):
    """Two-site DMRG for the lowest eigenpair of ``operator`` from the state ``init`` (dmrg/mod.rs:631-725) -> DmrgResult."""
    _operands(operator, init)
    if int(center) < 0:
        raise T4aError(INVALID_ARGUMENT, "dmrg: center must not be negative")
    o = (DmrgOptions() if options is None else options).to_c()
    h = c_void_p()
    energy, sweeps, updates, conv, res = c_double(0.0), c_size_t(0), c_size_t(0), c_int32(0), c_double(0.0)
    stats = DmrgStatsC()
    _check(_lib.t4a_gpu_dmrg(operator._h, init._h, c_size_t(int(center)), ctypes.byref(o), ctypes.byref(h), ctypes.byref(energy),
                             ctypes.byref(sweeps), ctypes.byref(updates), ctypes.byref(conv), ctypes.byref(res), ctypes.byref(stats)))
    return DmrgResult(SimpleTensorTrain._adopt(h), energy.value, sweeps.value, updates.value, bool(conv.value), res.value,
                      {"local_solves": stats.local_solves, "lanczos_steps": stats.lanczos_steps, "apply_calls": stats.apply_calls})


def dmrg_energy(operator, state, center=0):
    """<theta|H theta> / <theta|theta> at the region of ``center`` of a copy of ``state`` canonicalised onto it: the energy of
    DmrgResult for any state."""
    _operands(operator, state)
    if int(center) < 0:
        raise T4aError(INVALID_ARGUMENT, "dmrg_energy: center must not be negative")
    v = c_double(0.0)
    _check(_lib.t4a_gpu_dmrg_energy(operator._h, state._h, c_size_t(int(center)), ctypes.byref(v)))
    return v.value


def _lanczos_dense(h, v0, options=None):
    """Test hook (t4a_gpu_lanczos_dense) -> (eigenvalue, eigenvector, iterations, residual_norm, converged)."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    if h.shape != (n, n) or np.asarray(v0).size != n:
        raise T4aError(INVALID_ARGUMENT, "lanczos_dense: H must be square and v0 of its order")
    o = (HermitianLanczosOptions() if options is None else options).to_c()
    vec = np.zeros(max(n, 1))
    lam, it, res, conv = c_double(0.0), c_size_t(0), c_double(0.0), c_int32(0)
    _check(_lib.t4a_gpu_lanczos_dense(_p(_flat(h)), c_size_t(n), _p(_flat(v0)), ctypes.byref(o), ctypes.byref(lam), _p(vec), ctypes.byref(it),
                                      ctypes.byref(res), ctypes.byref(conv)))
    return lam.value, vec[:n], it.value, res.value, bool(conv.value)


def _krylov_combine(basis, coef):
    """Test hook (t4a_gpu_krylov_combine): basis (len, nb), coef (nb) -> (sum_i coef[i] basis[:, i], its squared norm)."""
    basis = np.asarray(basis, dtype=np.float64)
    ln, nb = basis.shape
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(-1))
    if coef.size != nb:
        raise T4aError(INVALID_ARGUMENT, "krylov_combine: one coefficient per basis vector")
    out = np.zeros(max(ln, 1))
    n2 = c_double(0.0)
    _check(_lib.t4a_gpu_krylov_combine(_p(_flat(basis)), c_size_t(ln), c_size_t(nb), _p(coef if nb else np.zeros(1)), _p(out), ctypes.byref(n2)))
    return out[:ln], n2.value


def _eig_residual(v, hv, lam, with_residual=True):
    """Test hook (t4a_gpu_eig_residual) -> (r = hv - lam v, or None, and the sums (|r|^2, <v, hv>, <v, v>))."""
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    hv = np.ascontiguousarray(np.asarray(hv, dtype=np.float64).reshape(-1))
    if v.size != hv.size:
        raise T4aError(INVALID_ARGUMENT, "eig_residual: v and hv must have the same length")
    r = np.zeros(max(v.size, 1)) if with_residual else None
    sums = np.zeros(3)
    _check(_lib.t4a_gpu_eig_residual(_p(v if v.size else np.zeros(1)), _p(hv if v.size else np.zeros(1)), c_size_t(v.size), c_double(lam),
                                     None if r is None else _p(r), _p(sums)))
    return (None if r is None else r[:v.size]), sums


def _time_finalise(length, nb, reps=20):
    """Probe (t4a_gpu_lanczos_time_finalise): device milliseconds of the launches of a finalise with nb basis vectors of the given length
    -> {"krylov_combine", "eig_residual", "krylov_finish"}."""
    ms = np.zeros(3)
    _check(_lib.t4a_gpu_lanczos_time_finalise(c_size_t(length), c_size_t(nb), c_size_t(reps), _p(ms)))
    return dict(zip(("krylov_combine", "eig_residual", "krylov_finish"), (float(x) for x in ms)))
