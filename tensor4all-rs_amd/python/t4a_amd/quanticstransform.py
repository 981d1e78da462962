"""Quantics transform operators as MPOs — the real-valued part of tensor4all-quanticstransform.

Mirrors the Rust crate: ``BoundaryCondition``, ``TriangleType``, ``AffineParams``, ``shift_operator``, ``flip_operator``,
``cumsum_operator``, ``triangle_operator``, ``shift_operator_multivar``, ``flip_operator_multivar``, ``affine_operator``,
``affine_transform_matrix``, ``identity_mpo``, ``difference_kernel_mpo`` and ``apply``.

An operator acts on a function held as a quantics tensor train with site 0 the most significant bit.  Its site tensors are
(left, s1 = out, s2 = in, right), the layout of ``MPO``.  Building an operator is exact integer bookkeeping on the host:
``QuanticsOperator.site_tensors()`` needs no device.  ``QuanticsOperator.mpo()`` is the one upload; applying the operator is the
MPO contraction of ``t4a_amd.mpo`` on the device.

Not here: ``quantics_fourier_operator`` and ``phase_rotation_operator*`` need complex scalars (this library is f64 only), and
``affine_operator_interleaved`` / ``affine_transform_tensors_unfused`` / ``LinearConstraintRow`` are not ported.
"""
import ctypes
from fractions import Fraction
from math import gcd

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, c_size_t, c_int32, c_void_p)
from .mpo import MPO, ContractionAlgorithm, contract, contract_naive

c_int64 = ctypes.c_int64


class BoundaryCondition:
    """BoundaryCondition (common.rs): what a coordinate that leaves [0, 2^r) is weighted with: 1, (-1)^wraps, 0."""
    Periodic, AntiPeriodic, Open = 0, 1, 2


class TriangleType:
    """TriangleType (cumsum.rs): Lower is M[i, j] = [i > j], Upper is M[i, j] = [i < j]."""
    Lower, Upper = 0, 1


class QuanticsOperator:
    """A quantics operator built on the host; ``mpo()`` uploads it once and caches the device ``MPO``."""

    def __init__(self, handle):
        self._h = handle
        self._mpo = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.t4a_gpu_qt_op_release(h)
            self._h = None

    def __len__(self):
        v = c_size_t(0)
        _check(_lib.t4a_gpu_qt_op_len(self._h, ctypes.byref(v)))
        return v.value

    def dims(self):
        """(n_sites, 4) array of (left, s1, s2, right)."""
        n = len(self)
        d = np.zeros(max(4 * n, 1), dtype=np.uintp)
        _check(_lib.t4a_gpu_qt_op_dims(self._h, _p(d)))
        return d[:4 * n].reshape(-1, 4).astype(np.int64)

    def site_dims(self):
        return [(int(a), int(b)) for a, b in self.dims()[:, 1:3]]

    def link_dims(self):
        return [int(x) for x in self.dims()[1:, 0]]

    def site_tensor(self, site):
        if not 0 <= site < len(self):
            raise T4aError(INVALID_ARGUMENT, "site out of range")
        shape = tuple(int(x) for x in self.dims()[site])
        buf = np.zeros(int(np.prod(shape)))
        _check(_lib.t4a_gpu_qt_op_site_tensor(self._h, c_size_t(site), _p(buf)))
        return buf.reshape(shape, order="F")

    def site_tensors(self):
        """The site tensors (left, out, in, right) from the host copy: no device is needed."""
        return [self.site_tensor(s) for s in range(len(self))]

    def mpo(self):
        """The operator as a device-resident ``MPO`` (uploaded on the first call)."""
        if self._mpo is None:
            h = c_void_p()
            _check(_lib.t4a_gpu_qt_op_to_mpo(self._h, ctypes.byref(h)))
            self._mpo = MPO._adopt(h)
        return self._mpo


def _op(status, handle):
    _check(status)
    return QuanticsOperator(handle)


def _count(value, name):
    if int(value) != value or value < 0:
        raise T4aError(INVALID_ARGUMENT, f"{name} must be a non-negative integer, got {value!r}")
    return c_size_t(int(value))


def _offset(value):
    if int(value) != value or not -(1 << 63) <= int(value) < (1 << 63):
        raise T4aError(INVALID_ARGUMENT, f"offset {value!r} is not a 64-bit integer")
    return c_int64(int(value))


def shift_operator(r, offset, bc):
    """shift_operator (shift.rs:49-62): ``(M g)[x] = g[x - offset]``; any offset, negative or beyond 2^r."""
    h = c_void_p()
    return _op(_lib.t4a_gpu_qt_shift_operator(_count(r, "r"), _offset(offset), c_int32(bc), ctypes.byref(h)), h)


def shift_operator_multivar(r, offset, bc, nvariables, target_var):
    """shift_operator_multivar (shift.rs:91-108): shift of one variable of a fused train (site index var0 + 2 var1 + ...)."""
    h = c_void_p()
    return _op(_lib.t4a_gpu_qt_shift_operator_multivar(_count(r, "r"), _offset(offset), c_int32(bc), _count(nvariables, "nvariables"),
                                                       _count(target_var, "target_var"), ctypes.byref(h)), h)


def flip_operator(r, bc):
    """flip_operator (flip.rs:44-61): x -> 2^r - x; x = 0 keeps its place with the boundary weight 1 / -1 / 0."""
    h = c_void_p()
    return _op(_lib.t4a_gpu_qt_flip_operator(_count(r, "r"), c_int32(bc), ctypes.byref(h)), h)


def flip_operator_multivar(r, bc, nvariables, target_var):
    """flip_operator_multivar (flip.rs:89-110)."""
    h = c_void_p()
    return _op(_lib.t4a_gpu_qt_flip_operator_multivar(_count(r, "r"), c_int32(bc), _count(nvariables, "nvariables"),
                                                      _count(target_var, "target_var"), ctypes.byref(h)), h)


def cumsum_operator(r):
    """cumsum_operator (cumsum.rs:76-87): ``(M g)[i] = sum_{j < i} g[j]``."""
    h = c_void_p()
    return _op(_lib.t4a_gpu_qt_cumsum_operator(_count(r, "r"), ctypes.byref(h)), h)


def triangle_operator(r, triangle):
    """triangle_operator (cumsum.rs:114-128)."""
    h = c_void_p()
    return _op(_lib.t4a_gpu_qt_triangle_operator(_count(r, "r"), c_int32(triangle), ctypes.byref(h)), h)


def identity_mpo(r):
    """identity_mpo (common.rs:675-700): ``MPO.identity([2] * r)``."""
    if r == 0:
        raise T4aError(INVALID_ARGUMENT, "Number of sites must be positive")
    return MPO.identity([2] * int(r))


def _rational(value, name, index):
    """int, Fraction or a (numerator, denominator) pair"""
    if isinstance(value, tuple):
        num, den = value
        if den == 0:
            raise T4aError(INVALID_ARGUMENT, f"{name}[{index}] has zero denominator")
        return Fraction(int(num), int(den))
    if isinstance(value, (int, np.integer)):
        return Fraction(int(value))
    if isinstance(value, Fraction):
        return value
    raise T4aError(INVALID_ARGUMENT, f"{name}[{index}] must be an int, a Fraction or a (numerator, denominator) pair")


class AffineParams:
    """AffineParams (affine.rs): y = A x + b with a rational m x n matrix, ``a`` column-major (``a[i + m * j]``)."""

    def __init__(self, a, b, m, n):
        self.m, self.n = int(m), int(n)
        self.a = [_rational(v, "affine matrix", i) for i, v in enumerate(a)]
        self.b = [_rational(v, "affine translation", i) for i, v in enumerate(b)]
        if len(self.a) != self.m * self.n:
            raise T4aError(INVALID_ARGUMENT, f"Matrix A has {len(self.a)} elements but expected {self.m}×{self.n}={self.m * self.n}")
        if len(self.b) != self.m:
            raise T4aError(INVALID_ARGUMENT, f"Vector b has {len(self.b)} elements but expected {self.m}")

    @classmethod
    def from_integers(cls, a, b, m, n):
        return cls([int(v) for v in a], [int(v) for v in b], m, n)

    def to_integer_scaled(self):
        """(a_int, b_int, scale): every entry times the least common multiple of all denominators (affine.rs:497-523)."""
        scale = 1
        for v in self.a + self.b:
            scale = scale * v.denominator // gcd(scale, v.denominator)
        return [int(v * scale) for v in self.a], [int(v * scale) for v in self.b], scale


def _int64_array(values, what):
    for v in values:
        if not -(1 << 63) <= v < (1 << 63):
            raise T4aError(INVALID_ARGUMENT, f"affine operator: {what} {v} does not fit int64")
    return np.array(values, dtype=np.int64).reshape(-1)


def _bc_list(bc):
    return [int(c) for c in bc] if isinstance(bc, (list, tuple, np.ndarray)) else [int(bc)]


def affine_operator(r, params, bc):
    """affine_operator (affine.rs:673-711): the forward map |x> -> |y = A x + b>, site dims (2^m, 2^n); ``bc`` has one entry per
    output variable.  The pull-back f(y) = g(A y + b) is ``affine_operator(...).mpo().transpose()``."""
    a_int, b_int, scale = params.to_integer_scaled()
    a = _int64_array(a_int, "coefficient")
    b = _int64_array(b_int, "translation")
    if not scale < (1 << 63):
        raise T4aError(INVALID_ARGUMENT, f"affine operator: the common denominator {scale} does not fit int64")
    conditions = np.array(_bc_list(bc), dtype=np.int32).reshape(-1)
    h = c_void_p()
    return _op(_lib.t4a_gpu_qt_affine_operator(_count(r, "r"), _p(a) if a.size else None, c_size_t(a.size), _p(b) if b.size else None,
                                               c_size_t(b.size), c_int64(scale), c_size_t(params.m), c_size_t(params.n),
                                               _p(conditions) if conditions.size else None, c_size_t(conditions.size),
                                               ctypes.byref(h)), h)


def affine_transform_matrix(r, params, bc):
    """affine_transform_matrix (affine.rs:820-934): the dense 2^(r m) x 2^(r n) matrix of ``affine_operator`` by brute force over
    every (x, y) — for verification at small sizes (``r * (m + n) <= 20``).  Flat indices are ``v0 + 2^r v1 + ...``."""
    r, m, n = int(r), params.m, params.n
    conditions = _bc_list(bc)
    if r == 0:
        raise T4aError(INVALID_ARGUMENT, "Number of bits must be positive")
    if len(conditions) != m:
        raise T4aError(INVALID_ARGUMENT, f"Boundary conditions length {len(conditions)} doesn't match output dimensions {m}")
    if r * (m + n) > 20:
        raise T4aError(INVALID_ARGUMENT, f"affine_transform_matrix: r * (m + n) = {r * (m + n)} exceeds 20")
    a, b, scale = params.to_integer_scaled()
    size, mask = 1 << r, (1 << r) - 1
    out = np.zeros((1 << (r * m), 1 << (r * n)))
    for x_flat in range(1 << (r * n)):
        x = [(x_flat >> (r * j)) & mask for j in range(n)]
        # per output variable: every y_i with a x + b - scale y_i a multiple of 2^r (zero when Open), and its weight
        choices = []
        for i in range(m):
            v = b[i] + sum(a[i + m * j] * x[j] for j in range(n))
            fits = []
            for y in range(size):
                diff = v - scale * y
                if conditions[i] == BoundaryCondition.Open:
                    if diff == 0:
                        fits.append((y, 1.0))
                elif diff % size == 0:
                    wraps = diff // size
                    fits.append((y, -1.0 if conditions[i] == BoundaryCondition.AntiPeriodic and wraps % 2 else 1.0))
            choices.append(fits)
        rows = [(0, 1.0)]
        for i, fits in enumerate(choices):
            rows = [(y_flat | (y << (r * i)), w * wi) for y_flat, w in rows for y, wi in fits]
        for y_flat, w in rows:
            out[y_flat, x_flat] += w
    return out


def difference_kernel_mpo(f, bc):
    """difference_kernel_mpo (difference_kernel.rs:29-107): the MPO of ``A[x, x'] = f((x - x') mod 2^r)`` (times -1 for x < x'
    when AntiPeriodic) from a ``SimpleTensorTrain`` with binary sites; ``f`` stays on the device, the bonds are twice ``f``'s."""
    h = c_void_p()
    _check(_lib.t4a_gpu_qt_difference_kernel(f._h, c_int32(bc), ctypes.byref(h)))
    return MPO._adopt(h)


def apply(op, tt, algorithm=ContractionAlgorithm.Naive, options=None):
    """Apply an operator (``QuanticsOperator`` or ``MPO``) to a state: ``MPO.from_tensor_train`` -> contraction ->
    ``to_tensor_train``.  Naive with ``options=None`` is the exact product ``contract_naive(op, state, None)``; otherwise
    ``mpo.contract(op, state, algorithm, options)`` truncates."""
    in_dims = [d for _, d in op.site_dims()]
    state_dims = tt.site_dims()
    if len(in_dims) != len(state_dims):
        raise T4aError(INVALID_ARGUMENT, f"operator has {len(in_dims)} sites, the state has {len(state_dims)}")
    for s, (want, got) in enumerate(zip(in_dims, state_dims)):
        if want != got:
            raise T4aError(INVALID_ARGUMENT, f"Shared shape mismatch at site {s}: operator has input dim {want}, the state has site dim {got}")
    m = op.mpo() if isinstance(op, QuanticsOperator) else op
    state = MPO.from_tensor_train(tt)
    if options is None and algorithm == ContractionAlgorithm.Naive:
        out = contract_naive(m, state, None)
    else:
        out = contract(m, state, algorithm, options)
    return out.to_tensor_train()
