"""MPO<f64> and the contraction of two MPOs (tensor4all-simplett/src/mpo/) — site tensors (left, s1, s2, right) live on the device.

Mirrors the Rust module ``mpo``: ``MPO``, ``ContractionOptions``, ``ContractionAlgorithm``, ``FactorizeMethod``, ``contract``,
``contract_naive``, ``contract_zipup``.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, c_size_t, c_double, c_int32, c_void_p)


class ContractionAlgorithm:
    """ContractionAlgorithm (mpo/dispatch.rs:8-16)."""
    Naive, ZipUp, Fit = 0, 1, 2


class FactorizeMethod:
    """FactorizeMethod (mpo/factorize.rs:12-20); LU and CI fall back to SVD, RSVD is not implemented (as in the reference)."""
    SVD, RSVD, LU, CI = 0, 1, 2, 3


class ContractionOptions:
    """ContractionOptions (mpo/contraction.rs:17-42); the defaults are ContractionOptions::default()."""

    def __init__(self, tolerance=1e-12, max_bond_dim=None, factorize_method=FactorizeMethod.SVD):
        self.tolerance = tolerance
        self.max_bond_dim = max_bond_dim
        self.factorize_method = factorize_method


class MPO:
    """MPO<f64> (simplett/src/mpo/mpo.rs) — site tensors (left, s1, s2, right) live on the device."""

    def __init__(self, tensors):
        tensors = [np.asarray(t, dtype=np.float64) for t in tensors]
        for t in tensors:
            if t.ndim != 4:
                raise T4aError(INVALID_ARGUMENT, "site tensors must have four legs (left, s1, s2, right)")
        dims = np.array([t.shape for t in tensors], dtype=np.uintp).reshape(-1)
        flat = np.ascontiguousarray(np.concatenate([t.reshape(-1, order="F") for t in tensors])
                                    if tensors else np.zeros(1))
        self._h = c_void_p()
        _check(_lib.t4a_gpu_mpo_new(_p(dims) if len(tensors) else None, c_size_t(len(tensors)), _p(flat),
                                    ctypes.byref(self._h)))

    @classmethod
    def _adopt(cls, handle):
        self = cls.__new__(cls)
        self._h = handle
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.t4a_gpu_mpo_release(h)
            self._h = None

    @classmethod
    def zeros(cls, site_dims):
        """MPO::zeros (mpo.rs:69-78): bond dimension 1 everywhere."""
        return cls([np.zeros((1, int(d1), int(d2), 1)) for d1, d2 in site_dims])

    @classmethod
    def constant(cls, site_dims, value):
        """MPO::constant (mpo.rs:80-138): ones everywhere, `value` on the last site."""
        tensors = [np.ones((1, int(d1), int(d2), 1)) for d1, d2 in site_dims]
        if tensors:
            tensors[-1] = tensors[-1] * value
        return cls(tensors)

    @classmethod
    def identity(cls, site_dims):
        """MPO::identity (mpo.rs:140-164)."""
        return cls([np.eye(int(d)).reshape(1, int(d), int(d), 1) for d in site_dims])

    @classmethod
    def from_tensor_train(cls, tt):
        """A state as an MPO: site dims (d, 1), the cores copied unchanged (t4a_gpu_mpo_from_tt)."""
        h = c_void_p()
        _check(_lib.t4a_gpu_mpo_from_tt(tt._h, ctypes.byref(h)))
        return cls._adopt(h)

    def to_tensor_train(self):
        """SimpleTensorTrain over the fused site index s1 + S1 * s2 (t4a_gpu_mpo_to_tt)."""
        h = c_void_p()
        _check(_lib.t4a_gpu_mpo_to_tt(self._h, ctypes.byref(h)))
        return SimpleTensorTrain._adopt(h)

    def clone(self):
        h = c_void_p()
        _check(_lib.t4a_gpu_mpo_clone(self._h, ctypes.byref(h)))
        return MPO._adopt(h)

    def transpose(self):
        """s1 <-> s2 of every site (LinearOperator::transpose), permuted on the device (t4a_gpu_mpo_transpose)."""
        h = c_void_p()
        _check(_lib.t4a_gpu_mpo_transpose(self._h, ctypes.byref(h)))
        return MPO._adopt(h)

    def __len__(self):
        v = c_size_t(0)
        _check(_lib.t4a_gpu_mpo_len(self._h, ctypes.byref(v)))
        return v.value

    def len(self):
        return len(self)

    def dims(self):
        """(n_sites, 4) array of (left, s1, s2, right)."""
        n = len(self)
        d = np.zeros(max(4 * n, 1), dtype=np.uintp)
        _check(_lib.t4a_gpu_mpo_dims(self._h, _p(d)))
        return d[:4 * n].reshape(-1, 4).astype(np.int64)

    def site_dims(self):
        return [(int(a), int(b)) for a, b in self.dims()[:, 1:3]]

    def link_dims(self):
        return [int(x) for x in self.dims()[1:, 0]]

    def rank(self):
        ld = self.link_dims()
        return max(ld) if ld else 1

    def site_tensor(self, site):
        if not 0 <= site < len(self):
            raise T4aError(INVALID_ARGUMENT, "site out of range")
        l, s1, s2, r = (int(x) for x in self.dims()[site])
        buf = np.zeros(max(l * s1 * s2 * r, 1))
        _check(_lib.t4a_gpu_mpo_site_tensor(self._h, c_size_t(site), _p(buf)))
        return buf[:l * s1 * s2 * r].reshape((l, s1, s2, r), order="F")

    def site_tensors(self):
        return [self.site_tensor(s) for s in range(len(self))]

    def evaluate(self, indices):
        """evaluate (mpo.rs:245-340): indices [i1, j1, i2, j2, ...] -> float; a 2-D array (n_pts, 2 n) -> values."""
        n = len(self)
        idx = np.asarray(indices, dtype=np.int64)
        single = idx.ndim == 1
        idx = idx.reshape(1, -1) if single else idx
        if idx.ndim != 2 or idx.shape[1] != 2 * n:
            raise T4aError(INVALID_ARGUMENT, f"Expected {2 * n} indices (2*{n}), got {idx.shape[-1]}")
        if (idx < 0).any():
            raise T4aError(INVALID_ARGUMENT, "negative index")
        idx = np.ascontiguousarray(idx.astype(np.uintp))
        out = np.zeros(idx.shape[0])
        _check(_lib.t4a_gpu_mpo_evaluate(self._h, _p(idx), c_size_t(idx.shape[0]), _p(out)))
        return float(out[0]) if single else out

    def sum(self):
        """sum (mpo.rs:341-392): over every index; the empty MPO sums to 0."""
        v = c_double(0)
        _check(_lib.t4a_gpu_mpo_sum(self._h, ctypes.byref(v)))
        return v.value

    def full_tensor(self):
        """full_tensor (mpo.rs:428-480): the dense operator of shape (s1_1, s2_1, s1_2, s2_2, ...), leftmost index fastest."""
        shape = [d for pair in self.site_dims() for d in pair]
        if not shape:
            return np.zeros(0)
        total = int(np.prod(shape))
        grid = np.indices(shape[::-1]).reshape(len(shape), -1)[::-1].T  # leftmost fastest
        return self.evaluate(grid.reshape(total, len(shape))).reshape(shape, order="F")


def _contract(a, b, algorithm, compress, options):
    o = ContractionOptions() if options is None else options
    h = c_void_p()
    _check(_lib.t4a_gpu_mpo_contract(a._h, b._h, c_int32(algorithm), c_int32(1 if compress else 0), c_int32(o.factorize_method),
                                     c_double(o.tolerance), c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim),
                                     ctypes.byref(h)))
    return MPO._adopt(h)


def contract_naive(a, b, options=None):
    """contract_naive (mpo/contract_naive.rs:41-98): the exact site-wise product (bonds la * lb) for options None, else
    compressed by right-canonicalisation and a left-to-right SVD sweep (:100-172)."""
    return _contract(a, b, ContractionAlgorithm.Naive, options is not None, options)


def contract_zipup(a, b, options=None):
    """contract_zipup (mpo/contract_zipup.rs:45-167); options None = ContractionOptions()."""
    return _contract(a, b, ContractionAlgorithm.ZipUp, True, options)


def contract(a, b, algorithm=ContractionAlgorithm.Naive, options=None):
    """contract (mpo/dispatch.rs:67-92): Naive always compresses; Fit raises NOT_IMPLEMENTED."""
    return _contract(a, b, algorithm, True, options)
