"""Gauge forms of a tensor train (tensor4all-simplett/src/canonical.rs, vidal.rs) — tensors and bond vectors live on the device.

Mirrors ``SiteTensorTrain`` (canonical.rs:102-393), ``center_canonicalize`` (:439-544), ``VidalTensorTrain`` (vidal.rs:199-493) and
``InverseTensorTrain`` (:535-767) with the reference's method names.  The reference gauges with a rank-revealing LU in place of a
QR (its ``qr_decomp`` is ``rrlu`` with both tolerances zero), so the "orthogonal" cores are unit-lower-trapezoidal LU factors and
the Vidal singular values are those of the LU-gauged bond matrices — not the Schmidt values of the tensor.  This module restates
that behaviour.  ``evaluate`` / ``sum`` / ``norm2`` act on the stored tensors, like the trait ``AbstractTensorTrain``.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, c_size_t, c_void_p)


def _tensor(t):
    t = np.asarray(t, dtype=np.float64)
    if t.ndim != 3:
        raise T4aError(INVALID_ARGUMENT, "site tensors must have three legs (left, site, right)")
    dims = np.array(t.shape, dtype=np.uintp)
    flat = np.ascontiguousarray(t.reshape(-1, order="F")) if t.size else np.zeros(1)
    return dims, flat


def _vector(v):
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    return (v if v.size else np.zeros(1)), int(v.size)


class _Form:
    """What the three forms share: the trait AbstractTensorTrain on the stored tensors (traits.rs:75-355)."""
    _prefix = None

    def _fn(self, name):
        return getattr(_lib, f"t4a_gpu_{self._prefix}_{name}")

    @classmethod
    def _adopt(cls, handle):
        self = cls.__new__(cls)
        self._h = handle
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._fn("release")(h)
            self._h = None

    def _tt(self, name):
        h = c_void_p()
        _check(self._fn(name)(self._h, ctypes.byref(h)))
        return SimpleTensorTrain._adopt(h)

    def len(self):
        v = c_size_t(0)
        _check(self._fn("len")(self._h, ctypes.byref(v)))
        return v.value

    __len__ = len

    def dims(self):
        n = self.len()
        d = np.zeros(max(3 * n, 1), dtype=np.uintp)
        _check(self._fn("dims")(self._h, _p(d)))
        return d[:3 * n].reshape(-1, 3).astype(np.int64)

    def site_dims(self):
        return [int(x) for x in self.dims()[:, 1]]

    def link_dims(self):
        return [int(x) for x in self.dims()[1:, 0]]

    def rank(self):
        ld = self.link_dims()
        return max(ld) if ld else 1

    def site_tensor(self, site):
        n = self.len()
        if not 0 <= site < n:
            raise T4aError(INVALID_ARGUMENT, f"site {site} is out of range for {n} tensors")
        l, s, r = (int(x) for x in self.dims()[site])
        buf = np.zeros(max(l * s * r, 1))
        _check(self._fn("site_tensor")(self._h, c_size_t(site), _p(buf)))
        return buf[:l * s * r].reshape((l, s, r), order="F")

    def site_tensors(self):
        return [self.site_tensor(s) for s in range(self.len())]

    def tensors_tt(self):
        """The stored tensors as a plain train (a device-to-device copy)."""
        return self._tt("tensors_tt")

    def to_tensor_train(self):
        return self._tt("to_tt")

    def evaluate(self, idx):
        return self.tensors_tt().evaluate(idx)

    def sum(self):
        return self.tensors_tt().sum()

    def norm2(self):
        return self.tensors_tt().norm2()

    def _vector_of(self, name, i):
        n = c_size_t(0)
        _check(self._fn(name)(self._h, c_size_t(i), None, c_size_t(0), ctypes.byref(n)))
        out = np.zeros(max(n.value, 1))
        _check(self._fn(name)(self._h, c_size_t(i), _p(out), c_size_t(n.value), ctypes.byref(n)))
        return out[:n.value]

    def partition(self):
        a, b = c_size_t(0), c_size_t(0)
        _check(self._fn("partition")(self._h, ctypes.byref(a), ctypes.byref(b)))
        return range(a.value, b.value)


def _index(i, what="site"):
    if i < 0:
        raise T4aError(INVALID_ARGUMENT, f"negative {what}")
    return c_size_t(i)


class SiteTensorTrain(_Form):
    """SiteTensorTrain<f64> (canonical.rs:102-393): cores left of the centre are left(true) factors of the LU gauge, cores right of it
    the transposed ones."""
    _prefix = "site_tt"

    def __init__(self, tensors, center):
        """SiteTensorTrain::new(tensors, center) (canonical.rs:118-143)"""
        self._h = SiteTensorTrain.from_tensor_train(SimpleTensorTrain(tensors), center)._steal()

    def _steal(self):
        h, self._h = self._h, None
        return h

    @classmethod
    def new(cls, tensors, center):
        return cls(tensors, center)

    @classmethod
    def from_tensor_train(cls, tt, center):
        h = c_void_p()
        _check(_lib.t4a_gpu_site_tt_from_tt(tt._h, _index(center, "center"), ctypes.byref(h)))
        return cls._adopt(h)

    def center(self):
        v = c_size_t(0)
        _check(_lib.t4a_gpu_site_tt_center(self._h, ctypes.byref(v)))
        return v.value

    def partition(self):
        return range(0, self.len())

    def move_center_left(self):
        _check(_lib.t4a_gpu_site_tt_move_center_left(self._h))

    def move_center_right(self):
        _check(_lib.t4a_gpu_site_tt_move_center_right(self._h))

    def set_center(self, new_center):
        _check(_lib.t4a_gpu_site_tt_set_center(self._h, _index(new_center, "center")))

    def set_site_tensor(self, i, tensor):
        d, f = _tensor(tensor)
        _check(_lib.t4a_gpu_site_tt_set_site_tensor(self._h, _index(i), _p(d), _p(f)))

    def set_two_site_tensors(self, i, tensor1, tensor2):
        d1, f1 = _tensor(tensor1)
        d2, f2 = _tensor(tensor2)
        _check(_lib.t4a_gpu_site_tt_set_two_site_tensors(self._h, _index(i), _p(d1), _p(f1), _p(d2), _p(f2)))


def center_canonicalize(tt, center):
    """center_canonicalize(tensors, center) (canonical.rs:439-544) in place on a SimpleTensorTrain; a no-op for n <= 1 or center >= n."""
    _check(_lib.t4a_gpu_tt_center_canonicalize(tt._h, _index(center, "center")))


class VidalTensorTrain(_Form):
    """VidalTensorTrain<f64> (vidal.rs:199-493): site tensors and the bond vectors between them."""
    _prefix = "vidal_tt"

    def __init__(self, tensors, singular_values):
        """VidalTensorTrain::new(tensors, singular_values) (vidal.rs:403-428): only the number of vectors is checked."""
        ts = [_tensor(t) for t in tensors]
        svs = [_vector(v) for v in singular_values]
        dims = np.concatenate([d for d, _ in ts]) if ts else np.zeros(1, dtype=np.uintp)
        flat = np.ascontiguousarray(np.concatenate([f[:int(np.prod(d))] for d, f in ts])) if ts else np.zeros(1)
        lens = np.array([k for _, k in svs] + [0], dtype=np.uintp)
        vals = np.ascontiguousarray(np.concatenate([v[:k] for v, k in svs] + [np.zeros(1)]))
        self._h = c_void_p()
        _check(_lib.t4a_gpu_vidal_tt_new(_p(dims), c_size_t(len(ts)), _p(flat), _p(lens), c_size_t(len(svs)), _p(vals),
                                         ctypes.byref(self._h)))

    @classmethod
    def new(cls, tensors, singular_values):
        return cls(tensors, singular_values)

    @classmethod
    def from_tensor_train(cls, tt):
        return cls.from_tensor_train_with_partition(tt, range(0, len(tt)))

    @classmethod
    def from_tensor_train_with_partition(cls, tt, partition):
        """partition: a range (or a (start, end) pair) of sites, vidal.rs:229-395"""
        start, end = (partition.start, partition.stop) if isinstance(partition, range) else partition
        h = c_void_p()
        _check(_lib.t4a_gpu_vidal_tt_from_tt(tt._h, _index(start, "partition start"), _index(end, "partition end"), ctypes.byref(h)))
        return cls._adopt(h)

    def singular_values(self, i):
        return self._vector_of("singular_values", _index(i, "bond").value)

    def all_singular_values(self):
        return [self.singular_values(i) for i in range(max(self.len() - 1, 0))]

    def set_singular_values(self, i, values):
        v, k = _vector(values)
        _check(_lib.t4a_gpu_vidal_tt_set_singular_values(self._h, _index(i, "bond"), _p(v), c_size_t(k)))

    def set_site_tensor(self, i, tensor):
        d, f = _tensor(tensor)
        _check(_lib.t4a_gpu_vidal_tt_set_site_tensor(self._h, _index(i), _p(d), _p(f)))


class InverseTensorTrain(_Form):
    """InverseTensorTrain<f64> (vidal.rs:535-767): tensors scaled by the neighbouring bond vectors, and the inverse values."""
    _prefix = "inverse_tt"

    def __init__(self, vidal):
        h = c_void_p()
        _check(_lib.t4a_gpu_inverse_tt_from_vidal(vidal._h, ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_vidal(cls, vidal):
        return cls(vidal)

    @classmethod
    def from_tensor_train(cls, tt):
        h = c_void_p()
        _check(_lib.t4a_gpu_inverse_tt_from_tt(tt._h, ctypes.byref(h)))
        return cls._adopt(h)

    def inverse_singular_values(self, i):
        return self._vector_of("inverse_singular_values", _index(i, "bond").value)

    def all_inverse_singular_values(self):
        return [self.inverse_singular_values(i) for i in range(max(self.len() - 1, 0))]

    def set_two_site_tensors(self, i, tensor1, inv_sv, tensor2):
        d1, f1 = _tensor(tensor1)
        d2, f2 = _tensor(tensor2)
        v, k = _vector(inv_sv)
        _check(_lib.t4a_gpu_inverse_tt_set_two_site_tensors(self._h, _index(i), _p(d1), _p(f1), _p(v), c_size_t(k), _p(d2), _p(f2)))
