"""MPO<f64> and the contraction of two MPOs (tensor4all-simplett/src/mpo/) — site tensors (left, s1, s2, right) live on the device.

Mirrors the Rust module ``mpo``: ``MPO``, ``ContractionOptions``, ``ContractionAlgorithm``, ``FactorizeMethod``, ``contract``,
``contract_naive``, ``contract_zipup``, and the lazy product ``Contraction`` (mpo/contraction.rs:60-383).  ``contract_tci`` is this
project's: the product as an MPO by cross interpolation of its elements (the ``algorithm = :TCI`` contraction of
TensorCrossInterpolation.jl).  ``contract_fit`` with ``FitOptions`` is this project's too: the variational two-site fit the
reference reserves ``FitOptions`` for (mpo/contract_fit.rs) and implements for tree networks (tensor4all-treetn/src/treetn/fit.rs).
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, TCI2Options, c_size_t, c_double, c_int32, c_void_p)


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


class FitOptionsC(ctypes.Structure):
    """t4a_gpu_mpo_fit_options"""
    _fields_ = [("tolerance", c_double), ("has_max_bond_dim", c_int32), ("max_bond_dim", c_size_t), ("max_sweeps", c_size_t),
                ("convergence_tol", c_double), ("factorize_method", c_int32)]


class FitOptions:
    """FitOptions (mpo/contract_fit.rs:19-46); the defaults are FitOptions::default().  ``max_bond_dim=None`` is no cap."""

    def __init__(self, tolerance=1e-12, max_bond_dim=100, max_sweeps=10, convergence_tol=1e-10, factorize_method=FactorizeMethod.SVD):
        self.tolerance = tolerance
        self.max_bond_dim = max_bond_dim
        self.max_sweeps = max_sweeps
        self.convergence_tol = convergence_tol
        self.factorize_method = factorize_method

    def to_c(self):
        for name in ("tolerance", "convergence_tol"):
            v = float(getattr(self, name))
            if not (np.isfinite(v) and v >= 0.0):
                raise T4aError(INVALID_ARGUMENT, f"contract_fit: {name} must be finite and not negative")
        if self.max_bond_dim is not None and int(self.max_bond_dim) < 1:
            raise T4aError(INVALID_ARGUMENT, "contract_fit: max_bond_dim must be at least 1")
        if int(self.max_sweeps) < 0:
            raise T4aError(INVALID_ARGUMENT, "contract_fit: max_sweeps must not be negative")
        if self.factorize_method not in (0, 1, 2, 3):
            raise T4aError(INVALID_ARGUMENT, "unknown factorize method")
        return FitOptionsC(float(self.tolerance), 0 if self.max_bond_dim is None else 1,
                           0 if self.max_bond_dim is None else int(self.max_bond_dim), int(self.max_sweeps),
                           float(self.convergence_tol), int(self.factorize_method))


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

    def compress(self, options=None):
        """The compress stage of ``contract_naive`` (compress_mpo, contract_naive.rs:100-172) on a copy of this MPO
        (t4a_gpu_mpo_compress): right-canonicalisation by thin QR, then the left-to-right SVD sweep with the rank rule of ``options``
        (default ``ContractionOptions()``; the factorize method is SVD).  ``self`` is untouched."""
        o = ContractionOptions() if options is None else options
        h = c_void_p()
        _check(_lib.t4a_gpu_mpo_compress(self._h, c_double(o.tolerance), c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim),
                                         ctypes.byref(h)))
        return MPO._adopt(h)


COMPRESS_MANY_BMAX = 64  # T4A_GPU_COMPRESS_MANY_BMAX: the largest bond (after the shape-only bound) of a batched item
_ROUTES = {"auto": 0, "batched": 1, "serial": 2}


def _route_code(route):
    if route not in _ROUTES:
        raise T4aError(INVALID_ARGUMENT, f"unknown compress route {route!r}: one of 'auto', 'batched', 'serial'")
    return _ROUTES[route]


def _compress_many(mpos, options, route):
    """(results, counts) with counts = {"launches", "syncs", "n_batched", "n_serial"} as the driver counted them"""
    mpos = list(mpos)
    for m in mpos:
        if not isinstance(m, MPO):
            raise T4aError(INVALID_ARGUMENT, "compress_many: every item must be an MPO")
    o = ContractionOptions() if options is None else options
    code = _route_code(route)
    arr = (c_void_p * max(len(mpos), 1))(*[m._h for m in mpos])
    out = (c_void_p * max(len(mpos), 1))()
    counts = np.zeros(4, dtype=np.uintp)
    _check(_lib.t4a_gpu_mpo_compress_many_counted(arr, c_size_t(len(mpos)), c_double(o.tolerance),
                                                  c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim), c_int32(code), out, _p(counts)))
    res = [MPO._adopt(c_void_p(out[k])) for k in range(len(mpos))]
    return res, dict(zip(("launches", "syncs", "n_batched", "n_serial"), (int(v) for v in counts)))


def compress_many(mpos, options=None, route="auto"):
    """``[m.compress(options) for m in mpos]`` for MPOs of the same number of sites, in lock step (t4a_gpu_mpo_compress_many).
    ``route="batched"``: every item whose bonds, after the bound the shapes give, are at most ``COMPRESS_MANY_BMAX`` goes through the
    batched site-step kernels — one workgroup per item, ``2 (n - 1)`` launches and one host synchronisation for the whole call — and
    every other item through the serial stage; ``"serial"``: the serial stage for every item (the bits of ``MPO.compress``);
    ``"auto"``: ``"batched"`` when no bond of the items inside the envelope is above 16 (after the bound of the shapes) or when at
    least 16 items are inside it, else ``"serial"`` (the measured rule).  Ranks, the dense operator and the left-orthogonality of the sites
    are those of ``MPO.compress``; the gauge is not.  The operands are untouched."""
    return _compress_many(mpos, options, route)[0]


def compress_many_plan(shapes, options=None, route="auto"):
    """What ``compress_many`` will do, from shapes alone (t4a_gpu_mpo_compress_many_plan; host only, no device needed).  ``shapes``:
    per item the list of ``(l, s1, s2, r)`` per site.  Returns ``{"routes": ["batched" | "serial"], "bonds": [...], "qr_bonds": [...],
    "launches", "syncs", "n_batched"}``: per item the bounds of the result's bonds and the bonds after the right sweep (``n + 1``
    values each), and the kernel launches and host synchronisations of the batched part of the call."""
    shapes = [[tuple(int(x) for x in site) for site in item] for item in shapes]
    for item in shapes:
        for site in item:
            if len(site) != 4 or min(site) < 0:
                raise T4aError(INVALID_ARGUMENT, "compress_many_plan: a site is (l, s1, s2, r)")
    o = ContractionOptions() if options is None else options
    code = _route_code(route)
    flat = [x for item in shapes for site in item for x in site]
    dims = np.ascontiguousarray(np.array(flat or [0], dtype=np.uintp))
    lens = np.ascontiguousarray(np.array([len(item) for item in shapes] or [0], dtype=np.uintp))
    nb = sum(len(item) + 1 for item in shapes)
    batched = np.zeros(max(len(shapes), 1), dtype=np.int32)
    bonds = np.zeros(max(nb, 1), dtype=np.uintp)
    qr_bonds = np.zeros(max(nb, 1), dtype=np.uintp)
    counts = np.zeros(3, dtype=np.uintp)
    _check(_lib.t4a_gpu_mpo_compress_many_plan(_p(dims), _p(lens), c_size_t(len(shapes)), c_double(o.tolerance),
                                               c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim), c_int32(code), _p(batched), _p(bonds),
                                               _p(qr_bonds), _p(counts)))
    out = {"routes": ["batched" if batched[k] else "serial" for k in range(len(shapes))], "bonds": [], "qr_bonds": [],
           "launches": int(counts[0]), "syncs": int(counts[1]), "n_batched": int(counts[2])}
    at = 0
    for item in shapes:
        out["bonds"].append([int(v) for v in bonds[at:at + len(item) + 1]])
        out["qr_bonds"].append([int(v) for v in qr_bonds[at:at + len(item) + 1]])
        at += len(item) + 1
    return out


def _truncate_args(n_items, policies, max_bond_dims, who):
    """one policy and one cap per item, or one of either for all -> (SvdPolicyC array, uintp array)"""
    from . import SvdPolicyC, SvdTruncationPolicy
    if policies is None or isinstance(policies, SvdTruncationPolicy):
        policies = [policies] * n_items
    if max_bond_dims is None or isinstance(max_bond_dims, (int, np.integer)):
        max_bond_dims = [max_bond_dims] * n_items
    policies, max_bond_dims = list(policies), list(max_bond_dims)
    if len(policies) != n_items or len(max_bond_dims) != n_items:
        raise T4aError(INVALID_ARGUMENT, f"{who}: {len(policies)} policies and {len(max_bond_dims)} caps for {n_items} items")
    pol = (SvdPolicyC * max(n_items, 1))()
    for k, p in enumerate(policies):
        pol[k] = (SvdTruncationPolicy() if p is None else p).to_c()
    for c in max_bond_dims:
        if c is not None and int(c) < 1:
            raise T4aError(INVALID_ARGUMENT, f"{who}: max_bond_dim must be at least 1")
    caps = np.ascontiguousarray(np.array([0 if c is None else int(c) for c in max_bond_dims] or [0], dtype=np.uintp))
    return pol, caps


def _truncate_many(mpos, policies, max_bond_dims, route, ranks_only, trace=False):
    """(results or None, bonds, counts[, trace]) as the driver counted them"""
    mpos = list(mpos)
    for m in mpos:
        if not isinstance(m, MPO):
            raise T4aError(INVALID_ARGUMENT, "truncate_many: every item must be an MPO")
    code = _route_code(route)
    pol, caps = _truncate_args(len(mpos), policies, max_bond_dims, "truncate_many")
    arr = (c_void_p * max(len(mpos), 1))(*[m._h for m in mpos])
    n = len(mpos[0]) if mpos else 0
    bonds = np.zeros(max(len(mpos) * (n + 1), 1), dtype=np.uintp)
    counts = np.zeros(4, dtype=np.uintp)
    names = ("launches", "syncs", "n_batched", "n_serial")
    if trace:
        steps2 = 2 * max(n - 1, 0)
        norm2 = np.zeros(max(len(mpos), 1))
        ranks = np.zeros(max(len(mpos) * steps2, 1), dtype=np.int32)
        sv = np.zeros(max(len(mpos) * steps2 * 64, 1))
        _check(_lib.t4a_gpu_mpo_truncate_many_trace(arr, c_size_t(len(mpos)), pol, _p(caps), c_int32(code), _p(bonds), _p(counts), _p(norm2),
                                                    _p(ranks), _p(sv)))
        tr = {"norm2": norm2[:len(mpos)], "ranks": ranks[:len(mpos) * steps2].reshape(len(mpos), steps2),
              "sv": sv[:len(mpos) * steps2 * 64].reshape(len(mpos), steps2, 64)}
        return None, bonds[:len(mpos) * (n + 1)].reshape(len(mpos), n + 1).astype(np.int64).tolist(), dict(zip(names, (int(v) for v in counts))), tr
    out = (c_void_p * max(len(mpos), 1))()
    _check(_lib.t4a_gpu_mpo_truncate_many_counted(arr, c_size_t(len(mpos)), pol, _p(caps), c_int32(code), c_int32(1 if ranks_only else 0),
                                                  None if ranks_only else out, _p(bonds), _p(counts)))
    res = None if ranks_only else [MPO._adopt(c_void_p(out[k])) for k in range(len(mpos))]
    return res, bonds[:len(mpos) * (n + 1)].reshape(len(mpos), n + 1).astype(np.int64).tolist(), dict(zip(names, (int(v) for v in counts)))


def truncate_many(mpos, policies=None, max_bond_dims=None, route="auto", ranks_only=False):
    """``TensorTrain::truncate`` for MPOs of the same number of sites, in lock step, each under its own rule
    (t4a_gpu_mpo_truncate_many): canonicalise onto the last site, then truncate every bond twice — from ``n - 1`` down to ``0`` and
    back — with ``policies[k]`` (an ``SvdTruncationPolicy``; all eight combinations) and ``max_bond_dims[k]`` (``None``: no cap); one
    policy or one cap stands for all items.  Routes and envelope as ``compress_many``; the batched part is ``3 (n - 1)`` launches and
    one host synchronisation.  ``ranks_only=True`` runs the same launches and returns the bonds (``n + 1`` per item) in place of
    the MPOs.  The operands are untouched."""
    res, bonds, _ = _truncate_many(mpos, policies, max_bond_dims, route, ranks_only)
    return bonds if ranks_only else res


def truncate_many_plan(shapes, max_bond_dims=None, route="auto", rules_from_norms=False):
    """What ``truncate_many`` will do, from shapes alone (t4a_gpu_mpo_truncate_many_plan; host only).  As ``compress_many_plan``;
    ``launches`` is ``3 (n - 1)``, ``syncs`` 1 — 2 with ``rules_from_norms``, the call shape of the patching driver, which reads the
    norms after the QR sweep to derive its budgets."""
    shapes = [[tuple(int(x) for x in site) for site in item] for item in shapes]
    for item in shapes:
        for site in item:
            if len(site) != 4 or min(site) < 0:
                raise T4aError(INVALID_ARGUMENT, "truncate_many_plan: a site is (l, s1, s2, r)")
    code = _route_code(route)
    _, caps = _truncate_args(len(shapes), None, max_bond_dims, "truncate_many_plan")
    flat = [x for item in shapes for site in item for x in site]
    dims = np.ascontiguousarray(np.array(flat or [0], dtype=np.uintp))
    lens = np.ascontiguousarray(np.array([len(item) for item in shapes] or [0], dtype=np.uintp))
    nb = sum(len(item) + 1 for item in shapes)
    batched = np.zeros(max(len(shapes), 1), dtype=np.int32)
    bonds = np.zeros(max(nb, 1), dtype=np.uintp)
    qr_bonds = np.zeros(max(nb, 1), dtype=np.uintp)
    counts = np.zeros(3, dtype=np.uintp)
    _check(_lib.t4a_gpu_mpo_truncate_many_plan(_p(dims), _p(lens), c_size_t(len(shapes)), _p(caps), c_int32(code),
                                               c_int32(1 if rules_from_norms else 0), _p(batched), _p(bonds), _p(qr_bonds), _p(counts)))
    out = {"routes": ["batched" if batched[k] else "serial" for k in range(len(shapes))], "bonds": [], "qr_bonds": [],
           "launches": int(counts[0]), "syncs": int(counts[1]), "n_batched": int(counts[2])}
    at = 0
    for item in shapes:
        out["bonds"].append([int(v) for v in bonds[at:at + len(item) + 1]])
        out["qr_bonds"].append([int(v) for v in qr_bonds[at:at + len(item) + 1]])
        at += len(item) + 1
    return out


def _time_compress_many(mpos, options=None, reps=5):
    """Probe (t4a_gpu_mpo_time_compress_many): ms per repetition of (the serial stage item by item, one batched call) on copies."""
    mpos = list(mpos)
    o = ContractionOptions() if options is None else options
    arr = (c_void_p * max(len(mpos), 1))(*[m._h for m in mpos])
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_mpo_time_compress_many(arr, c_size_t(len(mpos)), c_double(o.tolerance),
                                               c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim), c_size_t(reps), _p(ms)))
    return float(ms[0]), float(ms[1])


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


def contract_fit(a, b, options=None, initial=None, return_info=False):
    """The truncated product C ~ A·B by the variational two-site fit (t4a_gpu_mpo_contract_fit; this project's, the reference's
    contract_fit answers Unsupported and ``contract(a, b, ContractionAlgorithm.Fit)`` keeps doing so).  ``options``: a FitOptions,
    default FitOptions(); ``initial``: the MPO the sweeps start from (same length and site dims as the product, any bonds), default
    the zip-up product with the same tolerance, cap and method.  ``return_info=True`` gives ``(mpo, info)`` with info
    ``{"n_sweeps", "norms", "link_dims"}``: norms[0] belongs to the start, norms[k] to sweep k; it is empty when no sweep ran
    (max_sweeps == 0, fewer than two sites)."""
    o = (FitOptions() if options is None else options).to_c()
    if initial is not None and not isinstance(initial, MPO):
        raise T4aError(INVALID_ARGUMENT, "contract_fit: initial must be an MPO")
    h = c_void_p()
    n_sweeps = c_size_t(0)
    norms = np.full(o.max_sweeps + 1, np.nan)
    _check(_lib.t4a_gpu_mpo_contract_fit(a._h, b._h, ctypes.byref(o), initial._h if initial is not None else None, ctypes.byref(h),
                                         ctypes.byref(n_sweeps), _p(norms)))
    m = MPO._adopt(h)
    if not return_info:
        return m
    k = n_sweeps.value
    return m, {"n_sweeps": k, "norms": [float(v) for v in norms[:k + 1]] if k else [], "link_dims": m.link_dims()}


def _fit_half(env, side, a, b, site):
    """Test hook (t4a_gpu_mpo_fit_half): side 0, env L[n, la, lb] -> P[n, s1, s2, ra, rb]; side 1, env R[ra, rb, n] ->
    Q[la, lb, s1, s2, n], with the dims of site ``site`` of ``a`` and ``b``."""
    env = np.asarray(env, dtype=np.float64)
    if env.ndim != 3:
        raise T4aError(INVALID_ARGUMENT, "fit_half: the environment has three legs")
    la, s1, _, ra = (int(x) for x in a.dims()[site])
    lb, _, s2, rb = (int(x) for x in b.dims()[site])
    n = env.shape[2] if side == 1 else env.shape[0]
    if env.shape != ((ra, rb, n) if side == 1 else (n, la, lb)):
        raise T4aError(INVALID_ARGUMENT, f"fit_half: the environment has shape {env.shape}")
    shape = (la, lb, s1, s2, n) if side == 1 else (n, s1, s2, ra, rb)
    out = np.zeros(max(int(np.prod(shape)), 1))
    flat = np.ascontiguousarray(env.reshape(-1, order="F")) if env.size else np.zeros(1)
    _check(_lib.t4a_gpu_mpo_fit_half(_p(flat), c_size_t(n), c_int32(side), a._h, b._h, c_size_t(site), _p(out)))
    return out[:int(np.prod(shape))].reshape(shape, order="F")


def _index_pairs(indices, n, need, exact):
    """[(i1, j1), ...] or an (n_pts, m, 2) array -> ((n_pts, n, 2) uintp array padded with zeros behind the m pairs given, single).
    m must equal `need` (exact) or reach it; the messages are those of contraction.rs:187-192, :275-279, :340-348."""
    idx = np.asarray(indices, dtype=np.int64)
    if idx.size == 0 and idx.ndim < 3:
        idx = idx.reshape(0, 2)
    single = idx.ndim == 2
    idx = idx[None] if single else idx
    if idx.ndim != 3 or idx.shape[2] != 2:
        raise T4aError(INVALID_ARGUMENT, "indices must be [(i1, j1), ...] or an (n_pts, n, 2) array")
    got = idx.shape[1]
    if exact and got != need:
        raise T4aError(INVALID_ARGUMENT, f"Invalid operation: Expected {need} index pairs, got {got}")
    if got < need:
        raise T4aError(INVALID_ARGUMENT, f"Invalid operation: Expected at least {need} index pairs, got {got}")
    if (idx < 0).any():
        raise T4aError(INVALID_ARGUMENT, "negative index")
    full = np.zeros((idx.shape[0], n, 2), dtype=np.uintp)
    k = min(got, n)
    full[:, :k] = idx[:, :k]
    return np.ascontiguousarray(full), single


def _fused_pivots(initial_pivots, n):
    """fused multi-indices -> ((n_pivots, n) uintp array, n_pivots); None or an empty list -> no pivots"""
    if initial_pivots is None or len(initial_pivots) == 0:
        return np.zeros(1, dtype=np.uintp), 0
    piv = np.asarray(initial_pivots, dtype=np.int64)
    if piv.ndim != 2 or piv.shape[1] != n:
        raise T4aError(INVALID_ARGUMENT, "Pivot length must match number of sites")
    if (piv < 0).any():
        raise T4aError(INVALID_ARGUMENT, "negative index")
    return np.ascontiguousarray(piv.astype(np.uintp)), piv.shape[0]


class Contraction:
    """Contraction<f64> (mpo/contraction.rs:60-383): single elements and left / right environments of A·B without forming the product.

    Both operands are copied on the device: ``a`` and ``b`` may be dropped afterwards.  The reference memoises environments across
    calls; this one keeps nothing between calls (``clear_cache`` is a no-op), the results are identical either way.
    An index tuple is ``[(i_1, j_1), (i_2, j_2), ...]``: ``i_k`` indexes s1 of A, ``j_k`` indexes s2 of B."""

    def __init__(self, a, b):
        self._h = c_void_p()
        self._f = None
        _check(_lib.t4a_gpu_contraction_new(a._h, b._h, ctypes.byref(self._h)))

    @classmethod
    def with_transform(cls, a, b, f):
        """Contraction::with_transform (contraction.rs:118-125): ``f`` is applied on the host to every value ``evaluate`` and
        ``evaluate_many`` return — to the whole array at once when it accepts one, else element by element.  It is not part of the
        C ABI, so ``as_callback`` (the native route) refuses a contraction that has one."""
        self = cls(a, b)
        self._f = f
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.t4a_gpu_contraction_release(h)
            self._h = None

    def __len__(self):
        v = c_size_t(0)
        _check(_lib.t4a_gpu_contraction_len(self._h, ctypes.byref(v)))
        return v.value

    def len(self):
        return len(self)

    def result_site_dims(self):
        """[(s1_a, s2_b)] per site (contraction.rs:142-147)."""
        n = len(self)
        d = np.zeros(max(2 * n, 1), dtype=np.uintp)
        _check(_lib.t4a_gpu_contraction_result_site_dims(self._h, _p(d)))
        return [(int(a), int(b)) for a, b in d[:2 * n].reshape(-1, 2)]

    def clear_cache(self):
        """clear_cache (contraction.rs:150-153): nothing is cached between calls here, so nothing happens."""
        _check(_lib.t4a_gpu_contraction_clear_cache(self._h))

    def n_evaluated(self):
        """Points evaluated so far through evaluate, evaluate_many and the native callback."""
        v = c_size_t(0)
        _check(_lib.t4a_gpu_contraction_n_evaluated(self._h, ctypes.byref(v)))
        return v.value

    def _transform(self, vals):
        if self._f is None:
            return vals
        try:
            out = np.asarray(self._f(vals), dtype=np.float64)
            if out.shape == vals.shape:
                return out
        except (TypeError, ValueError):
            pass
        return np.array([self._f(float(v)) for v in vals], dtype=np.float64)

    def _pairs(self, indices, need, exact):
        idx, single = _index_pairs(indices, len(self), need, exact)
        return (idx if idx.size else np.zeros((idx.shape[0], 1, 2), dtype=np.uintp)), single  # never a NULL buffer

    def evaluate(self, indices):
        """evaluate (contraction.rs:187-252): [(i1, j1), ...] -> float; an (n_pts, n, 2) array -> values."""
        idx, single = self._pairs(indices, len(self), True)
        out = np.zeros(idx.shape[0])
        _check(_lib.t4a_gpu_contraction_evaluate(self._h, _p(idx), c_size_t(idx.shape[0]), _p(out)))
        out = self._transform(out)
        return float(out[0]) if single else out

    def _environment(self, fn, n, indices, need):
        total = len(self)
        if n > total:  # contraction.rs:263-267, :326-330
            raise T4aError(INVALID_ARGUMENT, f"Invalid operation: Site {n} is out of range [0, {total}]")
        if n < 0:
            raise T4aError(INVALID_ARGUMENT, "negative site")
        idx, single = self._pairs(indices, need, False)
        dims = np.zeros(2, dtype=np.uintp)
        _check(fn(self._h, c_size_t(n), None, c_size_t(0), None, _p(dims)))
        rows, cols = int(dims[0]), int(dims[1])
        out = np.zeros(max(idx.shape[0] * rows * cols, 1))
        _check(fn(self._h, c_size_t(n), _p(idx), c_size_t(idx.shape[0]), _p(out), _p(dims)))
        mats = out[:idx.shape[0] * rows * cols].reshape((idx.shape[0], cols, rows)).transpose(0, 2, 1)
        return mats[0].copy() if single else mats.copy()

    def evaluate_left(self, n, indices):
        """evaluate_left (contraction.rs:262-314): the ra x rb environment of sites 0 .. n-1; [[1]] for n == 0.  At least n pairs."""
        return self._environment(_lib.t4a_gpu_contraction_evaluate_left, n, indices, 0 if n == 0 else n)

    def evaluate_right(self, n, indices):
        """evaluate_right (contraction.rs:324-383): the la x lb environment of sites n .. len-1; [[1]] for n == len.  The pairs are
        read at their absolute positions, so all len of them are needed."""
        return self._environment(_lib.t4a_gpu_contraction_evaluate_right, n, indices, 0 if n == len(self) else len(self))

    def evaluate_many(self, indices, split=None):
        """Batch evaluation with shared halves computed once (TTCache::evaluate_many, cache.rs:558-744): (values, split used);
        ``split=None`` applies find_split_heuristic."""
        idx, single = self._pairs(indices, len(self), True)
        if split is not None and split <= 0:
            raise T4aError(INVALID_ARGUMENT, f"Invalid split position: {split} (n_sites={len(self)})")
        out = np.zeros(idx.shape[0])
        used = c_size_t(0)
        _check(_lib.t4a_gpu_contraction_evaluate_many(self._h, _p(idx), c_size_t(idx.shape[0]), c_size_t(0 if split is None else split),
                                                      _p(out), ctypes.byref(used)))
        return self._transform(out), used.value

    def evaluate_matrix(self, cut, rows, cols):
        """A candidate matrix of A·B (t4a_gpu_contraction_evaluate_matrix): ``rows`` are index halves over sites 0 .. cut-1, an
        (n_rows, cut, 2) array, ``cols`` halves over sites cut .. len-1, an (n_cols, len - cut, 2) array -> the (n_rows, n_cols) array
        of (A·B)(rows[r] + cols[c]).  The environments of every half are computed once on the device and paired on the matrix cores;
        the bits of an entry depend on its two halves alone, not on the request around it.  ``cut`` may be 0 or len (halves of width
        0, e.g. ``np.zeros((1, 0, 2))``).  The transform of ``with_transform`` is applied to the result."""
        n = len(self)
        if cut < 0 or cut > n:
            raise T4aError(INVALID_ARGUMENT, f"Invalid split position: {cut} (n_sites={n})")
        halves = []
        for name, h, w in (("rows", rows, cut), ("cols", cols, n - cut)):
            h = np.asarray(h, dtype=np.int64)
            if h.size == 0 and h.ndim < 3:  # [] is no halves, [[]] one half of width 0
                count = h.shape[0] if h.ndim else 0
                h = np.zeros((count, w if count == 0 else 0, 2), dtype=np.int64)
            if h.ndim != 3 or h.shape[2] != 2:
                raise T4aError(INVALID_ARGUMENT, f"{name} must be an (n, width, 2) array of (i, j) pairs")
            if h.shape[1] != w:
                raise T4aError(INVALID_ARGUMENT, f"Invalid operation: Expected {w} index pairs, got {h.shape[1]}")
            if (h < 0).any():
                raise T4aError(INVALID_ARGUMENT, "negative index")
            halves.append(np.ascontiguousarray(h.astype(np.uintp)))
        r, c = halves
        n_rows, n_cols = r.shape[0], c.shape[0]
        out = np.zeros(max(n_rows * n_cols, 1))
        pad = np.zeros(1, dtype=np.uintp)  # never a NULL buffer
        _check(_lib.t4a_gpu_contraction_evaluate_matrix(self._h, c_size_t(cut), _p(r if r.size else pad), c_size_t(n_rows),
                                                        _p(c if c.size else pad), c_size_t(n_cols), _p(out)))
        vals = self._transform(out[:n_rows * n_cols])
        return vals.reshape(n_cols, n_rows).T.copy()

    def as_callback(self):
        """(function pointer, ctx, keepalive) for ``TensorCI2.set_callback_raw``: t4a_gpu_contraction_batch_eval over this handle, which
        takes the fused site index i + s1_a * j.  The third element keeps the contraction alive as long as the TensorCI2 holds it."""
        if self._f is not None:
            raise T4aError(INVALID_ARGUMENT, "a contraction with a transform has no native callback: the transform runs in Python")
        fn = ctypes.cast(_lib.t4a_gpu_contraction_batch_eval, c_void_p).value
        return fn, self._h.value, self


def contract_tci(a, b, options=None, initial_pivots=None, route="host"):
    """The product A·B as an MPO by cross interpolation over the fused site index i + s1_a * j (t4a_gpu_mpo_contract_tci; this
    project's).  ``options``: a TCI2Options, default tolerance 1e-12 without global pivot search; ``initial_pivots``: fused
    multi-indices, default the result of opt_first_pivot from the all-zero index.  The result carries ``tci_info``:
    termination, rank, n_evaluations, error.  ``route``: "host" feeds the TensorCI2 through the batch callback, "device" sets the
    contraction as its device matrix source (t4a_gpu_mpo_contract_tci_device): candidate matrices never leave the device; the two
    agree to rounding, not bit for bit."""
    if route not in ("host", "device"):
        raise T4aError(INVALID_ARGUMENT, f"unknown route {route!r}: \"host\" or \"device\"")
    o = (TCI2Options(tolerance=1e-12, max_nglobal_pivot=0, nsearch=0) if options is None else options).to_c()
    piv, n_piv = _fused_pivots(initial_pivots, len(a))
    h = c_void_p()
    info = np.zeros(4)
    fn = _lib.t4a_gpu_mpo_contract_tci_device if route == "device" else _lib.t4a_gpu_mpo_contract_tci
    _check(fn(a._h, b._h, ctypes.byref(o), _p(piv), c_size_t(n_piv), ctypes.byref(h), _p(info)))
    m = MPO._adopt(h)
    m.tci_info = {"termination": int(info[0]), "rank": int(info[1]), "n_evaluations": int(info[2]), "error": float(info[3])}
    return m
