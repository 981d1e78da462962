"""Partial contraction of two MPOs: every leg is contracted, identified (diagonal) or kept — partial_contract with
PartialContractionSpec of tensor4all-treetn (treetn/partial_contraction.rs), on a chain and by position.

A leg is ``(site, leg)`` with leg 0 or 1 of the site tensor (left, leg 0, leg 1, right); a tensor train is an MPO whose second leg
is 1.  A pair is ``((site, leg_a), (site, leg_b))``.  At a site the legs fall into three groups, each fused with the first leg
fastest: S, the legs of ``a`` in no contract pair (a diagonal pair keeps a's leg); K, the contract pairs; T, the legs of ``b`` in no
pair.  The result is an MPO with site dims (|S|, |T|).  ``hadamard`` is the elementwise product f(x)·g(x) with an SVD-controlled
error.  Pairs across two sites and ``output_order`` raise NOT_IMPLEMENTED; the site and half products are HIP kernels of their own
(csrc/kernels_partial.hip), no copy tensor is multiplied into an operand.
"""
import ctypes

import numpy as np

from . import _lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, c_size_t, c_double, c_int32, c_void_p
from .mpo import MPO, ContractionAlgorithm, ContractionOptions, FitOptions


class PartialContractionSpec:
    """PartialContractionSpec (partial_contraction.rs): ``contract_pairs`` are summed away, ``diagonal_pairs`` identified with the
    leg of the first operand kept.  ``output_order`` is accepted to answer NOT_IMPLEMENTED as the C ABI does."""

    def __init__(self, contract_pairs=(), diagonal_pairs=(), output_order=None):
        self.contract_pairs = [self._pair(p) for p in contract_pairs]
        self.diagonal_pairs = [self._pair(p) for p in diagonal_pairs]
        self.output_order = None if output_order is None else list(output_order)

    @staticmethod
    def _pair(p):
        try:
            (sa, la), (sb, lb) = p
            quad = (int(sa), int(la), int(sb), int(lb))
        except (TypeError, ValueError):
            raise T4aError(INVALID_ARGUMENT, "partial_contract: a pair is ((site, leg), (site, leg))") from None
        if min(quad) < 0:
            raise T4aError(INVALID_ARGUMENT, "partial_contract: a pair is ((site, leg), (site, leg)) of non-negative numbers")
        return ((quad[0], quad[1]), (quad[2], quad[3]))

    @classmethod
    def matrix_product(cls, n):
        """C(x, z) = sum_y A(x, y) B(y, z): what contract_naive / contract_zipup / contract_fit compute."""
        return cls(contract_pairs=[((i, 1), (i, 0)) for i in range(n)])

    @classmethod
    def hadamard(cls, n):
        """C(x, y) = A(x, y) B(x, y); the result has site dims (x0 * x1, 1)."""
        return cls(diagonal_pairs=[((i, leg), (i, leg)) for i in range(n) for leg in (0, 1)])

    def _c(self):
        """(contract array, n, diagonal array, n, n_output_order) as the C ABI takes them"""
        out = []
        for pairs in (self.contract_pairs, self.diagonal_pairs):
            flat = np.array([[a[0], a[1], b[0], b[1]] for a, b in pairs], dtype=np.uintp).reshape(-1)
            keep = np.ascontiguousarray(flat) if len(pairs) else np.zeros(4, dtype=np.uintp)
            out += [keep, len(pairs)]
        return out + [0 if self.output_order is None else max(len(self.output_order), 1)]


def _spec_args(spec, with_order=True):
    if not isinstance(spec, PartialContractionSpec):
        raise T4aError(INVALID_ARGUMENT, "partial_contract: spec must be a PartialContractionSpec")
    c, nc, d, nd, no = spec._c()
    args = [_p(c) if nc else None, c_size_t(nc), _p(d) if nd else None, c_size_t(nd)]
    return (args + [c_size_t(no)] if with_order else args), (c, d)


def _site_dims(dims):
    d = np.asarray(dims, dtype=np.int64)
    if d.size == 0:
        return np.zeros((0, 2), dtype=np.uintp)
    if d.ndim != 2 or d.shape[1] != 2 or (d < 0).any():
        raise T4aError(INVALID_ARGUMENT, "partial_plan: site dims are (leg 0, leg 1) per site")
    return np.ascontiguousarray(d.astype(np.uintp))


def partial_plan(a_dims, b_dims, spec):
    """The host plan (t4a_gpu_mpo_partial_plan, no device needed): ``a_dims`` / ``b_dims`` are the (leg 0, leg 1) dims per site.
    Returns ``{"site_dims": [(|S|, |T|), ...], "s_legs": [[dims of the legs of S], ...], "t_legs": [[...], ...]}`` or raises the
    error of the spec."""
    a, b = _site_dims(a_dims), _site_dims(b_dims)
    args, keep = _spec_args(spec)
    n = len(a)
    sd = np.zeros(max(2 * n, 1), dtype=np.uintp)
    legs = np.zeros(max(4 * n, 1), dtype=np.uintp)
    _check(_lib.t4a_gpu_mpo_partial_plan(_p(a) if len(a) else None, c_size_t(len(a)), _p(b) if len(b) else None, c_size_t(len(b)), *args,
                                         _p(sd), _p(legs)))
    legs = legs[:4 * n].reshape(-1, 4)
    return {"site_dims": [(int(s), int(t)) for s, t in sd[:2 * n].reshape(-1, 2)],
            "s_legs": [[int(x) for x in row[:2] if x] for row in legs],
            "t_legs": [[int(x) for x in row[2:] if x] for row in legs]}


def partial_contract(a, b, spec, algorithm=ContractionAlgorithm.Naive, options=None):
    """partial_contract (t4a_gpu_mpo_partial_contract).  Naive: the exact site-wise product for ``options`` None, else compressed as
    contract_naive compresses; ZipUp: always truncates (``options`` None = ContractionOptions()); Fit raises NOT_IMPLEMENTED, as
    ``contract`` does — the fit is ``partial_contract_fit``."""
    o = ContractionOptions() if options is None else options
    compress = options is not None or algorithm != ContractionAlgorithm.Naive
    args, keep = _spec_args(spec)
    h = c_void_p()
    _check(_lib.t4a_gpu_mpo_partial_contract(a._h, b._h, *args, c_int32(algorithm), c_int32(1 if compress else 0),
                                             c_int32(o.factorize_method), c_double(o.tolerance),
                                             c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim), ctypes.byref(h)))
    return MPO._adopt(h)


def partial_contract_fit(a, b, spec, options=None, initial=None, return_info=False):
    """contract_fit for a spec (t4a_gpu_mpo_partial_contract_fit): options, initial (site dims (|S|, |T|)) and info as there."""
    o = (FitOptions() if options is None else options).to_c()
    if initial is not None and not isinstance(initial, MPO):
        raise T4aError(INVALID_ARGUMENT, "contract_fit: initial must be an MPO")
    args, keep = _spec_args(spec)
    h = c_void_p()
    n_sweeps = c_size_t(0)
    norms = np.full(o.max_sweeps + 1, np.nan)
    _check(_lib.t4a_gpu_mpo_partial_contract_fit(a._h, b._h, *args, ctypes.byref(o), initial._h if initial is not None else None,
                                                 ctypes.byref(h), ctypes.byref(n_sweeps), _p(norms)))
    m = MPO._adopt(h)
    if not return_info:
        return m
    k = n_sweeps.value
    return m, {"n_sweeps": k, "norms": [float(v) for v in norms[:k + 1]] if k else [], "link_dims": m.link_dims()}


def _partial_half(env, side, a, b, spec, site):
    """Test hook (t4a_gpu_mpo_partial_half): side 0, env L[n, la, lb] -> P[n, s, t, ra, rb]; side 1, env R[ra, rb, n] ->
    Q[la, lb, s, t, n], with the groups of ``spec`` at ``site``."""
    env = np.asarray(env, dtype=np.float64)
    if env.ndim != 3:
        raise T4aError(INVALID_ARGUMENT, "partial_half: the environment has three legs")
    s, t = partial_plan(a.site_dims(), b.site_dims(), spec)["site_dims"][site]
    la, _, _, ra = (int(x) for x in a.dims()[site])
    lb, _, _, rb = (int(x) for x in b.dims()[site])
    n = env.shape[2] if side == 1 else env.shape[0]
    if env.shape != ((ra, rb, n) if side == 1 else (n, la, lb)):
        raise T4aError(INVALID_ARGUMENT, f"partial_half: the environment has shape {env.shape}")
    shape = (la, lb, s, t, n) if side == 1 else (n, s, t, ra, rb)
    out = np.zeros(max(int(np.prod(shape)), 1))
    flat = np.ascontiguousarray(env.reshape(-1, order="F")) if env.size else np.zeros(1)
    args, keep = _spec_args(spec, with_order=False)
    _check(_lib.t4a_gpu_mpo_partial_half(_p(flat), c_size_t(n), c_int32(side), a._h, b._h, *args, c_size_t(site), _p(out)))
    return out[:int(np.prod(shape))].reshape(shape, order="F")


def _relabel(m, site_dims):
    sd = np.ascontiguousarray(np.asarray(site_dims, dtype=np.uintp).reshape(-1))
    _check(_lib.t4a_gpu_mpo_relabel_site_dims(m._h, _p(sd) if sd.size else None, c_size_t(sd.size // 2)))
    return m


def hadamard(a, b, algorithm=ContractionAlgorithm.ZipUp, options=None):
    """The elementwise product: of two MPOs, C(x, y) = A(x, y) B(x, y), returned with the site dims of ``a``; of two
    SimpleTensorTrains, f(x) g(x), returned as a train.  Deterministic, with the SVD rank rule of ``options`` (the product of a
    train with itself has bond chi (chi + 1) / 2, which the rule finds by cutting exact zeros)."""
    trains = isinstance(a, SimpleTensorTrain) and isinstance(b, SimpleTensorTrain)
    if trains:
        a, b = MPO.from_tensor_train(a), MPO.from_tensor_train(b)
    elif not (isinstance(a, MPO) and isinstance(b, MPO)):
        raise T4aError(INVALID_ARGUMENT, "hadamard: two MPOs or two SimpleTensorTrains are needed")
    dims = a.site_dims()
    c = partial_contract(a, b, PartialContractionSpec.hadamard(len(a)), algorithm, options)
    return c.to_tensor_train() if trains else _relabel(c, dims)
