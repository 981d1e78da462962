"""swap_site_indices on a chain: which site holds which site index — SwapOptions, ScheduledSwapStep, SwapSchedule::build
(tensor4all-treetn, treetn/swap.rs), swap_on_edge and swap_site_indices (treetn/mod.rs), for f64 and by position.

A *leg train* is a device-resident tensor train over fused site indices plus, per site, an ordered list of legs ``(key, dim)``.
Keys are unique across the train and mutually comparable (tuples or numbers); the first leg of a site is the fastest in its fused
index (``s1 + S1 * s2`` of an MPO, the groups of the partial contraction); a site may hold no leg (``s = 1``) or several.  An MPO
enters with the keys ``(i, 0)``, ``(i, 1)``, a SimpleTensorTrain with ``(i, 0)``.

Leg order written by a step (this project's rule: the reference has index objects and no positional order): on both sites of a
step the legs are stored in ascending key order; sites that no step touches keep their order.  ``LegTrain.reorder_legs`` applies
any other order in one gather launch.

The schedule is host work (``SwapSchedule.build`` needs no device).  A step is one HIP kernel (csrc/kernels_swap.hip: the two sites
contracted and written, legs redistributed, as the matrix the SVD reads), the Jacobi SVD with the rank rule of ``SwapOptions``, and
the split that leaves the centre on ``node_b``.
"""
import ctypes

import numpy as np

from . import _lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, c_size_t, c_double, c_int32, c_void_p
from .mpo import MPO

ROUTE_SCALAR, ROUTE_MFMA = 1, 2
_DIAMETER = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1


class SwapOptions:
    """SwapOptions (swap.rs): ``max_bond_dim`` caps every bond a step writes, ``rtol`` cuts singular values with
    ``s / s_max <= rtol``.  ``None`` is "no truncation" (threshold 0), never a global default."""

    def __init__(self, max_bond_dim=None, rtol=None):
        self.max_bond_dim = max_bond_dim
        self.rtol = rtol

    def _c(self):
        return (c_int32(0 if self.max_bond_dim is None else 1), c_size_t(0 if self.max_bond_dim is None else int(self.max_bond_dim)),
                c_int32(0 if self.rtol is None else 1), c_double(0.0 if self.rtol is None else float(self.rtol)))


class ScheduledSwapStep:
    """One two-site update: ``transport_path`` is empty when the centre is on the edge, else ``[centre, ..., node_a]``; after the step
    the keys of ``a_side_sites`` live on ``node_a``, those of ``b_side_sites`` on ``node_b``, and the centre is ``node_b``."""

    def __init__(self, transport_path, node_a, node_b, a_side_sites, b_side_sites):
        self.transport_path = list(transport_path)
        self.node_a = node_a
        self.node_b = node_b
        self.a_side_sites = set(a_side_sites)
        self.b_side_sites = set(b_side_sites)

    def as_tuple(self):
        return (self.transport_path, self.node_a, self.node_b, self.a_side_sites, self.b_side_sites)

    def __eq__(self, other):
        return isinstance(other, ScheduledSwapStep) and self.as_tuple() == other.as_tuple()

    def __repr__(self):
        return "ScheduledSwapStep(transport_path=%r, node_a=%r, node_b=%r, a_side_sites=%r, b_side_sites=%r)" % self.as_tuple()


def _ranks(keys, what):
    """key -> int64 whose order is the order of the keys"""
    try:
        ordered = sorted(keys)
    except TypeError:
        raise T4aError(INVALID_ARGUMENT, f"{what}: leg keys must be mutually comparable") from None
    return {k: i for i, k in enumerate(ordered)}, ordered


def _i64(values):
    return np.ascontiguousarray(np.asarray(list(values), dtype=np.int64).reshape(-1))


def _usz(values):
    return np.ascontiguousarray(np.asarray(list(values), dtype=np.uintp).reshape(-1))


def _ptr(a):
    return _p(a) if a.size else None


def _nonneg(v, what):
    v = int(v)
    if v < 0:
        raise T4aError(INVALID_ARGUMENT, f"{what} must not be negative")
    return v


class SwapSchedule:
    """SwapSchedule (swap.rs): ``root`` and the ordered ``steps``; a pure function of the chain length and the two assignments."""

    def __init__(self, root, steps):
        self.root = root
        self.steps = list(steps)

    def __len__(self):
        return len(self.steps)

    @staticmethod
    def build(n_sites, current, target, root=0, dims=None, link_dims=None, max_bond_dim=None, max_passes=None):
        """SwapSchedule::build on a chain of ``n_sites`` (t4a_gpu_swap_schedule_build; no device needed).  ``current`` maps every
        leg key of the train to its site, ``target`` some of them to the site they must reach.  The base sweep from root 0 is the
        edges (i, i+1) rightwards, then (i+1, i) leftwards; at most ``max_passes`` passes run (default: the diameter n - 1).
        ``dims`` (key -> dim) adds the plan checks — at most 8 legs in a merged pair, no side above the fused-dimension limit 65535 —
        and ``link_dims`` the check that no work matrix exceeds INT_MAX elements.  Raises INVALID_ARGUMENT with the reference's
        messages."""
        current, target = dict(current), dict(target)
        for k in target:
            if k not in current:
                raise T4aError(INVALID_ARGUMENT, f"SwapSchedule::build: target_assignment contains index {k!r} which is not in the network")
        rank, ordered = _ranks(current.keys(), "SwapSchedule::build")
        ck, cs = _i64(rank[k] for k in ordered), _usz(_nonneg(current[k], "a site") for k in ordered)
        tk, ts = _i64(rank[k] for k in target), _usz(_nonneg(v, "a site") for v in target.values())
        cd = None if dims is None else _usz(_nonneg(dict(dims)[k], "a leg dimension") for k in ordered)
        ld = None if link_dims is None else _usz(_nonneg(v, "a bond") for v in link_dims)
        if ld is not None and len(ld) != max(int(n_sites) - 1, 0):
            raise T4aError(INVALID_ARGUMENT, f"SwapSchedule::build: {n_sites} sites have {max(int(n_sites) - 1, 0)} bonds, got {len(ld)}")
        if ld is not None and cd is None:
            raise T4aError(INVALID_ARGUMENT, "SwapSchedule::build: link_dims needs dims")
        h = c_void_p()
        _check(_lib.t4a_gpu_swap_schedule_build(c_size_t(_nonneg(n_sites, "n_sites")), _ptr(ck), _ptr(cs), None if cd is None or not cd.size else _p(cd),
                                                c_size_t(len(ordered)), _ptr(tk), _ptr(ts), c_size_t(len(target)),
                                                c_size_t(_nonneg(root, "root")), c_size_t(_DIAMETER if max_passes is None else _nonneg(max_passes, "max_passes")),
                                                None if ld is None or not ld.size else _p(ld),
                                                c_size_t(0 if max_bond_dim is None else int(max_bond_dim)), ctypes.byref(h)))
        try:
            n = c_size_t(0)
            _check(_lib.t4a_gpu_swap_schedule_len(h, ctypes.byref(n)))
            steps = []
            for i in range(n.value):
                sizes = np.zeros(3, dtype=np.uintp)
                _check(_lib.t4a_gpu_swap_schedule_step_sizes(h, c_size_t(i), _p(sizes)))
                path = np.zeros(max(int(sizes[0]), 1), dtype=np.uintp)
                ab = np.zeros(2, dtype=np.uintp)
                a = np.zeros(max(int(sizes[1]), 1), dtype=np.int64)
                b = np.zeros(max(int(sizes[2]), 1), dtype=np.int64)
                _check(_lib.t4a_gpu_swap_schedule_step(h, c_size_t(i), _p(path), _p(ab), _p(a), _p(b)))
                steps.append(ScheduledSwapStep([int(v) for v in path[:int(sizes[0])]], int(ab[0]), int(ab[1]),
                                               {ordered[int(v)] for v in a[:int(sizes[1])]}, {ordered[int(v)] for v in b[:int(sizes[2])]}))
        finally:
            _lib.t4a_gpu_swap_schedule_release(h)
        return SwapSchedule(int(root), steps)


def _check_legs(legs, site_dims):
    out = []
    if len(legs) != len(site_dims):
        raise T4aError(INVALID_ARGUMENT, f"LegTrain: legs are given for {len(legs)} sites of {len(site_dims)}")
    seen = set()
    for i, site in enumerate(legs):
        row = []
        for key, dim in site:
            if key in seen:
                raise T4aError(INVALID_ARGUMENT, f"LegTrain: leg key {key!r} occurs twice")
            seen.add(key)
            row.append((key, _nonneg(dim, "a leg dimension")))
        if int(np.prod([d for _, d in row], dtype=np.int64)) != int(site_dims[i]):
            raise T4aError(INVALID_ARGUMENT, f"LegTrain: the legs of site {i} do not make up its site dimension {int(site_dims[i])}")
        out.append(row)
    return out


class LegTrain:
    """A SimpleTensorTrain over fused site indices read as legs: ``legs[i]`` is the ordered list of ``(key, dim)`` of site i, first
    leg fastest.  ``center`` is the orthogonality centre when a swap left one, else None.  The train is shared, not copied."""

    def __init__(self, tt, legs, center=None):
        if not isinstance(tt, SimpleTensorTrain):
            raise T4aError(INVALID_ARGUMENT, "LegTrain: a SimpleTensorTrain over the fused site indices is needed")
        self._tt = tt
        self.legs = _check_legs([list(s) for s in legs], tt.site_dims())
        self.center = center

    @classmethod
    def from_mpo(cls, m):
        """keys (i, 0), (i, 1) with the dims (s1, s2) of site i"""
        return cls(m.to_tensor_train(), [[((i, 0), s1), ((i, 1), s2)] for i, (s1, s2) in enumerate(m.site_dims())])

    @classmethod
    def from_train(cls, tt):
        """keys (i, 0); the train is shared"""
        return cls(tt, [[((i, 0), d)] for i, d in enumerate(tt.site_dims())])

    def __len__(self):
        return len(self.legs)

    @property
    def dims(self):
        """the leg dims per site"""
        return [[d for _, d in site] for site in self.legs]

    def keys(self):
        """every key in train order: sites left to right, the legs of a site first to last"""
        return [k for site in self.legs for k, _ in site]

    def assignment(self):
        return {k: i for i, site in enumerate(self.legs) for k, _ in site}

    def link_dims(self):
        return self._tt.link_dims()

    def _flat(self, rank):
        counts = _usz(len(s) for s in self.legs)
        return counts, _i64(rank[k] for k in self.keys()), _usz(d for site in self.legs for _, d in site)

    def as_train(self):
        """The SimpleTensorTrain when every site holds exactly one leg (the shared train itself, no copy)."""
        if any(len(s) != 1 for s in self.legs):
            raise T4aError(INVALID_ARGUMENT, "LegTrain.as_train: every site must hold exactly one leg")
        return self._tt

    def as_mpo(self):
        """The MPO when every site holds exactly two legs: site dims (first leg, second leg)."""
        if any(len(s) != 2 for s in self.legs):
            raise T4aError(INVALID_ARGUMENT, "LegTrain.as_mpo: every site must hold exactly two legs")
        m = MPO.from_tensor_train(self._tt)
        sd = _usz(d for site in self.legs for _, d in site)
        _check(_lib.t4a_gpu_mpo_relabel_site_dims(m._h, _ptr(sd), c_size_t(len(self.legs))))
        return m

    def to_dense(self, keys=None):
        """The dense tensor with one axis per leg, in train order (``self.keys()``) or in the order of ``keys``."""
        cores = self._tt.site_tensors()
        if not cores:
            return np.zeros(0)
        acc = cores[0].reshape(-1, cores[0].shape[2], order="F")
        for c in cores[1:]:
            acc = (acc @ c.reshape(c.shape[0], -1, order="F")).reshape(-1, c.shape[2], order="F")
        own = self.keys()
        dense = acc.reshape([d for site in self.legs for _, d in site], order="F")
        if keys is None:
            return dense
        keys = list(keys)
        if sorted(map(repr, keys)) != sorted(map(repr, own)):
            raise T4aError(INVALID_ARGUMENT, "LegTrain.to_dense: keys must be a permutation of the train's keys")
        return np.transpose(dense, [own.index(k) for k in keys])

    def reorder_legs(self, orders):
        """``{site: [keys]}``: the legs of the named sites in the given order, in place, one gather launch over all of them
        (t4a_gpu_legtrain_reorder).  Returns self."""
        orders = {int(s): list(ks) for s, ks in dict(orders).items()}
        rank, _ = _ranks(self.keys(), "reorder_legs")
        for s, ks in orders.items():
            if not 0 <= s < len(self.legs):
                raise T4aError(INVALID_ARGUMENT, f"reorder_legs: site {s} is not in the train")
            if len(set(ks)) != len(ks) or set(ks) != {k for k, _ in self.legs[s]}:
                raise T4aError(INVALID_ARGUMENT, f"reorder_legs: the order of site {s} is not a permutation of its legs")
        counts, keys, dims = self._flat(rank)
        sites = _usz(orders.keys())
        oc = _usz(len(ks) for ks in orders.values())
        ok = _i64(rank[k] for ks in orders.values() for k in ks)
        _check(_lib.t4a_gpu_legtrain_reorder(self._tt._h, _ptr(counts), _ptr(keys), _ptr(dims), _ptr(sites), _ptr(oc), _ptr(ok), c_size_t(len(orders))))
        for s, ks in orders.items():
            d = dict(self.legs[s])
            self.legs[s] = [(k, d[k]) for k in ks]
        return self


def _as_leg_train(x, what):
    if isinstance(x, LegTrain):
        return x
    if isinstance(x, MPO):
        return LegTrain.from_mpo(x)
    if isinstance(x, SimpleTensorTrain):
        return LegTrain.from_train(x)
    raise T4aError(INVALID_ARGUMENT, f"{what}: an MPO, a SimpleTensorTrain or a LegTrain is needed")


def _swap(lt, target, options, timings=False):
    o = SwapOptions() if options is None else options
    if not isinstance(o, SwapOptions):
        raise T4aError(INVALID_ARGUMENT, "swap_site_indices: options must be SwapOptions")
    target = dict(target)
    own = set(lt.keys())
    for k in target:
        if k not in own:
            raise T4aError(INVALID_ARGUMENT, f"SwapSchedule::build: target_assignment contains index {k!r} which is not in the network")
    if not target:
        return lt, 0, None
    rank, ordered = _ranks(lt.keys(), "swap_site_indices")
    counts, keys, dims = lt._flat(rank)
    tk, ts = _i64(rank[k] for k in target), _usz(_nonneg(v, "a site") for v in target.values())
    n_legs = len(ordered)
    oc = np.zeros(max(len(lt), 1), dtype=np.uintp)
    okeys = np.zeros(max(n_legs, 1), dtype=np.int64)
    odims = np.zeros(max(n_legs, 1), dtype=np.uintp)
    moved, center, n_steps = c_int32(0), c_size_t(0), c_size_t(0)
    ms = np.zeros(3)
    h = c_void_p()
    _check(_lib.t4a_gpu_tt_swap_site_indices(lt._tt._h, _ptr(counts), _ptr(keys), _ptr(dims), _ptr(tk), _ptr(ts), c_size_t(len(target)), *o._c(),
                                             ctypes.byref(h), _p(oc), _p(okeys), _p(odims), ctypes.byref(moved), ctypes.byref(center),
                                             ctypes.byref(n_steps), _p(ms) if timings else None))
    out = SimpleTensorTrain._adopt(h)
    if not moved.value:
        return lt, 0, None
    legs, at = [], 0
    for i in range(len(lt)):
        c = int(oc[i])
        legs.append([(ordered[int(okeys[at + j])], int(odims[at + j])) for j in range(c)])
        at += c
    res = LegTrain(out, legs, center=int(center.value))
    return res, int(n_steps.value), ({"kernel_ms": float(ms[0]), "svd_ms": float(ms[1]), "qr_ms": float(ms[2])} if timings else None)


def swap_site_indices(x, target_assignment, options=None):
    """swap_site_indices (t4a_gpu_tt_swap_site_indices): ``x`` is an MPO, a SimpleTensorTrain or a LegTrain, ``target_assignment``
    maps leg keys to the site they must reach; legs it does not name stay on their side of every step.  An empty target or an
    empty schedule returns ``x`` itself, unchanged and not canonicalised.  Otherwise the result is an MPO when every site ends with
    exactly two legs, a SimpleTensorTrain when with exactly one, else a LegTrain (whose ``center`` is ``node_b`` of the last step)."""
    lt = _as_leg_train(x, "swap_site_indices")
    res, n_steps, _ = _swap(lt, target_assignment, options)
    if n_steps == 0:
        return x
    if all(len(s) == 2 for s in res.legs):
        return res.as_mpo()
    if all(len(s) == 1 for s in res.legs):
        return res.as_train()
    return res


swap_site_indices_by_index = swap_site_indices


def swap_site_indices_legs(x, target_assignment, options=None, timings=False):
    """As swap_site_indices, but the result always comes back as a LegTrain with its centre; with ``timings`` also the device ms of the
    step kernel, the SVD with the split and the QR steps."""
    lt = _as_leg_train(x, "swap_site_indices")
    res, n_steps, ms = _swap(lt, target_assignment, options, timings)
    return (res, ms) if timings else res


def quantics_target(n_sites, n_vars, to):
    """The target assignment {(i, 0): site} between the two quantics layouts of ``n_vars`` variables with R = n_sites / n_vars bits:
    interleaved x1 y1 x2 y2 ... (site = bit * n_vars + var) and sequential x1 .. xR y1 .. yR (site = var * R + bit)."""
    n_sites, n_vars = int(n_sites), int(n_vars)
    if n_vars < 1 or n_sites % n_vars:
        raise T4aError(INVALID_ARGUMENT, f"regroup_quantics: {n_sites} sites do not hold {n_vars} variables of equally many bits")
    r = n_sites // n_vars
    if to == "sequential":  # the input is interleaved
        return {(b * n_vars + v, 0): v * r + b for b in range(r) for v in range(n_vars)}
    if to == "interleaved":
        return {(v * r + b, 0): b * n_vars + v for b in range(r) for v in range(n_vars)}
    raise T4aError(INVALID_ARGUMENT, 'regroup_quantics: to is "sequential" or "interleaved"')


def regroup_quantics(tt, n_vars, to="sequential", options=None):
    """A quantics train from the interleaved layout to the variable-major one (``to="sequential"``) or back (``"interleaved"``);
    returns a SimpleTensorTrain (``tt`` itself when nothing has to move)."""
    if not isinstance(tt, SimpleTensorTrain):
        raise T4aError(INVALID_ARGUMENT, "regroup_quantics: a SimpleTensorTrain is needed")
    return swap_site_indices(tt, quantics_target(len(tt), n_vars, to), options)


def swap_theta(left_core, right_core, legs_left, legs_right, a_side, b_side, left_moving=False):
    """Test hook (t4a_gpu_swap_theta), the counterpart of ``_partial_half``: the step kernel on the host cores ``left_core[l, X, m]``
    and ``right_core[m, Y, r]`` (chain order) with the legs ``[(key, dim), ...]`` of the two sites.  After the step the keys of
    ``a_side`` live on node_a and those of ``b_side`` on node_b, in ascending order; node_a is the left site unless ``left_moving``.
    Returns ``(theta, route)``: Theta' of shape (l |left'|, |right'| r) and the ROUTE_* bits the launch took."""
    a = np.asarray(left_core, dtype=np.float64)
    b = np.asarray(right_core, dtype=np.float64)
    if a.ndim != 3 or b.ndim != 3 or a.shape[2] != b.shape[0]:
        raise T4aError(INVALID_ARGUMENT, "swap_theta: cores (l, X, m) and (m, Y, r) are needed")
    legs_left, legs_right = [tuple(g) for g in legs_left], [tuple(g) for g in legs_right]
    to_left, to_right = (b_side, a_side) if left_moving else (a_side, b_side)
    rank, _ = _ranks([k for k, _ in legs_left + legs_right], "swap_theta")
    for k in list(to_left) + list(to_right):
        if k not in rank:
            raise T4aError(INVALID_ARGUMENT, f"swap_theta: {k!r} is no leg of the two sites")
    if int(np.prod([d for _, d in legs_left], dtype=np.int64)) != a.shape[1] or int(np.prod([d for _, d in legs_right], dtype=np.int64)) != b.shape[1]:
        raise T4aError(INVALID_ARGUMENT, "swap_theta: the legs do not make up the site dimensions of the cores")
    lk, ld = _i64(rank[k] for k, _ in legs_left), _usz(d for _, d in legs_left)
    rk, rd = _i64(rank[k] for k, _ in legs_right), _usz(d for _, d in legs_right)
    tl, tr = _i64(rank[k] for k in to_left), _i64(rank[k] for k in to_right)
    total = a.shape[0] * a.shape[1] * b.shape[1] * b.shape[2]
    out = np.zeros(max(total, 1))
    mn = np.zeros(2, dtype=np.uintp)
    route = c_int32(0)
    fa = np.ascontiguousarray(a.reshape(-1, order="F")) if a.size else np.zeros(1)
    fb = np.ascontiguousarray(b.reshape(-1, order="F")) if b.size else np.zeros(1)
    _check(_lib.t4a_gpu_swap_theta(_p(fa), c_size_t(a.shape[0]), c_size_t(a.shape[2]), _p(fb), c_size_t(b.shape[2]), _ptr(lk), _ptr(ld),
                                   c_size_t(len(legs_left)), _ptr(rk), _ptr(rd), c_size_t(len(legs_right)), _ptr(tl), c_size_t(len(tl)),
                                   _ptr(tr), c_size_t(len(tr)), _p(out), _p(mn), ctypes.byref(route)))
    return out[:total].reshape((int(mn[0]), int(mn[1])), order="F"), int(route.value)


def swap_theta_time(bond, reps=20):
    """Probe (t4a_gpu_swap_theta_time): device ms per launch of (the step kernel, GEMM plus one permutation launch) for binary legs
    exchanged at l = m = r = ``bond``."""
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_swap_theta_time(c_size_t(int(bond)), c_size_t(int(reps)), _p(ms)))
    return float(ms[0]), float(ms[1])
