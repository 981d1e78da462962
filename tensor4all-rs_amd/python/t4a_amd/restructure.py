"""fuse_to, split_to and restructure_to on a chain: the operations that change the number of sites — fuse_to, contract_node_group,
split_to, split_tensor_for_targets (tensor4all-treetn, treetn/transform.rs), build_plan, execute_plan,
build_path_swap_then_fuse_assignment, apply_final_truncation (treetn/restructure/mod.rs), SplitOptions and RestructureOptions
(options.rs), for f64 and by position.  With ``swap_site_indices`` (swap.py) they are the structural family.

A *target* is an ordered list of groups of leg keys, ``target[j] = [key, ...]``: group ``j`` is site ``j`` of the result, the target
topology is the path in list order, and the order of the keys inside a group is the leg order of the result site, first leg fastest
(this project's rule for these operations; swap steps keep their ascending-key rule).  Refused in the plan, before the device is
touched: an empty group, a key in two groups, a key set that differs from the train's.

``fuse_to`` is exact: all groups are contracted in lock step, left to right inside a group, one launch of ``fuse_round_kernel``
(csrc/kernels_restructure.hip) per round for all groups — ``k_max - 1`` launches for a largest group of ``k_max`` sites —, a group's
last round writing its legs in the target's order.  ``split_to`` reorders the legs of every site fragment-major in one launch and
peels fragment after fragment from the left with the thin QR (rank rule: ``qr_retained_rank`` at rtol 0); ``final_sweep`` adds
``TensorTrain::truncate`` by the serial stage of ``truncate_many``.  ``restructure_to`` plans first (``restructure_plan``: host
only) and runs the phases of the kind: FuseOnly, SwapThenFuse, SplitOnly, SwapOnly, SplitThenFuse.
"""
import ctypes

import numpy as np

from . import _lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, SvdTruncationPolicy, c_size_t, c_int32, c_void_p
from .swap import LegTrain, SwapOptions, _as_leg_train, _ranks, _i64, _usz, _ptr, _nonneg

KINDS = ("FuseOnly", "SwapThenFuse", "SplitOnly", "SwapOnly", "SplitThenFuse")
FUSE_MAX_LEGS = 16
ROUTE_SCALAR, ROUTE_MFMA = 1, 2
_OPS = {"restructure_to": 0, "fuse_to": 1, "split_to": 2}


class SplitOptions:
    """SplitOptions (options.rs): ``form`` — only ``"unitary"`` is accepted, ``"lu"`` / ``"ci"`` are NOT_IMPLEMENTED —, and for the
    optional ``final_sweep`` (TensorTrain::truncate after the exact split) an ``SvdTruncationPolicy`` (``None``: the default policy) and
    ``max_bond_dim``."""

    def __init__(self, form="unitary", policy=None, max_bond_dim=None, final_sweep=False):
        self.form, self.policy, self.max_bond_dim, self.final_sweep = form, policy, max_bond_dim, final_sweep

    def _c(self):
        forms = {"unitary": 0, "lu": 1, "ci": 2}
        if self.form not in forms:
            raise T4aError(INVALID_ARGUMENT, 'split_to: form is "unitary" ("lu" and "ci" are not implemented)')
        if self.policy is not None and not isinstance(self.policy, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "split_to: policy must be an SvdTruncationPolicy")
        pc = None if self.policy is None else self.policy.to_c()
        return (pc, (c_int32(forms[self.form]), None if pc is None else ctypes.byref(pc), c_int32(0 if self.max_bond_dim is None else 1),
                     c_size_t(0 if self.max_bond_dim is None else int(self.max_bond_dim)), c_int32(1 if self.final_sweep else 0)))


class RestructureOptions:
    """RestructureOptions (options.rs): the options of the split phase, of the swap phase, and ``final_truncation``: ``None`` or an
    ``(SvdTruncationPolicy, max_bond_dim)`` pair (``max_bond_dim`` may be ``None``) applied to the restructured train."""

    def __init__(self, split=None, swap=None, final_truncation=None):
        self.split = SplitOptions() if split is None else split
        self.swap = SwapOptions() if swap is None else swap
        self.final_truncation = final_truncation


def _legs_of(x, what):
    """[[(key, dim), ...], ...] of a LegTrain, an MPO, a train or such a list itself (plans need no device)"""
    if isinstance(x, (list, tuple)):
        return [[(k, _nonneg(d, "a leg dimension")) for k, d in site] for site in x]
    return _as_leg_train(x, what).legs


def _check_target(op, legs, target):
    """the refusals every entry point shares, with the keys as the caller wrote them"""
    try:
        target = [list(g) for g in target]
    except TypeError:
        raise T4aError(INVALID_ARGUMENT, f"{op}: the target is a list of groups of leg keys") from None
    site_of, group_of = {}, {}
    for i, site in enumerate(legs):
        for k, _ in site:
            if k in site_of:
                raise T4aError(INVALID_ARGUMENT, f"{op}: site index {k!r} appears in both current nodes {site_of[k]} and {i}")
            site_of[k] = i
    for j, g in enumerate(target):
        if not g:
            raise T4aError(INVALID_ARGUMENT, f"{op}: target node {j} has no site indices")
        for k in g:
            if k in group_of:
                raise T4aError(INVALID_ARGUMENT, f"{op}: site index {k!r} appears in both target nodes {group_of[k]} and {j}")
            group_of[k] = j
    for k, j in group_of.items():
        if k not in site_of:
            if op == "fuse_to":
                raise T4aError(INVALID_ARGUMENT, f"fuse_to: incompatible target structure: target node {j} has site indices not found in the current train")
            if op == "split_to":
                raise T4aError(INVALID_ARGUMENT, f"split_to: target site index {k!r} is missing from the current network")
            raise T4aError(INVALID_ARGUMENT, f"{op}: current and target must contain the same site indices")
    for k, i in site_of.items():
        if k not in group_of:
            if op == "fuse_to":
                raise T4aError(INVALID_ARGUMENT, f"fuse_to: missing target for current node {i}: it has site indices but no corresponding target node")
            if op == "split_to":
                raise T4aError(INVALID_ARGUMENT, f"split_to: incompatible target structure: site index {k!r} in current node {i} has no corresponding target node")
            raise T4aError(INVALID_ARGUMENT, f"{op}: current and target must contain the same site indices")
    return target


def _flat(legs, target, op):
    target = _check_target(op, legs, target)
    rank, ordered = _ranks([k for site in legs for k, _ in site], op)
    counts = _usz(len(s) for s in legs)
    keys = _i64(rank[k] for site in legs for k, _ in site)
    dims = _usz(d for site in legs for _, d in site)
    gc = _usz(len(g) for g in target)
    gk = _i64(rank[k] for g in target for k in g)
    return target, ordered, counts, keys, dims, gc, gk


def _read_legs(ordered, n_sites, oc, okeys, odims):
    legs, at = [], 0
    for i in range(n_sites):
        c = int(oc[i])
        legs.append([(ordered[int(okeys[at + j])], int(odims[at + j])) for j in range(c)])
        at += c
    return legs


def _plan(op, legs, target, link_dims):
    legs = _legs_of(legs, op)
    target, ordered, counts, keys, dims, gc, gk = _flat(legs, target, op)
    ld = None if link_dims is None else _usz(_nonneg(v, "a bond") for v in link_dims)
    if ld is not None and len(ld) != max(len(legs) - 1, 0):
        raise T4aError(INVALID_ARGUMENT, f"{op}: {len(legs)} sites have {max(len(legs) - 1, 0)} bonds, got {len(ld)}")
    n_legs = len(ordered)
    kind = c_int32(0)
    oc = np.zeros(max(len(target), 1), dtype=np.uintp)
    okeys = np.zeros(max(n_legs, 1), dtype=np.int64)
    odims = np.zeros(max(n_legs, 1), dtype=np.uintp)
    counts4 = np.zeros(4, dtype=np.uintp)
    sk = np.zeros(max(n_legs, 1), dtype=np.int64)
    ss = np.zeros(max(n_legs, 1), dtype=np.uintp)
    _check(_lib.t4a_gpu_restructure_plan(c_int32(_OPS[op]), c_size_t(len(legs)), _ptr(counts), _ptr(keys), _ptr(dims),
                                         None if ld is None or not ld.size else _p(ld), c_size_t(len(target)), _ptr(gc), _ptr(gk),
                                         ctypes.byref(kind), _p(oc), _p(okeys), _p(odims), _p(counts4), _p(sk), _p(ss)))
    return {"kind": KINDS[kind.value], "legs": _read_legs(ordered, len(target), oc, okeys, odims), "fuse_rounds": int(counts4[0]),
            "fuse_launches": int(counts4[1]), "n_qr": int(counts4[2]),
            "swap_target": {ordered[int(sk[k])]: int(ss[k]) for k in range(int(counts4[3]))}}


def restructure_plan(legs, target, link_dims=None):
    """What ``restructure_to`` will do (t4a_gpu_restructure_plan; host only, no device needed).  ``legs`` is ``[[(key, dim), ...], ...]``
    per site, or a LegTrain / MPO / SimpleTensorTrain.  Returns ``kind`` (one of ``KINDS``, with the precedence of build_plan), the
    ``legs`` of the result, the ``fuse_rounds`` (``k_max - 1``) and ``fuse_launches`` (plus one when a group of one site is
    reordered) of the fuse phase, ``n_qr`` of the split phase, and the ``swap_target`` of the swap kinds."""
    return _plan("restructure_to", legs, target, link_dims)


def fuse_plan(legs, target, link_dims=None):
    """The plan of ``fuse_to`` alone, with its conditions and messages: ``legs``, ``rounds``, ``launches``."""
    p = _plan("fuse_to", legs, target, link_dims)
    return {"legs": p["legs"], "rounds": p["fuse_rounds"], "launches": p["fuse_launches"]}


def split_plan(legs, target):
    """The plan of ``split_to`` alone, with its conditions and messages: ``legs``, ``n_qr``, ``launches`` (the reorder launch)."""
    p = _plan("split_to", legs, target, None)
    return {"legs": p["legs"], "n_qr": p["n_qr"], "launches": p["fuse_launches"]}


def _result(res, as_legs):
    if as_legs:
        return res
    if res.legs and all(len(s) == 2 for s in res.legs):
        return res.as_mpo()
    if res.legs and all(len(s) == 1 for s in res.legs):
        return res.as_train()
    return res


def _out_buffers(n_groups, n_legs):
    return (np.zeros(max(n_groups, 1), dtype=np.uintp), np.zeros(max(n_legs, 1), dtype=np.int64), np.zeros(max(n_legs, 1), dtype=np.uintp))


def _center_c(lt):
    return ctypes.c_int64(-1 if lt.center is None else int(lt.center))


def fuse_to(x, target, as_legs=False, counted=False):
    """fuse_to (t4a_gpu_tt_fuse_to): merge neighbouring sites of ``x`` (an MPO, a SimpleTensorTrain or a LegTrain) into the groups of
    ``target``; exact, no truncation.  Every site's legs lie in one group, the sites of a group are contiguous, groups ascend along the
    chain; sites without legs are absorbed as in the reference.  The result is an MPO when every site ends with exactly two legs, a
    SimpleTensorTrain when with exactly one, else a LegTrain (always with ``as_legs``) whose ``center`` is the group that holds the
    centre of ``x``.  ``counted``: also the number of kernel launches, ``(result, launches)``."""
    lt = _as_leg_train(x, "fuse_to")
    target, ordered, counts, keys, dims, gc, gk = _flat(lt.legs, target, "fuse_to")
    oc, okeys, odims = _out_buffers(len(target), len(ordered))
    h, center, launches = c_void_p(), ctypes.c_int64(-1), c_size_t(0)
    _check(_lib.t4a_gpu_tt_fuse_to_counted(lt._tt._h, _ptr(counts), _ptr(keys), _ptr(dims), _center_c(lt), c_size_t(len(target)), _ptr(gc), _ptr(gk),
                                           ctypes.byref(h), _p(oc), _p(okeys), _p(odims), ctypes.byref(center), ctypes.byref(launches)))
    out = SimpleTensorTrain._adopt(h)
    res = LegTrain(out, _read_legs(ordered, len(target), oc, okeys, odims), center=None if center.value < 0 else int(center.value))
    res = _result(res, as_legs)
    return (res, int(launches.value)) if counted else res


def split_to(x, target, options=None, as_legs=False):
    """split_to (t4a_gpu_tt_split_to): split sites of ``x`` into the groups of ``target``.  Every group's legs lie on one site, the
    groups of a site are consecutive in the list and sites ascend.  Exact unless ``options.final_sweep`` truncates afterwards; the
    fragments are peeled from the left (this project's rule) and every fragment but a site's last is left-orthogonal.  The result has no
    centre; its type follows ``fuse_to``'s rule."""
    o = SplitOptions() if options is None else options
    if not isinstance(o, SplitOptions):
        raise T4aError(INVALID_ARGUMENT, "split_to: options must be SplitOptions")
    lt = _as_leg_train(x, "split_to")
    target, ordered, counts, keys, dims, gc, gk = _flat(lt.legs, target, "split_to")
    oc, okeys, odims = _out_buffers(len(target), len(ordered))
    keep, oargs = o._c()
    h, n_qr = c_void_p(), c_size_t(0)
    _check(_lib.t4a_gpu_tt_split_to(lt._tt._h, _ptr(counts), _ptr(keys), _ptr(dims), c_size_t(len(target)), _ptr(gc), _ptr(gk), *oargs,
                                    ctypes.byref(h), _p(oc), _p(okeys), _p(odims), ctypes.byref(n_qr)))
    out = SimpleTensorTrain._adopt(h)
    return _result(LegTrain(out, _read_legs(ordered, len(target), oc, okeys, odims)), as_legs)


def restructure_to(x, target, options=None, as_legs=False, info=False):
    """restructure_to (t4a_gpu_tt_restructure_to): bring ``x`` to the grouping of ``target`` by the phases ``restructure_plan`` names.
    ``info``: also ``{"kind", "launches", "n_qr", "n_swap_steps"}``, ``(result, info)``."""
    o = RestructureOptions() if options is None else options
    if not isinstance(o, RestructureOptions) or not isinstance(o.split, SplitOptions) or not isinstance(o.swap, SwapOptions):
        raise T4aError(INVALID_ARGUMENT, "restructure_to: options must be RestructureOptions of SplitOptions and SwapOptions")
    lt = _as_leg_train(x, "restructure_to")
    target, ordered, counts, keys, dims, gc, gk = _flat(lt.legs, target, "restructure_to")
    oc, okeys, odims = _out_buffers(len(target), len(ordered))
    keep, split_args = o.split._c()
    fpc, fcap = None, 0
    if o.final_truncation is not None:
        try:
            policy, cap = o.final_truncation
        except (TypeError, ValueError):
            raise T4aError(INVALID_ARGUMENT, "restructure_to: final_truncation is None or (SvdTruncationPolicy, max_bond_dim)") from None
        if not isinstance(policy, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "restructure_to: final_truncation is None or (SvdTruncationPolicy, max_bond_dim)")
        fpc, fcap = policy.to_c(), 0 if cap is None else _nonneg(cap, "max_bond_dim")
    h, kind, center = c_void_p(), c_int32(0), ctypes.c_int64(-1)
    counts3 = np.zeros(3, dtype=np.uintp)
    _check(_lib.t4a_gpu_tt_restructure_to(lt._tt._h, _ptr(counts), _ptr(keys), _ptr(dims), _center_c(lt), c_size_t(len(target)), _ptr(gc), _ptr(gk),
                                          *split_args, *o.swap._c(), None if fpc is None else ctypes.byref(fpc), c_size_t(fcap),
                                          ctypes.byref(h), _p(oc), _p(okeys), _p(odims), ctypes.byref(kind), ctypes.byref(center), _p(counts3)))
    out = SimpleTensorTrain._adopt(h)
    res = LegTrain(out, _read_legs(ordered, len(target), oc, okeys, odims), center=None if center.value < 0 else int(center.value))
    res = _result(res, as_legs)
    if info:
        return res, {"kind": KINDS[kind.value], "launches": int(counts3[0]), "n_qr": int(counts3[1]), "n_swap_steps": int(counts3[2])}
    return res


def _quantics_bits(n_sites, n_vars, what):
    n_sites, n_vars = int(n_sites), int(n_vars)
    if n_vars < 1:
        raise T4aError(INVALID_ARGUMENT, f"{what}: n_vars must be positive")
    return n_sites, n_vars


def fuse_quantics(tt, n_vars):
    """A quantics train from the interleaved layout x1 y1 x2 y2 ... (one variable's bit per site) to the fused one (x1 y1)(x2 y2) ...
    (one site per bit, all variables): site index ``sum_v bit_v * 2**v``, the first variable least significant — the convention of
    ``Unfolding::Fused`` in csrc/quantics.hpp.  Exact; returns a SimpleTensorTrain."""
    if not isinstance(tt, SimpleTensorTrain):
        raise T4aError(INVALID_ARGUMENT, "fuse_quantics: a SimpleTensorTrain is needed")
    n, n_vars = _quantics_bits(len(tt), n_vars, "fuse_quantics")
    if n % n_vars:
        raise T4aError(INVALID_ARGUMENT, f"fuse_quantics: {n} sites do not hold {n_vars} variables of equally many bits")
    lt = LegTrain.from_train(tt)
    res = fuse_to(lt, [[(b * n_vars + v, 0) for v in range(n_vars)] for b in range(n // n_vars)], as_legs=True)
    return res._tt


def unfuse_quantics(tt, n_vars, options=None):
    """The inverse of ``fuse_quantics``: every site of dimension ``2**n_vars`` split into ``n_vars`` binary sites, first variable
    first (``split_to`` with ``options``: a SplitOptions).  Returns a SimpleTensorTrain."""
    if not isinstance(tt, SimpleTensorTrain):
        raise T4aError(INVALID_ARGUMENT, "unfuse_quantics: a SimpleTensorTrain is needed")
    n, n_vars = _quantics_bits(len(tt), n_vars, "unfuse_quantics")
    for i, d in enumerate(tt.site_dims()):
        if int(d) != 2 ** n_vars:
            raise T4aError(INVALID_ARGUMENT, f"unfuse_quantics: site {i} has dimension {int(d)}, not 2**{n_vars}")
    lt = LegTrain(tt, [[((b * n_vars + v, 0), 2) for v in range(n_vars)] for b in range(n)])
    res = split_to(lt, [[(i, 0)] for i in range(n * n_vars)], options, as_legs=True)
    return res._tt


def fuse_round(jobs):
    """Test hook (t4a_gpu_fuse_round), the counterpart of ``swap_theta``: ONE launch of the fuse kernel over ``jobs``, each
    ``(A, B)`` or ``(A, B, leg_dims, order)`` with host cores ``A[l, X, m]``, ``B[m, Y, r]``, the dims of the result's legs in chain
    order and, per leg of the result in its new order, its position in chain order (absent: chain order).  Returns
    ``[(out[l, X * Y, r], route), ...]`` with the ROUTE_* bits of each job."""
    jobs = [tuple(j) for j in jobs]
    if not jobs:
        raise T4aError(INVALID_ARGUMENT, "fuse_round: no job")
    fa, fb, shapes, lc, ld, lo, sizes = [], [], [], [], [], [], []
    for j in jobs:
        a, b = np.asarray(j[0], dtype=np.float64), np.asarray(j[1], dtype=np.float64)
        if a.ndim != 3 or b.ndim != 3 or a.shape[2] != b.shape[0] or a.size == 0 or b.size == 0:
            raise T4aError(INVALID_ARGUMENT, "fuse_round: non-empty cores (l, X, m) and (m, Y, r) are needed")
        fa.append(a.reshape(-1, order="F"))
        fb.append(b.reshape(-1, order="F"))
        shapes += [a.shape[0], a.shape[1], a.shape[2], b.shape[1], b.shape[2]]
        sizes.append((a.shape[0], a.shape[1] * b.shape[1], b.shape[2]))
        dims, order = (list(j[2]), list(j[3])) if len(j) == 4 else ([], [])
        if len(dims) != len(order):
            raise T4aError(INVALID_ARGUMENT, "fuse_round: one position per leg is needed")
        lc.append(len(dims))
        ld += [_nonneg(d, "a leg dimension") for d in dims]
        lo += [_nonneg(p, "a position") for p in order]
    a, b = np.ascontiguousarray(np.concatenate(fa)), np.ascontiguousarray(np.concatenate(fb))
    out = np.zeros(sum(s[0] * s[1] * s[2] for s in sizes))
    routes = np.zeros(len(jobs), dtype=np.int32)
    sh, lc, ld, lo = _usz(shapes), _usz(lc), _usz(ld), _usz(lo)
    _check(_lib.t4a_gpu_fuse_round(c_size_t(len(jobs)), _p(a), _p(b), _p(sh), _p(lc), _ptr(ld), _ptr(lo), _p(out), _p(routes)))
    res, at = [], 0
    for k, s in enumerate(sizes):
        n = s[0] * s[1] * s[2]
        res.append((out[at:at + n].reshape(s, order="F").copy(), int(routes[k])))
        at += n
    return res


def fuse_time(n_groups, bond, reps=20):
    """Probe (t4a_gpu_fuse_time): device ms per repetition of fusing ``n_groups`` pairs of binary-leg sites at bond ``bond`` by (the one
    lock-step launch, one swap_theta launch per pair issued group by group)."""
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_fuse_time(c_size_t(int(n_groups)), c_size_t(int(bond)), c_size_t(int(reps)), _p(ms)))
    return float(ms[0]), float(ms[1])
