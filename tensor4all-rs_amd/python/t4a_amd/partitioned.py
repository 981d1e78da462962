"""Partitioned MPOs: patch-wise projection, sum and contraction (tensor4all-partitionedtt) — the patches live on the device.

Mirrors ``Projector`` (projector.rs:39-268), ``SubDomainTT::project`` / ``contract`` (subdomain_tt.rs:171-443),
``PartitionedTT::{from_subdomains, norm, contract, add, to_tensor_train}`` (partitioned_tt.rs:104-480) and ``contract`` /
``proj_contract`` (contract.rs:41-110) for this project's slice: f64 on a chain, sites identified by position, every site an MPO site
``(left, s1, s2, right)`` (a train is the case ``s2 = 1``).  The reference's index objects are legs here: a projector key is
``(site, leg)``, leg 0 = s1, leg 1 = s2, and the shared index of ``A·B`` is ``A.(i, 1) == B.(i, 0)``.  Deviations: the task order of a
contraction is fixed (a-major, insertion order; the reference iterates a hash map), patches keep their insertion order, ``to_mpo``
sorts by keys then values with a shorter prefix first.  ``Projector`` and ``contract_plan`` touch no device.

Adaptive patching (patching.rs; "Adaptive Patching for Tensor Train Computations", arXiv:2602.22372): ``PatchingOptions``,
``PatchSplitStrategy``, ``truncate_adaptive``, ``add_with_patching`` and ``contract_adaptive``; ``patch_volume``, ``patch_budgets``, ``split_candidates`` and
``validate_patching_options`` are their host arithmetic and touch no device; ``contract_adaptive`` is the patch-wise product with
the same splitting.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, c_size_t, c_double, c_int32, c_void_p)
from .mpo import MPO, ContractionAlgorithm, ContractionOptions, FactorizeMethod, _route_code


def _triples(entries):
    """{(site, leg): value} or [((site, leg), value), ...] -> (3 * count uintp array (never empty), count); later pairs win in C"""
    items = list(entries.items()) if isinstance(entries, dict) else list(entries)
    flat = []
    for key, value in items:
        site, leg = key
        if int(site) < 0 or int(leg) < 0 or int(value) < 0:
            raise T4aError(INVALID_ARGUMENT, f"projector entry ({site}, {leg}) -> {value} is negative")
        flat += [int(site), int(leg), int(value)]
    return np.ascontiguousarray(np.array(flat if flat else [0, 0, 0], dtype=np.uintp)), len(items)


def _from_triples(buf, count):
    return {(int(buf[3 * i]), int(buf[3 * i + 1])): int(buf[3 * i + 2]) for i in range(count)}


def _projector_list(projectors):
    """[Projector] -> (entries, counts) as the C lists take them"""
    flat, counts = [], []
    for p in projectors:
        t, c = Projector._of(p)._c()
        flat.append(t[:3 * c])
        counts.append(c)
    entries = np.concatenate(flat) if flat else np.zeros(0, dtype=np.uintp)
    if entries.size == 0:
        entries = np.zeros(3, dtype=np.uintp)
    return np.ascontiguousarray(entries.astype(np.uintp)), np.ascontiguousarray(np.array(counts if counts else [0], dtype=np.uintp))


class Projector:
    """Projector (projector.rs:34-268) over legs: ``{(site, leg): value}``, leg 0 = s1, leg 1 = s2.  Pure host code over the C
    functions ``t4a_gpu_projector_*``; a key given twice keeps its last value (from_pairs)."""

    def __init__(self, entries=None):
        t, c = _triples({} if entries is None else entries)
        out = np.zeros(max(3 * c, 3), dtype=np.uintp)
        n = c_size_t(0)
        # the filter over its own keys normalises: duplicate keys collapse, legs are checked, the order becomes (site, leg)
        keys = np.ascontiguousarray(t.reshape(-1, 3)[:, :2]).reshape(-1)
        _check(_lib.t4a_gpu_projector_filter(_p(t), c_size_t(c), _p(keys), c_size_t(c), _p(out), ctypes.byref(n)))
        self._data = _from_triples(out, n.value)

    @classmethod
    def _of(cls, p):
        return p if isinstance(p, Projector) else cls(p)

    def _c(self):
        return _triples(self._data)

    def items(self):
        """[((site, leg), value)] ascending by (site, leg): the canonical entries (projector.rs:227-235)."""
        return sorted(self._data.items())

    def as_dict(self):
        return dict(self._data)

    def get(self, site, leg):
        return self._data.get((int(site), int(leg)))

    def is_projected_at(self, site, leg):
        return (int(site), int(leg)) in self._data

    def __len__(self):
        return len(self._data)

    def __eq__(self, other):
        return isinstance(other, Projector) and self._data == other._data

    def __hash__(self):
        return hash(tuple(self.items()))

    def __repr__(self):
        return f"Projector({dict(self.items())})"

    def validate(self, site_dims):
        """validate_invariants: a key outside the chain or a value >= the dim of its leg raises INVALID_ARGUMENT."""
        sd = np.ascontiguousarray(np.array([[int(a), int(b)] for a, b in site_dims], dtype=np.uintp).reshape(-1))
        t, c = self._c()
        _check(_lib.t4a_gpu_projector_validate(_p(sd) if sd.size else None, c_size_t(sd.size // 2), _p(t), c_size_t(c)))
        return self

    def _flag(self, fn, other):
        a, ca = self._c()
        b, cb = Projector._of(other)._c()
        v = c_int32(0)
        _check(fn(_p(a), c_size_t(ca), _p(b), c_size_t(cb), ctypes.byref(v)))
        return v.value

    def is_compatible_with(self, other):
        """is_compatible_with (:172-174): no key carries two different values."""
        return bool(self._flag(_lib.t4a_gpu_projector_is_compatible, other))

    def is_subset_of(self, other):
        """is_subset_of (:183-194): self projects every key of other to the same value."""
        return bool(self._flag(_lib.t4a_gpu_projector_is_subset_of, other))

    def compare(self, other):
        """The total order of ``PartitionedMPO.to_mpo``: -1, 0 or 1."""
        return self._flag(_lib.t4a_gpu_projector_compare, other)

    def intersection(self, other):
        """intersection (:130-145): the merged projector, or None on a conflict."""
        a, ca = self._c()
        b, cb = Projector._of(other)._c()
        ok = c_int32(0)
        n = c_size_t(0)
        out = np.zeros(3 * (ca + cb) + 3, dtype=np.uintp)
        _check(_lib.t4a_gpu_projector_intersection(_p(a), c_size_t(ca), _p(b), c_size_t(cb), ctypes.byref(ok), _p(out), ctypes.byref(n)))
        return Projector(_from_triples(out, n.value)) if ok.value else None

    __and__ = intersection

    def common_restriction(self, other):
        """common_restriction (:157-167): the keys both project to the same value."""
        a, ca = self._c()
        b, cb = Projector._of(other)._c()
        n = c_size_t(0)
        out = np.zeros(3 * ca + 3, dtype=np.uintp)
        _check(_lib.t4a_gpu_projector_common_restriction(_p(a), c_size_t(ca), _p(b), c_size_t(cb), _p(out), ctypes.byref(n)))
        return Projector(_from_triples(out, n.value))

    __or__ = common_restriction

    def filter_indices(self, keys):
        """filter_indices (:214-224): the entries whose (site, leg) is in ``keys``."""
        keys = [(int(s), int(l)) for s, l in keys]
        k = np.ascontiguousarray(np.array(keys if keys else [(0, 0)], dtype=np.uintp).reshape(-1))
        t, c = self._c()
        n = c_size_t(0)
        out = np.zeros(3 * c + 3, dtype=np.uintp)
        _check(_lib.t4a_gpu_projector_filter(_p(t), c_size_t(c), _p(k), c_size_t(len(keys)), _p(out), ctypes.byref(n)))
        return Projector(_from_triples(out, n.value))

    @staticmethod
    def are_disjoint(projectors):
        """are_disjoint (:199-208): no two of them are compatible."""
        e, c = _projector_list(projectors)
        v = c_int32(0)
        _check(_lib.t4a_gpu_projector_are_disjoint(_p(e), _p(c), c_size_t(len(projectors)), ctypes.byref(v)))
        return bool(v.value)


def contract_plan(projectors_a, projectors_b):
    """contraction_tasks (partitioned_tt.rs:401-445) from two projector lists (t4a_gpu_pmpo_contract_plan, host only):
    ``(tasks, results)`` with tasks ``[(i, j, slot)]`` a-major in insertion order and results the distinct result projectors
    (A's leg-0 entries plus B's leg-1 entries) in order of first appearance."""
    ea, ca = _projector_list(projectors_a)
    eb, cb = _projector_list(projectors_b)
    nt, nr, ne = c_size_t(0), c_size_t(0), c_size_t(0)
    args = (_p(ea), _p(ca), c_size_t(len(projectors_a)), _p(eb), _p(cb), c_size_t(len(projectors_b)))
    _check(_lib.t4a_gpu_pmpo_contract_plan(*args, c_size_t(0), c_size_t(0), ctypes.byref(nt), None, None, None, ctypes.byref(nr), None, None,
                                           ctypes.byref(ne)))
    cap_t, cap_e = max(nt.value, 1), max(ne.value, 1)
    ta, tb, tr, rc = (np.zeros(cap_t, dtype=np.uintp) for _ in range(4))
    re = np.zeros(3 * cap_e, dtype=np.uintp)
    _check(_lib.t4a_gpu_pmpo_contract_plan(*args, c_size_t(cap_t), c_size_t(cap_e), ctypes.byref(nt), _p(ta), _p(tb), _p(tr), ctypes.byref(nr),
                                           _p(rc), _p(re), ctypes.byref(ne)))
    tasks = [(int(ta[t]), int(tb[t]), int(tr[t])) for t in range(nt.value)]
    results, off = [], 0
    for r in range(nr.value):
        results.append(Projector(_from_triples(re[3 * off:], int(rc[r]))))
        off += int(rc[r])
    return tasks, results


def _check_patches(site_dims, patch_site_dims, projectors):
    """The host checks of PartitionedMPO(...) on plain dimension lists (t4a_gpu_pmpo_check): raises INVALID_ARGUMENT."""
    sd = np.ascontiguousarray(np.array([[int(a), int(b)] for a, b in site_dims] or [[0, 0]], dtype=np.uintp).reshape(-1))
    flat = [[int(a), int(b)] for p in patch_site_dims for a, b in p]
    pd = np.ascontiguousarray(np.array(flat or [[0, 0]], dtype=np.uintp).reshape(-1))
    lens = np.ascontiguousarray(np.array([len(p) for p in patch_site_dims] or [0], dtype=np.uintp))
    e, c = _projector_list(projectors)
    _check(_lib.t4a_gpu_pmpo_check(_p(sd), c_size_t(len(site_dims)), _p(pd), _p(lens), c_size_t(len(patch_site_dims)), _p(e), _p(c)))


class PartitionedMPO:
    """PartitionedTT over MPO patches (partitioned_tt.rs): ``PartitionedMPO(patches, projectors)`` takes device copies of the MPOs in
    the order given and checks, before the device is touched, that they share length and site dims, that every projector fits the
    chain and that the projectors are pairwise disjoint.  Patches are not masked on the way in (as in the reference); ``project``
    with a patch's own projector does that."""

    def __init__(self, patches, projectors, site_dims=None):
        patches = list(patches)
        projectors = [Projector._of(p) for p in projectors]
        if len(patches) != len(projectors):
            raise T4aError(INVALID_ARGUMENT, f"partitioned MPO: {len(patches)} patches but {len(projectors)} projectors")
        for m in patches:
            if not isinstance(m, MPO):
                raise T4aError(INVALID_ARGUMENT, "partitioned MPO: every patch must be an MPO")
        e, c = _projector_list(projectors)
        arr = (c_void_p * max(len(patches), 1))(*[m._h for m in patches])
        sd = None
        if site_dims is not None:
            sd = np.ascontiguousarray(np.array([[int(a), int(b)] for a, b in site_dims] or [[0, 0]], dtype=np.uintp).reshape(-1))
        self._h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_new(arr, c_size_t(len(patches)), _p(e), _p(c), None if sd is None else _p(sd),
                                     c_size_t(0 if site_dims is None else len(site_dims)), ctypes.byref(self._h)))

    @classmethod
    def _adopt(cls, handle):
        self = cls.__new__(cls)
        self._h = handle
        return self

    @classmethod
    def from_partitioned_tt(cls, ptt, site_dims=None):
        """The result of ``adaptiveinterpolate`` as a partitioned MPO (t4a_gpu_pmpo_from_ptt): cores copied on the device, site k read
        as ``site_dims[k] = (s1, s2)`` (default ``(d, 1)``), a projected fused value v as ``(v % s1, v // s1)`` on the two legs."""
        sd = None
        if site_dims is not None:
            if len(site_dims) != len(ptt.local_dims):
                raise T4aError(INVALID_ARGUMENT, "relabel_site_dims: one (s1, s2) pair per site is needed")
            sd = np.ascontiguousarray(np.array([[int(a), int(b)] for a, b in site_dims] or [[0, 0]], dtype=np.uintp).reshape(-1))
        h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_from_ptt(ptt._h, None if sd is None else _p(sd), ctypes.byref(h)))
        return cls._adopt(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.t4a_gpu_pmpo_release(h)
            self._h = None

    def __len__(self):
        v = c_size_t(0)
        _check(_lib.t4a_gpu_pmpo_len(self._h, ctypes.byref(v)))
        return v.value

    def n_sites(self):
        v = c_size_t(0)
        _check(_lib.t4a_gpu_pmpo_n_sites(self._h, ctypes.byref(v)))
        return v.value

    def site_dims(self):
        n = self.n_sites()
        d = np.zeros(max(2 * n, 1), dtype=np.uintp)
        _check(_lib.t4a_gpu_pmpo_site_dims(self._h, _p(d)))
        return [(int(a), int(b)) for a, b in d[:2 * n].reshape(-1, 2)]

    def projector(self, k):
        n = c_size_t(0)
        _check(_lib.t4a_gpu_pmpo_projector(self._h, c_size_t(k), ctypes.byref(n), None))
        buf = np.zeros(max(3 * n.value, 3), dtype=np.uintp)
        _check(_lib.t4a_gpu_pmpo_projector(self._h, c_size_t(k), ctypes.byref(n), _p(buf)))
        return Projector(_from_triples(buf, n.value))

    def projectors(self):
        return [self.projector(k) for k in range(len(self))]

    def patch(self, k):
        """Patch k as an MPO of its own (a device copy)."""
        h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_patch(self._h, c_size_t(k), ctypes.byref(h)))
        return MPO._adopt(h)

    def patches(self):
        return [self.patch(k) for k in range(len(self))]

    def link_dims(self):
        """[link_dims of patch k]"""
        return [m.link_dims() for m in self.patches()]

    def norm(self):
        """norm (partitioned_tt.rs:286-295): sqrt of the sum of the squared patch norms."""
        v = c_double(0)
        _check(_lib.t4a_gpu_pmpo_norm(self._h, ctypes.byref(v)))
        return v.value

    def evaluate(self, indices):
        """The sum over the patches at [i1, j1, i2, j2, ...] -> float, or at an (n_pts, 2 n) array -> values."""
        n = self.n_sites()
        idx = np.asarray(indices, dtype=np.int64)
        single = idx.ndim == 1
        idx = idx.reshape(1, -1) if single else idx
        if idx.ndim != 2 or idx.shape[1] != 2 * n:
            raise T4aError(INVALID_ARGUMENT, f"Expected {2 * n} indices (2*{n}), got {idx.shape[-1]}")
        if (idx < 0).any():
            raise T4aError(INVALID_ARGUMENT, "negative index")
        idx = np.ascontiguousarray(idx.astype(np.uintp))
        out = np.zeros(idx.shape[0])
        _check(_lib.t4a_gpu_pmpo_evaluate(self._h, _p(idx), c_size_t(idx.shape[0]), _p(out)))
        return float(out[0]) if single else out

    def full_tensor(self):
        """The dense operator of shape (s1_1, s2_1, s1_2, s2_2, ...), as ``MPO.full_tensor``."""
        shape = [d for pair in self.site_dims() for d in pair]
        total = int(np.prod(shape))
        grid = np.indices(shape[::-1]).reshape(len(shape), -1)[::-1].T
        return self.evaluate(grid.reshape(total, len(shape))).reshape(shape, order="F")

    def budget_squared(self, k):
        """The absolute squared-error budget adaptive patching gave patch k (``SubDomainTT::budget_squared``), or None where unset."""
        has, v = c_int32(0), c_double(0)
        _check(_lib.t4a_gpu_pmpo_budget_squared(self._h, c_size_t(k), ctypes.byref(has), ctypes.byref(v)))
        return v.value if has.value else None

    def project(self, projector):
        """SubDomainTT::project (subdomain_tt.rs:171-260) patch by patch: incompatible patches are dropped, the others are masked —
        zeros are stored outside the subdomain, in one launch for all sites of all patches — and carry the intersection."""
        t, c = Projector._of(projector)._c()
        h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_project(self._h, _p(t), c_size_t(c), ctypes.byref(h)))
        return PartitionedMPO._adopt(h)

    def add(self, other, tolerance=1e-12, max_bond_dim=None):
        """add (partitioned_tt.rs:356-398): the union of the projectors must be pairwise disjoint; patches on both sides are added by
        direct sum and truncated (s >= tolerance * s_max, at most max_bond_dim, at least one), the others cloned.  ``tolerance=0``
        without a cap returns the direct sums as they are."""
        h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_add(self._h, other._h, c_double(tolerance), c_size_t(0 if max_bond_dim is None else max_bond_dim),
                                     ctypes.byref(h)))
        return PartitionedMPO._adopt(h)

    def to_mpo(self):
        """to_tensor_train (partitioned_tt.rs:460-480): the direct sum of the patches in the order of ``Projector.compare``."""
        h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_to_mpo(self._h, ctypes.byref(h)))
        return MPO._adopt(h)

    def _to_mpo_route(self, route):
        """Test and probe hook (t4a_gpu_pmpo_to_mpo_route): 1 the chain of pairwise additions, 2 one launch, 0 what ``to_mpo`` takes."""
        h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_to_mpo_route(self._h, c_int32(route), ctypes.byref(h)))
        return MPO._adopt(h)

    def contract(self, other, algorithm=ContractionAlgorithm.Naive, compress=True, options=None, compress_route="serial"):
        """contract (partitioned_tt.rs:305-340): every compatible pair of patches contracted over ``self.(i, 1) == other.(i, 0)`` with
        both projected onto their own projectors, results of equal projector summed and truncated with the same options.
        ``compress_route`` (Naive with ``compress``): ``"serial"`` compresses the task products one after the other, ``"batched"`` and
        ``"auto"`` hand all of them to one ``mpo.compress_many`` call (t4a_gpu_pmpo_contract_routed); ZipUp refuses ``"batched"``.  The
        sum of results that share a projector is truncated serially on every route."""
        o = ContractionOptions() if options is None else options
        h = c_void_p()
        _check(_lib.t4a_gpu_pmpo_contract_routed(self._h, other._h, c_int32(algorithm), c_int32(1 if compress else 0),
                                                 c_int32(o.factorize_method), c_double(o.tolerance),
                                                 c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim), c_int32(_route_code(compress_route)),
                                                 ctypes.byref(h)))
        return PartitionedMPO._adopt(h)


def contract(a, b, algorithm=ContractionAlgorithm.Naive, compress=True, tolerance=1e-12, max_bond_dim=None,
             factorize_method=FactorizeMethod.SVD, compress_route="serial"):
    """contract (contract.rs:41-47, partitioned_tt.rs:305-340) of two PartitionedMPO.  ``compress=False`` (Naive only) keeps the
    exact products and direct sums; Fit and RSVD raise NOT_IMPLEMENTED as ``mpo.contract`` does.  ``compress_route``: see
    ``PartitionedMPO.contract``."""
    return a.contract(b, algorithm, compress, ContractionOptions(tolerance, max_bond_dim, factorize_method), compress_route)


def proj_contract(a, b, projector, shared=None, **options):
    """proj_contract (contract.rs:78-110): project both operands, then contract.  With positional legs ``projector`` speaks about the
    result: its leg-0 entries project ``a``'s s1 legs, its leg-1 entries ``b``'s s2 legs; ``shared = {site: value}`` projects the
    contracted index on both (``a``'s leg 1 and ``b``'s leg 0).  An operand left without a compatible patch gives an empty result."""
    p = Projector._of(projector)
    shared = {} if shared is None else shared
    pa = {k: v for k, v in p.items() if k[1] == 0}
    pb = {k: v for k, v in p.items() if k[1] == 1}
    pa.update({(int(s), 1): int(v) for s, v in shared.items()})
    pb.update({(int(s), 0): int(v) for s, v in shared.items()})
    return contract(a.project(pa), b.project(pb), **options)


def _time_compress(a, b, tolerance=1e-12, max_bond_dim=None, reps=5):
    """Probe (t4a_gpu_pmpo_time_compress): ms per repetition of the compress stage of every task product of a·b, (task by task on the
    serial stage, all tasks in one batched call)."""
    ms = np.zeros(2)
    _check(_lib.t4a_gpu_pmpo_time_compress(a._h, b._h, c_double(tolerance), c_size_t(0 if max_bond_dim is None else max_bond_dim),
                                           c_size_t(reps), _p(ms)))
    return float(ms[0]), float(ms[1])


def _pair_products(dims, sel, A, B):
    """Test hook (t4a_gpu_pmpo_pair_products): dims (n_jobs, 7) = (la, s1, k, ra, lb, t, rb), sel (n_jobs, 4) = (k0, k1, s mask, t
    mask; < 0 = none), A / B lists of site tensors [la, s1, k, ra] / [lb, k, t, rb] -> list of C [la*lb, s1, t, ra*rb]."""
    dims = np.ascontiguousarray(np.asarray(dims, dtype=np.uintp).reshape(-1, 7))
    sel = np.ascontiguousarray(np.asarray(sel, dtype=np.int64).reshape(-1, 4))
    fa = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, order="F") for x in A]))
    fb = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, order="F") for x in B]))
    shapes = [(int(d[0] * d[4]), int(d[1]), int(d[5]), int(d[3] * d[6])) for d in dims]
    out = np.full(sum(int(np.prod(s)) for s in shapes), np.nan)
    _check(_lib.t4a_gpu_pmpo_pair_products(_p(dims), _p(sel), c_size_t(len(dims)), _p(fa), _p(fb), _p(out)))
    res, off = [], 0
    for s in shapes:
        res.append(out[off:off + int(np.prod(s))].reshape(s, order="F"))
        off += int(np.prod(s))
    return res


def _mask_sites(sites, sel):
    """Test hook (t4a_gpu_pmpo_mask_sites): site tensors [l, s1, s2, r] and (s1 value, s2 value; < 0 = none) each -> masked copies."""
    sites = [np.asarray(x, dtype=np.float64) for x in sites]
    dims = np.ascontiguousarray(np.array([x.shape for x in sites], dtype=np.uintp))
    sel = np.ascontiguousarray(np.asarray(sel, dtype=np.int64).reshape(-1, 2))
    flat = np.ascontiguousarray(np.concatenate([x.reshape(-1, order="F") for x in sites]))
    _check(_lib.t4a_gpu_pmpo_mask_sites(_p(dims), _p(sel), c_size_t(len(sites)), _p(flat)))
    res, off = [], 0
    for x in sites:
        res.append(flat[off:off + x.size].reshape(x.shape, order="F"))
        off += x.size
    return res


def _launch_blocks(total):
    v = c_size_t(0)
    _check(_lib.t4a_gpu_pmpo_launch_blocks(c_size_t(total), ctypes.byref(v)))
    return v.value


def _time_contract(a, b, tolerance=1e-12, max_bond_dim=None, reps=10):
    """Probe (t4a_gpu_pmpo_time_contract): ms per repetition of (fused launch, mask + one site-contract launch per task, compress)."""
    ms = np.zeros(3)
    _check(_lib.t4a_gpu_pmpo_time_contract(a._h, b._h, c_double(tolerance), c_size_t(0 if max_bond_dim is None else max_bond_dim),
                                           c_size_t(reps), _p(ms)))
    return [float(v) for v in ms]


# ---------------------------------------------------------------------------------------- adaptive patching (patching.rs)
class PatchSplitStrategy:
    """PatchSplitStrategy (patching.rs:41-48); the default is ExactParameterGain."""
    Sequential, ExactParameterGain = 0, 1


class PatchingOptionsC(ctypes.Structure):
    """t4a_gpu_patching_options"""
    _fields_ = [("rtol", c_double), ("has_max_bond_dim", c_int32), ("max_bond_dim", c_size_t), ("patch_order", ctypes.POINTER(c_size_t)),
                ("n_patch_order", c_size_t), ("split_strategy", c_int32)]


class PatchingOptions:
    """PatchingOptions (patching.rs:68-107); the defaults are PatchingOptions::default().  ``patch_order`` is a list of legs
    ``(site, leg)``; ``max_bond_dim=None`` is no cap."""

    def __init__(self, rtol=1e-12, max_bond_dim=100, patch_order=(), split_strategy=PatchSplitStrategy.ExactParameterGain):
        self.rtol = rtol
        self.max_bond_dim = max_bond_dim
        self.patch_order = list(patch_order)
        self.split_strategy = split_strategy

    def to_c(self):
        """(struct, the array it points into): keep both alive through the call"""
        flat = []
        for site, leg in self.patch_order:
            if int(site) < 0 or int(leg) < 0:
                raise T4aError(INVALID_ARGUMENT, f"patch_order: leg ({site}, {leg}) is negative")
            flat += [int(site), int(leg)]
        if self.max_bond_dim is not None and int(self.max_bond_dim) < 0:
            raise T4aError(INVALID_ARGUMENT, "max_bond_dim must be at least 1")
        order = (c_size_t * max(len(flat), 1))(*flat)
        c = PatchingOptionsC(float(self.rtol), 0 if self.max_bond_dim is None else 1, 0 if self.max_bond_dim is None else int(self.max_bond_dim),
                             ctypes.cast(order, ctypes.POINTER(c_size_t)), len(self.patch_order), int(self.split_strategy))
        return c, order


def _site_dims(site_dims):
    return np.ascontiguousarray(np.array([[int(a), int(b)] for a, b in site_dims] or [[0, 0]], dtype=np.uintp).reshape(-1))


def validate_patching_options(options, site_dims):
    """validate_patching_options (patching.rs:617-627) on a chain, host only: raises INVALID_ARGUMENT with the reference's messages."""
    c, keep = options.to_c()
    _check(_lib.t4a_gpu_pmpo_validate_patching_options(ctypes.byref(c), _p(_site_dims(site_dims)), c_size_t(len(site_dims))))
    del keep


def patch_volume(projector, site_dims):
    """subdomain_volume (patching.rs:724-738), host only: the product of the dims of the unprojected legs."""
    t, c = Projector._of(projector)._c()
    v = c_size_t(0)
    _check(_lib.t4a_gpu_pmpo_patch_volume(_p(t), c_size_t(c), _p(_site_dims(site_dims)), c_size_t(len(site_dims)), ctypes.byref(v)))
    return v.value


def patch_budgets(volumes, norms_squared, rtol):
    """The budget arithmetic of ``truncate_adaptive`` (patching.rs:577-606), host only: ``(budgets, drop)`` with ``budgets[k] = rtol^2
    sum(norms_squared) volumes[k] / sum(volumes)`` and ``drop[k] = norms_squared[k] <= budgets[k]``; ``None`` for no patch or a zero
    total volume (the empty result)."""
    vol = [int(v) for v in volumes]
    if min(vol or [0]) < 0:
        raise T4aError(INVALID_ARGUMENT, "patch_budgets: a volume is negative")
    v = np.ascontiguousarray(np.array(vol or [0], dtype=np.uintp))
    n2 = np.ascontiguousarray(np.array(list(norms_squared) or [0.0], dtype=np.float64))
    if len(vol) != len(list(norms_squared)):
        raise T4aError(INVALID_ARGUMENT, f"patch_budgets: {len(vol)} volumes but {len(list(norms_squared))} norms")
    budgets, drop, empty = np.zeros(max(len(vol), 1)), np.zeros(max(len(vol), 1), dtype=np.int32), c_int32(0)
    _check(_lib.t4a_gpu_pmpo_patch_budgets(_p(v), _p(n2), c_size_t(len(vol)), c_double(rtol), _p(budgets), _p(drop), ctypes.byref(empty)))
    if empty.value:
        return None
    return budgets[:len(vol)], [bool(d) for d in drop[:len(vol)]]


def split_candidates(projector, site_dims, options):
    """split_candidates (patching.rs:801-823), host only: the unprojected legs of ``options.patch_order``, or all legs in chain order
    when it is empty; duplicates removed."""
    t, c = Projector._of(projector)._c()
    o, keep = options.to_c()
    legs, n = np.zeros(max(4 * len(site_dims), 2), dtype=np.uintp), c_size_t(0)
    _check(_lib.t4a_gpu_pmpo_split_candidates(_p(t), c_size_t(c), _p(_site_dims(site_dims)), c_size_t(len(site_dims)), ctypes.byref(o), _p(legs),
                                              ctypes.byref(n)))
    del keep
    return [(int(legs[2 * k]), int(legs[2 * k + 1])) for k in range(n.value)]


_COUNTS6 = ("rounds", "truncate_calls", "ranks_only_calls", "launches", "syncs", "splits")


def _truncate_adaptive(p, rtol, max_bond_dim, route):
    h = c_void_p()
    counts = np.zeros(6, dtype=np.uintp)
    if max_bond_dim is not None and int(max_bond_dim) < 0:
        raise T4aError(INVALID_ARGUMENT, "max_bond_dim must be at least 1")
    _check(_lib.t4a_gpu_pmpo_truncate_adaptive(p._h, c_double(rtol), c_int32(0 if max_bond_dim is None else 1),
                                               c_size_t(0 if max_bond_dim is None else int(max_bond_dim)), c_int32(_route_code(route)),
                                               ctypes.byref(h), _p(counts)))
    return PartitionedMPO._adopt(h), dict(zip(_COUNTS6, (int(v) for v in counts)))


def truncate_adaptive(p, rtol, max_bond_dim=None, route="auto"):
    """truncate_adaptive (patching.rs:566-615): every patch gets the absolute squared-error budget ``rtol^2 |F|^2 volume / total
    volume``; patches whose squared norm is at or below their budget are dropped, the others are truncated with Absolute /
    SquaredValue / DiscardedTailSum at the budget and ``max_bond_dim``, all in ONE ``mpo.truncate_many`` call whose QR sweep supplies the
    norms (two host synchronisations).  The survivors keep their order, are the truncations of the masked patches, and carry
    ``budget_squared``.  ``route``: that of ``mpo.truncate_many``."""
    return _truncate_adaptive(p, rtol, max_bond_dim, route)[0]


def _time_truncate_adaptive(p, rtol, max_bond_dim=None):
    """Probe (t4a_gpu_pmpo_truncate_adaptive_timed): wall ms of (QR sweep, first sync, leftward sweep, rightward sweep, last sync) of the
    batched part of one ``truncate_adaptive`` call, the stream drained after every sweep."""
    ms = np.zeros(5)
    _check(_lib.t4a_gpu_pmpo_truncate_adaptive_timed(p._h, c_double(rtol), c_int32(0 if max_bond_dim is None else 1),
                                                     c_size_t(0 if max_bond_dim is None else int(max_bond_dim)), _p(ms)))
    return [float(v) for v in ms]


def _add_with_patching(patches, projectors, options, route, site_dims=None):
    o = PatchingOptions() if options is None else options
    src = patches if isinstance(patches, PartitionedMPO) else None
    if src is None:
        patches = list(patches)
        if patches:
            validate_patching_options(o, site_dims if site_dims is not None else patches[0].site_dims())
        src = PartitionedMPO(patches, projectors, site_dims)
    c, keep = o.to_c()
    h = c_void_p()
    counts = np.zeros(6, dtype=np.uintp)
    cap = 2 * max(src.n_sites(), 1) * max(len(src), 1) * 64
    chosen, n_chosen = np.zeros(2 * cap, dtype=np.uintp), c_size_t(0)
    _check(_lib.t4a_gpu_pmpo_add_with_patching(src._h, ctypes.byref(c), c_int32(_route_code(route)), ctypes.byref(h), _p(counts), _p(chosen),
                                               c_size_t(cap), ctypes.byref(n_chosen)))
    del keep
    legs = [(int(chosen[2 * k]), int(chosen[2 * k + 1])) for k in range(min(n_chosen.value, cap))]
    return PartitionedMPO._adopt(h), dict(zip(_COUNTS6, (int(v) for v in counts))), legs


def add_with_patching(patches, projectors=None, options=None, route="auto", site_dims=None):
    """add_with_patching (patching.rs:154-198) over MPO patches with their projectors (or a ``PartitionedMPO``): each round assigns the
    volume budgets, budget-truncates without a cap, and replaces every patch that stays above ``options.max_bond_dim`` by its children
    along a leg — the first candidate (``Sequential``) or the one whose budget-truncated children hold the fewest parameters
    (``ExactParameterGain``: all children of all candidates of all such patches in one ranks-only ``mpo.truncate_many`` call; ties keep
    the first).  Ends with ``truncate_adaptive``."""
    return _add_with_patching(patches, projectors, options, route, site_dims)[0]


def _contract_adaptive(a, b, algorithm, options, patching_options, route):
    o = ContractionOptions() if options is None else options
    po = PatchingOptions() if patching_options is None else patching_options
    c, keep = po.to_c()
    h = c_void_p()
    counts = np.zeros(6, dtype=np.uintp)
    _check(_lib.t4a_gpu_pmpo_contract_adaptive(a._h, b._h, c_int32(algorithm), c_int32(o.factorize_method), c_double(o.tolerance),
                                               c_size_t(0 if o.max_bond_dim is None else o.max_bond_dim), ctypes.byref(c),
                                               c_int32(_route_code(route)), ctypes.byref(h), _p(counts)))
    del keep
    return PartitionedMPO._adopt(h), dict(zip(_COUNTS6, (int(v) for v in counts)))


def contract_adaptive(a, b, algorithm=ContractionAlgorithm.Naive, options=None, patching_options=None, route="auto"):
    """contract_adaptive (patching.rs:282-412): the pairwise products of the patches of ``a`` and ``b`` (``options``: the
    ``ContractionOptions`` of ``contract``) grouped by result projector; per group the contributions are summed by direct sum and
    truncated after each addition; when the sum or a contribution reaches ``patching_options.max_bond_dim`` the group is split along a leg
    of the result — ``(i, 0)`` is ``a``'s s1 leg of site i, ``(i, 1)`` ``b``'s s2 leg —, the operand that has the leg is projected per
    value and truncated with Relative / Value / PerValue at 64 eps, and the group recurses.  Ends with ``truncate_adaptive``."""
    return _contract_adaptive(a, b, algorithm, options, patching_options, route)[0]
