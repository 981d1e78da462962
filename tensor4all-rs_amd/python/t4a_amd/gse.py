"""Global subspace expansion (GSE) and GSE-TDVP on the device (tensor4all-treetn/src/gse.rs).

Mirrors ``global_subspace_expand``, ``global_subspace_expand_with_references``, ``gse_tdvp``, ``GseOptions``, ``GseResult``,
``GseTdvpOptions`` and ``GseTdvpResult`` of the Rust crate, restated for what ``tdvp`` covers: a chain, f64, one site index per node,
V_in = V_out.  The expansion widens every bond of the state by the directions of a few references (H psi, H^2 psi, ...) that the state
does not span yet; the state itself does not change.

Deviations from the reference: the missing directions of an edge come from the thin SVD of the stacked projected references where the
reference diagonalises the Hermitianised P rho P / t (the same eigenvalues sigma^2 / t and eigenspaces, the kept rows in descending
order: a permutation of the gauge; ``hermitian_tol`` is validated and has nothing else to check); ``krylov_references`` applies the
operator with this project's simplett zip-up (``contract_zipup(op, MPO.from_tensor_train(cur))``, SVD, ``max_bond_dim =
reference_max_bond_dim``), not with treetn's ``apply_linear_operator``; more than 8 references are NOT_IMPLEMENTED.  Trees, index
mappings, complex scalars and the reference's AD preservation are not mirrored.
"""
import ctypes

import numpy as np

from . import (_lib, _check, _p, T4aError, INVALID_ARGUMENT, SimpleTensorTrain, SvdPolicyC, SvdTruncationPolicy, c_size_t, c_double, c_int32,
               c_void_p)
from .linsolve import _operands, _flat
from .tdvp import TdvpOptions

ROUTE_FUSED, ROUTE_GEMM = 0, 1  # the route of the hooks _project and _absorb
MAX_REFERENCES = 8


class GseOptionsC(ctypes.Structure):
    """t4a_gpu_gse_options"""
    _fields_ = [("krylov_dim", c_size_t), ("has_reference_max_bond_dim", c_int32), ("reference_max_bond_dim", c_size_t),
                ("has_reference_svd_policy", c_int32), ("reference_svd_policy", SvdPolicyC), ("density_weight_cutoff", c_double),
                ("hermitian_tol", c_double), ("normalize_references", c_int32), ("expand_before_first_sweep", c_int32)]


class GseOptions:
    """GseOptions (gse.rs:31-72); the defaults are GseOptions::default().  ``reference_max_bond_dim`` None means
    max(link_dims(init)) + 1, ``reference_svd_policy`` (an SvdTruncationPolicy) None the threshold 1e-12."""

    def __init__(self, krylov_dim=0, reference_max_bond_dim=None, reference_svd_policy=None, density_weight_cutoff=1e-12, hermitian_tol=1e-12,
                 normalize_references=True, expand_before_first_sweep=True):
        self.krylov_dim = krylov_dim
        self.reference_max_bond_dim = reference_max_bond_dim
        self.reference_svd_policy = reference_svd_policy
        self.density_weight_cutoff = density_weight_cutoff
        self.hermitian_tol = hermitian_tol
        self.normalize_references = normalize_references
        self.expand_before_first_sweep = expand_before_first_sweep

    def to_c(self):
        if int(self.krylov_dim) < 0:
            raise T4aError(INVALID_ARGUMENT, "GseOptions: krylov_dim must not be negative")
        if self.reference_max_bond_dim is not None and int(self.reference_max_bond_dim) < 1:
            raise T4aError(INVALID_ARGUMENT, "invalid GSE option reference_max_bond_dim: must be greater than zero when set")
        if self.reference_svd_policy is not None and not isinstance(self.reference_svd_policy, SvdTruncationPolicy):
            raise T4aError(INVALID_ARGUMENT, "GseOptions::reference_svd_policy must be an SvdTruncationPolicy")
        pol = (self.reference_svd_policy or SvdTruncationPolicy()).to_c()
        return GseOptionsC(int(self.krylov_dim), 0 if self.reference_max_bond_dim is None else 1,
                           0 if self.reference_max_bond_dim is None else int(self.reference_max_bond_dim),
                           0 if self.reference_svd_policy is None else 1, pol, float(self.density_weight_cutoff), float(self.hermitian_tol),
                           1 if self.normalize_references else 0, 1 if self.expand_before_first_sweep else 0)


class GseResult:
    """GseResult (gse.rs:118-134): ``edges_processed`` directed edges visited, ``bonds_expanded`` those that gained at least one basis
    vector, ``max_added_basis`` the most one edge gained."""

    def __init__(self, state, references_built, edges_processed, bonds_expanded, max_added_basis):
        self.state = state
        self.references_built = references_built
        self.edges_processed = edges_processed
        self.bonds_expanded = bonds_expanded
        self.max_added_basis = max_added_basis


class GseTdvpOptions:
    """GseTdvpOptions (gse.rs:136-143): ``gse`` a GseOptions, ``tdvp`` a TdvpOptions."""

    def __init__(self, gse=None, tdvp=None):
        self.gse = GseOptions() if gse is None else gse
        self.tdvp = TdvpOptions() if tdvp is None else tdvp


class GseTdvpResult:
    """GseTdvpResult (gse.rs:145-163)"""

    def __init__(self, state, sweeps_completed, local_updates, gse_expansions, max_error_estimate, max_krylov_iterations):
        self.state = state
        self.sweeps_completed = sweeps_completed
        self.local_updates = local_updates
        self.gse_expansions = gse_expansions
        self.max_error_estimate = max_error_estimate
        self.max_krylov_iterations = max_krylov_iterations


def _options(options):
    o = GseOptions() if options is None else options
    if not isinstance(o, GseOptions):
        raise T4aError(INVALID_ARGUMENT, "gse: options must be a GseOptions")
    return o.to_c()


def _center(center):
    if int(center) < 0:
        raise T4aError(INVALID_ARGUMENT, "gse: center must not be negative")
    return c_size_t(int(center))


def _result(h, counters):
    return GseResult(SimpleTensorTrain._adopt(h), *(c.value for c in counters))


def krylov_references(operator, init, options=None):
    """build_references (gse.rs:450-506) -> [SimpleTensorTrain]: H psi, H^2 psi, ... (``krylov_dim`` of them), each the zip-up product
    capped at ``reference_max_bond_dim`` and divided by its norm when ``normalize_references`` is set and the norm is positive."""
    _operands(operator, init)
    o = _options(options)
    k = int(o.krylov_dim)
    hs = (c_void_p * max(k, 1))()
    n = c_size_t(0)
    _check(_lib.t4a_gpu_gse_krylov_references(operator._h, init._h, ctypes.byref(o), c_size_t(k), hs, ctypes.byref(n)))
    return [SimpleTensorTrain._adopt(c_void_p(hs[j])) for j in range(n.value)]


def global_subspace_expand_with_references(init, references, center=0, options=None):
    """global_subspace_expand_with_references (gse.rs:306-366) -> GseResult.  Any ``center``; an empty list returns the canonicalised
    state with zero counters."""
    references = list(references)
    for s in [init] + references:
        if not isinstance(s, SimpleTensorTrain):
            raise T4aError(INVALID_ARGUMENT, "states must be SimpleTensorTrain objects")
    o = _options(options)
    c = _center(center)
    hs = (c_void_p * max(len(references), 1))(*[r._h for r in references])
    h = c_void_p()
    counters = [c_size_t(0) for _ in range(4)]
    _check(_lib.t4a_gpu_gse_expand_with_references(init._h, hs, c_size_t(len(references)), c, ctypes.byref(o), ctypes.byref(h),
                                                   *[ctypes.byref(x) for x in counters]))
    return _result(h, counters)


def global_subspace_expand(operator, init, center=0, options=None):
    """global_subspace_expand (gse.rs:272-294): ``krylov_references`` followed by ``global_subspace_expand_with_references``."""
    _operands(operator, init)
    o = _options(options)
    c = _center(center)
    h = c_void_p()
    counters = [c_size_t(0) for _ in range(4)]
    _check(_lib.t4a_gpu_gse_expand(operator._h, init._h, c, ctypes.byref(o), ctypes.byref(h), *[ctypes.byref(x) for x in counters]))
    return _result(h, counters)


def _gse_tdvp(fn, who, default_nsite, operator, init, center, options):
    """The driver ``fn`` (t4a_gpu_gse_tdvp or t4a_gpu_gse_tdvp_one_site) -> GseTdvpResult"""
    _operands(operator, init)
    o = GseTdvpOptions(tdvp=TdvpOptions(nsite=default_nsite)) if options is None else options
    if not isinstance(o, GseTdvpOptions) or not isinstance(o.tdvp, TdvpOptions):
        raise T4aError(INVALID_ARGUMENT, who + ": options must be a GseTdvpOptions of a GseOptions and a TdvpOptions")
    g, t = _options(o.gse), o.tdvp.to_c()
    c = _center(center)
    h = c_void_p()
    sweeps, updates, expansions, err, iters = c_size_t(0), c_size_t(0), c_size_t(0), c_double(0.0), c_size_t(0)
    _check(fn(operator._h, init._h, c, ctypes.byref(g), ctypes.byref(t), ctypes.byref(h), ctypes.byref(sweeps), ctypes.byref(updates), ctypes.byref(expansions),
              ctypes.byref(err), ctypes.byref(iters)))
    return GseTdvpResult(SimpleTensorTrain._adopt(h), sweeps.value, updates.value, expansions.value, err.value, iters.value)


def gse_tdvp(operator, init, center=0, options=None):
    """gse_tdvp (gse.rs:374-424) -> GseTdvpResult: before sweep s an expansion when ``krylov_dim > 0 and (s > 0 or
    expand_before_first_sweep)``, then ``tdvp`` with ``nsweeps = 1``.  tdvp's own refusals apply unchanged (``nsite = 1`` is
    ``gse_tdvp_one_site``)."""
    return _gse_tdvp(_lib.t4a_gpu_gse_tdvp, "gse_tdvp", 2, operator, init, center, options)


def gse_tdvp_one_site(operator, init, center=0, options=None):
    """The loop of ``gse_tdvp`` with ``tdvp_one_site`` for the one-sweep evolution after each expansion -> GseTdvpResult: the expansion
    grows the bonds globally, the fixed-rank integrator evolves inside them.  Any ``center``.  ``options`` defaults to a GseTdvpOptions
    whose ``tdvp`` has ``nsite = 1``; the refusals are those of the expansion and of ``tdvp_one_site``."""
    return _gse_tdvp(_lib.t4a_gpu_gse_tdvp_one_site, "gse_tdvp_one_site", 1, operator, init, center, options)


def _project(refs, basis, orient=0, route=ROUTE_FUSED):
    """Test hook (t4a_gpu_gse_project).  orient 0: refs[j] (rho_j, q), basis (kb, q) -> (stack (sum rho, q), trace); orient 1: every
    matrix transposed, refs[j] (q, rho_j), basis (q, kb) -> (stack (q, sum rho), trace)."""
    refs = [np.asarray(r, dtype=np.float64) for r in refs]
    basis = np.asarray(basis, dtype=np.float64)
    ax = 1 if orient == 0 else 0
    q, kb = basis.shape[ax], basis.shape[1 - ax]
    rho = np.array([r.shape[1 - ax] for r in refs], dtype=np.uintp)
    if any(r.ndim != 2 or r.shape[ax] != q for r in refs):
        raise T4aError(INVALID_ARGUMENT, "gse_project: every reference has the q dimension of the basis")
    total = int(rho.sum())
    flat = np.ascontiguousarray(np.concatenate([_flat(r) for r in refs])) if refs else np.zeros(1)
    stack = np.zeros(max(total * q, 1))
    trace = c_double(0.0)
    _check(_lib.t4a_gpu_gse_project(c_int32(orient), c_size_t(q), _p(flat), _p(rho), c_size_t(len(refs)), _p(_flat(basis)), c_size_t(kb), c_int32(route),
                                    _p(stack), ctypes.byref(trace)))
    shape = (total, q) if orient == 0 else (q, total)
    return stack[:total * q].reshape(shape, order="F"), trace.value


def _absorb(children, parents, basis, orient=0, route=ROUTE_FUSED):
    """Test hook (t4a_gpu_gse_absorb).  orient 0: children[j] (r_j, q), parents[j] (L_j, r_j), basis (kn, q) -> [parent_j (child_j
    basis^T), (L_j, kn)]; orient 1: children[j] (q, r_j), parents[j] (r_j, L_j), basis (q, kn) -> [(basis^T child_j) parent_j, (kn, L_j)]."""
    children = [np.asarray(c, dtype=np.float64) for c in children]
    parents = [np.asarray(p, dtype=np.float64) for p in parents]
    basis = np.asarray(basis, dtype=np.float64)
    ax = 1 if orient == 0 else 0
    q, kn = basis.shape[ax], basis.shape[1 - ax]
    if len(children) != len(parents) or any(c.ndim != 2 or c.shape[ax] != q for c in children):
        raise T4aError(INVALID_ARGUMENT, "gse_absorb: one parent per child, every child with the q dimension of the basis")
    r = np.array([c.shape[1 - ax] for c in children], dtype=np.uintp)
    ls = np.array([p.shape[0] if orient == 0 else p.shape[1] for p in parents], dtype=np.uintp)
    if any(p.ndim != 2 or (p.shape[1] if orient == 0 else p.shape[0]) != rj for p, rj in zip(parents, r)):
        raise T4aError(INVALID_ARGUMENT, "gse_absorb: the bond of a parent differs from its child's")
    cf = np.ascontiguousarray(np.concatenate([_flat(c) for c in children])) if children else np.zeros(1)
    pf = np.ascontiguousarray(np.concatenate([_flat(p) for p in parents])) if parents else np.zeros(1)
    out = np.zeros(max(int(ls.sum()) * kn, 1))
    _check(_lib.t4a_gpu_gse_absorb(c_int32(orient), c_size_t(q), _p(cf), _p(r), _p(pf), _p(ls), c_size_t(len(children)), _p(_flat(basis)), c_size_t(kn),
                                   c_int32(route), _p(out)))
    res, off = [], 0
    for lj in ls:
        lj = int(lj)
        res.append(out[off:off + lj * kn].reshape((lj, kn) if orient == 0 else (kn, lj), order="F").copy())
        off += lj * kn
    return res


def _route(q, bond):
    """gse_use_fused(q, bond) (t4a_gpu_gse_route, host only) -> ROUTE_FUSED or ROUTE_GEMM"""
    r = c_int32(0)
    _check(_lib.t4a_gpu_gse_route(c_size_t(q), c_size_t(bond), ctypes.byref(r)))
    return r.value


def _set_route(route=None):
    """Test hook (t4a_gpu_gse_set_route): every edge of every later call takes ROUTE_FUSED or ROUTE_GEMM; None: back to the rule."""
    _check(_lib.t4a_gpu_gse_set_route(c_int32(-1 if route is None else route)))


def _time_routes(chi, d=2, n_refs=2, reps=20):
    """Probe (t4a_gpu_gse_time_routes): device milliseconds -> {"project_fused", "project_gemm", "absorb_fused", "absorb_gemm"}."""
    ms = np.zeros(4)
    _check(_lib.t4a_gpu_gse_time_routes(c_size_t(chi), c_size_t(d), c_size_t(n_refs), c_size_t(reps), _p(ms)))
    return dict(zip(("project_fused", "project_gemm", "absorb_fused", "absorb_gemm"), (float(x) for x in ms)))
