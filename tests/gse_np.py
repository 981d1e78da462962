"""numpy restatement of the global subspace expansion (t4a_gpu_gse_expand*) that follows tensor4all-treetn's gse.rs literally on a
chain: per edge the density of the reference children, P rho P / t with P = 1 - B^T B, its Hermitianisation, numpy's eigh and the cutoff
on the eigenvalues (expand_one_edge, gse.rs:601-809); the references by the zip-up of tests/fit_np.py (build_references :450-506 with
this project's simplett zip-up in place of apply_linear_operator); gse_tdvp (:374-424) composed with tests/tdvp_np.py's np_tdvp.  Also
the gauge-invariant quantities the device tests compare and the cases the CPU and the device tests share.  State sites are [l, s, r],
operator sites [w_l, s1, s2, w_r]."""
import numpy as np

from fit_np import SEED, np_zipup
from linsolve_np import np_canonicalize, np_state_full
from dmrg_np import tfim, heisenberg, random_state  # noqa: F401
from tdvp_np import np_tdvp, _move_center, Options as TdvpOptions, perturbed, relative_distance, spread_tolerance  # noqa: F401


class Options:
    """GseOptions::default() (gse.rs:59-72); reference_svd_threshold None is the 1e-12 of the zip-up"""

    def __init__(self, krylov_dim=0, reference_max_bond_dim=None, reference_svd_threshold=None, density_weight_cutoff=1e-12, hermitian_tol=1e-12,
                 normalize_references=True, expand_before_first_sweep=True):
        self.krylov_dim = krylov_dim
        self.reference_max_bond_dim = reference_max_bond_dim
        self.reference_svd_threshold = reference_svd_threshold
        self.density_weight_cutoff = density_weight_cutoff
        self.hermitian_tol = hermitian_tol
        self.normalize_references = normalize_references
        self.expand_before_first_sweep = expand_before_first_sweep


def validate_options(o):
    """validate_options (gse.rs:426-448) with the reference's messages"""
    if not np.isfinite(o.density_weight_cutoff) or o.density_weight_cutoff < 0.0:
        raise ValueError("invalid GSE option density_weight_cutoff: must be finite and non-negative")
    if not np.isfinite(o.hermitian_tol) or o.hermitian_tol < 0.0:
        raise ValueError("invalid GSE option hermitian_tol: must be finite and non-negative")
    if o.reference_max_bond_dim is not None and o.reference_max_bond_dim == 0:
        raise ValueError("invalid GSE option reference_max_bond_dim: must be greater than zero when set")


def validate_reference(target, reference):
    """validate_reference (gse.rs:524-546) on a chain: the same length, the same site dimensions"""
    if len(reference) != len(target):
        raise ValueError("GSE requires target, references, and operator support to have the same tree topology")
    for node, (t, r) in enumerate(zip(target, reference)):
        if t.shape[1] != r.shape[1]:
            raise ValueError("invalid GSE mapping at node %d: reference site dimension does not match target" % node)


class _ZipOptions:
    def __init__(self, tolerance, max_bond_dim):
        self.tolerance = tolerance
        self.max_bond_dim = max_bond_dim


def np_krylov_references(ops, init, options):
    """build_references: H psi, H^2 psi, ... each the zip-up product capped at reference_max_bond_dim (None: max link + 1), divided by
    its norm when normalize_references is set and the norm is positive"""
    validate_options(options)
    cap = options.reference_max_bond_dim
    if cap is None:
        cap = max([t.shape[0] for t in init[1:]] + [1]) + 1
    zo = _ZipOptions(1e-12 if options.reference_svd_threshold is None else options.reference_svd_threshold, cap)
    refs, cur = [], init
    for _ in range(options.krylov_dim):
        nxt = [t[:, :, 0, :] for t in np_zipup(ops, [c[:, :, None, :] for c in cur], zo)]
        if options.normalize_references:
            nrm = float(np.linalg.norm(np_state_full(nxt)))
            if nrm > 0.0:
                nxt[-1] = nxt[-1] * (1.0 / nrm)
        refs.append(nxt)
        cur = nxt
    return refs


def _rows(core, child_left_of_parent):
    """the child as r x q, the bond to the parent as rows"""
    l, s, r = core.shape
    return core.reshape((l * s, r), order="F").T if child_left_of_parent else core.reshape((l, s * r), order="F")


def _core(mat, shape, child_left_of_parent):
    """the inverse of _rows for a k x q matrix: the far legs of `shape` are kept"""
    l, s, r = shape
    k = mat.shape[0]
    return mat.T.reshape((l, s, k), order="F") if child_left_of_parent else mat.reshape((k, s, r), order="F")


def _expand_one_edge(trains, child, parent, o, log):
    """expand_one_edge and update_reference_edge: trains[0] is the target -> rows appended"""
    mirror = child < parent
    c = _rows(trains[0][child], mirror)
    q = c.shape[1]
    _, sv, vt = np.linalg.svd(c, full_matrices=False)  # factorize_full_rank(SVD, Canonical::Right): all min(r, q) rows
    basis = vt
    density = np.zeros((q, q))
    for ref in trains[1:]:
        r = _rows(ref[child], mirror)
        if r.shape[1] != q:
            raise ValueError("invalid GSE mapping at node %d: reference child-side bond dimension does not match target" % child)
        density = density + r.T @ r
    trace = float(np.trace(density))
    rows = [basis[i] for i in range(basis.shape[0])]
    lams = np.zeros(0)
    if trace > 0.0:
        p = np.eye(q) - basis.T @ basis
        missing = p @ (density * (1.0 / trace)) @ p
        if not np.all(np.abs(missing - missing.T) <= o.hermitian_tol * np.maximum(1.0, np.abs(missing))):
            raise ValueError("GSE failed to diagonalize projected reference density")
        lams, vecs = np.linalg.eigh(0.5 * (missing + missing.T))
        for col, lam in enumerate(lams):
            if lam > o.density_weight_cutoff:
                rows.append(vecs[:, col])
    log["eigenvalues"].append(np.array(lams))
    log["child_singular_values"].append(np.array(sv))
    new_basis = np.stack(rows)
    for t in trains:
        coeff = _rows(t[child], mirror) @ new_basis.T  # r_t x kn
        shape = t[child].shape
        if mirror:
            t[parent] = np.einsum("ar,asq->rsq", coeff, t[parent])
        else:
            t[parent] = np.einsum("lsa,ak->lsk", t[parent], coeff)
        t[child] = _core(new_basis, shape, mirror)
    return new_basis.shape[0] - basis.shape[0]


def np_gse_with_references(init, references, center=0, options=None):
    """global_subspace_expand_with_references -> dict(state, trains, references_built, edges_processed, bonds_expanded, max_added_basis,
    eigenvalues, child_singular_values): eigenvalues[e] holds every eigenvalue of the Hermitianised P rho P / t of edge e in the order
    the edges are walked (the left arm 0->1 .. c-1->c, then the right arm n-1->n-2 .. c+1->c)."""
    o = Options() if options is None else options
    validate_options(o)
    n = len(init)
    if not 0 <= center < n:
        raise ValueError("GSE center %d is not a state node" % center)
    for ref in references:
        validate_reference(init, ref)
    trains = [np_canonicalize(init, center)] + [np_canonicalize(r, center) for r in references]
    out = {"references_built": len(references), "edges_processed": 0, "bonds_expanded": 0, "max_added_basis": 0, "eigenvalues": [],
           "child_singular_values": []}
    if references:
        edges = [(i, i + 1) for i in range(center)] + [(i, i - 1) for i in range(n - 1, center, -1)]
        cur = center
        for child, parent in edges:
            for t in trains:
                _move_center(t, cur, child)  # move_center_to_region_full_rank
            added = _expand_one_edge(trains, child, parent, o, out)
            cur = parent
            out["edges_processed"] += 1
            if added > 0:
                out["bonds_expanded"] += 1
                out["max_added_basis"] = max(out["max_added_basis"], added)
    out["state"] = trains[0]
    out["trains"] = trains
    return out


def np_gse(ops, init, center=0, options=None):
    """global_subspace_expand: the references, then the expansion"""
    o = Options() if options is None else options
    validate_options(o)
    if len(ops) != len(init):
        raise ValueError("GSE requires target, references, and operator support to have the same tree topology")
    return np_gse_with_references(init, np_krylov_references(ops, init, o), center, o)


def np_gse_tdvp(ops, init, center=0, gse_options=None, tdvp_options=None):
    """gse_tdvp -> dict(state, sweeps_completed, local_updates, gse_expansions, max_error_estimate, max_krylov_iterations)"""
    g = Options() if gse_options is None else gse_options
    t = TdvpOptions() if tdvp_options is None else tdvp_options
    validate_options(g)
    out = {"sweeps_completed": 0, "local_updates": 0, "gse_expansions": 0, "max_error_estimate": 0.0, "max_krylov_iterations": 0}
    state = [c.copy() for c in init]
    one = TdvpOptions(nsweeps=1, order=t.order, exponent_step=t.exponent_step, max_bond_dim=t.max_bond_dim, krylov=t.krylov,
                      svd_threshold=t.svd_threshold, cgs2=t.cgs2)
    for sweep in range(t.nsweeps):
        if g.krylov_dim > 0 and (sweep > 0 or g.expand_before_first_sweep):
            state = np_gse(ops, state, center, g)["state"]
            out["gse_expansions"] += 1
        r = np_tdvp(ops, state, center, one)
        state = r["state"]
        out["sweeps_completed"] += r["sweeps_completed"]
        out["local_updates"] += r["local_updates"]
        out["max_error_estimate"] = max(out["max_error_estimate"], r["max_error_estimate"])
        out["max_krylov_iterations"] = max(out["max_krylov_iterations"], r["max_krylov_iterations"])
    out["state"] = state
    return out


# ------------------------------------------------------------------------------------------------ gauge-invariant quantities
def link_dims(cores):
    return [int(c.shape[0]) for c in cores[1:]]


def far_block(cores, bond, center):
    """the block on the far side of the centre at the bond between sites bond - 1 and bond, as (physical indices) x (bond)"""
    if bond <= center:
        acc = cores[0].reshape((cores[0].shape[1], cores[0].shape[2]), order="F")
        for c in cores[1:bond]:
            acc = np.tensordot(acc, c, axes=([-1], [0]))
            acc = acc.reshape((-1, c.shape[2]), order="F")
        return acc
    acc = cores[-1].reshape((cores[-1].shape[0], cores[-1].shape[1]), order="F")  # bond x physical
    for c in reversed(cores[bond:-1]):
        acc = np.tensordot(c, acc, axes=([2], [0])).reshape((c.shape[0], -1), order="F")
    return acc.T


def bond_projectors(cores, center):
    """for every bond the orthogonal projector onto the span of its far block, on the physical indices"""
    out = []
    for bond in range(1, len(cores)):
        q, _ = np.linalg.qr(far_block(cores, bond, center))
        out.append(q @ q.T)
    return out


def projector_vector(cores, center):
    return np.concatenate([p.reshape(-1) for p in bond_projectors(cores, center)])


def row_defect(cores, center):
    """the largest deviation of a non-centre core from an isometry towards the centre"""
    worst = 0.0
    for i, c in enumerate(cores):
        if i == center:
            continue
        m = _rows(c, i < center)
        worst = max(worst, float(np.abs(m @ m.T - np.eye(m.shape[0])).max()))
    return worst


def containment_residual(cores, references, center):
    """the largest |(1 - P) M| / |M| over the bonds and the references: P the projector of the expanded state at the bond, M the dense
    reference matricised at the bond with the far side as rows (its column space is what the reference occupies there, whatever the
    gauge and the rank of its own bond)"""
    projs = bond_projectors(cores, center)
    dims = [c.shape[1] for c in cores]
    worst = 0.0
    for ref in references:
        psi = np_state_full(ref)
        nrm = float(np.linalg.norm(psi))
        if nrm == 0.0:
            continue
        for bond in range(1, len(cores)):
            m = psi.reshape((int(np.prod(dims[:bond])), -1), order="F")
            m = m if bond <= center else m.T
            worst = max(worst, float(np.linalg.norm(m - projs[bond - 1] @ m)) / nrm)
    return worst


# ------------------------------------------------------------------------------------------------ the cases the CPU and the device tests share
CASES = {  # name: (site dimensions, state bonds, [reference bonds], centre)
    "mixed5": ((2, 3, 2, 2, 3), [1, 2, 2, 2, 2, 1], [[1, 3, 3, 3, 3, 1]] * 2, 0),
    "bits6": ((2,) * 6, [1, 2, 2, 2, 2, 2, 1], [[1, 3, 3, 3, 3, 3, 1]], 0),
    "mixed4": ((3, 2, 4, 2), [1, 2, 2, 2, 1], [[1, 2, 2, 2, 1]] * 3, 0),
    "mixed5_last": ((2, 3, 2, 2, 3), [1, 2, 2, 2, 2, 1], [[1, 3, 3, 3, 3, 1]] * 2, 4),
    "bits6_inner": ((2,) * 6, [1, 2, 2, 2, 2, 2, 1], [[1, 3, 3, 3, 3, 3, 1]], 3),
    "cores4": ((5, 5, 5, 5), [1, 5, 17, 5, 1], [[1, 5, 18, 5, 1]], 0),  # the matrix-core route
}
SEEDS = {name: SEED ^ (0x65E0 + 17 * k) for k, name in enumerate(CASES)}
# The TDVP splits cut at 1e-5 of the largest singular value: with the default 1e-12 every state that leaves a sweep carries singular
# values down to 1e-11 of the largest, and the children of the second expansion miss the gap condition (1e-6) whatever the seed.
TDVP_CASE = {"n": 6, "g": 0.7, "bond": 2, "krylov_dim": 1, "nsweeps": 2, "order": 2, "tau": -0.05, "max_bond_dim": 8, "svd_threshold": 1e-5,
             "seed": SEED ^ 0x65ED}

_CACHE = {}


def make_case(name):
    """-> (init, references, centre)"""
    dims, bonds, ref_bonds, center = CASES[name]
    seed = SEEDS[name]
    init = random_state(dims, bonds, seed)
    refs = [random_state(dims, rb, seed ^ (0xA5 * (k + 1))) for k, rb in enumerate(ref_bonds)]
    return init, refs, center


def restated(name):
    if name not in _CACHE:
        init, refs, center = make_case(name)
        _CACHE[name] = np_gse_with_references(init, refs, center)
    return _CACHE[name]


def tdvp_case():
    """-> (operator sites, start): TFIM n = 6, bond 2"""
    c = TDVP_CASE
    n = c["n"]
    return tfim(n, c["g"]), random_state((2,) * n, [1] + [c["bond"]] * (n - 1) + [1], c["seed"])


def tdvp_options(expand_before_first_sweep=True):
    c = TDVP_CASE
    return (Options(krylov_dim=c["krylov_dim"], expand_before_first_sweep=expand_before_first_sweep),
            TdvpOptions(nsweeps=c["nsweeps"], order=c["order"], exponent_step=c["tau"], max_bond_dim=c["max_bond_dim"], svd_threshold=c["svd_threshold"]))


def gap_report(result):
    """-> (eigenvalues inside (1e-14, 1e-8), the smallest ratio of a child's smallest to its largest singular value)"""
    inside = [float(v) for lams in result["eigenvalues"] for v in lams if 1e-14 < v < 1e-8]
    ratio = min(float(sv.min() / sv.max()) for sv in result["child_singular_values"]) if result["child_singular_values"] else 1.0
    return inside, ratio
