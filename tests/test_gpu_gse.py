"""Global subspace expansion and GSE-TDVP on the device (t4a_amd.gse) against the numpy restatement (tests/gse_np.py, itself checked
without a device in tests/test_cpu_gse.py).  The device selects the missing directions of an edge from the SVD of the stacked projected
references, the restatement from the eigendecomposition of the projected density as the reference does: the gauges differ, so only
gauge-invariant quantities are compared — bond dimensions and counters exactly; the dense state against the dense start; per bond the
orthogonal projector onto the span of the block on the far side of the centre; the isometries; the containment of the references.

Tolerances.  Preservation: 100 times the restatement's own preservation error on the same case, floor 1e-12 (the factor covers the
different factorisation route, as in the tdvp tests).  Projectors and containment: tdvp_np.spread_tolerance — the restatement rerun
with the start perturbed in its last bits (seeds 1 - 3), 100 times the largest spread, floor 1e-12.  Isometries: 1e-12, a hundred times
what an orthogonal factor of these sizes (at most 25 columns) loses in f64, 25 * 2.2e-16 * a small constant."""
import numpy as np
import pytest

import gse_np as g
from linsolve_np import np_state_full
import t4a_amd
from t4a_amd import (MPO, SimpleTensorTrain, ContractionOptions, GseOptions, GseTdvpOptions, TdvpOptions, SvdTruncationPolicy, contract_zipup, tdvp,
                     krylov_references, global_subspace_expand, global_subspace_expand_with_references, gse_tdvp)

pytestmark = pytest.mark.gpu

ISOMETRY_TOL = 1e-12


def same_train(a, b):
    ta, tb = a.site_tensors(), b.site_tensors()
    return len(ta) == len(tb) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(ta, tb))


# ------------------------------------------------------------------------------------------------ the expansion
@pytest.mark.parametrize("name", sorted(g.CASES))
def test_expansion_against_the_restatement(name):
    check_expansion(name)


@pytest.mark.parametrize("name", ("bits6_inner", "cores4", "mixed5_last"))
def test_expansion_through_the_gemm_route_against_the_restatement(name):
    """The driver takes the GEMM composition above q * bond = 8192, trains far larger than a test's: the route is
    forced here, on both orientations (bits6_inner has both arms) and on the matrix-core sizes (cores4)."""
    from t4a_amd.gse import _set_route, _route, ROUTE_FUSED, ROUTE_GEMM
    _set_route(ROUTE_GEMM)
    try:
        assert _route(4, 4) == ROUTE_GEMM
        check_expansion(name)
    finally:
        _set_route(None)
    assert _route(4, 4) == ROUTE_FUSED


def check_expansion(name):
    init, refs, center = g.make_case(name)
    want = g.restated(name)
    r = global_subspace_expand_with_references(SimpleTensorTrain(init), [SimpleTensorTrain(x) for x in refs], center)
    cores = r.state.site_tensors()
    # bond dimensions and counters
    assert g.link_dims(cores) == g.link_dims(want["state"])
    assert (r.references_built, r.edges_processed, r.bonds_expanded, r.max_added_basis) == \
        (len(refs), want["edges_processed"], want["bonds_expanded"], want["max_added_basis"])
    # preservation
    psi0 = np_state_full(init)
    own = g.relative_distance(np_state_full(want["state"]), psi0)
    dist = g.relative_distance(np_state_full(cores), psi0)
    # projectors
    tol, spread = g.spread_tolerance(lambda start: g.projector_vector(g.np_gse_with_references(start, refs, center)["state"], center), init)
    pdist = g.relative_distance(g.projector_vector(cores, center), g.projector_vector(want["state"], center))
    defect = g.row_defect(cores, center)
    contain = g.containment_residual(cores, refs, center)
    print(name, "links", g.link_dims(cores), "preservation", dist, "restatement's", own, "projector distance", pdist, "tol", tol, "spread", spread,
          "isometry defect", defect, "containment", contain)
    assert dist <= max(100.0 * own, 1e-12)
    assert pdist <= tol
    assert defect <= ISOMETRY_TOL
    assert contain <= tol


def test_no_references_give_the_canonical_state_and_zero_counters():
    init, _, _ = g.make_case("mixed5")
    for center in (0, 2, 4):
        r = global_subspace_expand_with_references(SimpleTensorTrain(init), [], center)
        assert (r.references_built, r.edges_processed, r.bonds_expanded, r.max_added_basis) == (0, 0, 0, 0)
        cores = r.state.site_tensors()
        assert g.link_dims(cores) == g.link_dims(init) and g.row_defect(cores, center) <= ISOMETRY_TOL
        assert g.relative_distance(np_state_full(cores), np_state_full(init)) <= 1e-12
    ops, start = g.tdvp_case()
    r = global_subspace_expand(MPO(ops), SimpleTensorTrain(start), 0, GseOptions(krylov_dim=0))
    assert (r.references_built, r.edges_processed, r.bonds_expanded, r.max_added_basis) == (0, 0, 0, 0)
    assert r.state.link_dims() == g.link_dims(start)
    assert g.relative_distance(np_state_full(r.state.site_tensors()), np_state_full(start)) <= 1e-12


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("normalize", (True, False))
def test_krylov_references_are_the_public_zipup_chain_bit_for_bit(normalize):
    ops, start = g.tdvp_case()
    op, psi = MPO(ops), SimpleTensorTrain(start)
    for cap, policy in ((None, None), (4, SvdTruncationPolicy(1e-8))):
        o = GseOptions(krylov_dim=2, reference_max_bond_dim=cap, reference_svd_policy=policy, normalize_references=normalize)
        refs = krylov_references(op, psi, o)
        assert len(refs) == 2
        cur = psi
        for ref in refs:
            co = ContractionOptions(tolerance=1e-12 if policy is None else 1e-8, max_bond_dim=max(psi.link_dims()) + 1 if cap is None else cap)
            nxt = contract_zipup(op, MPO.from_tensor_train(cur), co).to_tensor_train()
            if normalize:
                nrm = nxt.norm()
                assert nrm > 0.0
                nxt.scale_mut(1.0 / nrm)
            assert same_train(ref, nxt)
            cur = nxt
        if normalize:
            assert all(abs(ref.norm() - 1.0) < 1e-12 for ref in refs)
    # against the restatement's references: the same bonds, the same dense vectors
    want = g.np_krylov_references(ops, start, g.Options(krylov_dim=2, normalize_references=normalize))
    got = krylov_references(op, psi, GseOptions(krylov_dim=2, normalize_references=normalize))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.link_dims() == g.link_dims(b)
        tol, spread = g.spread_tolerance(
            lambda s: np_state_full(g.np_krylov_references(ops, s, g.Options(krylov_dim=2, normalize_references=normalize))[k]), start)
        dist = g.relative_distance(np_state_full(a.site_tensors()), np_state_full(b))
        print("reference", k, "normalize", normalize, "tol", tol, "spread", spread, "device distance", dist)
        assert dist <= tol


def test_global_subspace_expand_is_references_then_expansion_bit_for_bit():
    ops, start = g.tdvp_case()
    op, psi = MPO(ops), SimpleTensorTrain(start)
    for center in (0, 3, 5):
        o = GseOptions(krylov_dim=1)
        a = global_subspace_expand(op, psi, center, o)
        b = global_subspace_expand_with_references(psi, krylov_references(op, psi, o), center, o)
        assert same_train(a.state, b.state)
        assert (a.references_built, a.edges_processed, a.bonds_expanded, a.max_added_basis) == (b.references_built, b.edges_processed, b.bonds_expanded, b.max_added_basis)
        want = g.np_gse(ops, start, center, g.Options(krylov_dim=1))
        assert a.state.link_dims() == g.link_dims(want["state"])
        assert (a.edges_processed, a.bonds_expanded, a.max_added_basis) == (want["edges_processed"], want["bonds_expanded"], want["max_added_basis"])


# ------------------------------------------------------------------------------------------------ GSE-TDVP
def device_tdvp_options(to):
    return TdvpOptions(nsweeps=to.nsweeps, order=to.order, exponent_step=to.exponent_step, max_bond_dim=to.max_bond_dim,
                       svd_policy=SvdTruncationPolicy(to.svd_threshold))


def test_gse_tdvp_without_references_is_successive_one_sweep_tdvp_bit_for_bit():
    ops, start = g.tdvp_case()
    op, psi = MPO(ops), SimpleTensorTrain(start)
    _, to = g.tdvp_options()
    r = gse_tdvp(op, psi, 0, GseTdvpOptions(GseOptions(krylov_dim=0), device_tdvp_options(to)))
    one = device_tdvp_options(to)
    one.nsweeps = 1
    cur, updates, err, iters = psi, 0, 0.0, 0
    for _ in range(to.nsweeps):
        step = tdvp(op, cur, 0, one)
        cur, updates, err, iters = step.state, updates + step.local_updates, max(err, step.max_error_estimate), max(iters, step.max_krylov_iterations)
    assert same_train(r.state, cur)
    assert (r.sweeps_completed, r.local_updates, r.gse_expansions, r.max_error_estimate, r.max_krylov_iterations) == (to.nsweeps, updates, 0, err, iters)


@pytest.mark.parametrize("first", (True, False))
def test_gse_tdvp_on_the_ising_chain_against_the_restatement(first):
    """TFIM n = 6, bond 2, one Krylov reference, two sweeps of order 2, tau = -0.05, max_bond_dim = 8"""
    ops, start = g.tdvp_case()
    go, to = g.tdvp_options(first)
    want = g.np_gse_tdvp(ops, start, 0, go, to)
    r = gse_tdvp(MPO(ops), SimpleTensorTrain(start), 0,
                 GseTdvpOptions(GseOptions(krylov_dim=go.krylov_dim, expand_before_first_sweep=first), device_tdvp_options(to)))
    assert (r.sweeps_completed, r.local_updates, r.gse_expansions) == (want["sweeps_completed"], want["local_updates"], want["gse_expansions"])
    assert r.gse_expansions == (2 if first else 1)
    assert r.state.link_dims() == g.link_dims(want["state"])
    tol, spread = g.spread_tolerance(lambda s: np_state_full(g.np_gse_tdvp(ops, s, 0, go, to)["state"]), start)
    dist = g.relative_distance(np_state_full(r.state.site_tensors()), np_state_full(want["state"]))
    print("gse_tdvp first", first, "tol", tol, "spread", spread, "device distance", dist, "links", r.state.link_dims())
    assert dist <= tol
    assert 0 < r.max_krylov_iterations <= 30 and 0.0 <= r.max_error_estimate <= 1e-12 * max(1.0, np.linalg.norm(np_state_full(start)))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_arrive_with_the_documented_status_and_text():
    init, refs, _ = g.make_case("mixed4")
    psi, rs = SimpleTensorTrain(init), [SimpleTensorTrain(x) for x in refs]
    bad = t4a_amd.INVALID_ARGUMENT
    for kw, text in (({"density_weight_cutoff": -1.0}, "invalid GSE option density_weight_cutoff: must be finite and non-negative"),
                     ({"density_weight_cutoff": float("nan")}, "invalid GSE option density_weight_cutoff: must be finite and non-negative"),
                     ({"hermitian_tol": float("inf")}, "invalid GSE option hermitian_tol: must be finite and non-negative")):
        with pytest.raises(t4a_amd.T4aError) as e:
            global_subspace_expand_with_references(psi, rs, 0, GseOptions(**kw))
        assert e.value.code == bad and text in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        global_subspace_expand_with_references(psi, rs, 4)
    assert e.value.code == bad and "GSE center 4 is not a state node" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        global_subspace_expand_with_references(psi, [SimpleTensorTrain(init[:2] + [init[2][:, :, :1]])], 0)
    assert e.value.code == bad and "the same tree topology" in e.value.message
    other = [np.ones((1, 3, 1)), np.ones((1, 3, 1)), np.ones((1, 4, 1)), np.ones((1, 2, 1))]
    with pytest.raises(t4a_amd.T4aError) as e:
        global_subspace_expand_with_references(psi, [SimpleTensorTrain(other)], 0)
    assert e.value.code == bad and "invalid GSE mapping at node 1: reference site dimension does not match target" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        global_subspace_expand_with_references(psi, rs * 3, 0)
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED and "more than 8 references" in e.value.message
    # the operator routes
    ops, start = g.tdvp_case()
    op, st = MPO(ops), SimpleTensorTrain(start)
    with pytest.raises(t4a_amd.T4aError) as e:
        global_subspace_expand(MPO(ops[:4] + [ops[4][:, :, :, :1]]), st, 0, GseOptions(krylov_dim=1))
    assert e.value.code == bad and "the same tree topology" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        global_subspace_expand(op, st, 0, GseOptions(krylov_dim=9))
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED
    # gse_tdvp: tdvp's own refusals, unchanged
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp(op, st, 2, GseTdvpOptions(GseOptions(krylov_dim=1), TdvpOptions()))
    assert e.value.code == bad and "center 2 is an inner node of the chain" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp(op, st, 0, GseTdvpOptions(GseOptions(krylov_dim=1), TdvpOptions(nsite=1)))
    assert e.value.code == bad and "one-site TDVP (nsite=1) is not implemented here" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp(op, st, 0, GseTdvpOptions(GseOptions(krylov_dim=1), TdvpOptions(exponent_step=-0.1j)))
    assert e.value.code == bad and "complex tensor trains" in e.value.message
