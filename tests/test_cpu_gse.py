"""Global subspace expansion without a GPU: the numpy restatement (tests/gse_np.py) on the real-valued chain cases of the reference's
tests (crates/tensor4all-treetn/tests/gse.rs) — it is the yardstick of the device tests, so state preservation, the isometries and the
gap condition on the shared cases come first —, the options struct, the exported symbols, and the argument checks answered on the host
before the device is touched."""
import ctypes

import numpy as np
import pytest

import gse_np as g
from gse_np import Options, np_gse, np_gse_tdvp, np_gse_with_references
from linsolve_np import np_state_full

E0, E1 = np.array([1.0, 0.0]), np.array([0.0, 1.0])


def product_chain(*vectors):
    """product_chain_state / product_chain3_state / product_chain_state_from_vectors (tests/gse.rs:10-104): bonds of dimension 1"""
    return [np.asarray(v, dtype=np.float64).reshape((1, -1, 1)) for v in vectors]


def entangled_chain3(leaf):
    """entangled_chain3_state (tests/gse.rs:179-213): |0> (x) sum_b |b> (x) leaf[b, :]"""
    t1 = np.zeros((1, 2, 2))
    t1[0, 0, 0] = t1[0, 1, 1] = 1.0
    return [E0.reshape((1, 2, 1)), t1, np.asarray(leaf, dtype=np.float64).reshape((2, 2, 1))]


def identity_or_x(n, x_nodes):
    """identity_or_x_operator (tests/gse.rs:215-290): operator bonds 1, X on the nodes of x_nodes"""
    x = np.array([[0.0, 1.0], [1.0, 0.0]])
    return [(x if k in x_nodes else np.eye(2)).reshape((1, 2, 2, 1)) for k in range(n)]


def distance(a, b):
    return float(np.linalg.norm(np_state_full(a) - np_state_full(b)))


def row_basis(core):
    return core.reshape((core.shape[0], -1), order="F")


def projected_weight(basis, vector):
    return float(((basis @ vector) ** 2).sum() / (vector ** 2).sum())


# ------------------------------------------------------------------------------------------------ the cases of the reference's tests
def test_preserves_state_and_grows_chain_bond():
    state, reference = product_chain(E0, E0), product_chain(E0, E1)
    r = np_gse_with_references(state, [reference], 0, Options(density_weight_cutoff=1e-14))
    assert (r["references_built"], r["edges_processed"]) == (1, 1) and r["bonds_expanded"] >= 1
    assert g.link_dims(r["state"]) == [2] and distance(r["state"], state) < 1e-10
    child = row_basis(r["state"][1])
    assert child[1, 1] ** 2 > 1.0 - 1e-10  # the appended row is the missing site direction


def test_maps_processed_child_bond_in_chain_q_space():
    state = product_chain(E0, E0, E0)
    refs = [product_chain(E0, E0, E1), product_chain(E0, E1, E1)]
    r = np_gse_with_references(state, refs, 0, Options(density_weight_cutoff=1e-14))
    assert r["edges_processed"] == 2 and r["bonds_expanded"] >= 2
    links = g.link_dims(r["state"])
    assert links[1] == 2 and links[0] >= 2 and distance(r["state"], state) < 1e-10


def test_handles_nonproduct_processed_child_bond_basis():
    state, reference = entangled_chain3([[1.0, 0.0], [0.0, 0.5]]), entangled_chain3([[0.0, 1.0], [0.5, 0.0]])
    r = np_gse_with_references(state, [reference], 0, Options(density_weight_cutoff=1e-14))
    assert r["edges_processed"] == 2 and r["bonds_expanded"] >= 1
    links = g.link_dims(r["state"])
    assert links[1] == 2 and links[0] >= 2 and distance(r["state"], state) < 1e-10
    basis = row_basis(r["state"][1])  # rows over (site 1, the processed bond)
    assert np.abs(basis @ basis.T - np.eye(basis.shape[0])).max() < 1e-10
    # the reference's block on sites 1 and 2 (t1 is delta(s1, b): the block is its leaf matrix) lies in the expanded span of bond 1
    block = g.far_block(r["state"], 1, 0)
    direction = np.array([[0.0, 1.0], [0.5, 0.0]]).reshape(-1, order="F")
    assert projected_weight(block.T, direction) > 1.0 - 1e-10


def test_builds_operator_references():
    state = product_chain(E0, E0)
    for krylov_dim in (1, 2):
        r = np_gse(identity_or_x(2, (1,)), state, 0, Options(krylov_dim=krylov_dim, density_weight_cutoff=1e-14))
        assert r["references_built"] == krylov_dim and g.link_dims(r["state"]) == [2] and distance(r["state"], state) < 1e-10


def test_centre_on_the_right_site_and_a_direction_in_a_larger_q_space():
    state = product_chain([1.0, 0.0, 0.0, 0.0], E0)
    ref_left = np.array([0.0, np.sqrt(0.5), np.sqrt(0.5), 0.0])
    r = np_gse_with_references(state, [product_chain(ref_left, E0)], 1, Options(density_weight_cutoff=1e-14))
    assert g.link_dims(r["state"]) == [2] and distance(r["state"], state) < 1e-10
    basis = r["state"][0].reshape((4, 2), order="F").T
    assert np.abs(basis @ basis.T - np.eye(2)).max() < 1e-10 and projected_weight(basis, ref_left) > 1.0 - 1e-10


def test_respects_density_weight_cutoff_without_dropping_target():
    state = product_chain(E0, E0)
    r = np_gse_with_references(state, [product_chain(E0, E1)], 0, Options(density_weight_cutoff=2.0))
    assert r["bonds_expanded"] == 0 and g.link_dims(r["state"]) == [1] and distance(r["state"], state) < 1e-10


def test_with_empty_references_is_noop():
    state = product_chain(E0, E0, E0)
    r = np_gse_with_references(state, [], 0)
    assert (r["references_built"], r["edges_processed"], r["bonds_expanded"], r["max_added_basis"]) == (0, 0, 0, 0)
    assert distance(r["state"], state) < 1e-10


@pytest.mark.parametrize("first", [True, False])
def test_gse_tdvp_runs_tdvp_after_expansion(first):
    """gse_tdvp_runs_existing_tdvp_after_expansion and .._can_skip_first_expansion_and_expand_later_sweeps with this project's
    two-site sweeps and real exponent, against the dense exponential"""
    state = product_chain(E0, E0)
    nsweeps = 1 if first else 2
    r = np_gse_tdvp(identity_or_x(2, (1,)), state, 0, Options(krylov_dim=1, density_weight_cutoff=1e-14, expand_before_first_sweep=first),
                    g.TdvpOptions(nsweeps=nsweeps, exponent_step=-0.01))
    assert r["gse_expansions"] == 1 and r["sweeps_completed"] == nsweeps and r["local_updates"] > 0
    # (the two-site split truncates the expanded bond again: exp(t 1 (x) X) |00> = |0> (x) (cosh t |0> + sinh t |1>) is a product)
    t = -0.01 * nsweeps
    assert np.abs(np_state_full(r["state"]) - np.array([np.cosh(t), 0.0, np.sinh(t), 0.0])).max() < 1e-12


def test_rejects_invalid_options_center_and_mismatched_references():
    state = product_chain(E0, E0)
    for kw, text in (({"density_weight_cutoff": -1.0}, "invalid GSE option density_weight_cutoff: must be finite and non-negative"),
                     ({"hermitian_tol": -1.0}, "invalid GSE option hermitian_tol: must be finite and non-negative"),
                     ({"reference_max_bond_dim": 0}, "invalid GSE option reference_max_bond_dim: must be greater than zero when set")):
        with pytest.raises(ValueError, match=text):
            np_gse_with_references(state, [], 0, Options(**kw))
    with pytest.raises(ValueError, match="GSE center 2 is not a state node"):
        np_gse_with_references(state, [], 2)
    with pytest.raises(ValueError, match="the same tree topology"):
        np_gse_with_references(state, [product_chain(E0, E0, E0)], 0)
    with pytest.raises(ValueError, match="reference site dimension does not match target"):
        np_gse_with_references(state, [product_chain([1.0, 0.0, 0.0], E0)], 0)


# ------------------------------------------------------------------------------------------------ the shared cases
@pytest.mark.parametrize("name", sorted(g.CASES))
def test_restatement_preserves_the_state_and_leaves_isometries(name):
    init, refs, center = g.make_case(name)
    r = g.restated(name)
    assert g.relative_distance(np_state_full(r["state"]), np_state_full(init)) < 1e-12
    assert g.row_defect(r["state"], center) < 1e-12
    assert r["edges_processed"] == len(init) - 1 and r["bonds_expanded"] >= 1
    assert g.containment_residual(r["state"], refs, center) < 1e-11
    assert all(a >= b for a, b in zip(g.link_dims(r["state"]), g.link_dims(init)))


def _gap_cases():
    for name in sorted(g.CASES):
        yield name, lambda name=name: g.restated(name)
    ops, init = g.tdvp_case()
    for center in (0, 3, 5):  # the centres of the device test of global_subspace_expand on the Krylov reference
        yield "tfim6_center%d" % center, lambda center=center: np_gse(ops, init, center, g.tdvp_options()[0])


@pytest.mark.parametrize("name, run", list(_gap_cases()), ids=[n for n, _ in _gap_cases()])
def test_gap_condition_of_every_case_the_device_tests_use(name, run):
    """No normalised eigenvalue of any edge inside (1e-14, 1e-8): the eigen and the SVD selection then keep the same directions; every
    child's smallest singular value above 1e-6 of its largest: the old basis is well defined.  A condition on the inputs, not a tolerance."""
    inside, ratio = g.gap_report(run())
    assert inside == [] and ratio > 1e-6


def test_gap_condition_holds_along_the_gse_tdvp_run():
    """the expansions of the second sweep see the evolved state: their eigenvalues are checked as well"""
    ops, init = g.tdvp_case()
    for first in (True, False):
        go, to = g.tdvp_options(first)
        state = [c.copy() for c in init]
        one = g.TdvpOptions(nsweeps=1, order=to.order, exponent_step=to.exponent_step, max_bond_dim=to.max_bond_dim, svd_threshold=to.svd_threshold)
        for sweep in range(to.nsweeps):
            if sweep > 0 or first:
                r = np_gse(ops, state, 0, go)
                inside, ratio = g.gap_report(r)
                assert inside == [] and ratio > 1e-6, (first, sweep)
                state = r["state"]
            state = g.np_tdvp(ops, state, 0, one)["state"]


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_options_default_matches_the_reference():
    import t4a_amd
    o = t4a_amd.GseOptionsC()
    assert t4a_amd._lib.t4a_gpu_gse_options_default(ctypes.byref(o)) == 0
    assert (o.krylov_dim, o.has_reference_max_bond_dim, o.has_reference_svd_policy, o.density_weight_cutoff, o.hermitian_tol, o.normalize_references,
            o.expand_before_first_sweep) == (0, 0, 0, 1e-12, 1e-12, 1, 1)
    d = t4a_amd.GseOptions().to_c()
    for name, _ in t4a_amd.GseOptionsC._fields_:
        if name != "reference_svd_policy":
            assert getattr(d, name) == getattr(o, name), name
    assert t4a_amd._lib.t4a_gpu_gse_options_default(None) == t4a_amd.NULL_POINTER
    c = t4a_amd.GseOptions(krylov_dim=2, reference_max_bond_dim=7, reference_svd_policy=t4a_amd.SvdTruncationPolicy(1e-8), normalize_references=False,
                           expand_before_first_sweep=False).to_c()
    assert (c.krylov_dim, c.has_reference_max_bond_dim, c.reference_max_bond_dim, c.has_reference_svd_policy, c.reference_svd_policy.threshold,
            c.normalize_references, c.expand_before_first_sweep) == (2, 1, 7, 1, 1e-8, 0, 0)
    t = t4a_amd.GseTdvpOptions()
    assert isinstance(t.gse, t4a_amd.GseOptions) and isinstance(t.tdvp, t4a_amd.TdvpOptions)


def test_symbols_are_exported():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("gse_options_default", "gse_check_shapes", "gse_krylov_references", "gse_expand_with_references", "gse_expand", "gse_tdvp", "gse_project",
                 "gse_absorb", "gse_route", "gse_set_route", "gse_time_routes"):
        assert hasattr(lib, "t4a_gpu_" + name), name
    from t4a_amd.gse import _project, _absorb, _time_routes  # noqa: F401
    assert t4a_amd.gse_tdvp is t4a_amd.gse.gse_tdvp and t4a_amd.GseResult is t4a_amd.gse.GseResult
    assert t4a_amd.global_subspace_expand is t4a_amd.gse.global_subspace_expand
    assert t4a_amd.global_subspace_expand_with_references is t4a_amd.gse.global_subspace_expand_with_references
    assert t4a_amd.krylov_references is t4a_amd.gse.krylov_references


def test_the_route_rule_is_a_function_of_the_shape():
    """fused up to q * bond = 128 * 64, the measured win; the GEMM composition above"""
    from t4a_amd.gse import _route, _set_route, ROUTE_FUSED, ROUTE_GEMM
    assert [_route(q, b) for q, b in ((1, 1), (25, 17), (128, 64), (64, 128), (129, 64), (256, 128), (512, 256))] == \
        [ROUTE_FUSED] * 4 + [ROUTE_GEMM] * 3
    _set_route(ROUTE_GEMM)
    assert _route(1, 1) == ROUTE_GEMM
    _set_route(ROUTE_FUSED)
    assert _route(512, 256) == ROUTE_FUSED
    _set_route(None)
    assert (_route(1, 1), _route(512, 256)) == (ROUTE_FUSED, ROUTE_GEMM)
    import t4a_amd
    assert t4a_amd._lib.t4a_gpu_gse_set_route(ctypes.c_int32(2)) == t4a_amd.INVALID_ARGUMENT
    assert t4a_amd._lib.t4a_gpu_gse_route(ctypes.c_size_t(0), ctypes.c_size_t(1), ctypes.byref(ctypes.c_int32(0))) == t4a_amd.INVALID_ARGUMENT
    assert t4a_amd._lib.t4a_gpu_gse_route(ctypes.c_size_t(1), ctypes.c_size_t(1), None) == t4a_amd.NULL_POINTER


INF, NAN = float("inf"), float("nan")
BAD_OPTIONS = ([("density_weight_cutoff", v, "invalid GSE option density_weight_cutoff: must be finite and non-negative") for v in (-1.0, NAN, INF, -INF)]
               + [("hermitian_tol", v, "invalid GSE option hermitian_tol: must be finite and non-negative") for v in (-1.0, NAN, INF, -INF)]
               + [("reference_max_bond_dim", 0, "invalid GSE option reference_max_bond_dim: must be greater than zero when set"),
                  ("reference_svd_policy.threshold", -1e-3, "Invalid SVD truncation threshold: threshold must be finite and non-negative")])


def _bad(field, value):
    import t4a_amd
    o = t4a_amd.GseOptionsC()
    t4a_amd._lib.t4a_gpu_gse_options_default(ctypes.byref(o))
    if field == "reference_max_bond_dim":
        o.has_reference_max_bond_dim = 1
    if field.startswith("reference_svd_policy."):
        o.has_reference_svd_policy = 1
        setattr(o.reference_svd_policy, field.split(".")[1], value)
    else:
        setattr(o, field, value)
    return o


@pytest.mark.parametrize("field, value, message", BAD_OPTIONS, ids=["%s=%s" % (f, v) for f, v, _ in BAD_OPTIONS])
def test_bad_options_are_refused_before_an_operand_is_looked_at(field, value, message):
    """The operands are NULL: an answer other than INVALID_ARGUMENT would mean they were looked at first."""
    import t4a_amd
    lib = t4a_amd._lib
    o = _bad(field, value)
    h = ctypes.c_void_p()
    zero = ctypes.c_size_t(0)
    t = t4a_amd.TdvpOptions().to_c()
    for st in (lib.t4a_gpu_gse_expand_with_references(None, None, zero, zero, ctypes.byref(o), ctypes.byref(h), None, None, None, None),
               lib.t4a_gpu_gse_expand(None, None, zero, ctypes.byref(o), ctypes.byref(h), None, None, None, None),
               lib.t4a_gpu_gse_tdvp(None, None, zero, ctypes.byref(o), ctypes.byref(t), ctypes.byref(h), None, None, None, None, None),
               lib.t4a_gpu_gse_krylov_references(None, None, ctypes.byref(o), zero, None, ctypes.byref(zero)),
               lib.t4a_gpu_gse_check_shapes(ctypes.byref(o), None, zero, None, None, zero, zero)):
        assert st == t4a_amd.INVALID_ARGUMENT, t4a_amd.last_error_message()
        assert not h and message in t4a_amd.last_error_message()


def test_gse_tdvp_refuses_what_tdvp_refuses_before_an_operand_is_looked_at():
    import t4a_amd
    lib = t4a_amd._lib
    o = t4a_amd.GseOptions(krylov_dim=1).to_c()
    h = ctypes.c_void_p()
    for kw, text in (({"nsite": 1}, "one-site TDVP (nsite=1) is not implemented here"), ({"order": 3}, "order 3 is not supported"),
                     ({"nsweeps": 0}, "invalid TDVP option nsweeps: must be greater than zero")):
        t = t4a_amd.TdvpOptions(**kw).to_c()
        st = lib.t4a_gpu_gse_tdvp(None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.byref(t), ctypes.byref(h), None, None, None, None, None)
        assert st == t4a_amd.INVALID_ARGUMENT and text in t4a_amd.last_error_message()
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.TdvpOptions(exponent_step=-0.1j).to_c()
    assert "complex tensor trains" in e.value.message


def check_shapes(state, refs, center=0, options=None):
    import t4a_amd
    o = (t4a_amd.GseOptions() if options is None else options).to_c()
    s = np.array(state, dtype=np.uintp).reshape(-1)
    flat = np.array([d for r in refs for d in r], dtype=np.uintp).reshape(-1) if refs else np.zeros(1, dtype=np.uintp)
    lens = np.array([len(r) for r in refs], dtype=np.uintp) if refs else np.zeros(1, dtype=np.uintp)
    st = t4a_amd._lib.t4a_gpu_gse_check_shapes(ctypes.byref(o), t4a_amd._p(s), ctypes.c_size_t(len(state)), t4a_amd._p(flat), t4a_amd._p(lens),
                                               ctypes.c_size_t(len(refs)), ctypes.c_size_t(center))
    return st, t4a_amd.last_error_message()


def test_shape_checks_need_no_device():
    import t4a_amd
    tt = [(1, 2, 4), (4, 3, 4), (4, 2, 1)]
    ref = [(1, 2, 2), (2, 3, 5), (5, 2, 1)]
    bad = t4a_amd.INVALID_ARGUMENT
    for center in (0, 1, 2):
        assert check_shapes(tt, [ref, ref], center)[0] == 0
    assert check_shapes(tt, [])[0] == 0
    st, msg = check_shapes(tt, [ref], 3)
    assert st == bad and "GSE center 3 is not a state node" in msg
    st, msg = check_shapes(tt, [ref[:2]])
    assert st == bad and "GSE requires target, references, and operator support to have the same tree topology" in msg
    st, msg = check_shapes(tt, [ref, [(1, 2, 2), (2, 2, 5), (5, 2, 1)]])
    assert st == bad and "invalid GSE mapping at node 1: reference site dimension does not match target" in msg
    assert check_shapes(tt, [ref] * 8)[0] == 0
    st, msg = check_shapes(tt, [ref] * 9)
    assert st == t4a_amd.NOT_IMPLEMENTED and "more than 8 references" in msg


def test_null_arguments_and_python_side_checks():
    import t4a_amd
    lib = t4a_amd._lib
    o = t4a_amd.GseOptions().to_c()
    t = t4a_amd.TdvpOptions().to_c()
    h = ctypes.c_void_p()
    zero, one_ = ctypes.c_size_t(0), ctypes.c_size_t(1)
    assert lib.t4a_gpu_gse_expand(None, None, zero, ctypes.byref(o), None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gse_expand(None, None, zero, None, ctypes.byref(h), None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gse_expand(None, None, zero, ctypes.byref(o), ctypes.byref(h), None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gse_expand_with_references(None, None, zero, zero, ctypes.byref(o), ctypes.byref(h), None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gse_tdvp(None, None, zero, ctypes.byref(o), ctypes.byref(t), ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gse_tdvp(None, None, zero, ctypes.byref(o), None, ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    for kw in ({"reference_max_bond_dim": 0}, {"krylov_dim": -1}, {"reference_svd_policy": 1e-8}):
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.GseOptions(**kw).to_c()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    for call in (lambda: t4a_amd.global_subspace_expand(None, None), lambda: t4a_amd.global_subspace_expand_with_references(None, []),
                 lambda: t4a_amd.gse_tdvp(None, None), lambda: t4a_amd.krylov_references(None, None)):
        with pytest.raises(t4a_amd.T4aError) as e:
            call()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    # the hooks: shapes come before the pointers and the device
    p = t4a_amd._p
    one = np.ones(1)
    v = ctypes.c_double(0.0)
    dims1, dims0, dims9 = np.ones(1, dtype=np.uintp), np.zeros(1, dtype=np.uintp), np.ones(9, dtype=np.uintp)
    i0 = ctypes.c_int32(0)
    assert lib.t4a_gpu_gse_project(ctypes.c_int32(2), one_, p(one), p(dims1), one_, p(one), one_, i0, p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_project(i0, one_, p(one), p(dims1), one_, p(one), one_, ctypes.c_int32(2), p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_project(i0, one_, p(one), p(dims0), one_, p(one), one_, i0, p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_project(i0, one_, p(one), p(dims9), ctypes.c_size_t(9), p(one), one_, i0, p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_project(i0, zero, p(one), p(dims1), one_, p(one), one_, i0, p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_project(i0, one_, None, p(dims1), one_, p(one), one_, i0, p(one), ctypes.byref(v)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gse_absorb(i0, one_, p(one), p(dims0), p(one), p(dims1), one_, p(one), one_, i0, p(one)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_absorb(i0, one_, p(one), p(dims1), p(one), p(dims1), zero, p(one), one_, i0, p(one)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_absorb(i0, one_, p(one), p(dims1), p(one), p(dims1), one_, p(one), zero, i0, p(one)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_absorb(i0, one_, p(one), p(dims1), None, p(dims1), one_, p(one), one_, i0, p(one)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gse_time_routes(zero, one_, one_, one_, p(np.zeros(4))) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_time_routes(one_, one_, ctypes.c_size_t(9), one_, p(np.zeros(4))) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_gse_time_routes(one_, one_, one_, one_, None) == t4a_amd.NULL_POINTER
