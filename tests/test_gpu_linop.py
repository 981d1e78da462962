"""apply_linear_operator on the device against the numpy restatement (tests/apply_np.py) and the dense reference
(identities (x) O) x: the three methods on the routes fused and composed, with and without a cap below the exact bond, for a
full-coverage operator, k = 1, an inner block, the interleaved layout, mixed site dims and an operator with s1 != s2.  The operand sets
satisfy the gap condition (tests/test_cpu_linop.py), so the link dims of a correct run are those of the restatement; dense tensors agree
within the project's rel = 1e-10 (assert_matches of tests/test_gpu_mpo.py).  Then extend and compose, the fit's start, and the user's
case: a one-variable shift on the x bits of an interleaved two-variable train."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import ApplyOptions, LinearOperator, MPO, SimpleTensorTrain, SvdTruncationPolicy

import apply_np as A

pytestmark = pytest.mark.gpu

REL = 1e-10
ROUTES = ("fused", "composed")


def close(got, want, rel=REL):
    scale = max(float(np.abs(want).max()), 1e-300)
    assert np.abs(np.asarray(got) - want).max() <= rel * scale


def dense(tt):
    return tt.full_tensor().reshape(tt.site_dims(), order="F")


def assert_matches(tt, cores, rel=REL):
    assert tt.link_dims() == [c.shape[0] for c in cores[1:]]
    assert tt.site_dims() == [c.shape[1] for c in cores]
    close(dense(tt), A.np_dense_state(cores), rel)


def device_options(method, cap, sweeps=2):
    o = {"naive": ApplyOptions.naive(), "zipup": ApplyOptions.zipup(), "fit": ApplyOptions.fit()}[method]
    o = o.with_svd_policy(SvdTruncationPolicy(A.TOLERANCE)).with_nfullsweeps(sweeps)
    return o if cap is None else o.with_max_bond_dim(cap)


_CACHE = {}


def case(name):
    """operands on the device and the references, computed once per case and left unchanged"""
    if name not in _CACHE:
        op, sites, x, cap = A.case_operands(name)
        ref = {"dense": A.np_dense_apply(op, sites, x), "naive": A.np_naive(op, sites, x)}
        for c in (None, cap):
            o = A.options_for(c)
            ref["zipup", c] = A.np_zipup(op, sites, x, o)
            ref["fit", c] = A.np_fit(op, sites, x, o)
        _CACHE[name] = (LinearOperator(MPO(op), sites), SimpleTensorTrain(x), cap, ref)
    return _CACHE[name]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(A.CASES))
def test_naive(name, route):
    lin, state, cap, ref = case(name)
    for c in (None, cap):  # the cap and the tolerance are ignored, as in the reference's local exact apply
        got = t4a_amd.apply_linear_operator(lin, state, device_options("naive", c), route=route)
        assert_matches(got, ref["naive"])
        close(dense(got), ref["dense"])


@pytest.mark.parametrize("capped", (False, True))
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(A.CASES))
def test_zipup(name, route, capped):
    lin, state, cap, ref = case(name)
    c = cap if capped else None
    got, info = t4a_amd.apply_linear_operator(lin, state, device_options("zipup", c), route=route, return_info=True)
    assert info["route"] == route and info["n_sweeps"] == 0 and info["norms"] == []
    assert_matches(got, ref["zipup", c])
    if capped:
        assert max(got.link_dims()) <= cap
    else:
        close(dense(got), ref["dense"], 1e-7)  # tolerance 1e-9 at each of at most 7 cuts


@pytest.mark.parametrize("capped", (False, True))
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(A.CASES))
def test_fit(name, route, capped):
    lin, state, cap, ref = case(name)
    c = cap if capped else None
    want, winfo = ref["fit", c]
    got, info = t4a_amd.apply_linear_operator(lin, state, device_options("fit", c), route=route, return_info=True)
    assert info["route"] == route
    assert info["n_sweeps"] == winfo["n_sweeps"] == 2
    assert len(info["norms"]) == 3 and np.allclose(info["norms"], winfo["norms"], rtol=REL, atol=0)
    assert_matches(got, want)
    if not capped:
        close(dense(got), ref["dense"], 1e-7)


@pytest.mark.parametrize("route", ROUTES)
def test_fit_from_an_initial_train_and_the_convergence_rule(route):
    lin, state, cap, ref = case("interleaved")
    op, sites, x, start, o = A.initial_fit_case()
    want, winfo = A.np_fit(op, sites, x, o, initial=start)
    assert 1 <= winfo["n_sweeps"] < 6  # the stop test ends the sweeps
    dev = device_options("fit", cap, sweeps=6).with_convergence_tol(1e-3)
    got, info = t4a_amd.apply_linear_operator(lin, state, dev, route=route, initial=SimpleTensorTrain(start), return_info=True)
    assert info["n_sweeps"] == winfo["n_sweeps"] and np.allclose(info["norms"], winfo["norms"], rtol=REL, atol=0)
    assert_matches(got, want)
    # no sweep: the start comes back as it is
    got = t4a_amd.apply_linear_operator(lin, state, device_options("fit", cap, sweeps=0), route=route, initial=SimpleTensorTrain(start))
    assert_matches(got, start)
    bad = SimpleTensorTrain([np.ones((1, 2, 1))] * 7)
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.apply_linear_operator(lin, state, dev, route=route, initial=bad)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT


def test_refusals_reach_the_caller_from_the_driver():
    lin, state, _, _ = case("interleaved")
    op, sites, x, _ = A.case_operands("interleaved")
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.apply_linear_operator(LinearOperator(lin.mpo(), (0, 2, 4, 8)), state)
    assert "Operator nodes [0, 2, 4, 8] are not a subset of state nodes [0, 1, 2, 3, 4, 5, 6, 7]" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.apply_linear_operator(LinearOperator(lin.mpo(), (0, 4, 2, 6)), state)
    assert "strictly ascending" in e.value.message
    three = SimpleTensorTrain([np.ones((1, 3, 1))] * 8)
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.apply_linear_operator(lin, three)
    assert "Shared shape mismatch at site 0: operator has input dim 2, the state has site dim 3" in e.value.message
    with pytest.raises(t4a_amd.T4aError):
        t4a_amd.apply_linear_operator(lin, state, route="eager")


def test_extend_operator_to_full_space():
    op, sites, x, _ = A.case_operands("interleaved")
    want = A.np_extend(op, sites, [c.shape[1] for c in x])
    full = t4a_amd.extend_operator_to_full_space(LinearOperator(MPO(op), sites), [2] * 8)
    assert len(full) == 8
    for g, w in zip(full.site_tensors(), want):
        assert g.shape == w.shape and np.array_equal(g, w)  # operator sites are copies, gap sites exact


def test_compose_of_two_disjoint_blocks_is_one_after_the_other():
    rng = np.random.default_rng(5)
    dims = (2, 3, 2, 2, 3, 2)
    x = [rng.uniform(-1, 1, s) for s in ((1, 2, 3), (3, 3, 4), (4, 2, 4), (4, 2, 3), (3, 3, 2), (2, 2, 1))]
    a = [rng.uniform(-1, 1, s) for s in ((1, 2, 2, 2), (2, 3, 3, 1))]            # on (0, 1)
    b = [rng.uniform(-1, 1, s) for s in ((1, 2, 2, 3), (3, 2, 3, 1))]            # on (3, 4), the second site maps 3 -> 2
    la, lb = LinearOperator(MPO(a), (0, 1)), LinearOperator(MPO(b), (3, 4))
    assert t4a_amd.are_exclusive_operators(6, [la, lb])
    both = t4a_amd.compose_exclusive_linear_operators(dims, [la, lb])
    assert both.sites == tuple(range(6)) and both.mpo().link_dims() == [2, 1, 1, 3, 1]
    assert both.mpo().site_dims() == [(2, 2), (3, 3), (2, 2), (2, 2), (2, 3), (2, 2)]
    state = SimpleTensorTrain(x)
    naive = ApplyOptions.naive()
    for route in ROUTES:
        once = t4a_amd.apply_linear_operator(both, state, naive, route=route)
        twice = t4a_amd.apply_linear_operator(lb, t4a_amd.apply_linear_operator(la, state, naive, route=route), naive, route=route)
        assert once.link_dims() == twice.link_dims()
        close(dense(once), dense(twice), 1e-13)
        close(dense(once), A.np_dense_apply(b, (3, 4), A.np_naive(a, (0, 1), x)), 1e-13)
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.compose_exclusive_linear_operators(dims, [la, LinearOperator(MPO(a), (1, 2))])
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    assert "Operators are not exclusive: they may overlap or not form connected subtrees" in e.value.message


@pytest.mark.parametrize("route", ROUTES)
def test_shift_in_x_of_an_interleaved_two_variable_train(route):
    """f(x, y) on bits x1 y1 x2 y2 x3 y3 x4 y4, R = 4; shift_operator(4, 1, Periodic) on the x bits: g(x, y) = f(x - 1 mod 16, y)"""
    r = 4
    rng = np.random.default_rng(2)
    bonds = [1, 2, 4, 5, 6, 5, 4, 2, 1]
    x = [rng.uniform(-1, 1, (bonds[i], 2, bonds[i + 1])) for i in range(2 * r)]
    state = SimpleTensorTrain(x)
    shift = t4a_amd.shift_operator(r, 1, t4a_amd.BoundaryCondition.Periodic)
    lin = LinearOperator(shift, (0, 2, 4, 6))
    psi = A.np_dense_state(x)  # [x1, y1, x2, y2, ...], the first bit the most significant
    f = psi.transpose(0, 2, 4, 6, 1, 3, 5, 7).reshape(16, 16)
    want = np.roll(f, 1, axis=0).reshape((2,) * 8).transpose(0, 4, 1, 5, 2, 6, 3, 7)
    for o in (ApplyOptions.naive(), ApplyOptions.zipup(), ApplyOptions.fit()):
        got = t4a_amd.apply_linear_operator(lin, state, o, route=route)
        close(dense(got), want, 1e-10)
    # against the route every user had before: the same operator on all x bits of the one-variable reading is quanticstransform.apply
    one = SimpleTensorTrain([rng.uniform(-1, 1, (1 if i == 0 else 3, 2, 1 if i == r - 1 else 3)) for i in range(r)])
    close(dense(t4a_amd.apply_linear_operator(shift, one, ApplyOptions.naive(), route=route)), dense(t4a_amd.quanticstransform.apply(shift, one)), 1e-13)
