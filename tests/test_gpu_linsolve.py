"""square_linsolve on the device against the numpy restatement (tests/linsolve_np.py, checked by tests/test_cpu_linsolve.py) and
dense linear algebra: the GMRES the sweeps run, the projected operator with its cached environments, and the sweeps."""
import numpy as np
import pytest

import linsolve_np as ln
from linsolve_np import CASES, make_case, dense_cases
import t4a_amd
from t4a_amd import (MPO, SimpleTensorTrain, ProjectedOperator, LinsolveOptions, GmresToleranceMode, square_linsolve,
                     relative_linear_system_residual)
from t4a_amd.linsolve import _gmres_dense
from t4a_amd.quanticstransform import shift_operator, BoundaryCondition

pytestmark = pytest.mark.gpu

_RESTATED = {}


def restated(name):
    """the restatement's run of a case, once"""
    if name not in _RESTATED:
        ops, rhs, init, a0, cap = make_case(name)
        o = ln.Options(a0=a0, a1=1.0, max_bond_dim=cap, gmres_tol=1e-10, gmres_restart_dim=10, gmres_max_restarts=30, convergence_tol=1e-8)
        _RESTATED[name] = ln.np_square_linsolve(ops, rhs, init, 0, o)
    return _RESTATED[name]


def device_options(a0, cap, **kw):
    base = dict(a0=a0, a1=1.0, max_bond_dim=cap, gmres_tol=1e-10, gmres_restart_dim=10, gmres_max_restarts=30, convergence_tol=1e-8)
    base.update(kw)
    return LinsolveOptions(**base)


# ------------------------------------------------------------------------------------------------ GMRES
@pytest.mark.parametrize("name", sorted(dense_cases()))
def test_gmres_dense_against_the_restatement(name):
    h, b, x0, a0, a1, kw = dense_cases()[name]
    want_x, want_it, want_res, want_conv = ln.np_gmres_affine(lambda v: h @ v, b, x0, a0, a1, **kw)
    x, it, res, conv = _gmres_dense(h, b, x0, a0, a1, **kw)
    assert conv == want_conv
    if name in ("identity", "three_eigenvalues"):
        assert it == want_it
    true = float(np.linalg.norm(b - (a0 * x + a1 * (h @ x))))
    bn = float(np.linalg.norm(b))
    if conv and bn > 0:
        tol, mode = kw.get("tol", 1e-10), kw.get("mode", ln.RELATIVE)
        # the true residual recomputed here: two f64 evaluations of an O(1) quantity of a few hundred terms apart
        assert (true / bn if mode == ln.RELATIVE else true) < tol + 1e-12
    if name == "zero_rhs":
        assert it == 0 and np.array_equal(x, x0)
    if name == "a1_zero":
        assert it == 0 and np.array_equal(x, b * (1.0 / a0))
    if name == "not_converged":
        assert it == 2 and res == pytest.approx(true / bn, rel=1e-9)


def test_gmres_dense_refuses_two_zero_coefficients():
    h, b, x0, _, _, _ = dense_cases()["restart"]
    with pytest.raises(t4a_amd.T4aError) as e:
        _gmres_dense(h, b, x0, 0.0, 0.0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ the projected operator
def test_projected_operator_apply_against_the_dense_projection():
    ops, rhs, init, a0, cap = make_case("n6")
    x = ln.np_canonicalize(ln.random_state([1, 2, 4, 7, 4, 2, 1], 2, ln.SEED ^ 0x51), 2)
    po = ProjectedOperator(MPO(ops), SimpleTensorTrain(x))
    rng = np.random.default_rng(3)

    def check(site, x):
        left = np.ones((1, 1, 1))
        for k in range(site):
            left = ln.np_left_env(left, ops[k], x[k])
        right = np.ones((1, 1, 1))
        for k in range(len(x) - 1, site + 1, -1):
            right = ln.np_right_env(right, ops[k], x[k])
        dense = ln.np_projected_dense(left, right, ops[site], ops[site + 1])
        shape = po.local_dimension(site)
        assert shape == (x[site].shape[0], 2, 2, x[site + 1].shape[2])
        v = rng.standard_normal(shape)
        want = dense @ v.reshape(-1, order="F")
        got = po.apply(site, v).reshape(-1, order="F")
        # sums of fewer than 10^4 terms of O(1) operands
        assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
        got_l, got_r = po.environment("left", site), po.environment("right", site + 2)
        assert np.abs(got_l - left).max() <= 1e-12 * np.abs(left).max() and np.abs(got_r - right).max() <= 1e-12 * np.abs(right).max()

    for site in (2, 0, 4, 3):
        check(site, x)
    # two site tensors change (the shared bond too): without the invalidation the cached environments would still be the old ones
    new_a, new_b = rng.standard_normal((2, 2, 3)), rng.standard_normal((3, 2, 7))
    po.set_site_tensors(1, new_a, new_b)
    y = [t.copy() for t in x]
    y[1], y[2] = new_a, new_b
    for site in (3, 0, 1):
        check(site, y)
    po.invalidate(0)
    po.invalidate(5)
    check(2, y)
    with pytest.raises(t4a_amd.T4aError):
        po.apply(5, np.zeros((1, 2, 2, 1)))
    with pytest.raises(t4a_amd.T4aError):
        po.set_site_tensors(1, np.zeros((3, 2, 3)), new_b)


# ------------------------------------------------------------------------------------------------ the sweeps
def dense_checks(ops, rhs, a0, a1, result, tol=1e-8):
    x = result.solution.site_tensors()
    again = ln.np_residual(ops, x, rhs, a0, a1)
    assert result.residual is not None and abs(result.residual - again) <= 1e-10, (result.residual, again)
    return x, again


@pytest.mark.parametrize("name", sorted(CASES))
def test_square_linsolve_on_the_shared_cases(name):
    ops, rhs, init, a0, cap = make_case(name)
    r = square_linsolve(MPO(ops), SimpleTensorTrain(rhs), SimpleTensorTrain(init), 0, device_options(a0, cap))
    assert r.converged and r.residual < 1e-8
    x, again = dense_checks(ops, rhs, a0, 1.0, r)
    am, bv = ln.np_operator_full(ops), ln.np_state_full(rhs)
    want = np.linalg.solve(a0 * np.eye(am.shape[0]) + am, bv)
    # cond(a0 + A) <= 3 (a0 = 2 ||A||): a residual of 1e-8 is an error of at most 3e-8
    assert np.linalg.norm(ln.np_state_full(x) - want) <= 1e-6 * np.linalg.norm(want)
    assert r.sweeps <= restated(name)[1] + 1
    assert r.stats["local_solves"] == r.sweeps * 2 * (len(ops) - 1) and r.stats["apply_calls"] > r.stats["arnoldi_steps"] > 0
    assert all(b <= cap for b in r.solution.link_dims())
    assert relative_linear_system_residual(MPO(ops), r.solution, SimpleTensorTrain(rhs), a0, 1.0) == r.residual


def test_two_solves_give_the_same_bits():
    ops, rhs, init, a0, cap = make_case("n6")
    runs = [square_linsolve(MPO(ops), SimpleTensorTrain(rhs), SimpleTensorTrain(init), 0, device_options(a0, cap)) for _ in range(2)]
    assert runs[0].residual == runs[1].residual and runs[0].stats == runs[1].stats
    for a, b in zip(runs[0].solution.site_tensors(), runs[1].solution.site_tensors()):
        assert a.tobytes() == b.tobytes()


def test_bond_cap():
    ops, rhs, init, a0, _ = make_case("n6")
    r = square_linsolve(MPO(ops), SimpleTensorTrain(rhs), SimpleTensorTrain(init), 0, device_options(a0, 3, nfullsweeps=3))
    assert all(b <= 3 for b in r.solution.link_dims())
    x, again = dense_checks(ops, rhs, a0, 1.0, r)
    assert all(np.isfinite(t).all() for t in x) and np.isfinite(r.residual)


def test_quantics_shift_system():
    """(2.5 I - S) x = b with the periodic shift by one of 8 bits"""
    op = shift_operator(8, 1, BoundaryCondition.Periodic).mpo()
    ops = op.site_tensors()
    rhs = ln.random_state([1, 2, 3, 3, 3, 3, 3, 2, 1], 2, ln.SEED ^ 0x5F)
    init = ln.random_state([1] + [2] * 7 + [1], 2, ln.SEED ^ 0x60)
    o = LinsolveOptions(a0=2.5, a1=-1.0, gmres_tol=1e-10, gmres_restart_dim=10, gmres_max_restarts=30, convergence_tol=1e-8)
    r = square_linsolve(op, SimpleTensorTrain(rhs), SimpleTensorTrain(init), 0, o)
    assert r.converged and r.residual < 1e-8
    x, again = dense_checks(ops, rhs, 2.5, -1.0, r)
    am, bv = ln.np_operator_full(ops), ln.np_state_full(rhs)
    want = np.linalg.solve(2.5 * np.eye(256) - am, bv)
    assert np.linalg.norm(ln.np_state_full(x) - want) <= 1e-6 * np.linalg.norm(want)


def test_identity_operator_with_a_zero_guess_returns_the_rhs():
    """the reference's doctest (square/mod.rs)"""
    n, d = 4, 2
    rhs = ln.random_state([1, 2, 2, 2, 1], d, ln.SEED ^ 0x1D)
    zero = [np.zeros((1, d, 1)) for _ in range(n)]
    r = square_linsolve(MPO.identity([d] * n), SimpleTensorTrain(rhs), SimpleTensorTrain(zero), 0, LinsolveOptions())
    got, want = ln.np_state_full(r.solution.site_tensors()), ln.np_state_full(rhs)
    assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)
    assert r.sweeps == 5 and r.residual < 1e-9 and not r.converged  # no convergence_tol was given


def test_special_cases():
    ops, rhs, init, a0, cap = make_case("n5")
    op, b, x0 = MPO(ops), SimpleTensorTrain(rhs), SimpleTensorTrain(init)
    r = square_linsolve(op, b, x0, 0, LinsolveOptions(a0=4.0, a1=0.0))
    assert r.sweeps == 0 and r.residual <= 1e-15 and not r.converged
    assert np.allclose(ln.np_state_full(r.solution.site_tensors()), ln.np_state_full(rhs) / 4.0, rtol=0, atol=1e-15)
    with pytest.raises(t4a_amd.T4aError) as e:
        square_linsolve(op, b, x0, 0, LinsolveOptions(a0=0.0, a1=0.0))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    for center in (4, 2):
        r = square_linsolve(op, b, x0, center, device_options(a0, cap))
        assert r.converged and r.residual < 1e-8
        dense_checks(ops, rhs, a0, 1.0, r)
    r = square_linsolve(op, b, x0, 0, device_options(a0, cap, gmres_tolerance_mode=GmresToleranceMode.Absolute, gmres_tol=1e-9))
    assert r.converged and r.residual < 1e-8
    dense_checks(ops, rhs, a0, 1.0, r)
    r = square_linsolve(op, b, x0, 0, LinsolveOptions(a0=a0, a1=1.0, max_bond_dim=cap, nfullsweeps=1, check_residual=False))
    assert r.residual is None and not r.converged and r.sweeps == 1


def test_guess_with_bonds_the_chain_cannot_carry():
    """The QR sweeps to centre 2 meet (l s) < r from the left and l > (s r) from the right: the bonds [4, 6, 6, 4] of the guess shrink
    to [2, 4, 4, 2] before the first local solve.  a0 = 2 ||A||_2 as in make_case, so the same conditioning argument holds."""
    n, d = 5, 2
    ops = ln.random_tensors([1, 2, 2, 2, 2, 1], d, d, ln.SEED ^ 0x51)
    rhs = ln.random_state([1, 2, 2, 2, 2, 1], d, ln.SEED ^ 0x52)
    init = ln.random_state([1, 4, 6, 6, 4, 1], d, ln.SEED ^ 0x53)
    am, bv = ln.np_operator_full(ops), ln.np_state_full(rhs)
    a0 = 2.0 * float(np.linalg.norm(am, 2))
    r = square_linsolve(MPO(ops), SimpleTensorTrain(rhs), SimpleTensorTrain(init), 2, device_options(a0, 16))
    assert r.converged and r.residual < 1e-8
    x, again = dense_checks(ops, rhs, a0, 1.0, r)
    want = np.linalg.solve(a0 * np.eye(d ** n) + am, bv)
    assert np.linalg.norm(ln.np_state_full(x) - want) <= 1e-6 * np.linalg.norm(want)
    assert all(got <= most for got, most in zip(r.solution.link_dims(), [2, 4, 4, 2]))


def test_shape_errors_through_the_handles():
    ops, rhs, init, a0, cap = make_case("n5")
    op, b, x0 = MPO(ops), SimpleTensorTrain(rhs), SimpleTensorTrain(init)
    short = SimpleTensorTrain(ln.random_state([1, 2, 2, 1], 3, 1))
    with pytest.raises(t4a_amd.T4aError) as e:
        square_linsolve(op, short, x0, 0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "lengths differ" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        square_linsolve(op, b, x0, 5)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "center 5" in e.value.message
    wrong = SimpleTensorTrain(ln.random_state([1, 2, 2, 2, 2, 1], 2, 1))
    with pytest.raises(t4a_amd.T4aError) as e:
        square_linsolve(op, b, wrong, 0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "site 0" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        ProjectedOperator(MPO(ops[:1] + [np.ones((2, 3, 2, 2))] + ops[2:]), x0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "not square" in e.value.message
