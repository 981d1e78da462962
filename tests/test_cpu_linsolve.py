"""square_linsolve without a GPU: the numpy restatement (tests/linsolve_np.py) against dense linear algebra — it is the yardstick of
the device tests —, the options struct, the exported symbols, and the argument checks answered on the host before the device is
touched."""
import ctypes

import numpy as np
import pytest

import linsolve_np as ln
from linsolve_np import SEED, CASES, Options, random_tensors, make_case, dense_cases, np_gmres_affine, np_square_linsolve


# ------------------------------------------------------------------------------------------------ GMRES of the restatement
def run_dense(name):
    h, b, x0, a0, a1, kw = dense_cases()[name]
    x, it, res, conv = np_gmres_affine(lambda v: h @ v, b, x0, a0, a1, **kw)
    true = float(np.linalg.norm(b - (a0 * x + a1 * (h @ x))))
    return x, it, res, conv, true, float(np.linalg.norm(b))


def test_gmres_identity_breaks_down_at_step_zero():
    x, it, res, conv, true, bn = run_dense("identity")
    assert conv and it == 1 and true <= 1e-14 * bn
    assert np.allclose(x, dense_cases()["identity"][1], rtol=0, atol=1e-14)


def test_gmres_three_distinct_eigenvalues_take_three_iterations():
    x, it, res, conv, true, bn = run_dense("three_eigenvalues")
    assert conv and it == 3 and true / bn < 1e-10


def test_gmres_restarts():
    x, it, res, conv, true, bn = run_dense("restart")
    h, b, _, a0, a1, _ = dense_cases()["restart"]
    assert conv and it > 2 and true / bn < 1e-10
    assert np.allclose(x, np.linalg.solve(a0 * np.eye(12) + a1 * h, b), rtol=0, atol=1e-9)


def test_gmres_special_cases():
    x, it, res, conv, _, _ = run_dense("zero_rhs")
    assert conv and it == 0 and res == 0.0 and np.array_equal(x, dense_cases()["zero_rhs"][2])  # b = 0 returns x0
    x, it, res, conv, _, _ = run_dense("a1_zero")
    assert conv and it == 0 and np.array_equal(x, dense_cases()["a1_zero"][1] * (1.0 / 4.0))
    with pytest.raises(ValueError):
        np_gmres_affine(lambda v: v, np.ones(3), np.zeros(3), 0.0, 0.0)
    x, it, res, conv, true, bn = run_dense("not_converged")
    assert not conv and it == 2 and res == pytest.approx(true / bn, rel=1e-12) and res > 1e-10
    x, it, res, conv, true, bn = run_dense("absolute")
    assert conv and true < 1e-9 and res == pytest.approx(true, rel=1e-6, abs=1e-12)


# ------------------------------------------------------------------------------------------------ the sweeps of the restatement
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_local_solves_reach_the_dense_solution(name):
    ops, rhs, init, a0, cap = make_case(name)
    o = Options(a0=a0, a1=1.0, max_bond_dim=cap, nfullsweeps=2)
    x, sweeps, res, conv, stats = np_square_linsolve(ops, rhs, init, 0, o, exact_local=True)
    assert sweeps == 2 and res <= 3e-15 and not conv
    assert [t.shape[0] for t in x[1:]] == CASES[name][6]
    am, bv = ln.np_operator_full(ops), ln.np_state_full(rhs)
    want = np.linalg.solve(a0 * np.eye(am.shape[0]) + am, bv)
    assert np.linalg.norm(ln.np_state_full(x) - want) <= 1e-13 * np.linalg.norm(want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_gmres_sweeps_converge(name):
    ops, rhs, init, a0, cap = make_case(name)
    o = Options(a0=a0, a1=1.0, max_bond_dim=cap, gmres_tol=1e-10, gmres_restart_dim=10, gmres_max_restarts=30, convergence_tol=1e-8)
    x, sweeps, res, conv, stats = np_square_linsolve(ops, rhs, init, 0, o)
    assert conv and res < 1e-8 and sweeps <= 3
    am, bv = ln.np_operator_full(ops), ln.np_state_full(rhs)
    want = np.linalg.solve(a0 * np.eye(am.shape[0]) + am, bv)
    assert np.linalg.norm(ln.np_state_full(x) - want) <= 1e-6 * np.linalg.norm(want)
    assert stats["local_solves"] == sweeps * 2 * (len(ops) - 1)


def test_inner_centre_plan_and_identity_case():
    assert ln.sweep_plan(5, 0) == [(0, True), (1, True), (2, True), (3, True), (3, False), (2, False), (1, False), (0, False)]
    assert ln.sweep_plan(5, 2) == [(2, True), (3, True), (3, False), (2, False), (1, False), (0, False), (0, True), (1, True)]
    ops, rhs, init, a0, cap = make_case("n5")
    x, sweeps, res, conv, _ = np_square_linsolve(ops, rhs, init, 2, Options(a0=a0, max_bond_dim=cap, nfullsweeps=2, convergence_tol=1e-8))
    assert conv and res < 1e-8
    x, sweeps, res, conv, _ = np_square_linsolve(ops, rhs, init, 0, Options(a0=4.0, a1=0.0))
    assert sweeps == 0 and res <= 1e-15 and not conv
    assert np.allclose(ln.np_state_full(x), ln.np_state_full(rhs) / 4.0, rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        np_square_linsolve(ops, rhs, init, 0, Options(a0=0.0, a1=0.0))


def test_projected_pieces_agree_with_each_other():
    ops, rhs, init, a0, cap = make_case("n6")
    x = ln.np_canonicalize(init, 2)
    left = np.ones((1, 1, 1))
    for k in range(2):
        left = ln.np_left_env(left, ops[k], x[k])
    right = np.ones((1, 1, 1))
    for k in range(5, 3, -1):
        right = ln.np_right_env(right, ops[k], x[k])
    v = random_tensors([left.shape[0], right.shape[0]], 2, 2, SEED ^ 0x77)[0]
    y = ln.np_projected_apply(left, right, ops[2], ops[3], v)
    h = ln.np_projected_dense(left, right, ops[2], ops[3])
    assert np.allclose(h @ v.reshape(-1, order="F"), y.reshape(-1, order="F"), rtol=0, atol=1e-13)
    hl, hr = ln.np_half_operators(left, right, ops[2], ops[3])
    m, n, w = v.shape[0] * 2, 2 * v.shape[3], ops[2].shape[3]
    t = hl @ v.reshape((m, n), order="F")                                    # (W M) x N
    y2 = t.reshape((m, w * n), order="F") @ hr                                # the same memory as M x (W N)
    assert np.allclose(y2, y.reshape((m, n), order="F"), rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_options_default_matches_the_reference():
    import t4a_amd
    o = t4a_amd.LinsolveOptionsC()
    assert t4a_amd._lib.t4a_gpu_linsolve_options_default(ctypes.byref(o)) == 0
    assert (o.nfullsweeps, o.has_max_bond_dim, o.has_svd_policy, o.gmres_tol, o.gmres_tolerance_mode, o.gmres_max_restarts,
            o.gmres_restart_dim, o.a0, o.a1, o.has_convergence_tol, o.check_residual) == (5, 0, 0, 1e-10, 0, 100, 30, 0.0, 1.0, 0, 1)
    d = t4a_amd.LinsolveOptions().to_c()
    for name, _ in t4a_amd.LinsolveOptionsC._fields_:
        if name != "svd_policy":
            assert getattr(d, name) == getattr(o, name), name
    assert (d.svd_policy.threshold, d.svd_policy.scale, d.svd_policy.measure, d.svd_policy.rule) == \
        (o.svd_policy.threshold, o.svd_policy.scale, o.svd_policy.measure, o.svd_policy.rule) == (1e-12, 0, 0, 0)
    assert t4a_amd._lib.t4a_gpu_linsolve_options_default(None) == t4a_amd.NULL_POINTER


def test_symbols_are_exported():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("linsolve_options_default", "linsolve_check_shapes", "square_linsolve", "relative_linear_system_residual",
                 "projected_operator_new", "projected_operator_release", "projected_operator_local_dims", "projected_operator_apply",
                 "projected_operator_environment", "projected_operator_invalidate", "projected_operator_set_site_tensors",
                 "projected_operator_apply_env", "linsolve_orth", "linsolve_gmres_dense"):
        assert hasattr(lib, "t4a_gpu_" + name), name
    assert t4a_amd.square_linsolve is t4a_amd.linsolve.square_linsolve and t4a_amd.ProjectedOperator is t4a_amd.linsolve.ProjectedOperator


@pytest.mark.parametrize("field, value", [("gmres_restart_dim", 0), ("gmres_max_restarts", 0), ("gmres_tol", -1e-3), ("gmres_tol", float("nan")),
                                          ("gmres_tol", float("inf")), ("convergence_tol", -1.0), ("convergence_tol", float("nan")),
                                          ("gmres_tolerance_mode", 2), ("max_bond_dim", 0)])
def test_bad_options_are_refused_before_an_operand_is_looked_at(field, value):
    """The operands are NULL: an answer other than INVALID_ARGUMENT would mean they were looked at first."""
    import t4a_amd
    o = t4a_amd.LinsolveOptionsC()
    t4a_amd._lib.t4a_gpu_linsolve_options_default(ctypes.byref(o))
    if field == "convergence_tol":
        o.has_convergence_tol = 1
    if field == "max_bond_dim":
        o.has_max_bond_dim = 1
    setattr(o, field, value)
    h = ctypes.c_void_p()
    st = t4a_amd._lib.t4a_gpu_square_linsolve(None, None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None)
    assert st == t4a_amd.INVALID_ARGUMENT, t4a_amd.last_error_message()
    assert not h and field.replace("_mode", "") in t4a_amd.last_error_message()


def check_shapes(op, rhs, state, center=0, restart_dim=30):
    import t4a_amd
    op, state = np.array(op, dtype=np.uintp).reshape(-1), np.array(state, dtype=np.uintp).reshape(-1)
    r = None if rhs is None else np.array(rhs, dtype=np.uintp).reshape(-1)
    st = t4a_amd._lib.t4a_gpu_linsolve_check_shapes(t4a_amd._p(op), ctypes.c_size_t(len(op) // 4), None if r is None else t4a_amd._p(r),
                                                    ctypes.c_size_t(0 if r is None else len(r) // 3), t4a_amd._p(state),
                                                    ctypes.c_size_t(len(state) // 3), ctypes.c_size_t(center), ctypes.c_size_t(restart_dim))
    return st, t4a_amd.last_error_message()


def test_shape_checks_need_no_device():
    import t4a_amd
    op = [(1, 2, 2, 3), (3, 2, 2, 3), (3, 2, 2, 1)]
    tt = [(1, 2, 4), (4, 2, 4), (4, 2, 1)]
    assert check_shapes(op, tt, tt)[0] == 0
    assert check_shapes(op, None, tt, center=2)[0] == 0
    bad = t4a_amd.INVALID_ARGUMENT
    st, msg = check_shapes(op[:1], [(1, 2, 1)], [(1, 2, 1)])
    assert st == bad and "one-site local solve is not implemented" in msg
    st, msg = check_shapes(op, tt[:2], tt)
    assert st == bad and "lengths differ" in msg
    st, msg = check_shapes(op[:2], tt, tt)
    assert st == bad and "lengths differ" in msg
    st, msg = check_shapes([(1, 2, 3, 3)] + op[1:], tt, tt)
    assert st == bad and "not square" in msg and "site 0" in msg
    st, msg = check_shapes(op, tt, [(1, 2, 4), (4, 3, 4), (4, 2, 1)])
    assert st == bad and "site 1" in msg and "state" in msg
    st, msg = check_shapes(op, [(1, 2, 4), (4, 2, 4), (4, 3, 1)], tt)
    assert st == bad and "site 2" in msg and "rhs" in msg
    st, msg = check_shapes(op, tt, tt, center=3)
    assert st == bad and "center 3" in msg
    # W M^2 = 3 * (20000 * 2)^2 > INT_MAX at the bond (1, 2)
    big = [(1, 2, 4), (4, 2, 20000), (20000, 2, 1)]
    st, msg = check_shapes(op, None, big)
    assert st == bad and "INT_MAX" in msg and "(0, 1)" in msg
    # the Krylov basis: (restart_dim + 1) M N
    st, msg = check_shapes(op, None, tt, restart_dim=2 ** 27)
    assert st == bad and "INT_MAX" in msg


def test_null_arguments_and_python_side_checks():
    import t4a_amd
    lib = t4a_amd._lib
    o = t4a_amd.LinsolveOptions().to_c()
    h = ctypes.c_void_p()
    assert lib.t4a_gpu_square_linsolve(None, None, None, ctypes.c_size_t(0), ctypes.byref(o), None, None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_square_linsolve(None, None, None, ctypes.c_size_t(0), None, ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_square_linsolve(None, None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_projected_operator_new(None, None, ctypes.byref(h)) == t4a_amd.NULL_POINTER
    v = ctypes.c_double(0)
    assert lib.t4a_gpu_relative_linear_system_residual(None, None, None, ctypes.c_double(1), ctypes.c_double(1), ctypes.byref(v)) == t4a_amd.NULL_POINTER
    for kw in ({"max_bond_dim": 0}, {"nfullsweeps": -1}, {"svd_policy": 1e-8}):
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.LinsolveOptions(**kw).to_c()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    # the test hooks: sizes and modes come before the pointers and the device
    one = np.ones(1)
    p = t4a_amd._p
    assert lib.t4a_gpu_linsolve_orth(p(one), ctypes.c_size_t(0), ctypes.c_size_t(1), p(one), p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_linsolve_orth(None, ctypes.c_size_t(1), ctypes.c_size_t(1), p(one), p(one), ctypes.byref(v)) == t4a_amd.NULL_POINTER
    it, conv = ctypes.c_size_t(0), ctypes.c_int32(0)
    args = (ctypes.c_double(0), ctypes.c_double(1), ctypes.c_double(1e-10))
    assert lib.t4a_gpu_linsolve_gmres_dense(p(one), ctypes.c_size_t(1), p(one), p(one), *args, ctypes.c_int32(7), ctypes.c_size_t(3),
                                            ctypes.c_size_t(3), p(one), ctypes.byref(it), ctypes.byref(v), ctypes.byref(conv)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_linsolve_gmres_dense(p(one), ctypes.c_size_t(1), p(one), p(one), *args, ctypes.c_int32(0), ctypes.c_size_t(0),
                                            ctypes.c_size_t(3), p(one), ctypes.byref(it), ctypes.byref(v), ctypes.byref(conv)) == t4a_amd.INVALID_ARGUMENT
    dims = np.array([0, 1], dtype=np.uintp)
    assert lib.t4a_gpu_projected_operator_apply_env(p(one), p(one), p(dims), None, ctypes.c_size_t(0), p(one), p(one), None, None) == t4a_amd.INVALID_ARGUMENT
