"""Two-site TDVP without a GPU: the numpy restatement (tests/tdvp_np.py) against dense exponentials — it is the yardstick of the device
tests, so its own accuracy and the condition on the capped input come first —, the region plan through the C ABI against the
restatement's, the options struct, the exported symbols, and the argument checks answered on the host before the device is touched."""
import ctypes

import numpy as np
import pytest

import tdvp_np as tn
from tdvp_np import TWO, CORR, TAU, KrylovOptions, np_krylov_expm, np_tdvp


# ------------------------------------------------------------------------------------------------ the plan
def test_first_order_plan_of_three_sites():
    tau = -0.2
    assert tn.tdvp_plan(3, 0, 1, tau) == [(TWO, (0, 1), 1, tau), (CORR, (1,), 1, -tau), (TWO, (1, 2), 2, tau)]
    assert tn.tdvp_plan(3, 2, 1, tau) == [(TWO, (2, 1), 1, tau), (CORR, (1,), 1, -tau), (TWO, (1, 0), 0, tau)]


def test_second_order_plan_reverses_the_second_half():
    tau, h = -0.2, -0.1
    assert tn.tdvp_plan(3, 0, 2, tau) == [(TWO, (0, 1), 1, h), (CORR, (1,), 1, -h), (TWO, (1, 2), 2, h),
                                          (TWO, (2, 1), 1, h), (CORR, (1,), 1, -h), (TWO, (1, 0), 0, h)]
    assert tn.tdvp_plan(2, 0, 1, tau) == [(TWO, (0, 1), 1, tau)]
    assert tn.tdvp_plan(2, 0, 2, tau) == [(TWO, (0, 1), 1, h), (TWO, (1, 0), 0, h)]
    assert tn.tdvp_plan(2, 1, 2, tau) == [(TWO, (1, 0), 0, h), (TWO, (0, 1), 1, h)]


def test_fourth_order_weights_and_alternating_substeps():
    w = tn.applyexp_sub_steps(4)
    assert len(w) == 6 and abs(sum(w) - 1.0) <= 1e-14
    n, tau = 5, -0.3
    plan = tn.tdvp_plan(n, 0, 4, tau)
    per = 2 * (n - 1) - 1
    assert len(plan) == 6 * per
    for k in range(6):
        part = plan[k * per:(k + 1) * per]
        assert part[0][1] == ((0, 1) if k % 2 == 0 else (n - 1, n - 2)) and part[-1][2] == (n - 1 if k % 2 == 0 else 0)
        assert all(abs(e - (tau if kind == TWO else -tau) * w[k]) <= 1e-16 for kind, _, _, e in part)
        assert [s[0] for s in part] == [TWO, CORR] * (n - 2) + [TWO]
        assert all(nodes[-1] == nc for _, nodes, nc, _ in part)
    with pytest.raises(ValueError, match="order 3 is not supported"):
        tn.applyexp_sub_steps(3)


@pytest.mark.parametrize("n, order", [(2, 1), (2, 2), (2, 4), (3, 1), (3, 2), (3, 4), (6, 1), (6, 2), (6, 4)])
def test_the_plan_of_the_library_equals_the_restatement(n, order):
    from t4a_amd.tdvp import tdvp_plan
    for center in (0, n - 1):
        for tau in (-0.05, 0.7):
            assert tdvp_plan(n, center, order, tau) == tn.tdvp_plan(n, center, order, tau)


# ------------------------------------------------------------------------------------------------ the Krylov exponential of the restatement
def dense_expm(h, tau, v):
    lams, q = np.linalg.eigh(h)
    return q @ (np.exp(tau * lams) * (q.T @ v))


def run_dense(name, cgs2=False):
    h, v0, tau, o = tn.dense_cases()[name]
    return (h, v0, tau, o) + np_krylov_expm(lambda v: h @ v, tau, v0, o, cgs2)


@pytest.mark.parametrize("cgs2", (False, True))
def test_expm_three_distinct_eigenvalues_break_down_after_three_steps(cgs2):
    h, v0, tau, o, out, it, err, conv, splits = run_dense("diag3", cgs2)
    assert conv and it == 3 and err == 0.0 and splits == 1
    assert np.linalg.norm(out - dense_expm(h, tau, v0)) <= 1e-14 * np.linalg.norm(v0)


@pytest.mark.parametrize("cgs2", (False, True))
def test_expm_eigenvector_start_takes_one_step(cgs2):
    h, v0, tau, o, out, it, err, conv, splits = run_dense("eigenvector_start", cgs2)
    assert conv and it == 1 and splits == 1
    assert np.linalg.norm(out - dense_expm(h, tau, v0)) <= 1e-14 * np.linalg.norm(v0)


def test_expm_early_returns():
    for name in ("tau_zero", "zero_start"):
        h, v0, tau, o, out, it, err, conv, splits = run_dense(name)
        assert conv and it == 0 and err == 0.0 and splits == 1 and np.array_equal(out, v0)


@pytest.mark.parametrize("cgs2", (False, True))
def test_expm_general_matrices_meet_the_estimate(cgs2):
    for name in ("symmetric12", "symmetric40"):
        h, v0, tau, o, out, it, err, conv, splits = run_dense(name, cgs2)
        threshold = o.tol * max(np.linalg.norm(v0), 1.0)
        assert conv and splits == 1 and err <= threshold
        assert np.linalg.norm(out - dense_expm(h, tau, v0)) <= 100 * threshold


def test_expm_two_steps_force_time_splits():
    h, v0, tau, o, out, it, err, conv, splits = run_dense("forced_split")
    threshold = o.tol * max(np.linalg.norm(v0), 1.0)
    print("forced_split: splits", splits, "iterations", it, "estimate", err, "threshold", threshold)
    assert conv and splits > 1 and it == 2 * splits and err <= threshold
    assert np.linalg.norm(out - dense_expm(h, tau, v0)) <= splits * threshold
    # the two orders of the orthogonalisation agree on the flags: the device is compared on them
    assert run_dense("forced_split", True)[5:] == (it, pytest.approx(err, rel=1e-9), conv, splits)


def test_expm_refusals():
    h, v0, tau, o = tn.failing_case()
    with pytest.raises(ValueError, match="did not converge within max_time_splits=1 and max_iter=1"):
        np_krylov_expm(lambda v: h @ v, tau, v0, o)
    h, v0 = tn.nonsymmetric_case()
    with pytest.raises(ValueError, match="not Hermitian"):
        np_krylov_expm(lambda v: h @ v, -0.3, v0)
    with pytest.raises(ValueError, match="max_iter must be greater than zero"):
        np_krylov_expm(lambda v: v, -0.3, np.ones(3), KrylovOptions(max_iter=0))
    with pytest.raises(ValueError, match="max_time_splits must be greater than zero"):
        np_krylov_expm(lambda v: v, -0.3, np.ones(3), KrylovOptions(max_time_splits=0))


# ------------------------------------------------------------------------------------------------ the sweeps of the restatement
@pytest.mark.parametrize("name", tn.DENSE_CHECKED)
def test_operator_is_symmetric_and_the_start_has_full_bonds(name):
    ops, init = tn.make_case(name)
    h = tn.np_operator_full(ops)
    assert np.array_equal(h, h.T)
    assert [t.shape[2] for t in init[:-1]] == tn.full_bonds(tn.CASES[name])[1:-1]


@pytest.mark.parametrize("order, end, nsweeps", tn.RUNS)
@pytest.mark.parametrize("name", tn.DENSE_CHECKED)
def test_full_bond_sweeps_reproduce_the_dense_exponential(name, order, end, nsweeps):
    """With every bond full the projectors are identities and each substep is exact up to the Krylov tolerance 1e-12: the bound is the
    1e-9 of the reference's two_site_tdvp_heisenberg_chain_matches_dense_exact_evolution."""
    n = len(tn.CASES[name])
    r = tn.restated(name, order, end, nsweeps)
    err = tn.relative_distance(tn.np_state_full(r["state"]), tn.dense_exponential(name, TAU * nsweeps))
    print(name, order, end, nsweeps, "relative error", err, "max estimate", r["max_error_estimate"], "max iterations", r["max_krylov_iterations"])
    assert err <= 1e-9
    substeps = len(tn.applyexp_sub_steps(order))
    assert r["sweeps_completed"] == nsweeps and r["local_updates"] == nsweeps * substeps * (2 * (n - 1) - 1)
    assert r["two_site_steps"] == nsweeps * substeps * (n - 1) and r["corrections"] == nsweeps * substeps * (n - 2)
    assert r["max_time_splits"] == 1 and r["max_error_estimate"] <= 1e-12 * max(1.0, np.linalg.norm(tn.np_state_full(tn.make_case(name)[1])))


def test_exact_local_exponentials_and_the_classical_order_agree_with_the_krylov_sweeps():
    ops, init = tn.make_case("tfim6")
    want = tn.dense_exponential("tfim6", TAU)
    for kw in ({"exact_local": True}, {}):
        r = np_tdvp(ops, init, 0, tn.Options(order=2, exponent_step=TAU), **kw)
        assert tn.relative_distance(tn.np_state_full(r["state"]), want) <= 1e-9
    r = tn.restated("tfim6", 2, 0, 1, cgs2=True)
    assert tn.relative_distance(tn.np_state_full(r["state"]), want) <= 1e-9
    with pytest.raises(ValueError):
        np_tdvp(ops[:1], init[:1])
    with pytest.raises(ValueError):
        np_tdvp(ops, init, 2)


def test_capped_case_stays_finite_and_cuts_at_a_gap():
    """The condition on the input of the device comparison: wherever a split of the restatement's run drops a non-zero singular value,
    sigma_k / sigma_{k+1} >= 10 at the cut — the kept subspace is then well conditioned against the rounding differences of another
    implementation (Wedin: the rotation is the perturbation over the gap)."""
    ops, init, o = tn.capped_case()
    r = tn.capped_restated()
    psi = tn.np_state_full(r["state"])
    h = tn.np_operator_full(ops)
    norm, energy = float(np.linalg.norm(psi)), float(psi @ (h @ psi)) / float(psi @ psi)
    print("capped: norm", norm, "energy", energy, "cuts", len(r["cut_ratios"]), "smallest ratio", min(r["cut_ratios"]))
    assert np.isfinite(norm) and np.isfinite(energy) and norm > 0
    assert max(t.shape[2] for t in r["state"][:-1]) <= o.max_bond_dim
    assert len(r["cut_ratios"]) >= 1 and min(r["cut_ratios"]) >= 10.0
    assert r["sweeps_completed"] == 3


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_options_default_matches_the_reference_but_for_the_real_exponent():
    import t4a_amd
    o = t4a_amd.TdvpOptionsC()
    assert t4a_amd._lib.t4a_gpu_tdvp_options_default(ctypes.byref(o)) == 0
    assert (o.nsite, o.nsweeps, o.order, o.exponent_step_re, o.exponent_step_im, o.has_max_bond_dim, o.has_svd_policy) == (2, 1, 2, -0.1, 0.0, 0, 0)
    assert (o.krylov.max_iter, o.krylov.max_time_splits, o.krylov.tol, o.krylov.breakdown_tol, o.krylov.hermitian_tol) == (30, 100, 1e-12, 1e-14, 1e-10)
    d = t4a_amd.TdvpOptions().to_c()
    for name, _ in t4a_amd.TdvpOptionsC._fields_:
        if name not in ("svd_policy", "krylov"):
            assert getattr(d, name) == getattr(o, name), name
    for name, _ in t4a_amd.KrylovExpmOptionsC._fields_:
        assert getattr(d.krylov, name) == getattr(o.krylov, name), name
    assert (d.svd_policy.threshold, d.svd_policy.scale, d.svd_policy.measure, d.svd_policy.rule) == \
        (o.svd_policy.threshold, o.svd_policy.scale, o.svd_policy.measure, o.svd_policy.rule) == (1e-12, 0, 0, 0)
    assert t4a_amd._lib.t4a_gpu_tdvp_options_default(None) == t4a_amd.NULL_POINTER
    assert t4a_amd.TdvpOptions(exponent_step=complex(-0.3, 0.0)).to_c().exponent_step_re == -0.3


def test_symbols_are_exported():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("tdvp_options_default", "tdvp_check_shapes", "tdvp_plan", "tdvp", "krylov_expm_dense", "krylov_orth", "krylov_dots_route",
                 "krylov_time_dots", "projected_operator_apply_one_site", "projected_operator_time_one_site"):
        assert hasattr(lib, "t4a_gpu_" + name), name
    from t4a_amd.tdvp import tdvp, tdvp_plan, _krylov_expm_dense, _krylov_orth, _apply_one_site  # noqa: F401
    assert t4a_amd.tdvp is tdvp and t4a_amd.TdvpResult is t4a_amd.tdvp_module.TdvpResult


def test_the_route_rule_is_a_function_of_the_shape():
    from t4a_amd.tdvp import _dots_route, ROUTE_SERIAL, ROUTE_WIDE
    for length in (1, 2048, 16384, 1 << 20):
        assert [_dots_route(length, nb) for nb in (1, 8, 9, 30)] == [ROUTE_SERIAL, ROUTE_SERIAL, ROUTE_WIDE, ROUTE_WIDE]


INF, NAN = float("inf"), float("nan")
def _tolerance_refusals(field, message):
    return [(field, v, message) for v in (-1e-3, NAN, INF, -INF)]


BAD_OPTIONS = ([("nsite", 3, "TDVP supports nsite=1 or nsite=2 in this version, got nsite=3"),
                ("nsite", 0, "TDVP supports nsite=1 or nsite=2 in this version, got nsite=0"),
                ("nsite", 1, "one-site TDVP (nsite=1) is not implemented here"),
                ("nsweeps", 0, "invalid TDVP option nsweeps: must be greater than zero"),
                ("order", 3, "TDVP applyexp order 3 is not supported; supported orders are 1, 2, and 4"),
                ("order", 0, "TDVP applyexp order 0 is not supported; supported orders are 1, 2, and 4"),
                ("exponent_step_re", NAN, "invalid TDVP option exponent_step: real and imaginary parts must be finite"),
                ("exponent_step_re", INF, "invalid TDVP option exponent_step: real and imaginary parts must be finite"),
                ("exponent_step_im", NAN, "invalid TDVP option exponent_step: real and imaginary parts must be finite"),
                ("exponent_step_im", -0.1, "real-time evolution (a non-zero imaginary part) needs complex tensor trains, which this project does not have"),
                ("max_bond_dim", 0, "invalid TDVP option max_bond_dim: must be greater than zero when set"),
                ("krylov.max_iter", 0, "hermitian_krylov_expm_multiply: max_iter must be greater than zero"),
                ("krylov.max_iter", 8192, "max_iter above 8191 is not supported"),
                ("krylov.max_time_splits", 0, "hermitian_krylov_expm_multiply: max_time_splits must be greater than zero")]
               + _tolerance_refusals("krylov.tol", "hermitian_krylov_expm_multiply: tol must be finite and non-negative")
               + _tolerance_refusals("krylov.breakdown_tol", "hermitian_krylov_expm_multiply: breakdown_tol must be finite and non-negative")
               + _tolerance_refusals("krylov.hermitian_tol", "hermitian_krylov_expm_multiply: hermitian_tol must be finite and non-negative"))


# Two violations at once: the message of the rule that comes first in the validator wins.  The order of tdvp: nsite outside {1, 2},
# nsweeps, order, the exponent finite, max_bond_dim == 0, nsite == 1, the exponent real, the Krylov options (max_iter, max_time_splits,
# tol, breakdown_tol, hermitian_tol), the SVD policy.  Every adjacent pair, the pairs tdvp_one_site orders the other way round (the real
# exponent against max_bond_dim == 0, the Krylov options against the SVD policy) and both nsite rules against every other rule.
_R = {"nsite3": (("nsite", 3), "TDVP supports nsite=1 or nsite=2 in this version, got nsite=3"),
      "nsweeps": (("nsweeps", 0), "invalid TDVP option nsweeps: must be greater than zero"),
      "order": (("order", 3), "TDVP applyexp order 3 is not supported; supported orders are 1, 2, and 4"),
      "finite": (("exponent_step_re", NAN), "invalid TDVP option exponent_step: real and imaginary parts must be finite"),
      "bond0": (("max_bond_dim", 0), "invalid TDVP option max_bond_dim: must be greater than zero when set"),
      "nsite1": (("nsite", 1), "tdvp: one-site TDVP (nsite=1) is not implemented here"),
      "real": (("exponent_step_im", -0.1), "tdvp: exponent_step must be real here"),
      "max_iter": (("krylov.max_iter", 0), "hermitian_krylov_expm_multiply: max_iter must be greater than zero"),
      "splits": (("krylov.max_time_splits", 0), "hermitian_krylov_expm_multiply: max_time_splits must be greater than zero"),
      "tol": (("krylov.tol", NAN), "hermitian_krylov_expm_multiply: tol must be finite and non-negative"),
      "breakdown": (("krylov.breakdown_tol", -1.0), "hermitian_krylov_expm_multiply: breakdown_tol must be finite and non-negative"),
      "hermitian": (("krylov.hermitian_tol", INF), "hermitian_krylov_expm_multiply: hermitian_tol must be finite and non-negative"),
      "policy": (("svd_policy.threshold", NAN), "Invalid SVD truncation threshold: threshold must be finite and non-negative")}
_ORDER = ["nsite3", "nsweeps", "order", "finite", "bond0", "nsite1", "real", "max_iter", "splits", "tol", "breakdown", "hermitian", "policy"]
# (the winner, the loser)
BAD_PAIRS = (list(zip(_ORDER, _ORDER[1:])) + [("finite", "real"), ("bond0", "real"), ("max_iter", "policy"), ("real", "policy")]
             + [("nsite3", r) for r in _ORDER[2:] if r != "nsite1"]
             + [(r, "nsite1") for r in ("nsweeps", "order", "finite")] + [("nsite1", r) for r in _ORDER[7:]])
CASES = [([(f, v)], m) for f, v, m in BAD_OPTIONS] + [([_R[a][0], _R[b][0]], _R[a][1]) for a, b in BAD_PAIRS]
CASE_IDS = ["%s=%s" % (f, v) for f, v, _ in BAD_OPTIONS] + ["%s-beats-%s" % p for p in BAD_PAIRS]


def set_option(o, field, value):
    if field == "max_bond_dim":
        o.has_max_bond_dim = 1
    if field.startswith("svd_policy."):
        o.has_svd_policy = 1
    if "." in field:
        setattr(getattr(o, field.split(".")[0]), field.split(".")[1], value)
    else:
        setattr(o, field, value)


@pytest.mark.parametrize("settings, message", CASES, ids=CASE_IDS)
def test_bad_options_are_refused_before_an_operand_is_looked_at(settings, message):
    """The operands are NULL: an answer other than INVALID_ARGUMENT would mean they were looked at first.  With two bad options the
    message is that of the rule the validator checks first."""
    import t4a_amd
    o = t4a_amd.TdvpOptionsC()
    t4a_amd._lib.t4a_gpu_tdvp_options_default(ctypes.byref(o))
    for field, value in settings:
        set_option(o, field, value)
    h = ctypes.c_void_p()
    st = t4a_amd._lib.t4a_gpu_tdvp(None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None)
    assert st == t4a_amd.INVALID_ARGUMENT, t4a_amd.last_error_message()
    assert not h and message in t4a_amd.last_error_message()
    g = t4a_amd.GseOptionsC()
    assert t4a_amd._lib.t4a_gpu_gse_options_default(ctypes.byref(g)) == 0
    st = t4a_amd._lib.t4a_gpu_gse_tdvp(None, None, ctypes.c_size_t(0), ctypes.byref(g), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None)
    assert st == t4a_amd.INVALID_ARGUMENT and not h and message in t4a_amd.last_error_message()


def check_shapes(op, state, center=0, max_iter=30):
    import t4a_amd
    op, state = np.array(op, dtype=np.uintp).reshape(-1), np.array(state, dtype=np.uintp).reshape(-1)
    st = t4a_amd._lib.t4a_gpu_tdvp_check_shapes(t4a_amd._p(op), ctypes.c_size_t(len(op) // 4), t4a_amd._p(state), ctypes.c_size_t(len(state) // 3),
                                                ctypes.c_size_t(center), ctypes.c_size_t(max_iter))
    return st, t4a_amd.last_error_message()


def test_shape_checks_need_no_device():
    import t4a_amd
    op = [(1, 2, 2, 3), (3, 3, 3, 3), (3, 2, 2, 1)]
    tt = [(1, 2, 4), (4, 3, 4), (4, 2, 1)]
    assert check_shapes(op, tt)[0] == 0
    assert check_shapes(op, tt, center=2)[0] == 0
    bad = t4a_amd.INVALID_ARGUMENT
    st, msg = check_shapes(op, tt, center=1)  # exact at n = 3, refused all the same: one rule
    assert st == bad and "center 1 is an inner node of the chain" in msg and "site correction" in msg and "0 or 2" in msg
    st, msg = check_shapes(op[:1], [(1, 2, 1)])
    assert st == bad and "two-site TDVP requires at least one state edge" in msg
    st, msg = check_shapes(op[:2], tt)
    assert st == bad and "lengths differ" in msg
    st, msg = check_shapes([(1, 2, 3, 3)] + op[1:], tt)
    assert st == bad and "not square" in msg and "site 0" in msg
    st, msg = check_shapes(op, [(1, 2, 4), (4, 2, 4), (4, 2, 1)])
    assert st == bad and "site 1" in msg and "state" in msg
    st, msg = check_shapes(op, tt, center=3)
    assert st == bad and "TDVP center 3 is not a state node" in msg
    # W N^2 = 3 * (3 * 20000)^2 > INT_MAX at the bond (0, 1)
    big = [(1, 2, 4), (4, 3, 20000), (20000, 2, 1)]
    st, msg = check_shapes(op, big)
    assert st == bad and "INT_MAX" in msg and "(0, 1)" in msg and msg.startswith("tdvp")
    # the one-site step alone: at site 1 the environment R_2 holds chi_r W chi_r = 20000 * 8 * 20000 = 3.2e9 elements, while the bond steps
    # around it stay below INT_MAX (the largest buffer is HR of (0, 1): 1 * (2 * 20000)^2 = 1.6e9)
    st, msg = check_shapes([(1, 2, 2, 1), (1, 2, 2, 8), (8, 2, 2, 1)], [(1, 2, 2), (2, 2, 20000), (20000, 2, 1)])
    assert st == bad and "INT_MAX" in msg and "one-site step at site 1" in msg and msg.startswith("tdvp")
    st, msg = check_shapes(op, tt, max_iter=0)
    assert st == bad and "max_iter must be greater than zero" in msg
    st, msg = check_shapes(op, tt, max_iter=8192)
    assert st == bad and "max_iter above 8191" in msg


def test_null_arguments_and_python_side_checks():
    import t4a_amd
    lib = t4a_amd._lib
    o = t4a_amd.TdvpOptions().to_c()
    h = ctypes.c_void_p()
    zero, one_ = ctypes.c_size_t(0), ctypes.c_size_t(1)
    assert lib.t4a_gpu_tdvp(None, None, zero, ctypes.byref(o), None, None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_tdvp(None, None, zero, None, ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_tdvp(None, None, zero, ctypes.byref(o), ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    for kw in ({"max_bond_dim": 0}, {"nsweeps": -1}, {"svd_policy": 1e-8}, {"krylov": 30}, {"exponent_step": -0.1j}, {"exponent_step": complex(-0.1, 1e-300)}):
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.TdvpOptions(**kw).to_c()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.TdvpOptions(exponent_step=-0.1j).to_c()
    assert "complex tensor trains" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.tdvp(None, None)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    # the plan: the count alone, a buffer that is too small, refusals
    count = ctypes.c_size_t(0)
    assert lib.t4a_gpu_tdvp_plan(ctypes.c_size_t(4), zero, ctypes.c_size_t(2), ctypes.c_double(-0.1), zero, None, None, None, None, ctypes.byref(count)) == 0
    assert count.value == 10
    kinds, nodes, centers, exps = np.zeros(10, dtype=np.int32), np.zeros(20, dtype=np.uintp), np.zeros(10, dtype=np.uintp), np.zeros(10)
    p = t4a_amd._p
    assert lib.t4a_gpu_tdvp_plan(ctypes.c_size_t(4), zero, ctypes.c_size_t(2), ctypes.c_double(-0.1), ctypes.c_size_t(9), p(kinds), p(nodes), p(centers), p(exps),
                                 ctypes.byref(count)) == t4a_amd.BUFFER_TOO_SMALL
    assert lib.t4a_gpu_tdvp_plan(ctypes.c_size_t(4), zero, ctypes.c_size_t(2), ctypes.c_double(-0.1), zero, None, None, None, None, None) == t4a_amd.NULL_POINTER
    from t4a_amd.tdvp import tdvp_plan
    for args, text in (((4, 1, 2, -0.1), "inner node"), ((4, 4, 2, -0.1), "not a state node"), ((1, 0, 2, -0.1), "at least one state edge"),
                       ((4, 0, 3, -0.1), "order 3 is not supported"), ((4, 0, 2, NAN), "must be finite")):
        with pytest.raises(t4a_amd.T4aError) as e:
            tdvp_plan(*args)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and text in e.value.message
    # the test hooks: sizes and options come before the pointers and the device
    one = np.ones(1)
    v, it, conv = ctypes.c_double(0), ctypes.c_size_t(0), ctypes.c_int32(0)
    ko = t4a_amd.HermitianKrylovExpmOptions(max_iter=0).to_c()
    tau = ctypes.c_double(-0.1)
    assert lib.t4a_gpu_krylov_expm_dense(p(one), one_, p(one), tau, ctypes.byref(ko), p(one), ctypes.byref(it), ctypes.byref(v), ctypes.byref(conv),
                                         ctypes.byref(it)) == t4a_amd.INVALID_ARGUMENT
    ko = t4a_amd.HermitianKrylovExpmOptions().to_c()
    assert lib.t4a_gpu_krylov_expm_dense(p(one), zero, p(one), tau, ctypes.byref(ko), p(one), ctypes.byref(it), ctypes.byref(v), ctypes.byref(conv),
                                         ctypes.byref(it)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_krylov_expm_dense(p(one), one_, p(one), ctypes.c_double(NAN), ctypes.byref(ko), p(one), ctypes.byref(it), ctypes.byref(v),
                                         ctypes.byref(conv), ctypes.byref(it)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_krylov_expm_dense(None, one_, p(one), tau, ctypes.byref(ko), p(one), ctypes.byref(it), ctypes.byref(v), ctypes.byref(conv),
                                         ctypes.byref(it)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_krylov_orth(p(one), zero, one_, p(one), ctypes.c_int32(1), p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_krylov_orth(p(one), one_, one_, p(one), ctypes.c_int32(3), p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_krylov_orth(None, one_, one_, p(one), ctypes.c_int32(1), p(one), ctypes.byref(v)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_projected_operator_apply_one_site(None, zero, p(one), p(one), None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_krylov_time_dots(zero, one_, one_, p(np.zeros(2))) == t4a_amd.INVALID_ARGUMENT
