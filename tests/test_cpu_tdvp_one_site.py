"""One-site TDVP without a GPU: the numpy restatement (tests/tdvp_one_site_np.py) against dense exponentials — it is the yardstick of the
device tests —, the one-site plan through the C ABI against the restatement's, the counts, the route rule of the bond-centre apply, the
exported symbols, and the refusals answered on the host before an operand is looked at."""
import ctypes

import numpy as np
import pytest

import tdvp_one_site_np as t1
from tdvp_one_site_np import ONE, np_tdvp_one_site
from tdvp_np import Options, applyexp_sub_steps

NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the plan
def nodes_of(plan):
    return [nodes[0] for _, nodes, _, _ in plan]


def test_plan_literal_cases():
    tau = -0.2
    assert t1.one_site_plan(3, 0, 1, tau) == [(ONE, (2,), 2, tau), (ONE, (1,), 1, tau), (ONE, (0,), 0, tau)]
    p = t1.one_site_plan(3, 0, 2, tau)
    assert nodes_of(p) == [2, 1, 0, 0, 1, 2] and all(e == tau / 2 for _, _, _, e in p)
    assert nodes_of(t1.one_site_plan(4, 1, 1, tau)) == [0, 3, 2, 1]
    assert nodes_of(t1.one_site_plan(5, 2, 2, tau)) == [0, 1, 4, 3, 2, 2, 3, 4, 1, 0]
    assert nodes_of(t1.one_site_plan(4, 0, 1, tau)) == [3, 2, 1, 0] and nodes_of(t1.one_site_plan(4, 3, 1, tau)) == [0, 1, 2, 3]
    w = applyexp_sub_steps(4)
    p = t1.one_site_plan(5, 2, 4, tau)
    assert len(w) == 6 and abs(sum(w) - 1.0) <= 1e-14 and len(p) == 6 * 5
    for k in range(6):
        part = p[5 * k:5 * k + 5]
        assert nodes_of(part) == ([0, 1, 4, 3, 2] if k % 2 == 0 else [2, 3, 4, 1, 0])
        assert all(e == tau * w[k] for _, _, _, e in part)
    for plan in (p, t1.one_site_plan(3, 0, 2, tau)):
        assert all(kind == 2 and nodes == (nc,) for kind, nodes, nc, _ in plan)


@pytest.mark.parametrize("n, order", [(1, 1), (2, 1), (2, 2), (3, 4), (4, 2), (5, 1), (5, 2), (5, 4), (6, 4)])
def test_the_plan_of_the_library_equals_the_restatement(n, order):
    from t4a_amd.tdvp import tdvp_one_site_plan
    for center in range(n):
        for tau in (-0.05, 0.7):
            assert tdvp_one_site_plan(n, center, order, tau) == t1.one_site_plan(n, center, order, tau)  # exact floats


def test_plan_count_only_call_small_buffer_and_refusals():
    import t4a_amd
    from t4a_amd.tdvp import tdvp_one_site_plan
    lib, p = t4a_amd._lib, t4a_amd._p
    sz, dbl = ctypes.c_size_t, ctypes.c_double
    count = sz(0)
    assert lib.t4a_gpu_tdvp_one_site_plan(sz(4), sz(1), sz(2), dbl(-0.1), sz(0), None, None, None, None, ctypes.byref(count)) == 0
    assert count.value == 8
    kinds, nodes, centers, exps = np.zeros(8, dtype=np.int32), np.zeros(16, dtype=np.uintp), np.zeros(8, dtype=np.uintp), np.zeros(8)
    assert lib.t4a_gpu_tdvp_one_site_plan(sz(4), sz(1), sz(2), dbl(-0.1), sz(7), p(kinds), p(nodes), p(centers), p(exps),
                                          ctypes.byref(count)) == t4a_amd.BUFFER_TOO_SMALL
    assert lib.t4a_gpu_tdvp_one_site_plan(sz(4), sz(1), sz(2), dbl(-0.1), sz(8), p(kinds), p(nodes), p(centers), p(exps), ctypes.byref(count)) == 0
    assert list(kinds) == [2] * 8 and list(nodes[0::2]) == list(nodes[1::2]) == list(centers) == [0, 3, 2, 1, 1, 2, 3, 0]
    assert lib.t4a_gpu_tdvp_one_site_plan(sz(4), sz(1), sz(2), dbl(-0.1), sz(0), None, None, None, None, None) == t4a_amd.NULL_POINTER
    for args, text in (((4, 4, 2, -0.1), "center 4 is not a state node"), ((0, 0, 2, -0.1), "empty chain"), ((4, 0, 3, -0.1), "order 3 is not supported"),
                       ((4, 0, 2, NAN), "must be finite")):
        with pytest.raises(t4a_amd.T4aError) as e:
            tdvp_one_site_plan(*args)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and text in e.value.message


# ------------------------------------------------------------------------------------------------ the restatement
FULL = [((2,) * 4, (1, 2, 4, 2, 1)), ((2,) * 5, (1, 2, 4, 4, 2, 1))]


@pytest.mark.parametrize("order", (1, 2, 4))
@pytest.mark.parametrize("dims, bonds", FULL, ids=["n4", "n5"])
def test_full_bond_sweeps_reproduce_the_dense_exponential_from_every_centre(dims, bonds, order):
    """At full bonds the one-site splitting is exact: every centre, exact local exponentials, relative error <= 1e-13 against
    expm(tau H) psi (measured: at most 1.2e-14).  tau = -1 / (2 ||H||_2): see tdvp_one_site_np.case_tau."""
    ops, init = t1.bonds_case(dims, bonds)
    h = t1.np_operator_full(ops)
    assert np.array_equal(h, h.T) and np.array_equal(h, np.round(h))
    tau = t1.case_tau(ops)
    want = t1.dense_exponential(ops, init, tau)
    n, w = len(dims), len(applyexp_sub_steps(order))
    for center in range(n):
        r = np_tdvp_one_site(ops, init, center, Options(order=order, exponent_step=tau), exact_local=True)
        err = t1.relative_distance(t1.np_state_full(r["state"]), want)
        print(n, center, order, "relative error", err)
        assert err <= 1e-13
        assert [t.shape for t in r["state"]] == [t.shape for t in t1.np_canonicalize(init, center)]
        assert (r["local_updates"], r["one_site_steps"], r["bond_corrections"]) == (w * (2 * n - 1), w * n, w * (n - 1))


def test_the_literal_jump_of_a_reversed_substep_is_not_a_splitting():
    """Why the reversed substeps correct the last edge of the path: with the reference's first edge a second-order sweep from an inner
    centre is percents away from the dense exponential at full bonds, from an end (no jump) the two rules are the same computation."""
    ops, init = t1.bonds_case(*FULL[1])
    tau = t1.case_tau(ops)
    want = t1.dense_exponential(ops, init, tau)
    o = Options(order=2, exponent_step=tau)
    inner = np_tdvp_one_site(ops, init, 2, o, exact_local=True, literal_jump=True)
    assert t1.relative_distance(t1.np_state_full(inner["state"]), want) >= 1e-3
    for center in (0, 4):
        a = np_tdvp_one_site(ops, init, center, o, exact_local=True, literal_jump=True)
        b = np_tdvp_one_site(ops, init, center, o, exact_local=True)
        assert all(np.array_equal(s, t) for s, t in zip(a["state"], b["state"]))


@pytest.mark.parametrize("center, nsweeps, order", [(0, 1, 1), (4, 2, 2), (2, 1, 4), (1, 3, 2)])
def test_counts_of_the_krylov_restatement(center, nsweeps, order):
    ops, init = t1.thin_case()
    n, w = len(ops), len(applyexp_sub_steps(order))
    r = np_tdvp_one_site(ops, init, center, Options(nsweeps=nsweeps, order=order, exponent_step=t1.TAU))
    assert r["sweeps_completed"] == nsweeps and r["local_updates"] == nsweeps * w * (2 * n - 1)
    assert r["one_site_steps"] == nsweeps * w * n and r["bond_corrections"] == nsweeps * w * (n - 1)
    assert [t.shape for t in r["state"]] == [t.shape for t in t1.np_canonicalize(init, center)]
    exact = np_tdvp_one_site(ops, init, center, Options(nsweeps=nsweeps, order=order, exponent_step=t1.TAU), exact_local=True)
    assert t1.relative_distance(t1.np_state_full(r["state"]), t1.np_state_full(exact["state"])) <= 1e-10


def test_thin_bonds_halving_the_step_reduces_the_error():
    """Bonds below full: the state leaves the manifold and the projection error, first order in tau over a fixed time, dominates; the
    two-site CPU test has no order check to mirror, so only the monotone decrease of the error of one step is asserted."""
    ops, init = t1.thin_case()
    for center in (0, 2):
        errs = []
        for tau in (-0.2, -0.1, -0.05):
            r = np_tdvp_one_site(ops, init, center, Options(order=2, exponent_step=tau), exact_local=True)
            errs.append(t1.relative_distance(t1.np_state_full(r["state"]), t1.dense_exponential(ops, init, tau)))
        print(center, errs)
        assert errs[0] > errs[1] > errs[2] > 0.0


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_symbols_are_exported_and_the_default_options_have_one_site():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("tdvp_one_site_options_default", "tdvp_one_site_check_shapes", "tdvp_one_site_plan", "tdvp_one_site", "gse_tdvp_one_site",
                 "tdvp_bond_apply", "tdvp_bond_apply_route", "tdvp_bond_apply_time", "tdvp_bond_apply_fused_admits", "tdvp_set_bond_apply_route",
                 "projected_operator_bond_center_env"):
        assert hasattr(lib, "t4a_gpu_" + name), name
    from t4a_amd.tdvp import tdvp_one_site, tdvp_one_site_plan, _apply_bond_center, _bond_apply_route  # noqa: F401
    from t4a_amd.gse import gse_tdvp_one_site
    assert t4a_amd.tdvp_one_site is tdvp_one_site and t4a_amd.tdvp_one_site_plan is tdvp_one_site_plan and t4a_amd.gse_tdvp_one_site is gse_tdvp_one_site
    o, d = t4a_amd.TdvpOptionsC(), t4a_amd.TdvpOptionsC()
    assert t4a_amd._lib.t4a_gpu_tdvp_one_site_options_default(ctypes.byref(o)) == 0 and t4a_amd._lib.t4a_gpu_tdvp_options_default(ctypes.byref(d)) == 0
    assert (o.nsite, d.nsite) == (1, 2)
    for name in ("nsweeps", "order", "exponent_step_re", "exponent_step_im", "has_max_bond_dim", "has_svd_policy"):
        assert getattr(o, name) == getattr(d, name)
    assert t4a_amd._lib.t4a_gpu_tdvp_one_site_options_default(None) == t4a_amd.NULL_POINTER


def test_the_route_rule_is_a_function_of_the_shape():
    from t4a_amd.tdvp import _bond_apply_route, _bond_apply_fused_admits, BOND_FUSED, BOND_GEMM
    shapes = [(ka, kb, w) for ka in (1, 3, 16, 17, 64, 65, 256) for kb in (1, 5, 16, 33, 128, 129, 513) for w in (1, 3, 4, 16)]
    first = [_bond_apply_route(*s) for s in shapes]
    assert first == [_bond_apply_route(*s) for s in shapes] and set(first) <= {BOND_FUSED, BOND_GEMM}
    for (ka, kb, w), r in zip(shapes, first):
        assert _bond_apply_fused_admits(ka, kb, w) == (w * kb <= 512)
        if r == BOND_FUSED:
            assert _bond_apply_fused_admits(ka, kb, w)
    # just outside the envelope: the GEMM route
    assert _bond_apply_route(16, 128, 4) in (BOND_FUSED, BOND_GEMM) and _bond_apply_route(16, 129, 4) == BOND_GEMM and _bond_apply_route(16, 171, 3) == BOND_GEMM


def one_site_options():
    import t4a_amd
    o = t4a_amd.TdvpOptionsC()
    assert t4a_amd._lib.t4a_gpu_tdvp_one_site_options_default(ctypes.byref(o)) == 0
    return o


BAD_OPTIONS = [("nsite", 2, "tdvp_one_site: one-site TDVP requires nsite=1, got nsite=2; nsite=2 is tdvp"),
               ("nsite", 0, "one-site TDVP requires nsite=1, got nsite=0"),
               ("nsweeps", 0, "invalid TDVP option nsweeps: must be greater than zero"),
               ("order", 3, "TDVP applyexp order 3 is not supported; supported orders are 1, 2, and 4"),
               ("exponent_step_re", NAN, "invalid TDVP option exponent_step: real and imaginary parts must be finite"),
               ("exponent_step_im", -0.1, "real-time evolution (a non-zero imaginary part) needs complex tensor trains"),
               ("max_bond_dim", 0, "invalid TDVP option max_bond_dim: must be greater than zero when set"),
               ("max_bond_dim", 8, "invalid TDVP option max_bond_dim: one-site TDVP has fixed ranks; use nsite=2 for truncation"),
               ("has_svd_policy", 1, "invalid TDVP option svd_policy: one-site TDVP has fixed ranks; use nsite=2 for truncation"),
               ("krylov.max_iter", 0, "hermitian_krylov_expm_multiply: max_iter must be greater than zero"),
               ("krylov.max_iter", 8192, "max_iter above 8191 is not supported"),
               ("krylov.max_time_splits", 0, "hermitian_krylov_expm_multiply: max_time_splits must be greater than zero"),
               ("krylov.tol", -1e-3, "hermitian_krylov_expm_multiply: tol must be finite and non-negative")]


# Two violations at once: the message of the rule that comes first in the validator wins.  The order of tdvp_one_site: nsite != 1,
# nsweeps, order, the exponent finite, the exponent real, max_bond_dim == 0, max_bond_dim set, svd_policy set, the Krylov options
# (max_iter, max_time_splits, tol, breakdown_tol, hermitian_tol).  Every adjacent pair, the pairs tdvp orders the other way round (the real
# exponent against max_bond_dim == 0, the SVD policy against the Krylov options) and the nsite rule against every other rule.
_R = {"nsite": (("nsite", 2), "tdvp_one_site: one-site TDVP requires nsite=1, got nsite=2; nsite=2 is tdvp"),
      "nsweeps": (("nsweeps", 0), "invalid TDVP option nsweeps: must be greater than zero"),
      "order": (("order", 3), "TDVP applyexp order 3 is not supported; supported orders are 1, 2, and 4"),
      "finite": (("exponent_step_re", NAN), "invalid TDVP option exponent_step: real and imaginary parts must be finite"),
      "real": (("exponent_step_im", -0.1), "tdvp_one_site: exponent_step must be real here"),
      "bond0": (("max_bond_dim", 0), "invalid TDVP option max_bond_dim: must be greater than zero when set"),
      "bond": (("max_bond_dim", 8), "invalid TDVP option max_bond_dim: one-site TDVP has fixed ranks; use nsite=2 for truncation"),
      "policy": (("has_svd_policy", 1), "invalid TDVP option svd_policy: one-site TDVP has fixed ranks; use nsite=2 for truncation"),
      "max_iter": (("krylov.max_iter", 0), "hermitian_krylov_expm_multiply: max_iter must be greater than zero"),
      "splits": (("krylov.max_time_splits", 0), "hermitian_krylov_expm_multiply: max_time_splits must be greater than zero"),
      "tol": (("krylov.tol", NAN), "hermitian_krylov_expm_multiply: tol must be finite and non-negative"),
      "breakdown": (("krylov.breakdown_tol", -1.0), "hermitian_krylov_expm_multiply: breakdown_tol must be finite and non-negative"),
      "hermitian": (("krylov.hermitian_tol", float("inf")), "hermitian_krylov_expm_multiply: hermitian_tol must be finite and non-negative")}
_ORDER = ["nsite", "nsweeps", "order", "finite", "real", "bond0", "bond", "policy", "max_iter", "splits", "tol", "breakdown", "hermitian"]
# (the winner, the loser); bond0 and bond set the same field, so bond0 meets its next neighbour, policy
BAD_PAIRS = ([(a, b) for a, b in zip(_ORDER, _ORDER[1:]) if (a, b) != ("bond0", "bond")] + [("bond0", "policy"), ("real", "bond"), ("finite", "bond0")]
             + [("nsite", r) for r in _ORDER[2:]])
CASES = [([(f, v)], m) for f, v, m in BAD_OPTIONS] + [([_R[a][0], _R[b][0]], _R[a][1]) for a, b in BAD_PAIRS]
CASE_IDS = ["%s=%s" % (f, v) for f, v, _ in BAD_OPTIONS] + ["%s-beats-%s" % p for p in BAD_PAIRS]


@pytest.mark.parametrize("settings, message", CASES, ids=CASE_IDS)
def test_bad_options_are_refused_before_an_operand_is_looked_at(settings, message):
    """The operands are NULL: an answer other than INVALID_ARGUMENT would mean they were looked at first.  With two bad options the
    message is that of the rule the validator checks first."""
    import t4a_amd
    o = one_site_options()
    for field, value in settings:
        if field == "max_bond_dim":
            o.has_max_bond_dim = 1
        if field.startswith("krylov."):
            setattr(o.krylov, field.split(".")[1], value)
        else:
            setattr(o, field, value)
    h = ctypes.c_void_p()
    st = t4a_amd._lib.t4a_gpu_tdvp_one_site(None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None)
    assert st == t4a_amd.INVALID_ARGUMENT, t4a_amd.last_error_message()
    assert not h and message in t4a_amd.last_error_message()
    g = t4a_amd.GseOptionsC()
    assert t4a_amd._lib.t4a_gpu_gse_options_default(ctypes.byref(g)) == 0
    st = t4a_amd._lib.t4a_gpu_gse_tdvp_one_site(None, None, ctypes.c_size_t(0), ctypes.byref(g), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None)
    assert st == t4a_amd.INVALID_ARGUMENT and not h and message in t4a_amd.last_error_message()


def test_good_options_reach_the_null_operands():
    import t4a_amd
    o, h = one_site_options(), ctypes.c_void_p()
    assert t4a_amd._lib.t4a_gpu_tdvp_one_site(None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert t4a_amd._lib.t4a_gpu_tdvp_one_site(None, None, ctypes.c_size_t(0), None, ctypes.byref(h), None, None, None, None, None) == t4a_amd.NULL_POINTER
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.tdvp_one_site(None, None)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT


def check_shapes(op, state, center=0, max_iter=30):
    import t4a_amd
    op, state = np.array(op, dtype=np.uintp).reshape(-1), np.array(state, dtype=np.uintp).reshape(-1)
    st = t4a_amd._lib.t4a_gpu_tdvp_one_site_check_shapes(t4a_amd._p(op), ctypes.c_size_t(len(op) // 4), t4a_amd._p(state), ctypes.c_size_t(len(state) // 3),
                                                         ctypes.c_size_t(center), ctypes.c_size_t(max_iter))
    return st, t4a_amd.last_error_message()


def test_shape_checks_need_no_device():
    import t4a_amd
    op = [(1, 2, 2, 3), (3, 3, 3, 3), (3, 2, 2, 1)]
    tt = [(1, 2, 4), (4, 3, 4), (4, 2, 1)]
    for center in (0, 1, 2):  # any centre
        assert check_shapes(op, tt, center)[0] == 0
    bad = t4a_amd.INVALID_ARGUMENT
    st, msg = check_shapes(op, tt, center=3)
    assert st == bad and "TDVP center 3 is not a state node" in msg and msg.startswith("tdvp_one_site")
    st, msg = check_shapes(op[:1], [(1, 2, 1)])
    assert st == bad and "a single site" in msg and "at least two sites" in msg
    st, msg = check_shapes(op[:2], tt)
    assert st == bad and "lengths differ" in msg
    st, msg = check_shapes([(1, 2, 3, 3)] + op[1:], tt)
    assert st == bad and "not square" in msg and "site 0" in msg
    st, msg = check_shapes(op, [(1, 2, 4), (4, 2, 4), (4, 2, 1)])
    assert st == bad and "site 1" in msg and "state" in msg
    # the one-site step at site 1: R_2 holds 20000 * 8 * 20000 elements
    st, msg = check_shapes([(1, 2, 2, 1), (1, 2, 2, 8), (8, 2, 2, 1)], [(1, 2, 2), (2, 2, 20000), (20000, 2, 1)])
    assert st == bad and "INT_MAX" in msg and "one-site step at site 1" in msg and msg.startswith("tdvp_one_site")
    # the bond-centre step alone: the basis of 31 columns of 9000 * 9000 elements at the bond (1, 2); every site step stays below
    st, msg = check_shapes([(1, 2, 2, 1)] * 3, [(1, 2, 2), (2, 2, 9000), (9000, 2, 1)], max_iter=30)
    assert st == bad and "INT_MAX" in msg and "bond-centre step at the bond (1, 2)" in msg
    st, msg = check_shapes(op, tt, max_iter=0)
    assert st == bad and "max_iter must be greater than zero" in msg


def test_hooks_check_their_arguments_before_the_device():
    import t4a_amd
    lib, p = t4a_amd._lib, t4a_amd._p
    sz, one = ctypes.c_size_t, np.ones(1)
    r = ctypes.c_int32(0)
    assert lib.t4a_gpu_tdvp_bond_apply(p(one), p(one), p(one), sz(0), sz(1), sz(1), ctypes.c_int32(2), p(one), None) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_tdvp_bond_apply(p(one), p(one), p(one), sz(1), sz(1), sz(1), ctypes.c_int32(3), p(one), None) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_tdvp_bond_apply(p(one), p(one), p(one), sz(16), sz(129), sz(4), ctypes.c_int32(0), p(one), None) == t4a_amd.INVALID_ARGUMENT
    assert "W k_b must be at most 512" in t4a_amd.last_error_message()
    assert lib.t4a_gpu_tdvp_bond_apply(None, p(one), p(one), sz(1), sz(1), sz(1), ctypes.c_int32(2), p(one), None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_tdvp_bond_apply_route(sz(0), sz(1), sz(1), ctypes.byref(r)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_tdvp_bond_apply_route(sz(1), sz(1), sz(1), None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_tdvp_bond_apply_time(sz(0), sz(1), sz(1), sz(1), p(np.zeros(2))) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_projected_operator_bond_center_env(None, sz(0), ctypes.c_int32(1), p(np.zeros(3, dtype=np.uintp)), None) == t4a_amd.NULL_POINTER
