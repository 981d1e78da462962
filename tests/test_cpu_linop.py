"""apply_linear_operator without a GPU: the plan and the kind of every site (against the numpy restatement, tests/apply_np.py), every
refusal that is answered on the host and its message, are_exclusive_operators, the mapping of ApplyOptions onto the options of the MPO
contraction, the route table, the restatement against the dense reference (identities (x) O) x, and the gap condition on the operand
sets of the GPU driver tests."""
import ctypes

import numpy as np
import pytest

import apply_np as A

OP2 = [(1, 2, 2, 2), (2, 2, 2, 3), (3, 2, 2, 2), (2, 2, 2, 1)]


def state_dims(n, d=2, bond=3):
    b = [1] + [bond] * (n - 1) + [1]
    return [(b[i], d, b[i + 1]) for i in range(n)]


PLANS = {
    "full": (OP2, (0, 1, 2, 3), state_dims(4), ["op"] * 4),
    "k1_first": ([(1, 2, 2, 1)], (0,), state_dims(4), ["op", "outside", "outside", "outside"]),
    "k1_inner": ([(1, 2, 2, 1)], (2,), state_dims(4), ["outside", "outside", "op", "outside"]),
    "k1_last": ([(1, 2, 2, 1)], (3,), state_dims(4), ["outside", "outside", "outside", "op"]),
    "inner_block": (OP2[:1] + [(2, 2, 2, 1)], (2, 3), state_dims(6), ["outside", "outside", "op", "op", "outside", "outside"]),
    "interleaved": (OP2, (0, 2, 4, 6), state_dims(8), ["op", "bridge", "op", "bridge", "op", "bridge", "op", "outside"]),
    "n1": ([(1, 3, 2, 1)], (0,), [(1, 2, 1)], ["op"]),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_and_kinds(name):
    import t4a_amd
    od, sites, sd, kinds = PLANS[name]
    got = t4a_amd.apply_plan(od, sites, sd)
    assert got["kinds"] == kinds
    assert got == A.np_plan(od, sites, sd)
    # the pass-through bond of a bridge is the operator bond between its neighbours, outside it is 1
    for i, k in enumerate(kinds):
        if k == "outside":
            assert got["bonds"][i] == (1, 1) and got["result_dims"][i] == tuple(sd[i])
        if k == "bridge":
            j = sum(s < i for s in sites)
            assert got["bonds"][i] == (od[j][0], od[j][0]) and got["result_dims"][i] == (od[j][0] * sd[i][0], sd[i][1], od[j][0] * sd[i][2])
    if name == "n1":
        assert got["result_dims"] == [(1, 3, 1)]
    if name == "interleaved":
        assert got["bonds"] == [(1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1)]


REFUSALS = [
    (OP2, (0, 2, 2, 6), state_dims(8), "sites must be strictly ascending"),
    (OP2, (0, 4, 2, 6), state_dims(8), "sites must be strictly ascending"),
    (OP2, (0, 2, 4), state_dims(8), "the operator has 4 sites, `sites` names 3 positions"),
    (OP2, (0, 2, 4, 8), state_dims(8), "Operator nodes [0, 2, 4, 8] are not a subset of state nodes [0, 1, 2, 3, 4, 5, 6, 7]"),
    ([(1, 2, 3, 1)], (1,), state_dims(3), "Shared shape mismatch at site 1: operator has input dim 3, the state has site dim 2"),
    ([(1, 2, 2, 300), (300, 2, 2, 1)], (0, 2), state_dims(3, bond=300), "site 0: the fused bond 300 * 300 is above 65535"),
    ([(1, 2, 2, 1)], (1,), [(1, 2, 60000), (60000, 2, 60000), (60000, 2, 1)], "holds more than INT_MAX elements"),
    ([], (), state_dims(3), "the operator has no sites"),
]


@pytest.mark.parametrize("od,sites,sd,msg", REFUSALS)
def test_every_refusal_happens_on_the_host_with_its_message(od, sites, sd, msg):
    import t4a_amd
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.apply_plan(od, sites, sd)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and msg in e.value.message, e.value.message
    if "INT_MAX" not in msg:  # (the restatement states the result's core only)
        with pytest.raises(A.PlanError) as r:
            A.np_plan(od, sites, sd)
        assert msg in str(r.value)


def test_the_bridge_bond_of_site_1_is_refused_too():
    """the refusal names the first site that fails: site 0's right bond 300 * 200 = 60000 passes, the bridge's 300 * 250 does not"""
    import t4a_amd
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.apply_plan([(1, 2, 2, 300), (300, 2, 2, 1)], (0, 2), [(1, 2, 200), (200, 2, 250), (250, 2, 1)])
    assert "site 1: the fused bond 300 * 250 is above 65535" in e.value.message


EXCLUSIVE = [
    (6, [(0, 1), (3, 4)], True),
    (6, [(0, 1, 2), (3,), (4, 5)], True),
    (6, [(3, 4), (0, 1)], True),
    (6, [], True),
    (6, [(0, 1), (1, 2)], False),      # overlapping
    (6, [(0, 2)], False),              # not contiguous: not a connected subtree
    (6, [(0, 3), (1, 2)], False),      # a third operator on the path between two sites of another
    (6, [(0, 1), (4, 6)], False),      # not a node of the target
    (6, [(0, 1), ()], False),
    (6, [(2, 2)], False),
]


@pytest.mark.parametrize("n,supports,want", EXCLUSIVE)
def test_are_exclusive_operators(n, supports, want):
    import t4a_amd
    assert t4a_amd.are_exclusive_operators(n, supports) is want


def test_options_mapping():
    import t4a_amd
    from t4a_amd import ApplyOptions, SvdTruncationPolicy
    o = t4a_amd.ApplyOptionsC()
    assert t4a_amd._lib.t4a_gpu_linop_options_default(ctypes.byref(o)) == 0
    # ApplyOptions::default(): zip-up, no cap, no policy (the project's 1e-12), one sweep, no convergence tolerance
    assert (o.method, o.tolerance, o.has_max_bond_dim, o.nfullsweeps, o.has_convergence_tol) == (1, 1e-12, 0, 1, 0)
    d = ApplyOptions().to_c()
    for name, _ in t4a_amd.ApplyOptionsC._fields_:
        assert getattr(d, name) == getattr(o, name), name
    assert t4a_amd._lib.t4a_gpu_linop_options_default(None) == t4a_amd.NULL_POINTER
    assert (ApplyOptions.zipup().method, ApplyOptions.fit().method, ApplyOptions.naive().method) == (1, 2, 0)
    c = ApplyOptions.fit().with_nfullsweeps(3).with_max_bond_dim(20).with_svd_policy(SvdTruncationPolicy(1e-5)).with_qr_rtol(1e-9) \
        .with_convergence_tol(1e-7).to_c()
    assert (c.method, c.nfullsweeps, c.has_max_bond_dim, c.max_bond_dim, c.tolerance, c.has_convergence_tol, c.convergence_tol) == \
        (2, 3, 1, 20, 1e-5, 1, 1e-7)
    base = ApplyOptions.fit()
    assert base.with_nfullsweeps(5).nfullsweeps == 5 and base.nfullsweeps == 1  # builders return copies
    for pol in (SvdTruncationPolicy(1e-5, scale=t4a_amd.ABSOLUTE), SvdTruncationPolicy(1e-5, measure=t4a_amd.SQUARED_VALUE),
                SvdTruncationPolicy(1e-5, rule=t4a_amd.DISCARDED_TAIL_SUM)):
        with pytest.raises(t4a_amd.T4aError) as e:
            ApplyOptions().with_svd_policy(pol).to_c()
        assert e.value.code == t4a_amd.NOT_IMPLEMENTED and "SvdTruncationPolicy(" in e.value.message
    assert "scale=Absolute" in pytest.raises(t4a_amd.T4aError, ApplyOptions().with_svd_policy(
        SvdTruncationPolicy(1e-5, scale=t4a_amd.ABSOLUTE)).to_c).value.message
    for bad in (ApplyOptions().with_qr_rtol(-1.0), ApplyOptions().with_qr_rtol(float("nan")), ApplyOptions().with_convergence_tol(-1e-3),
                ApplyOptions().with_convergence_tol(float("inf")), ApplyOptions().with_svd_policy(SvdTruncationPolicy(-1.0)),
                ApplyOptions().with_svd_policy(SvdTruncationPolicy(float("nan"))), ApplyOptions().with_max_bond_dim(0),
                ApplyOptions().with_nfullsweeps(-1), ApplyOptions(method=7), ApplyOptions().with_svd_policy("default")):
        with pytest.raises(t4a_amd.T4aError) as e:
            bad.to_c()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT


def test_the_c_entry_point_checks_options_and_route_before_the_operands():
    import t4a_amd
    lib = t4a_amd._lib
    out = ctypes.c_void_p()
    for field, value in (("tolerance", -1.0), ("tolerance", float("nan")), ("convergence_tol", -1.0), ("method", 3), ("max_bond_dim", 0)):
        o = t4a_amd.ApplyOptions.fit().with_max_bond_dim(4).with_convergence_tol(1e-3).to_c()
        setattr(o, field, value)
        assert lib.t4a_gpu_linop_apply(None, None, 0, None, ctypes.byref(o), 0, None, ctypes.byref(out), None, None, None) == t4a_amd.INVALID_ARGUMENT
    o = t4a_amd.ApplyOptions().to_c()
    assert lib.t4a_gpu_linop_apply(None, None, 0, None, ctypes.byref(o), 5, None, ctypes.byref(out), None, None, None) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_linop_apply(None, None, 0, None, ctypes.byref(o), 0, None, ctypes.byref(out), None, None, None) == t4a_amd.NULL_POINTER


def test_symbols_and_exports():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("t4a_gpu_linop_options_default", "t4a_gpu_linop_plan", "t4a_gpu_linop_apply", "t4a_gpu_linop_extend", "t4a_gpu_linop_exclusive",
                 "t4a_gpu_linop_compose", "t4a_gpu_linop_gap_half", "t4a_gpu_linop_route", "t4a_gpu_linop_time_half"):
        assert hasattr(lib, name), name
    for name in ("LinearOperator", "ApplyOptions", "apply_linear_operator", "apply_plan", "apply_route", "extend_operator_to_full_space",
                 "are_exclusive_operators", "compose_exclusive_linear_operators"):
        assert getattr(t4a_amd, name) is getattr(t4a_amd.linop, name)


def test_route_table():
    """auto takes fused exactly where the probe measured it faster by more than the spread (DESIGN.md section 8,
    profiles/linop_probe.json) and composed everywhere else, unmeasured sizes included"""
    import json
    import os
    import t4a_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "linop_probe.json")) as f:
        probe = json.load(f)
    for row in probe["drivers"]:
        want = "fused" if row["fused_wins"] else "composed"
        assert t4a_amd.apply_route(row["method"], row["n_sites"], row["n_gap_sites"], row["state_bond"], row["op_bond"]) == want, row
    for method in (0, 1, 2):
        # never measured: naive, no gap site, sizes outside the table
        assert t4a_amd.apply_route(0, 16, 8, 64, 2) == "composed"
        assert t4a_amd.apply_route(method, 16, 0, 64, 2) == "composed"
        assert t4a_amd.apply_route(method, 16, 8, 4096, 2) == "composed"
        assert t4a_amd.apply_route(method, 16, 8, 3, 2) == "composed"
        assert t4a_amd.apply_route(method, 16, 8, 64, 64) == "composed"
        assert t4a_amd.apply_route(method, 4000, 2000, 64, 2) == "composed"
    with pytest.raises(t4a_amd.T4aError):
        t4a_amd.apply_route(3, 16, 8, 64, 2)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", sorted(A.CASES))
def test_restatement_against_the_dense_reference(name):
    op, sites, x, cap = A.case_operands(name)
    want = A.np_dense_apply(op, sites, x)
    scale = np.linalg.norm(want)
    plan = A.np_plan([t.shape for t in op], sites, [c.shape for c in x])
    naive = A.np_naive(op, sites, x)
    assert [c.shape for c in naive] == plan["result_dims"]
    assert np.linalg.norm(A.np_dense_state(naive) - want) <= 1e-13 * scale
    o = A.options_for(None)
    assert np.linalg.norm(A.np_dense_state(A.np_zipup(op, sites, x, o)) - want) <= 1e-8 * scale  # tolerance 1e-9 per cut
    fit, info = A.np_fit(op, sites, x, o)
    assert np.linalg.norm(A.np_dense_state(fit) - want) <= 1e-8 * scale
    assert info["n_sweeps"] == (2 if len(x) > 1 else 0)
    capped = A.np_zipup(op, sites, x, A.options_for(cap))
    assert max(A.links([c[:, :, None, :] for c in capped])) <= cap < max(c.shape[2] for c in naive)


def test_the_dense_reference_is_the_operator_on_its_sites_only():
    """k = 1 on site 2 of four: the reference is a matrix product along axis 2"""
    op, sites, x, _ = A.case_operands("k1")
    psi = A.np_dense_state(x)
    want = np.einsum("yx,abxd->abyd", op[0][0, :, :, 0], psi)
    assert np.allclose(A.np_dense_apply(op, sites, x), want, rtol=0, atol=1e-15)


def test_extend_restated():
    op, sites, x, _ = A.case_operands("interleaved")
    full = A.np_extend(op, sites, [c.shape[1] for c in x])
    assert [t.shape for t in full] == [(1, 2, 2, 2), (2, 2, 2, 2), (2, 2, 2, 2), (2, 2, 2, 2), (2, 2, 2, 2), (2, 2, 2, 2), (2, 2, 2, 1), (1, 2, 2, 1)]
    assert np.array_equal(full[1], np.einsum("ab,yx->ayxb", np.eye(2), np.eye(2))) and np.array_equal(full[7][0, :, :, 0], np.eye(2))


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_gap_condition_of_the_gpu_driver_cases(name):
    """at every SVD of the restatement no singular value lies within a factor 1e3 of tolerance * s_max, and a cap never cuts between
    two values closer than one per cent: the ranks of a correct device run are determined"""
    op, sites, x, cap = A.case_operands(name)
    for c in (None, cap):
        o = A.options_for(c)
        _, log = A.record(lambda: A.np_zipup(op, sites, x, o))
        assert log.splits or len(x) == 1
        assert not A.gap_violations(log), (name, c, "zipup", A.gap_violations(log))
        _, log = A.record(lambda: A.np_fit(op, sites, x, o))
        assert not A.gap_violations(log), (name, c, "fit", A.gap_violations(log))


def test_gap_condition_and_stop_test_of_the_fit_from_an_initial_train():
    op, sites, x, start, o = A.initial_fit_case()
    (_, info), log = A.record(lambda: A.np_fit(op, sites, x, o, initial=start))
    assert not A.gap_violations(log), A.gap_violations(log)
    # the stop test is decided far from its threshold: the device stops at the same sweep
    n = info["norms"]
    assert 1 <= info["n_sweeps"] < 6
    assert all(not (1e-4 < abs(n[i + 1] / n[i] - 1.0) < 1e-2) for i in range(len(n) - 1))
