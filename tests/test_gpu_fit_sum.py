"""fit_sum on the device against the numpy restatement (tests/fit_sum_np.py) and dense sums, on both routes (forced: `auto` would
send shapes this small one way).  From an initial with full bonds one sweep returns sum_k w_k T_k: the deviation relative to
sum_k |w_k| |T_k|_F is asserted at 1e-12 for trains and MPOs.  The truncating cases are those of fit_sum_np.CASES, whose singular
values have a relative gap of at least 1e-6 at every cut (tests/test_cpu_fit_sum.py), so the device's Jacobi SVD and LAPACK keep the
same ranks; their dense results are compared with the restatement's at ten times the deviation measured on an MI355X (MEASURED, and
DESIGN.md §8 "Variational sum")."""
import ctypes
import functools

import numpy as np
import pytest

import t4a_amd
from t4a_amd import SimpleTensorTrain, MPO, FitSumOptions, SvdTruncationPolicy, fit_sum
import fit_sum_np as F

pytestmark = pytest.mark.gpu

ROUTES = ("fused", "gemm")
# the device's deviation from the restatement relative to sum_k |w_k| |T_k|_F, measured on an MI355X (the larger of the two routes);
# a test asserts ten times its figure
MEASURED = {"cap": 9.3e-16, "policy": 9.3e-16, "stop": 7.8e-16, "k40": 3.1e-15, "fixed": 1.5e-15, "none": 1.2e-15}


def tt(tensors):
    return SimpleTensorTrain(tensors)


def dense(state):
    ts = state.site_tensors()
    if ts[0].ndim == 4:
        ts = F.fuse(ts)
    return F.np_full(ts)


def options(o):
    pol = None if o.svd_policy is None else SvdTruncationPolicy(*o.svd_policy)
    return FitSumOptions(nfullsweeps=o.nfullsweeps, max_bond_dim=o.max_bond_dim, svd_policy=pol, convergence_tol=o.convergence_tol)


@functools.lru_cache(maxsize=None)
def restated(name):
    t, i, c, o, w = F.CASES[name]
    r, info = F.np_fit_sum(t, i, c, o, w)
    return F.np_full(r), info, F.np_sum(t, w), F.scale_of(t, w)


def deviation(got, want, scale):
    return float(np.linalg.norm(got - want) / scale)


# ------------------------------------------------------------------------------------------------ exact: full bonds
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n, site, K", F.EXACT)
def test_one_sweep_from_full_bonds_returns_the_sum_of_trains(n, site, K, route):
    w = None if K == 1 else [1.0, 0.5, -2.0]
    targets, initial, w = F.exact_case(n, site, K, w)
    res = fit_sum([tt(t) for t in targets], tt(initial), 0, FitSumOptions(), w, route, return_info=True)
    dev = deviation(dense(res.state), F.np_sum(targets, w), F.scale_of(targets, w))
    print(f"exact n={n} S={site} K={K} {route}: {dev:.3e}")
    assert res.sweeps_completed == 1 and res.local_updates == 2 * (n - 1) and not res.converged and len(res.norms) == 1
    assert dev <= 1e-12


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n, sd, K", [(4, (2, 2), 3), (5, (3, 1), 3), (4, (1, 2), 1)])
def test_one_sweep_from_full_bonds_returns_the_sum_of_mpos(n, sd, K, route):
    site = sd[0] * sd[1]
    w = None if K == 1 else [1.0, -0.25, 3.0]
    targets, initial, w = F.exact_case(n, site, K, w)
    sds = [sd] * n
    res = fit_sum([MPO(F.unfuse(t, sds)) for t in targets], MPO(F.unfuse(initial, sds)), n - 1, FitSumOptions(), w, route)
    assert isinstance(res, MPO) and res.site_dims() == sds
    dev = deviation(dense(res), F.np_sum(targets, w), F.scale_of(targets, w))
    print(f"exact mpo n={n} sd={sd} K={K} {route}: {dev:.3e}")
    assert dev <= 1e-12


@pytest.mark.parametrize("route", ROUTES)
def test_a_pair_that_cancels_gives_zero_without_nan(route):
    targets, initial, w = F.exact_case(4, 2, 2, cancel=True)
    for coefficients, pair in ((w, targets), (None, [targets[0], [targets[0][0] * -1.0] + targets[0][1:]])):
        got = dense(fit_sum([tt(t) for t in pair], tt(initial), 1, FitSumOptions(), coefficients, route))
        assert np.all(np.isfinite(got))
        assert np.linalg.norm(got) <= 1e-12 * F.scale_of(targets, w)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("center", range(5))
def test_every_center_of_a_five_site_chain(center, route):
    targets, initial, w = F.exact_case(5, 2, 3, [2.0, 1.0, -1.0])
    res = fit_sum([tt(t) for t in targets], tt(initial), center, FitSumOptions(), w, route, return_info=True)
    assert res.local_updates == 8
    assert deviation(dense(res.state), F.np_sum(targets, w), F.scale_of(targets, w)) <= 1e-12


# ------------------------------------------------------------------------------------------------ the short-circuits and the extensions
def test_the_doc_test_of_the_reference():
    """[1, 2] + [3, 4] -> [4, 6] from an initial of zeros"""
    make = lambda v: tt([np.array(v, dtype=np.float64).reshape(1, 2, 1)])  # noqa: E731
    for route in ROUTES + ("auto",):
        res = fit_sum([make([1.0, 2.0]), make([3.0, 4.0])], make([0.0, 0.0]), 0, FitSumOptions(nfullsweeps=1), route=route, return_info=True)
        assert np.array_equal(res.state.site_tensor(0).reshape(-1), [4.0, 6.0]) and res.link_dims == [] and res.sweeps_completed == 0
    three = fit_sum([make([1.0, 2.0]), make([3.0, 4.0]), make([0.5, 0.25])], None, 0, None, [2.0, -1.0, 4.0])
    assert np.array_equal(three.site_tensor(0).reshape(-1), [1.0, 1.0])


def test_no_sweep_returns_a_clone_of_the_initial():
    targets, initial, _ = F.exact_case(4, 2, 3)
    res = fit_sum([tt(t) for t in targets], tt(initial), 2, FitSumOptions(nfullsweeps=0), return_info=True)
    assert res.sweeps_completed == 0 and res.local_updates == 0 and res.norms == []
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res.state.site_tensors(), initial))
    none = fit_sum([tt(t) for t in targets], None, 0, FitSumOptions(nfullsweeps=0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(none.site_tensors(), targets[0]))


@pytest.mark.parametrize("route", ROUTES)
def test_initial_none_starts_from_the_first_target_and_grows_under_a_policy(route):
    targets = F.CASES["cap"][0]
    o = F.Options(nfullsweeps=3, svd_policy=(1e-10, 0, 0, 0))
    want, info = F.np_fit_sum(targets, None, 1, o)
    res = fit_sum([tt(t) for t in targets], None, 1, options(o), route=route, return_info=True)
    dev = deviation(dense(res.state), F.np_full(want), F.scale_of(targets))
    print(f"initial=None {route}: {dev:.3e} links {res.link_dims}")
    assert res.link_dims == info["link_dims"] and max(res.link_dims) > 3
    assert dev <= 10 * MEASURED["none"]


@pytest.mark.parametrize("route", ROUTES)
def test_with_no_option_set_the_ranks_are_fixed(route):
    targets, initial, center = F.CASES["cap"][0], F.CASES["cap"][1], 4
    want, info = F.np_fit_sum(targets, initial, center, F.Options(nfullsweeps=2))
    res = fit_sum([tt(t) for t in targets], tt(initial), center, FitSumOptions(nfullsweeps=2), route=route, return_info=True)
    dev = deviation(dense(res.state), F.np_full(want), F.scale_of(targets))
    print(f"fixed ranks {route}: {dev:.3e}")
    assert res.link_dims == F.links(initial) == info["link_dims"]
    assert np.allclose(res.norms, info["norms"], rtol=1e-12, atol=0)
    assert dev <= 10 * MEASURED["fixed"]


# ------------------------------------------------------------------------------------------------ truncating cases against the restatement
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ("cap", "policy", "stop", "k40"))
def test_truncating_cases_follow_the_restatement(name, route):
    t, i, c, o, w = F.CASES[name]
    want, info, exact, scale = restated(name)
    res = fit_sum([tt(x) for x in t], None if i is None else tt(i), c, options(o), w, route, return_info=True)
    got = dense(res.state)
    dev = deviation(got, want, scale)
    err, err_np = deviation(got, exact, scale), deviation(want, exact, scale)
    print(f"{name} {route}: deviation {dev:.3e}, error {err:.6e} against the restatement's {err_np:.6e}, links {res.link_dims}, sweeps {res.sweeps_completed}")
    assert res.link_dims == info["link_dims"]
    assert (res.sweeps_completed, res.local_updates, res.converged) == (info["sweeps_completed"], info["local_updates"], info["converged"])
    if o.max_bond_dim is not None:
        assert max(res.link_dims) <= o.max_bond_dim
    assert dev <= 10 * MEASURED[name]
    assert abs(err - err_np) <= 10 * MEASURED[name]


@pytest.mark.parametrize("route", ROUTES)
def test_two_identical_calls_give_identical_bytes(route):
    t, i, c, o, w = F.CASES["policy"]
    runs = [fit_sum([tt(x) for x in t], tt(i), c, options(o), w, route).site_tensors() for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ refusals
def test_error_answers_come_back_before_an_operand_is_read():
    lib = t4a_amd._lib
    o = t4a_amd.FitSumOptionsC()
    lib.t4a_gpu_fit_sum_options_default(ctypes.byref(o))
    o.has_convergence_tol, o.convergence_tol = 1, -1.0
    h, a, b, c = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    bad = (ctypes.c_void_p * 2)(1, 1)  # not handles: looking at them would fault
    for fn in (lib.t4a_gpu_tt_fit_sum, lib.t4a_gpu_mpo_fit_sum):
        st = fn(bad, ctypes.c_size_t(2), None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.c_int32(0), ctypes.byref(h), ctypes.byref(a), ctypes.byref(b),
                ctypes.byref(c), None)
        assert st == t4a_amd.INVALID_ARGUMENT and "convergence tolerance must be finite and non-negative" in t4a_amd.last_error_message()
    targets, initial, _ = F.exact_case(4, 2, 2)
    with pytest.raises(t4a_amd.T4aError, match="target 1 has an incompatible named topology"):
        fit_sum([tt(targets[0]), tt(targets[1][:2] + [targets[1][2][:, :, :1]])], tt(initial))
    with pytest.raises(t4a_amd.T4aError, match="center node is not in initial TreeTN"):
        fit_sum([tt(t) for t in targets], tt(initial), 4)
    with pytest.raises(t4a_amd.T4aError, match="not a mixture"):
        fit_sum([tt(targets[0]), MPO(F.unfuse(targets[1], [(2, 1)] * 4))])
