"""One-site TDVP on the device (t4a_amd.tdvp_one_site, t4a_amd.gse_tdvp_one_site) against dense exponentials and against the numpy
restatement (tests/tdvp_one_site_np.py, itself checked without a device in tests/test_cpu_tdvp_one_site.py).

The tolerances are those of tests/test_gpu_tdvp.py: against the dense exponential the 1e-9 of the CPU test (the reference's own bound at
the default Krylov tolerance 1e-12); "device against restatement" is tdvp_np.spread_tolerance, computed from the restatement alone — three
more runs with every entry of the start multiplied by 1 + 2^-50 u, tol = max(100 spread, 1e-12).  The dense state vector is compared: it
does not see the gauge, in which the device (Q stays, the neighbour absorbs C') and the restatement (Q C' stored) differ."""
import numpy as np
import pytest

import tdvp_one_site_np as t1
from tdvp_one_site_np import TAU, np_tdvp_one_site
from tdvp_np import Options
import t4a_amd
from t4a_amd import MPO, SimpleTensorTrain, TdvpOptions, GseOptions, GseTdvpOptions, tdvp_one_site, gse_tdvp, gse_tdvp_one_site
from t4a_amd.tdvp import _set_bond_apply_route, BOND_FUSED, BOND_GEMM, BOND_AUTO

pytestmark = pytest.mark.gpu

DENSE_TOL = 1e-9


def dense_state(tt):
    return t1.np_state_full(tt.site_tensors())


def substeps(order):
    return len(t1.applyexp_sub_steps(order))


_CASES = {}


def dense_case(name):
    """-> (ops, init, tau, exp(tau H) psi), once"""
    if name not in _CASES:
        if name == "mixed3":
            ops, init = t1.bonds_case((2, 3, 2), (1, 2, 2, 1))
        else:
            ops, init = t1.bonds_case((2,) * 4, (1, 2, 4, 2, 1), name)
        tau = TAU if name == "tfim" else t1.case_tau(ops)
        _CASES[name] = (ops, init, tau, t1.dense_exponential(ops, init, tau))
    return _CASES[name]


# ------------------------------------------------------------------------------------------------ against dense exponentials
@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("center", (0, 1, 3))
@pytest.mark.parametrize("name", ("sym", "tfim"))
def test_full_bond_sweeps_against_the_dense_exponential(name, center, order):
    ops, init, tau, want = dense_case(name)
    n, w = len(ops), substeps(order)
    r = tdvp_one_site(MPO(ops), SimpleTensorTrain(init), center, TdvpOptions(nsite=1, order=order, exponent_step=tau))
    err = t1.relative_distance(dense_state(r.state), want)
    print(name, center, order, "to the dense exponential", err, r.stats)
    assert err <= DENSE_TOL
    assert (r.sweeps_completed, r.local_updates) == (1, w * (2 * n - 1))
    assert (r.stats["one_site_steps"], r.stats["bond_corrections"], r.stats["max_time_splits"]) == (w * n, w * (n - 1), 1)
    assert r.stats["krylov_steps"] == r.stats["apply_calls"] >= r.local_updates
    assert r.stats["fused_applies"] + r.stats["gemm_applies"] > 0
    assert r.state.link_dims() == [t.shape[2] for t in t1.np_canonicalize(init, center)[:-1]]
    assert 0.0 <= r.max_error_estimate <= 1e-12 * max(1.0, np.linalg.norm(t1.np_state_full(init)))


@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("center", (0, 1, 2))
def test_mixed_site_dimensions_against_the_dense_exponential(center, order):
    ops, init, tau, want = dense_case("mixed3")
    r = tdvp_one_site(MPO(ops), SimpleTensorTrain(init), center, TdvpOptions(nsite=1, order=order, exponent_step=tau))
    err = t1.relative_distance(dense_state(r.state), want)
    print("mixed3", center, order, "to the dense exponential", err)
    assert err <= DENSE_TOL and r.local_updates == substeps(order) * 5


# ------------------------------------------------------------------------------------------------ against the restatement on thin bonds
def test_thin_bonds_against_the_restatement():
    ops, init = t1.thin_case()
    c, o = t1.THIN["center"], Options(nsweeps=t1.THIN["nsweeps"], order=t1.THIN["order"], exponent_step=TAU, cgs2=True)
    want = t1.thin_restated(cgs2=True)
    r = tdvp_one_site(MPO(ops), SimpleTensorTrain(init), c, TdvpOptions(nsite=1, nsweeps=o.nsweeps, order=o.order, exponent_step=TAU))
    tol, spread = t1.spread_tolerance(lambda start: t1.np_state_full(np_tdvp_one_site(ops, start, c, o)["state"]), init)
    dist = t1.relative_distance(dense_state(r.state), t1.np_state_full(want["state"]))
    print("thin: tol", tol, "spread", spread, "device distance", dist, r.stats, "restated iterations", want["max_krylov_iterations"],
          "modified Gram-Schmidt", t1.thin_restated(cgs2=False)["max_krylov_iterations"])
    assert dist <= tol
    assert (r.sweeps_completed, r.local_updates, r.max_krylov_iterations) == (want["sweeps_completed"], want["local_updates"], want["max_krylov_iterations"])
    assert (r.stats["one_site_steps"], r.stats["bond_corrections"]) == (want["one_site_steps"], want["bond_corrections"])
    assert r.state.link_dims() == [t.shape[2] for t in want["state"][:-1]] == list(t1.THIN["bonds"][1:-1])


# ------------------------------------------------------------------------------------------------ further cases
def test_a_product_state_keeps_its_bonds():
    ops = t1.tfim(4, 0.7)
    init = t1.random_state((2,) * 4, [1] * 5, t1.SEED ^ 0x9D)
    o = Options(order=2, exponent_step=TAU, cgs2=True)
    want = np_tdvp_one_site(ops, init, 1, o)
    r = tdvp_one_site(MPO(ops), SimpleTensorTrain(init), 1, TdvpOptions(nsite=1, order=2, exponent_step=TAU))
    assert r.state.link_dims() == [1, 1, 1]
    tol, spread = t1.spread_tolerance(lambda start: t1.np_state_full(np_tdvp_one_site(ops, start, 1, o)["state"]), init)
    dist = t1.relative_distance(dense_state(r.state), t1.np_state_full(want["state"]))
    print("product: tol", tol, "device distance", dist)
    assert dist <= tol and r.local_updates == want["local_updates"] == 2 * 7


def test_tau_zero_returns_init_and_two_runs_give_the_same_bits():
    ops, init = t1.thin_case()
    op, psi = MPO(ops), SimpleTensorTrain(init)
    r0 = tdvp_one_site(op, psi, 3, TdvpOptions(nsite=1, exponent_step=0.0))
    assert t1.relative_distance(dense_state(r0.state), t1.np_state_full(init)) <= 1e-13
    a = tdvp_one_site(op, psi, 3, TdvpOptions(nsite=1, exponent_step=TAU))
    b = tdvp_one_site(op, psi, 3, TdvpOptions(nsite=1, exponent_step=TAU))
    assert all(np.array_equal(s.view(np.uint64), t.view(np.uint64)) for s, t in zip(a.state.site_tensors(), b.state.site_tensors()))
    assert a.stats == b.stats and a.max_error_estimate == b.max_error_estimate


def test_both_apply_routes_give_the_same_state():
    ops, init, tau, want = dense_case("sym")
    op, psi = MPO(ops), SimpleTensorTrain(init)
    states = {}
    try:
        for route in (BOND_FUSED, BOND_GEMM):
            _set_bond_apply_route(route)
            r = tdvp_one_site(op, psi, 1, TdvpOptions(nsite=1, order=2, exponent_step=tau))
            assert r.stats["fused_applies" if route == BOND_GEMM else "gemm_applies"] == 0 and r.stats["apply_calls"] > 0
            assert r.stats["fused_applies"] + r.stats["gemm_applies"] > 0
            states[route] = dense_state(r.state)
            assert t1.relative_distance(states[route], want) <= DENSE_TOL
    finally:
        _set_bond_apply_route(BOND_AUTO)
    assert t1.relative_distance(states[BOND_FUSED], states[BOND_GEMM]) <= DENSE_TOL


def test_refusals_through_python():
    ops, init = t1.thin_case()
    op, psi = MPO(ops), SimpleTensorTrain(init)
    bad = t4a_amd.INVALID_ARGUMENT
    for kw, text in (({"nsite": 2}, "one-site TDVP requires nsite=1, got nsite=2; nsite=2 is tdvp"),
                     ({"nsite": 1, "max_bond_dim": 4}, "invalid TDVP option max_bond_dim: one-site TDVP has fixed ranks; use nsite=2 for truncation"),
                     ({"nsite": 1, "svd_policy": t4a_amd.SvdTruncationPolicy()}, "invalid TDVP option svd_policy: one-site TDVP has fixed ranks; use nsite=2 for truncation"),
                     ({"nsite": 1, "nsweeps": 0}, "invalid TDVP option nsweeps"), ({"nsite": 1, "order": 3}, "order 3 is not supported")):
        with pytest.raises(t4a_amd.T4aError) as e:
            tdvp_one_site(op, psi, 0, TdvpOptions(**kw))
        assert e.value.code == bad and text in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp_one_site(op, psi, 5)
    assert e.value.code == bad and "TDVP center 5 is not a state node" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp_one_site(MPO([np.eye(2).reshape((1, 2, 2, 1))]), SimpleTensorTrain([np.ones((1, 2, 1))]), 0)
    assert e.value.code == bad and "a single site" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp_one_site(MPO(t1.tfim(4, 0.7)), psi, 0)
    assert e.value.code == bad and "lengths differ" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp_one_site(op, psi, 0, TdvpOptions(nsite=1, exponent_step=-0.1j))
    assert e.value.code == bad and "complex tensor trains" in e.value.message


# ------------------------------------------------------------------------------------------------ gse_tdvp_one_site
def test_gse_grows_the_bonds_of_a_product_state_and_comes_closer_to_the_dense_exponential():
    ops = t1.tfim(4, 0.7)
    init = t1.random_state((2,) * 4, [1] * 5, t1.SEED ^ 0x9E)
    op, psi = MPO(ops), SimpleTensorTrain(init)
    want = t1.dense_exponential(ops, init, TAU)
    to = TdvpOptions(nsite=1, order=2, exponent_step=TAU)
    for center in (0, 2):
        plain = tdvp_one_site(op, psi, center, to)
        grown = gse_tdvp_one_site(op, psi, center, GseTdvpOptions(GseOptions(krylov_dim=2), to))
        e_plain, e_grown = t1.relative_distance(dense_state(plain.state), want), t1.relative_distance(dense_state(grown.state), want)
        print("gse one-site from", center, "links", plain.state.link_dims(), "->", grown.state.link_dims(), "errors", e_plain, "->", e_grown)
        assert plain.state.link_dims() == [1, 1, 1] and all(b > 1 for b in grown.state.link_dims())
        assert e_grown < e_plain
        assert (grown.sweeps_completed, grown.gse_expansions, grown.local_updates) == (1, 1, 2 * 7)


@pytest.mark.parametrize("first", (True, False))
def test_gse_at_full_bonds_meets_the_dense_tolerance_and_counts_its_expansions(first):
    ops, init, tau, _ = dense_case("tfim")
    want = t1.dense_exponential(ops, init, 2 * tau)
    r = gse_tdvp_one_site(MPO(ops), SimpleTensorTrain(init), 1,
                          GseTdvpOptions(GseOptions(krylov_dim=1, expand_before_first_sweep=first), TdvpOptions(nsite=1, nsweeps=2, order=2, exponent_step=tau)))
    err = t1.relative_distance(dense_state(r.state), want)
    print("gse one-site at full bonds: first", first, "error", err, "links", r.state.link_dims())
    assert err <= DENSE_TOL
    assert (r.sweeps_completed, r.gse_expansions, r.local_updates) == (2, 2 if first else 1, 2 * 2 * 7)
    # krylov_dim = 0: no expansion, the plain integrator
    r0 = gse_tdvp_one_site(MPO(ops), SimpleTensorTrain(init), 1, GseTdvpOptions(GseOptions(), TdvpOptions(nsite=1, nsweeps=2, order=2, exponent_step=tau)))
    assert r0.gse_expansions == 0 and t1.relative_distance(dense_state(r0.state), want) <= DENSE_TOL


def test_gse_refusals_old_and_new():
    ops, init = t1.thin_case()
    op, psi = MPO(ops), SimpleTensorTrain(init)
    bad = t4a_amd.INVALID_ARGUMENT
    with pytest.raises(t4a_amd.T4aError) as e:  # the two-site entry point still refuses nsite = 1, with its message
        gse_tdvp(op, psi, 0, GseTdvpOptions(GseOptions(krylov_dim=1), TdvpOptions(nsite=1)))
    assert e.value.code == bad and "one-site TDVP (nsite=1) is not implemented here" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp_one_site(op, psi, 0, GseTdvpOptions(GseOptions(krylov_dim=1), TdvpOptions()))
    assert e.value.code == bad and "one-site TDVP requires nsite=1, got nsite=2" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp_one_site(op, psi, 0, GseTdvpOptions(GseOptions(krylov_dim=1), TdvpOptions(nsite=1, max_bond_dim=4)))
    assert e.value.code == bad and "one-site TDVP has fixed ranks" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp_one_site(op, psi, 5, GseTdvpOptions(GseOptions(krylov_dim=1), TdvpOptions(nsite=1)))
    assert e.value.code == bad and "is not a state node" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp_one_site(op, psi, 0, GseTdvpOptions(GseOptions(density_weight_cutoff=-1.0), TdvpOptions(nsite=1)))
    assert e.value.code == bad and "invalid GSE option density_weight_cutoff" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        gse_tdvp_one_site(op, psi, 0, GseTdvpOptions(GseOptions(krylov_dim=9), TdvpOptions(nsite=1)))
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED
