"""Two-site DMRG on the device (t4a_amd.dmrg) against dense eigensolves and the numpy restatement (tests/dmrg_np.py, itself checked
without a device in tests/test_cpu_dmrg.py).  The bounds: a unit vector's Rayleigh quotient lies within its residual of an eigenvalue
and the local residuals are <= rtol max(1, |lambda|), hence 1e-10 max(1, ||H||_2) for the untruncated cases; rounding of sums of a few
thousand terms at the scale of the operator, hence 1e-12 ||H||_2 wherever two evaluations of the same quantity are compared."""
import numpy as np
import pytest

import dmrg_np as dn
from dmrg_np import UNTRUNCATED, np_energy, np_lanczos
import t4a_amd
from t4a_amd import MPO, SimpleTensorTrain, ProjectedOperator, DmrgOptions, HermitianLanczosOptions, dmrg, dmrg_energy
from t4a_amd.dmrg import _lanczos_dense

pytestmark = pytest.mark.gpu


def device_options(o):
    return HermitianLanczosOptions(max_iter=o.max_iter, rtol=o.rtol, atol=o.atol, breakdown_tol=o.breakdown_tol, hermitian_tol=o.hermitian_tol)


# ------------------------------------------------------------------------------------------------ Lanczos on dense matrices
@pytest.mark.parametrize("name", sorted(dn.dense_cases()))
def test_lanczos_dense_against_the_restatement(name):
    h, v0, o, breaks_down = dn.dense_cases()[name]
    want = np_lanczos(lambda v: h @ v, v0, o)
    lam, vec, it, res, conv = _lanczos_dense(h, v0, device_options(o))
    norm = float(np.linalg.norm(h, 2))
    threshold = o.threshold(lam)
    print(name, "device", lam, it, res, conv, "restated", want[0], want[2], want[3], want[4])
    assert conv == want[4]
    if breaks_down:
        assert it == want[2]
    assert abs(res - np.linalg.norm(h @ vec - lam * vec)) <= 1e-12 * norm
    assert abs(np.linalg.norm(vec) - 1.0) <= 1e-12
    if conv:
        assert res <= threshold + 1e-12 * norm
        assert abs(lam - np.linalg.eigvalsh(h)[0]) <= threshold
    else:
        assert it == o.max_iter and lam >= np.linalg.eigvalsh(h)[0] - 1e-12 * norm


def test_lanczos_dense_refuses_a_nonsymmetric_matrix_and_a_zero_start():
    h, v0 = dn.nonsymmetric_case()
    with pytest.raises(t4a_amd.T4aError) as e:
        _lanczos_dense(h, v0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "projected operator is not Hermitian" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        _lanczos_dense(np.eye(4), np.zeros(4))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "zero" in e.value.message


# ------------------------------------------------------------------------------------------------ the sweeps
_RUNS = {}


def device_run(name, nsweeps=2):
    """dmrg of the case with default options and `nsweeps` sweeps, once"""
    key = (name, nsweeps)
    if key not in _RUNS:
        ops, init, center, cap = dn.make_case(name)
        _RUNS[key] = dmrg(MPO(ops), SimpleTensorTrain(init), center, DmrgOptions(nsweeps=nsweeps, max_bond_dim=cap))
    return _RUNS[key]


@pytest.mark.parametrize("name", UNTRUNCATED)
def test_untruncated_cases_reach_the_dense_ground_state(name):
    ops, init, center, _ = dn.make_case(name)
    _, lams, ground, norm = dn.dense_spectrum(name)
    r = device_run(name)
    n = len(ops)
    x = r.state.site_tensors()
    print(name, "E - E0", r.energy - lams[0], "max residual", r.max_residual_norm, r.stats)
    assert abs(r.energy - lams[0]) <= 1e-10 * max(1.0, norm)
    assert abs(r.energy - np_energy(ops, x, center)) <= 1e-12 * norm
    assert abs(dmrg_energy(MPO(ops), r.state, center) - r.energy) <= 1e-12 * norm
    psi = dn.np_state_full(x)
    assert abs(psi @ ground) / np.linalg.norm(psi) >= 1 - 1e-8
    assert r.sweeps_completed == 2 and r.local_updates == 2 * 2 * (n - 1) == r.stats["local_solves"] and not r.converged
    # the largest threshold max(atol, rtol max(1, |lambda|)) over the local solves, from the restatement's Ritz values
    largest_threshold = dn.restated(name, 2)["max_threshold"]
    print(name, "largest threshold", largest_threshold)
    assert r.max_residual_norm <= largest_threshold + 1e-12 * norm
    assert r.stats["lanczos_steps"] >= r.local_updates and r.stats["apply_calls"] >= r.stats["lanczos_steps"] + r.local_updates


def test_capped_case_agrees_with_the_restatement_at_its_fixed_point():
    """The two implementations differ by rounding inside a converged fixed-point iteration; the restatement's own drift over sweeps
    3..6 is the scale of that, so the tolerance is 100 times it with the floor 1e-12 ||H||_2."""
    ops, _, center, cap = dn.make_case("tfim8_cap4")
    _, lams, _, norm = dn.dense_spectrum("tfim8_cap4")
    history = dn.restated("tfim8_cap4", 6)["history"]
    tolerance = max(100.0 * max(abs(history[k + 1] - history[k]) for k in range(2, 5)), 1e-12 * norm)
    r = device_run("tfim8_cap4", 4)
    print("tfim8_cap4: E_device - E_restated", r.energy - history[3], "tolerance", tolerance, "E - E0", r.energy - lams[0])
    assert all(b <= cap for b in r.state.link_dims())
    assert r.energy >= lams[0] - 1e-10 * norm
    assert abs(r.energy - history[3]) <= tolerance
    assert abs(r.energy - np_energy(ops, r.state.site_tensors(), center)) <= 1e-12 * norm


def test_energy_tolerance_stops_the_sweeps_early():
    ops, init, center, _ = dn.make_case("heis6_c3")
    _, lams, _, norm = dn.dense_spectrum("heis6_c3")
    r = dmrg(MPO(ops), SimpleTensorTrain(init), center, DmrgOptions(nsweeps=10, energy_tol=1e-9))
    assert r.converged and 2 <= r.sweeps_completed < 10 and r.local_updates == r.sweeps_completed * 2 * (len(ops) - 1)
    assert abs(r.energy - lams[0]) <= 1e-10 * max(1.0, norm)
    plain = device_run("heis6_c3")
    assert not plain.converged and plain.sweeps_completed == 2


def test_two_lanczos_steps_return_with_the_flag_semantics():
    ops, init, center, _ = dn.make_case("heis6_c3")
    _, lams, _, norm = dn.dense_spectrum("heis6_c3")
    r = dmrg(MPO(ops), SimpleTensorTrain(init), center, DmrgOptions(nsweeps=2, lanczos=HermitianLanczosOptions(max_iter=2)))
    assert r.sweeps_completed == 2 and r.local_updates == 20 and not r.converged
    assert r.stats["lanczos_steps"] <= 2 * r.local_updates
    assert r.max_residual_norm > 1e-10 * max(1.0, norm)  # some local solve did not converge: a flag, no error
    assert lams[0] - 1e-10 * norm <= r.energy <= lams[-1] + 1e-10 * norm
    assert abs(r.energy - np_energy(ops, r.state.site_tensors(), center)) <= 1e-12 * norm


def test_a_start_above_the_cap_is_truncated_by_the_first_sweep():
    ops = dn.tfim(6, 0.7)
    _, lams, _, norm = dn.dense_spectrum("tfim6")
    init = dn.random_state((2,) * 6, [1, 2, 4, 6, 4, 2, 1], dn.SEED ^ 0xCA9)
    r = dmrg(MPO(ops), SimpleTensorTrain(init), 0, DmrgOptions(nsweeps=1, max_bond_dim=3))
    assert r.state.link_dims() == [2, 3, 3, 3, 2]
    assert r.energy >= lams[0] - 1e-10 * norm
    assert abs(r.energy - np_energy(ops, r.state.site_tensors(), 0)) <= 1e-12 * norm


def test_projected_operator_on_the_result_reproduces_the_energy():
    for name in ("heis6_c3", "tfim6", "mixed5"):
        ops, _, center, _ = dn.make_case(name)
        norm = dn.dense_spectrum(name)[3]
        r = device_run(name)
        x = r.state.site_tensors()
        site = center if center + 1 < len(ops) else center - 1
        po = ProjectedOperator(MPO(ops), r.state)
        theta = np.einsum("lsm,mtr->lstr", x[site], x[site + 1])
        y = po.apply(site, theta)
        assert abs(float(np.sum(theta * y)) / float(np.sum(theta * theta)) - r.energy) <= 1e-12 * norm


def test_shape_and_state_errors_come_from_the_public_call():
    ops, init, center, _ = dn.make_case("n2")
    with pytest.raises(t4a_amd.T4aError) as e:
        dmrg(MPO(ops), SimpleTensorTrain(init), 2)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "center 2" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        dmrg(MPO(ops), SimpleTensorTrain([np.zeros_like(t) for t in init]), 0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "zero" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        dmrg_energy(MPO(ops), SimpleTensorTrain([np.zeros_like(t) for t in init]), 0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "denominator is zero" in e.value.message
