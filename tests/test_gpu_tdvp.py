"""Two-site TDVP on the device (t4a_amd.tdvp) against the numpy restatement (tests/tdvp_np.py, itself checked without a device in
tests/test_cpu_tdvp.py) and against dense exponentials.

The tolerance of "device against restatement" is computed from the restatement alone (tdvp_np.spread_tolerance): the same run three
more times with every entry of the start multiplied by 1 + 2^-50 u, u uniform in [-1, 1]; `spread` is the largest relative l2 distance
of those results to the unperturbed one, and tol = max(100 spread, 1e-12) — the factor and the floor of the capped DMRG comparison.
Two correct implementations differ by rounding, and what rounding does to this computation is what the spread measures.  Against the
dense exponential the bound is the 1e-9 of the CPU test (the reference's own bound at the default Krylov tolerance 1e-12)."""
import numpy as np
import pytest

import tdvp_np as tn
from tdvp_np import TAU, np_krylov_expm, np_tdvp
import t4a_amd
from t4a_amd import MPO, SimpleTensorTrain, ProjectedOperator, TdvpOptions, HermitianKrylovExpmOptions, tdvp, dmrg_energy
from t4a_amd.tdvp import _krylov_expm_dense, _apply_one_site

pytestmark = pytest.mark.gpu


def device_options(o):
    return HermitianKrylovExpmOptions(max_iter=o.max_iter, max_time_splits=o.max_time_splits, tol=o.tol, breakdown_tol=o.breakdown_tol,
                                      hermitian_tol=o.hermitian_tol)


# ------------------------------------------------------------------------------------------------ the Krylov exponential on dense matrices
@pytest.mark.parametrize("name", sorted(tn.dense_cases()))
def test_krylov_expm_dense_against_the_restatement(name):
    h, v0, tau, o = tn.dense_cases()[name]

    def run(start):
        return np_krylov_expm(lambda v: h @ v, tau, start[0], o, cgs2=True)[0]
    want = np_krylov_expm(lambda v: h @ v, tau, v0, o, cgs2=True)
    out, it, err, conv, splits = _krylov_expm_dense(h, v0, tau, device_options(o))
    print(name, "device", it, err, conv, splits, "restated", want[1:])
    assert (conv, splits) == (want[3], want[4])
    if name in ("diag3", "eigenvector_start", "forced_split", "tau_zero", "zero_start"):
        assert it == want[1]
    if np.linalg.norm(v0) == 0.0 or tau == 0.0:
        assert np.array_equal(out, v0) and it == 0 and err == 0.0
        return
    tol, spread = tn.spread_tolerance(run, [v0])
    dist = tn.relative_distance(out, want[0])
    print(name, "tol", tol, "spread", spread, "device distance", dist)
    assert dist <= tol
    assert err <= o.tol * max(np.linalg.norm(v0), 1.0)


def test_krylov_expm_dense_errors():
    h, v0, tau, o = tn.failing_case()
    with pytest.raises(t4a_amd.T4aError) as e:
        _krylov_expm_dense(h, v0, tau, device_options(o))
    assert e.value.code == t4a_amd.INTERNAL_ERROR and "hermitian_krylov_expm_multiply did not converge within max_time_splits=1 and max_iter=1" in e.value.message
    h, v0 = tn.nonsymmetric_case()
    with pytest.raises(t4a_amd.T4aError) as e:
        _krylov_expm_dense(h, v0, -0.3)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "projected operator is not Hermitian" in e.value.message


# ------------------------------------------------------------------------------------------------ the sweeps
def dense_state(tt):
    return tn.np_state_full(tt.site_tensors())


@pytest.mark.parametrize("order, end, nsweeps", tn.RUNS)
@pytest.mark.parametrize("name", sorted(tn.CASES))
def test_sweeps_against_the_restatement_and_the_dense_exponential(name, order, end, nsweeps):
    ops, init = tn.make_case(name)
    n = len(ops)
    center = 0 if end == 0 else n - 1
    o = tn.Options(nsweeps=nsweeps, order=order, exponent_step=TAU)
    want = tn.restated(name, order, end, nsweeps)
    r = tdvp(MPO(ops), SimpleTensorTrain(init), center, TdvpOptions(nsweeps=nsweeps, order=order, exponent_step=TAU))
    psi = dense_state(r.state)
    tol, spread = tn.spread_tolerance(lambda start: tn.np_state_full(np_tdvp(ops, start, center, o)["state"]), init)
    dist = tn.relative_distance(psi, tn.np_state_full(want["state"]))
    exact = tn.relative_distance(psi, tn.dense_exponential(name, TAU * nsweeps))
    print(name, order, end, nsweeps, "tol", tol, "spread", spread, "device distance", dist, "to the dense exponential", exact, r.stats)
    assert dist <= tol
    assert exact <= 1e-9
    assert (r.sweeps_completed, r.local_updates, r.max_krylov_iterations) == (want["sweeps_completed"], want["local_updates"], want["max_krylov_iterations"])
    assert (r.stats["two_site_steps"], r.stats["corrections"], r.stats["max_time_splits"]) == (want["two_site_steps"], want["corrections"], 1)
    assert r.stats["krylov_steps"] == r.stats["apply_calls"] >= r.local_updates
    assert 0.0 <= r.max_error_estimate <= 1e-12 * max(1.0, np.linalg.norm(tn.np_state_full(init)))


def test_capped_case_against_the_restatement():
    ops, init, o = tn.capped_case()
    want = tn.capped_restated()
    r = tdvp(MPO(ops), SimpleTensorTrain(init), 0, TdvpOptions(nsweeps=o.nsweeps, order=o.order, exponent_step=o.exponent_step, max_bond_dim=o.max_bond_dim))
    tol, spread = tn.spread_tolerance(lambda start: tn.np_state_full(np_tdvp(ops, start, 0, o)["state"]), init)
    dist = tn.relative_distance(dense_state(r.state), tn.np_state_full(want["state"]))
    print("capped: tol", tol, "spread", spread, "device distance", dist, r.stats)
    assert all(b <= o.max_bond_dim for b in r.state.link_dims()) and r.state.link_dims() == [t.shape[2] for t in want["state"][:-1]]
    assert dist <= tol
    assert (r.sweeps_completed, r.local_updates) == (3, want["local_updates"])


def test_imaginary_time_relaxation_lowers_the_energy():
    """40 calls of one first-order sweep with tau = -0.2 on the Ising chain, renormalised between the calls.  Without a bond cap every
    substep applies exp(tau H_projected), which cannot raise the Rayleigh quotient; the energies are compared at the tolerance rule
    applied to the sequence of the restatement's energies, scaled by ||H||_2."""
    n, calls = 6, 40
    ops = tn.tfim(n, 0.7)
    h = tn.np_operator_full(ops)
    lams = np.linalg.eigvalsh(h)
    norm = float(max(abs(lams[0]), abs(lams[-1])))
    init = tn.random_state((2,) * n, [1] + [2] * (n - 1) + [1], tn.SEED ^ 0x4E1)
    o = tn.Options(order=1, exponent_step=-0.2)

    def restated_energies(start):
        x, es = start, []
        for _ in range(calls):
            x = np_tdvp(ops, x, 0, o)["state"]
            psi = tn.np_state_full(x)
            x = [x[0] * (1.0 / np.linalg.norm(psi))] + x[1:]
            psi = psi * (1.0 / np.linalg.norm(psi))
            es.append(float(psi @ (h @ psi)))
        return np.array(es) / norm
    base = restated_energies(init)
    spread = max(float(np.abs(restated_energies(tn.perturbed(init, s)) - base).max()) for s in (1, 2, 3))
    tol = max(100.0 * spread, 1e-12) * norm
    mpo, state, energies = MPO(ops), SimpleTensorTrain(init), []
    for _ in range(calls):
        r = tdvp(mpo, state, 0, TdvpOptions(order=1, exponent_step=-0.2))
        state = r.state.scale(1.0 / r.state.norm())
        energies.append(dmrg_energy(mpo, state, 0))
    energies = np.array(energies)
    print("relaxation: tol", tol, "largest rise", float(np.diff(energies).max()), "E - E0 device", energies[-1] - lams[0], "restated", base[-1] * norm - lams[0],
          "largest difference", float(np.abs(energies - base * norm).max()))
    assert np.all(np.diff(energies) <= tol)
    assert energies[-1] >= lams[0] - tol
    assert energies[-1] - lams[0] <= (base[-1] * norm - lams[0]) + tol


def test_projected_operator_on_the_result_applies_the_one_site_region():
    ops, init = tn.make_case("mixed3")
    r = tdvp(MPO(ops), SimpleTensorTrain(init), 0, TdvpOptions(order=1, exponent_step=TAU))
    x = r.state.site_tensors()
    norm = float(np.linalg.norm(tn.np_operator_full(ops), 2))
    po = ProjectedOperator(MPO(ops), r.state)
    for c in range(len(ops)):
        left, right = tn._left(ops, x, c), tn._right(ops, x, c + 1)
        y, _ = _apply_one_site(po, c, x[c])
        want = tn.np_one_site_apply(left, right, ops[c], x[c])
        assert np.linalg.norm(y - want) <= 1e-12 * norm * np.linalg.norm(x[c])
    # the last site is the centre after a first-order sweep from 0: <x_c|H_c x_c> is the energy of the whole state
    psi = tn.np_state_full(x)
    y, _ = _apply_one_site(po, len(ops) - 1, x[-1])
    assert abs(float(np.sum(x[-1] * y)) - float(psi @ (tn.np_operator_full(ops) @ psi))) <= 1e-12 * norm * float(psi @ psi)


def test_errors_come_from_the_public_call():
    ops, init = tn.make_case("heis6")
    for center, text in ((2, "center 2 is an inner node of the chain"), (6, "TDVP center 6 is not a state node")):
        with pytest.raises(t4a_amd.T4aError) as e:
            tdvp(MPO(ops), SimpleTensorTrain(init), center)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and text in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp(MPO(ops), SimpleTensorTrain(init), 0, TdvpOptions(exponent_step=-0.1j))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "complex tensor trains" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp(MPO(ops), SimpleTensorTrain(init), 0, TdvpOptions(nsite=1))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "nsite=1" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp(MPO(tn.tfim(5, 0.7)), SimpleTensorTrain(init), 0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "lengths differ" in e.value.message
    nonsym = [t.copy() for t in ops]
    nonsym[2] = nonsym[2] + 0.3 * np.triu(np.ones((2, 2)), 1)[None, :, :, None]
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp(MPO(nonsym), SimpleTensorTrain(init), 0)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "projected operator is not Hermitian" in e.value.message
    # a step that does not converge within its time splits is an error with the reference's text
    with pytest.raises(t4a_amd.T4aError) as e:
        tdvp(MPO(ops), SimpleTensorTrain(init), 0, TdvpOptions(exponent_step=-0.5, krylov=HermitianKrylovExpmOptions(max_iter=1, max_time_splits=1)))
    assert e.value.code == t4a_amd.INTERNAL_ERROR and "did not converge within max_time_splits=1 and max_iter=1" in e.value.message
