"""Variational (fit) contraction of two MPOs on the device (t4a_gpu_mpo_contract_fit) against the numpy restatement of
tests/fit_np.py and the dense product.  Link dimensions and sweep counts are compared exactly, dense results at 1e-10 (this
layer's device-against-numpy tolerance, tests/test_gpu_mpo.py)."""
import functools

import numpy as np
import pytest

import t4a_amd
from t4a_amd import mpo, MPO, ContractionOptions, ContractionAlgorithm, FactorizeMethod, FitOptions, contract_fit
from fit_np import SEED, Options, random_tensors, np_fit, np_full, np_product, links, rel_error

pytestmark = pytest.mark.gpu

A8 = [1, 4, 16, 16, 16, 16, 16, 4, 1]
B8 = [1] + [3] * 7 + [1]


@functools.lru_cache(maxsize=None)
def operators(bonds_a, bonds_b):
    """(a, b, dense product) of LCG operators with site dims (2, 2); computed once, never written to"""
    a = random_tensors(list(bonds_a), 2, 2, SEED)
    b = random_tensors(list(bonds_b), 2, 2, SEED ^ 0xFF)
    return a, b, np_product(a, b)


def guess(bonds):
    return random_tensors(bonds, 2, 2, SEED ^ 0xABC)


def close(got, want, rel=1e-10):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    scale = max(1.0, float(np.abs(want).max()) if want.size else 1.0)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= rel * scale, f"max deviation {err:.3e} at scale {scale:.3e}"


def test_f1_one_sweep_from_a_random_guess():
    a, b, dense = operators((1, 2, 3, 2, 1), (1, 3, 2, 3, 1))
    r, info = contract_fit(MPO(a), MPO(b), FitOptions(max_sweeps=1), initial=MPO(guess([1, 4, 6, 4, 1])), return_info=True)
    assert r.link_dims() == [4, 6, 4] == info["link_dims"]
    assert info["n_sweeps"] == 1 and len(info["norms"]) == 2
    assert r.site_dims() == [(2, 2)] * 4
    close(r.full_tensor(), dense)


def test_f2_bonds_grow_from_a_guess_of_bond_one():
    a, b, dense = operators((1, 3, 3, 3, 3, 3, 1), (1, 2, 2, 2, 2, 2, 1))
    g = guess([1] * 7)
    r, info = contract_fit(MPO(a), MPO(b), initial=MPO(g), return_info=True)
    want, winfo = np_fit(a, b, Options(), g)
    assert r.link_dims() == [4, 6, 6, 6, 4] == links(want)
    assert info["n_sweeps"] == winfo["n_sweeps"]
    close(info["norms"], winfo["norms"])
    close(r.full_tensor(), dense)


def test_f3_untruncated_fit_reaches_the_exact_bonds_zipup_misses():
    a, b, dense = operators(tuple(A8), tuple(B8))
    ma, mb = MPO(a), MPO(b)
    z = t4a_amd.contract_zipup(ma, mb, ContractionOptions())
    assert z.link_dims() == [4, 16, 48, 48, 48, 48, 12]
    r, info = contract_fit(ma, mb, FitOptions(max_bond_dim=None), return_info=True)
    assert r.link_dims() == [4, 16, 48, 48, 48, 16, 4]
    assert info["n_sweeps"] == 1
    close(r.full_tensor(), dense)
    # the centre is back on site 0: every other site is right-orthogonal
    for t in r.site_tensors()[1:]:
        m = t.reshape((t.shape[0], -1), order="F")
        assert np.abs(m @ m.T - np.eye(t.shape[0])).max() <= 1e-9
    r = contract_fit(ma, mb, FitOptions(max_bond_dim=None), initial=MPO(guess([1] + [4] * 7 + [1])))
    assert r.link_dims() == [4, 16, 48, 48, 48, 16, 4]
    close(r.full_tensor(), dense)


# The relative error of the truncated fit, device against restatement (LAPACK SVD there, one-sided Jacobi here).  Measured on an
# MI355X the two agree to the last bit (both 0.29804314761942141): the deviation is below one unit in the last place of the error,
# 2^-54 = 5.6e-17 (C sits at a stationary point of the error, so rounding differences enter at second order).  The bound is ten
# times that ("Variational fit"), far below the 1e-8 it may not exceed.
F4_MEASURED_DEVIATION = 2.0 ** -54
F4_BOUND = min(10 * F4_MEASURED_DEVIATION, 1e-8)


def test_f4_truncated_fit_beats_zipup_at_the_same_cap():
    a, b, dense = operators(tuple(A8), tuple(B8))
    ma, mb = MPO(a), MPO(b)
    r, info = contract_fit(ma, mb, FitOptions(max_bond_dim=20, max_sweeps=2, convergence_tol=0.0), return_info=True)
    want, winfo = np_fit(a, b, Options(max_bond_dim=20, max_sweeps=2, convergence_tol=0.0))
    assert r.link_dims() == links(want) == [4, 16, 20, 20, 20, 16, 4]
    assert info["n_sweeps"] == 2 == winfo["n_sweeps"]
    err = rel_error(r.full_tensor(), dense)
    err_np = rel_error(np_full(want), dense)
    z = t4a_amd.contract_zipup(ma, mb, ContractionOptions(max_bond_dim=20))
    err_zip = rel_error(z.full_tensor(), dense)
    print(f"F4: fit {err:.17g} restatement {err_np:.17g} deviation {abs(err - err_np):.3e} zip-up {err_zip:.6f} "
          f"norms {info['norms']} / {winfo['norms']}")
    assert err < err_zip
    assert abs(err_np - 0.298) < 1e-3 and abs(err_zip - 0.667) < 1e-3
    assert abs(err - err_np) <= F4_BOUND


def test_f5_operator_times_state_untruncated():
    n = 10
    cores = [c[:, :, 0, :] for c in random_tensors([1, 2, 4] + [8] * (n - 5) + [4, 2, 1], 2, 1, SEED)]
    assert max(c.shape[2] for c in cores) == 8
    psi = MPO.from_tensor_train(t4a_amd.SimpleTensorTrain(cores))
    op = t4a_amd.shift_operator(n, 3, t4a_amd.BoundaryCondition.Periodic).mpo()
    want = t4a_amd.contract_naive(op, psi)
    r = contract_fit(op, psi, FitOptions(max_bond_dim=None))
    assert r.site_dims() == [(2, 1)] * n
    assert max(r.link_dims()) <= 16  # operator bond 2 times state bond 8
    close(r.full_tensor(), want.full_tensor())


def test_f6_edge_cases():
    a, b, dense = operators((1, 2, 3, 2, 1), (1, 3, 2, 3, 1))
    ma, mb = MPO(a), MPO(b)
    # max_sweeps == 0: the zip-up product, or the guess, as it is
    r, info = contract_fit(ma, mb, FitOptions(max_sweeps=0), return_info=True)
    z = t4a_amd.contract_zipup(ma, mb, ContractionOptions(max_bond_dim=100))
    assert info == {"n_sweeps": 0, "norms": [], "link_dims": z.link_dims()}
    for x, y in zip(r.site_tensors(), z.site_tensors()):
        assert np.array_equal(x, y)
    g = guess([1, 2, 2, 2, 1])
    r = contract_fit(ma, mb, FitOptions(max_sweeps=0), initial=MPO(g))
    for x, y in zip(r.site_tensors(), g):
        assert np.array_equal(x, y)
    # one site: the exact product, no sweep; no site: the empty MPO
    x, y = random_tensors([1, 1], 3, 2, SEED), random_tensors([1, 1], 2, 4, SEED ^ 0xFF)
    r, info = contract_fit(MPO(x), MPO(y), return_info=True)
    assert len(r) == 1 and info["n_sweeps"] == 0 and r.site_dims() == [(3, 4)]
    close(r.site_tensor(0)[0, :, :, 0], x[0][0, :, :, 0] @ y[0][0, :, :, 0], rel=1e-14)
    r, info = contract_fit(MPO([]), MPO([]), return_info=True)
    assert len(r) == 0 and info["n_sweeps"] == 0 and r.link_dims() == []
    # LU and CI fall back to SVD
    r = contract_fit(ma, mb, FitOptions(factorize_method=FactorizeMethod.LU))
    close(r.full_tensor(), dense)


def test_f6_error_answers():
    a, b, _ = operators((1, 2, 3, 2, 1), (1, 3, 2, 3, 1))
    ma, mb = MPO(a), MPO(b)
    with pytest.raises(t4a_amd.T4aError) as e:
        contract_fit(ma, MPO.constant([(2, 2)] * 3, 1.0))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "length mismatch: expected 4, got 3" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        contract_fit(MPO.constant([(2, 3)], 1.0), MPO.constant([(2, 2)], 1.0))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "site_dim_2=3" in e.value.message and "site_dim_1=2" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        contract_fit(ma, mb, initial=MPO(guess([1, 2, 2, 1])))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "initial has 3 sites" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        contract_fit(ma, mb, initial=MPO(random_tensors([1, 2, 2, 2, 1], 2, 3, SEED)))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "site dims (2, 3) at site 0" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        contract_fit(ma, mb, FitOptions(factorize_method=FactorizeMethod.RSVD))
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED and "RSVD factorization not yet implemented" in e.value.message
    for kw in ({"tolerance": -1.0}, {"tolerance": float("nan")}, {"convergence_tol": -1e-3}, {"convergence_tol": float("inf")}):
        with pytest.raises(t4a_amd.T4aError) as e:
            contract_fit(ma, mb, FitOptions(**kw))
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    # the dispatcher keeps the reference's answer
    with pytest.raises(t4a_amd.T4aError) as e:
        mpo.contract(ma, mb, ContractionAlgorithm.Fit)
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED
