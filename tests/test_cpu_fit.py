"""Variational (fit) MPO contraction without a GPU: the numpy restatement (tests/fit_np.py) against the dense product, the
options struct, the exported symbols, and the argument checks that are answered on the host before the device is touched."""
import ctypes

import numpy as np
import pytest

import fit_np
from fit_np import SEED, Options, random_tensors, np_fit, np_full, np_product, links, rel_error


# ------------------------------------------------------------------------------------------------ the restatement
def test_f1_one_sweep_from_a_random_guess_reaches_the_exact_product():
    a = random_tensors([1, 2, 3, 2, 1], 2, 2, SEED)
    b = random_tensors([1, 3, 2, 3, 1], 2, 2, SEED ^ 0xFF)
    guess = random_tensors([1, 4, 6, 4, 1], 2, 2, SEED ^ 0xABC)
    c, info = np_fit(a, b, Options(max_sweeps=1), guess)
    assert links(c) == [4, 6, 4] and info["n_sweeps"] == 1 and len(info["norms"]) == 2
    assert rel_error(np_full(c), np_product(a, b)) <= 1e-12


def test_f2_bonds_grow_from_a_guess_of_bond_one():
    a = random_tensors([1] + [3] * 5 + [1], 2, 2, SEED)
    b = random_tensors([1] + [2] * 5 + [1], 2, 2, SEED ^ 0xFF)
    guess = random_tensors([1] * 7, 2, 2, SEED ^ 0xABC)
    c, info = np_fit(a, b, Options(), guess)
    assert links(c) == [4, 6, 6, 6, 4]
    assert rel_error(np_full(c), np_product(a, b)) <= 1e-12
    assert len(info["norms"]) == info["n_sweeps"] + 1


def test_restatement_edge_cases():
    a = random_tensors([1, 2, 1], 2, 2, SEED)
    b = random_tensors([1, 3, 1], 2, 2, SEED ^ 0xFF)
    z = fit_np.np_zipup(a, b, Options())
    c, info = np_fit(a, b, Options(max_sweeps=0))
    assert info == {"n_sweeps": 0, "norms": []} and all(np.array_equal(x, y) for x, y in zip(c, z))
    x, y = random_tensors([1, 1], 3, 2, SEED), random_tensors([1, 1], 2, 4, SEED ^ 0xFF)
    one, info = np_fit(x, y, Options())
    assert info["n_sweeps"] == 0 and len(one) == 1 and one[0].shape == (1, 3, 4, 1)
    assert np.allclose(one[0][0, :, :, 0], x[0][0, :, :, 0] @ y[0][0, :, :, 0], rtol=0, atol=1e-15)
    assert np_fit([], [], Options()) == ([], {"n_sweeps": 0, "norms": []})


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_fit_options_default_matches_the_reference():
    import t4a_amd
    o = t4a_amd.FitOptionsC()
    assert t4a_amd._lib.t4a_gpu_mpo_fit_options_default(ctypes.byref(o)) == 0
    # FitOptions::default() (contract_fit.rs:36-46): 1e-12, Some(100), 10, 1e-10, SVD
    assert (o.tolerance, o.has_max_bond_dim, o.max_bond_dim, o.max_sweeps, o.convergence_tol, o.factorize_method) == \
        (1e-12, 1, 100, 10, 1e-10, t4a_amd.FactorizeMethod.SVD)
    d = t4a_amd.FitOptions().to_c()
    for name, _ in t4a_amd.FitOptionsC._fields_:
        assert getattr(d, name) == getattr(o, name), name
    n = t4a_amd.FitOptions(max_bond_dim=None).to_c()
    assert n.has_max_bond_dim == 0
    assert t4a_amd._lib.t4a_gpu_mpo_fit_options_default(None) == t4a_amd.NULL_POINTER


def test_symbols_are_exported():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("t4a_gpu_mpo_fit_options_default", "t4a_gpu_mpo_contract_fit", "t4a_gpu_mpo_fit_half"):
        assert hasattr(lib, name), name
    assert t4a_amd.contract_fit is t4a_amd.mpo.contract_fit and t4a_amd.FitOptions is t4a_amd.mpo.FitOptions


@pytest.mark.parametrize("field, value", [("tolerance", -1e-3), ("tolerance", float("nan")), ("tolerance", float("inf")),
                                          ("convergence_tol", -1.0), ("convergence_tol", float("nan")),
                                          ("convergence_tol", float("inf")), ("factorize_method", 4), ("factorize_method", -1)])
def test_bad_options_are_refused_before_an_operand_is_looked_at(field, value):
    """The operands are NULL: an answer other than INVALID_ARGUMENT would mean they were looked at first."""
    import t4a_amd
    o = t4a_amd.FitOptionsC()
    t4a_amd._lib.t4a_gpu_mpo_fit_options_default(ctypes.byref(o))
    setattr(o, field, value)
    h = ctypes.c_void_p()
    n = ctypes.c_size_t(7)
    st = t4a_amd._lib.t4a_gpu_mpo_contract_fit(None, None, ctypes.byref(o), None, ctypes.byref(h), ctypes.byref(n), None)
    assert st == t4a_amd.INVALID_ARGUMENT, t4a_amd.last_error_message()
    assert not h and n.value == 0
    if field != "factorize_method":
        assert field in t4a_amd.last_error_message()
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.FitOptions(**{field: value}).to_c()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and field in e.value.message


def test_null_arguments_and_python_side_checks():
    import t4a_amd
    o = t4a_amd.FitOptions().to_c()
    h = ctypes.c_void_p()
    lib = t4a_amd._lib
    assert lib.t4a_gpu_mpo_contract_fit(None, None, ctypes.byref(o), None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_mpo_contract_fit(None, None, None, None, ctypes.byref(h), None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_mpo_contract_fit(None, None, ctypes.byref(o), None, ctypes.byref(h), None, None) == t4a_amd.NULL_POINTER
    o.has_max_bond_dim, o.max_bond_dim = 1, 0
    assert lib.t4a_gpu_mpo_contract_fit(None, None, ctypes.byref(o), None, ctypes.byref(h), None, None) == t4a_amd.INVALID_ARGUMENT
    for kw in ({"max_bond_dim": 0}, {"max_sweeps": -1}, {"factorize_method": 9}):
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.FitOptions(**kw).to_c()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    # the test hook: side and the environment's size come before the handles
    env = np.ones(1)
    out = np.zeros(1)
    p = t4a_amd._p
    for n_env, side in ((1, 2), (1, -1), (0, 0)):
        st = lib.t4a_gpu_mpo_fit_half(p(env), ctypes.c_size_t(n_env), ctypes.c_int32(side), None, None, ctypes.c_size_t(0), p(out))
        assert st == t4a_amd.INVALID_ARGUMENT, (n_env, side)
    st = lib.t4a_gpu_mpo_fit_half(p(env), ctypes.c_size_t(1), ctypes.c_int32(0), None, None, ctypes.c_size_t(0), p(out))
    assert st == t4a_amd.NULL_POINTER
