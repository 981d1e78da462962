"""Two-site DMRG without a GPU: the numpy restatement (tests/dmrg_np.py) against dense eigensolves — it is the yardstick of the device
tests, so the conditions on its inputs (a symmetric operator, a unique ground state) and its own accuracy come first —, the options
struct, the exported symbols, and the argument checks answered on the host before the device is touched."""
import ctypes

import numpy as np
import pytest

import dmrg_np as dn
from dmrg_np import CASES, UNTRUNCATED, LanczosOptions, Options, np_dmrg, np_energy, np_lanczos


# ------------------------------------------------------------------------------------------------ the inputs and the sweeps of the restatement
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_is_symmetric_and_the_ground_state_unique(name):
    h, lams, _, norm = dn.dense_spectrum(name)
    assert np.array_equal(h, h.T)
    gap = (lams[1] - lams[0]) / norm
    print(name, "relative gap", gap, "E0", lams[0])
    assert gap >= 1e-3


@pytest.mark.parametrize("name", UNTRUNCATED)
def test_untruncated_sweeps_reach_the_dense_ground_energy(name):
    """A unit vector's Rayleigh quotient lies within its residual of an eigenvalue and the local residuals are <= rtol max(1, |lambda|):
    1e-10 max(1, ||H||_2) after 2 sweeps."""
    _, lams, ground, norm = dn.dense_spectrum(name)
    r = dn.restated(name, 2)
    print(name, "E - E0", r["energy"] - lams[0], "max residual", r["max_residual_norm"])
    assert abs(r["energy"] - lams[0]) <= 1e-10 * max(1.0, norm)
    n = len(CASES[name][0])
    assert r["sweeps_completed"] == 2 and r["local_updates"] == 2 * 2 * (n - 1) and not r["converged"]
    assert r["max_residual_norm"] <= r["max_threshold"]
    psi = dn.np_state_full(r["state"])
    assert abs(psi @ ground) / np.linalg.norm(psi) >= 1 - 1e-8
    ops, _, center, _ = dn.make_case(name)
    assert abs(np_energy(ops, r["state"], center) - r["energy"]) <= 1e-12 * norm
    assert abs(np_energy(ops, r["state"], 0) - r["energy"]) <= 1e-12 * norm


def test_capped_sweeps_stay_above_the_ground_energy_and_within_the_cap():
    _, lams, _, norm = dn.dense_spectrum("tfim8_cap4")
    r = dn.restated("tfim8_cap4", 6)
    print("tfim8_cap4: E - E0 per sweep", [e - lams[0] for e in r["history"]])
    assert r["energy"] >= lams[0] - 1e-10 * norm
    assert max(t.shape[2] for t in r["state"][:-1]) <= 4
    assert len(r["history"]) == 6 and max(abs(np.diff(r["history"][2:]))) <= 1e-10  # a converged fixed point: the scale of the device comparison


def test_exact_local_solves_and_the_energy_tolerance():
    ops, init, center, _ = dn.make_case("heis6_c3")
    _, lams, _, norm = dn.dense_spectrum("heis6_c3")
    r = np_dmrg(ops, init, center, Options(nsweeps=1), exact_local=True)
    assert abs(r["energy"] - lams[0]) <= 1e-12 * norm
    r = np_dmrg(ops, init, center, Options(nsweeps=10, energy_tol=1e-9))
    assert r["converged"] and 2 <= r["sweeps_completed"] < 10 and abs(r["energy"] - lams[0]) <= 1e-10 * norm
    r = np_dmrg(ops, init, center, Options(nsweeps=2, lanczos=LanczosOptions(max_iter=2)))
    assert r["sweeps_completed"] == 2 and r["max_residual_norm"] > r["max_threshold"] and r["energy"] >= lams[0] - 1e-10 * norm
    with pytest.raises(ValueError):
        np_dmrg(ops[:1], init[:1])
    zero = [np.zeros_like(t) for t in init]
    with pytest.raises(ValueError):
        np_dmrg(ops, zero, center)


# ------------------------------------------------------------------------------------------------ Lanczos of the restatement
def run_dense(name):
    h, v0, o, _ = dn.dense_cases()[name]
    lam, vec, it, res, conv = np_lanczos(lambda v: h @ v, v0, o)
    return h, o, lam, vec, it, res, conv


def test_lanczos_identity_ends_at_the_first_step():
    h, o, lam, vec, it, res, conv = run_dense("identity")
    assert conv and it == 1 and lam == 1.0 and res <= 1e-15 and abs(np.linalg.norm(vec) - 1) <= 1e-15


def test_lanczos_three_distinct_eigenvalues_break_down_after_three_steps():
    h, o, lam, vec, it, res, conv = run_dense("diag3")
    assert conv and it == 3 and abs(lam - 1.0) <= 1e-14 and res <= 1e-14


def test_lanczos_eigenvector_start_takes_one_step():
    h, o, lam, vec, it, res, conv = run_dense("eigenvector_start")
    assert conv and it == 1 and abs(lam - np.linalg.eigvalsh(h)[0]) <= 1e-14 and res <= 1e-14
    assert abs(np.linalg.norm(vec) - 1) <= 1e-15  # the start had norm 2.5


def test_lanczos_general_matrices_and_the_flag():
    for name in ("symmetric12", "symmetric40"):
        h, o, lam, vec, it, res, conv = run_dense(name)
        assert conv and res <= o.threshold(lam) and abs(lam - np.linalg.eigvalsh(h)[0]) <= o.threshold(lam)
        assert abs(np.linalg.norm(h @ vec - lam * vec) - res) <= 1e-14 and abs(np.linalg.norm(vec) - 1) <= 1e-13
    h, o, lam, vec, it, res, conv = run_dense("max_iter_2")
    assert not conv and it == 2 and res > o.threshold(lam) and abs(np.linalg.norm(vec) - 1) <= 1e-14  # a flag, no error
    assert lam >= np.linalg.eigvalsh(h)[0]


def test_lanczos_refuses_a_nonsymmetric_matrix_and_a_zero_start():
    h, v0 = dn.nonsymmetric_case()
    with pytest.raises(ValueError, match="not Hermitian"):
        np_lanczos(lambda v: h @ v, v0)
    with pytest.raises(ValueError, match="zero"):
        np_lanczos(lambda v: v, np.zeros(4))


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_options_default_matches_the_reference():
    import t4a_amd
    o = t4a_amd.DmrgOptionsC()
    assert t4a_amd._lib.t4a_gpu_dmrg_options_default(ctypes.byref(o)) == 0
    assert (o.nsite, o.nsweeps, o.has_max_bond_dim, o.has_svd_policy, o.has_energy_tol, o.real_scalar_tol) == (2, 5, 0, 0, 0, 1e-10)
    assert (o.lanczos.max_iter, o.lanczos.rtol, o.lanczos.atol, o.lanczos.breakdown_tol, o.lanczos.hermitian_tol) == (64, 1e-10, 0.0, 1e-14, 1e-10)
    d = t4a_amd.DmrgOptions().to_c()
    for name, _ in t4a_amd.DmrgOptionsC._fields_:
        if name not in ("svd_policy", "lanczos"):
            assert getattr(d, name) == getattr(o, name), name
    for name, _ in t4a_amd.LanczosOptionsC._fields_:
        assert getattr(d.lanczos, name) == getattr(o.lanczos, name), name
    assert (d.svd_policy.threshold, d.svd_policy.scale, d.svd_policy.measure, d.svd_policy.rule) == \
        (o.svd_policy.threshold, o.svd_policy.scale, o.svd_policy.measure, o.svd_policy.rule) == (1e-12, 0, 0, 0)
    assert t4a_amd._lib.t4a_gpu_dmrg_options_default(None) == t4a_amd.NULL_POINTER


def test_symbols_are_exported():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("dmrg_options_default", "dmrg_check_shapes", "dmrg", "dmrg_energy", "lanczos_dense", "krylov_combine", "eig_residual",
                 "lanczos_time_finalise"):
        assert hasattr(lib, "t4a_gpu_" + name), name
    from t4a_amd.dmrg import dmrg, dmrg_energy, _lanczos_dense, _krylov_combine, _eig_residual  # noqa: F401
    assert t4a_amd.dmrg is dmrg and t4a_amd.dmrg_energy is dmrg_energy and t4a_amd.DmrgResult is t4a_amd.dmrg_module.DmrgResult


INF, NAN = float("inf"), float("nan")
def _tolerance_refusals(field, message):
    return [(field, v, message) for v in (-1e-3, NAN, INF, -INF)]


BAD_OPTIONS = ([("nsite", 1, "DMRG supports only nsite=2 in this version, got nsite=1"),
                ("nsite", 3, "DMRG supports only nsite=2 in this version, got nsite=3"),
                ("nsweeps", 0, "invalid DMRG option nsweeps: must be greater than zero"),
                ("max_bond_dim", 0, "invalid DMRG option max_bond_dim: must be greater than zero when set"),
                ("lanczos.max_iter", 0, "max_iter must be greater than zero"),
                ("lanczos.max_iter", 8192, "max_iter above 8191 is not supported")]
               + _tolerance_refusals("energy_tol", "invalid DMRG option energy_tol: must be finite and non-negative")
               + _tolerance_refusals("real_scalar_tol", "invalid DMRG option real_scalar_tol: must be finite and non-negative")
               + _tolerance_refusals("lanczos.rtol", "rtol must be finite and non-negative")
               + _tolerance_refusals("lanczos.atol", "atol must be finite and non-negative")
               + _tolerance_refusals("lanczos.breakdown_tol", "breakdown_tol must be finite and non-negative")
               + _tolerance_refusals("lanczos.hermitian_tol", "hermitian_tol must be finite and non-negative"))


@pytest.mark.parametrize("field, value, message", BAD_OPTIONS, ids=["%s=%s" % (f, v) for f, v, _ in BAD_OPTIONS])
def test_bad_options_are_refused_before_an_operand_is_looked_at(field, value, message):
    """The operands are NULL: an answer other than INVALID_ARGUMENT would mean they were looked at first."""
    import t4a_amd
    o = t4a_amd.DmrgOptionsC()
    t4a_amd._lib.t4a_gpu_dmrg_options_default(ctypes.byref(o))
    if field == "energy_tol":
        o.has_energy_tol = 1
    if field == "max_bond_dim":
        o.has_max_bond_dim = 1
    if field.startswith("lanczos."):
        setattr(o.lanczos, field.split(".")[1], value)
    else:
        setattr(o, field, value)
    h = ctypes.c_void_p()
    st = t4a_amd._lib.t4a_gpu_dmrg(None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.byref(h), None, None, None, None, None, None)
    assert st == t4a_amd.INVALID_ARGUMENT, t4a_amd.last_error_message()
    assert not h and message in t4a_amd.last_error_message()


def check_shapes(op, state, center=0, max_iter=64):
    import t4a_amd
    op, state = np.array(op, dtype=np.uintp).reshape(-1), np.array(state, dtype=np.uintp).reshape(-1)
    st = t4a_amd._lib.t4a_gpu_dmrg_check_shapes(t4a_amd._p(op), ctypes.c_size_t(len(op) // 4), t4a_amd._p(state), ctypes.c_size_t(len(state) // 3),
                                                ctypes.c_size_t(center), ctypes.c_size_t(max_iter))
    return st, t4a_amd.last_error_message()


def test_shape_checks_need_no_device():
    import t4a_amd
    op = [(1, 2, 2, 3), (3, 3, 3, 3), (3, 2, 2, 1)]
    tt = [(1, 2, 4), (4, 3, 4), (4, 2, 1)]
    assert check_shapes(op, tt)[0] == 0
    assert check_shapes(op, tt, center=2)[0] == 0
    bad = t4a_amd.INVALID_ARGUMENT
    st, msg = check_shapes(op[:1], [(1, 2, 1)])
    assert st == bad and "two-site DMRG requires at least one state edge" in msg
    st, msg = check_shapes(op[:2], tt)
    assert st == bad and "lengths differ" in msg
    st, msg = check_shapes(op, tt[:2])
    assert st == bad and "lengths differ" in msg
    st, msg = check_shapes([(1, 2, 3, 3)] + op[1:], tt)
    assert st == bad and "not square" in msg and "site 0" in msg
    st, msg = check_shapes(op, [(1, 2, 4), (4, 2, 4), (4, 2, 1)])
    assert st == bad and "site 1" in msg and "state" in msg
    st, msg = check_shapes(op, tt, center=3)
    assert st == bad and "center 3" in msg
    # W N^2 = 3 * (3 * 20000)^2 > INT_MAX at the bond (0, 1)
    big = [(1, 2, 4), (4, 3, 20000), (20000, 2, 1)]
    st, msg = check_shapes(op, big)
    assert st == bad and "INT_MAX" in msg and "(0, 1)" in msg and msg.startswith("dmrg")
    # the Lanczos basis: (max_iter + 1) M N with M = N = 900 at the bond (1, 2) fits for max_iter = 2 and not for 8191
    op4 = [op[0], op[1], op[1], op[2]]
    wide = [(1, 2, 300), (300, 3, 300), (300, 3, 300), (300, 2, 1)]
    assert check_shapes(op4, wide, max_iter=2)[0] == 0
    st, msg = check_shapes(op4, wide, max_iter=8191)
    assert st == bad and "INT_MAX" in msg and "(1, 2)" in msg
    st, msg = check_shapes(op, tt, max_iter=0)
    assert st == bad and "max_iter must be greater than zero" in msg
    st, msg = check_shapes(op, tt, max_iter=8192)
    assert st == bad and "max_iter above 8191" in msg


def test_null_arguments_and_python_side_checks():
    import t4a_amd
    lib = t4a_amd._lib
    o = t4a_amd.DmrgOptions().to_c()
    h = ctypes.c_void_p()
    zero = ctypes.c_size_t(0)
    assert lib.t4a_gpu_dmrg(None, None, zero, ctypes.byref(o), None, None, None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_dmrg(None, None, zero, None, ctypes.byref(h), None, None, None, None, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_dmrg(None, None, zero, ctypes.byref(o), ctypes.byref(h), None, None, None, None, None, None) == t4a_amd.NULL_POINTER
    v = ctypes.c_double(0)
    assert lib.t4a_gpu_dmrg_energy(None, None, zero, ctypes.byref(v)) == t4a_amd.NULL_POINTER
    for kw in ({"max_bond_dim": 0}, {"nsweeps": -1}, {"svd_policy": 1e-8}, {"lanczos": 64}):
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.DmrgOptions(**kw).to_c()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.dmrg(None, None)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    # the test hooks: sizes and options come before the pointers and the device
    one = np.ones(1)
    p = t4a_amd._p
    it, conv = ctypes.c_size_t(0), ctypes.c_int32(0)
    lo = t4a_amd.HermitianLanczosOptions(max_iter=0).to_c()
    assert lib.t4a_gpu_lanczos_dense(p(one), ctypes.c_size_t(1), p(one), ctypes.byref(lo), ctypes.byref(v), p(one), ctypes.byref(it), ctypes.byref(v),
                                     ctypes.byref(conv)) == t4a_amd.INVALID_ARGUMENT
    lo = t4a_amd.HermitianLanczosOptions().to_c()
    assert lib.t4a_gpu_lanczos_dense(p(one), zero, p(one), ctypes.byref(lo), ctypes.byref(v), p(one), ctypes.byref(it), ctypes.byref(v),
                                     ctypes.byref(conv)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_lanczos_dense(None, ctypes.c_size_t(1), p(one), ctypes.byref(lo), ctypes.byref(v), p(one), ctypes.byref(it), ctypes.byref(v),
                                     ctypes.byref(conv)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_krylov_combine(p(one), zero, ctypes.c_size_t(1), p(one), p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_krylov_combine(p(one), ctypes.c_size_t(1), ctypes.c_size_t(8192), p(one), p(one), ctypes.byref(v)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_krylov_combine(None, ctypes.c_size_t(1), ctypes.c_size_t(1), p(one), p(one), ctypes.byref(v)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_eig_residual(p(one), p(one), zero, ctypes.c_double(1.0), None, p(one)) == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_eig_residual(p(one), None, ctypes.c_size_t(1), ctypes.c_double(1.0), None, p(one)) == t4a_amd.NULL_POINTER
