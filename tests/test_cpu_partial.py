"""Partial contraction of two MPOs without a GPU: the host plan (t4a_gpu_mpo_partial_plan) with every error message, the numpy
restatement (tests/partial_np.py) against the existing restatements on the matrix-product spec and against dense einsums, and the
gap condition for every operand set tests/test_gpu_partial.py compares ranks on."""
import ctypes

import numpy as np
import pytest

import fit_np
import partial_np as pn
from partial_np import SEED, Options, random_tensors, np_full, links


def dense(ts):
    """[i1, j1, i2, j2, ...] of site tensors [l, s, t, r]"""
    return np_full(ts)


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_tables_of_the_named_specs():
    import t4a_amd
    from t4a_amd import PartialContractionSpec as Spec, partial_plan
    a, b = [(2, 3), (4, 3)], [(3, 5), (3, 2)]
    p = partial_plan(a, b, Spec.matrix_product(2))
    assert p == {"site_dims": [(2, 5), (4, 2)], "s_legs": [[2], [4]], "t_legs": [[5], [2]]}
    p = partial_plan([(2, 3)] * 3, [(2, 3)] * 3, Spec.hadamard(3))
    assert p == {"site_dims": [(6, 1)] * 3, "s_legs": [[2, 3]] * 3, "t_legs": [[]] * 3}
    p = partial_plan(a, b, Spec())  # nothing paired: the outer product
    assert p == {"site_dims": [(6, 15), (12, 6)], "s_legs": [[2, 3], [4, 3]], "t_legs": [[3, 5], [3, 2]]}
    # f(x, y) g(y, z) with y kept at site 0 and summed at site 1
    p = partial_plan(a, b, Spec(contract_pairs=[((1, 1), (1, 0))], diagonal_pairs=[((0, 1), (0, 0))]))
    assert p == {"site_dims": [(6, 5), (4, 2)], "s_legs": [[2, 3], [4]], "t_legs": [[5], [2]]}
    # all legs contracted: site dims (1, 1)
    p = partial_plan([(2, 3)], [(3, 2)], Spec(contract_pairs=[((0, 0), (0, 1)), ((0, 1), (0, 0))]))
    assert p == {"site_dims": [(1, 1)], "s_legs": [[]], "t_legs": [[]]}
    assert partial_plan([], [], Spec()) == {"site_dims": [], "s_legs": [], "t_legs": []}
    assert t4a_amd.partial.hadamard is t4a_amd.hadamard and t4a_amd.partial_contract is t4a_amd.partial.partial_contract


def test_plan_agrees_with_the_restatement():
    from t4a_amd import PartialContractionSpec as Spec, partial_plan
    rng = np.random.default_rng(1)
    legs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for _ in range(60):
        n = int(rng.integers(1, 4))
        a = [tuple(int(x) for x in rng.integers(2, 4, 2)) for _ in range(n)]
        b = [tuple(int(x) for x in rng.integers(2, 4, 2)) for _ in range(n)]
        contract, diagonal = [], []
        for i in range(n):
            for la, lb in (legs[k] for k in rng.permutation(4)[:2]):
                kind = int(rng.integers(0, 3))
                if kind < 2 and a[i][la] == b[i][lb] and all((i, la) != p[0] and (i, lb) != p[1] for p in contract + diagonal):
                    (contract if kind == 0 else diagonal).append(((i, la), (i, lb)))
        want = pn.np_plan(a, b, contract, diagonal)
        got = partial_plan(a, b, Spec(contract, diagonal))
        assert got["site_dims"] == [(p.S, p.T) for p in want]
        assert got["s_legs"] == [p.s_dims for p in want] and got["t_legs"] == [p.t_dims for p in want]


ERRORS = [
    # (a dims, b dims, contract, diagonal, code, message)
    ([(2, 3)], [(3, 2)], [((0, 0), (0, 0))], [], "INVALID_ARGUMENT", "partial_contract: contract_pairs index shape mismatch: 2 != 3"),
    ([(2, 3)], [(3, 2)], [], [((0, 1), (0, 1))], "INVALID_ARGUMENT", "partial_contract: diagonal_pairs index shape mismatch: 3 != 2"),
    ([(2, 2)], [(2, 2)], [((0, 0), (0, 0))], [((0, 0), (0, 1))], "INVALID_ARGUMENT",
     "partial_contract: first MPO index (site 0, leg 0) appears in multiple pairs"),
    ([(2, 2)], [(2, 2)], [((0, 0), (0, 1)), ((0, 1), (0, 1))], [], "INVALID_ARGUMENT",
     "partial_contract: second MPO index (site 0, leg 1) appears in multiple pairs"),
    ([(2, 2)], [(2, 2)], [((1, 0), (0, 0))], [], "INVALID_ARGUMENT",
     "partial_contract: (site 1, leg 0) from contract_pairs not found in first MPO external indices"),
    ([(2, 2)], [(2, 2)], [((0, 2), (0, 0))], [], "INVALID_ARGUMENT",
     "partial_contract: (site 0, leg 2) from contract_pairs not found in first MPO external indices"),
    ([(2, 2)], [(2, 2)], [], [((0, 0), (0, 2))], "INVALID_ARGUMENT",
     "partial_contract: (site 0, leg 2) from diagonal_pairs not found in second MPO external indices"),
    ([(2, 2)], [(2, 2)], [], [((0, 0), (3, 0))], "INVALID_ARGUMENT",
     "partial_contract: (site 3, leg 0) from diagonal_pairs not found in second MPO external indices"),
    ([(2, 2), (2, 2)], [(2, 2)], [], [], "INVALID_ARGUMENT", "MPO length mismatch: expected 2, got 1"),
    ([(2, 2), (2, 2)], [(2, 2), (2, 2)], [((0, 1), (1, 0))], [], "NOT_IMPLEMENTED",
     "partial_contract: the pair (site 0, leg 1) - (site 1, leg 0) joins two sites; moving a site index (swap_site_indices) is not implemented"),
    ([(300, 300)], [(2, 2)], [], [], "INVALID_ARGUMENT", "partial_contract: site 0: dimensions above 65535 are not supported"),
]


@pytest.mark.parametrize("a, b, contract, diagonal, code, message", ERRORS, ids=[e[5][:60] for e in ERRORS])
def test_every_error_of_the_plan(a, b, contract, diagonal, code, message):
    import t4a_amd
    from t4a_amd import PartialContractionSpec as Spec, partial_plan
    with pytest.raises(t4a_amd.T4aError) as e:
        partial_plan(a, b, Spec(contract, diagonal))
    assert e.value.code == getattr(t4a_amd, code) and e.value.message == message
    # the restatement answers the same
    with pytest.raises((pn.PlanError, NotImplementedError)) as e2:
        pn.np_plan(a, b, contract, diagonal)
    assert str(e2.value) == message and isinstance(e2.value, NotImplementedError) == (code == "NOT_IMPLEMENTED")


def test_output_order_and_malformed_pairs():
    import t4a_amd
    from t4a_amd import PartialContractionSpec as Spec, partial_plan
    with pytest.raises(t4a_amd.T4aError) as e:
        partial_plan([(2, 2)], [(2, 2)], Spec(output_order=[(0, 0)]))
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED
    assert e.value.message == "partial_contract: output_order is not implemented (it needs swap_site_indices)"
    with pytest.raises(NotImplementedError):
        pn.np_plan([(2, 2)], [(2, 2)], output_order=[(0, 0)])
    # an invalid pair is answered before output_order
    with pytest.raises(t4a_amd.T4aError) as e:
        partial_plan([(2, 2)], [(2, 3)], Spec(contract_pairs=[((0, 0), (0, 1))], output_order=[]))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "shape mismatch: 2 != 3" in e.value.message
    for bad in ([(0, 0)], [((0, 0), (0,))], [((0, -1), (0, 0))], [((0, "x"), (0, 0))]):
        with pytest.raises(t4a_amd.T4aError) as e:
            Spec(contract_pairs=bad)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
    with pytest.raises(t4a_amd.T4aError) as e:
        partial_plan([(2, 2)], [(2, 2)], "hadamard")
    assert e.value.code == t4a_amd.INVALID_ARGUMENT


def test_symbols_and_null_arguments():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("t4a_gpu_mpo_partial_plan", "t4a_gpu_mpo_partial_contract", "t4a_gpu_mpo_partial_contract_fit", "t4a_gpu_mpo_partial_half",
                 "t4a_gpu_mpo_relabel_site_dims"):
        assert hasattr(lib, name), name
    lib, p, z = t4a_amd._lib, t4a_amd._p, ctypes.c_size_t(0)
    h = ctypes.c_void_p()
    args = (None, z, None, z, z)
    assert lib.t4a_gpu_mpo_partial_contract(None, None, *args, ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_double(0.0),
                                            z, ctypes.byref(h)) == t4a_amd.NULL_POINTER
    o = t4a_amd.FitOptions().to_c()
    assert lib.t4a_gpu_mpo_partial_contract_fit(None, None, *args, ctypes.byref(o), None, ctypes.byref(h), None, None) == t4a_amd.NULL_POINTER
    o.tolerance = -1.0  # the options are checked before an operand is looked at
    assert lib.t4a_gpu_mpo_partial_contract_fit(None, None, *args, ctypes.byref(o), None, ctypes.byref(h), None, None) == t4a_amd.INVALID_ARGUMENT
    env, out = np.ones(1), np.zeros(1)
    for n_env, side in ((1, 2), (0, 0)):
        st = lib.t4a_gpu_mpo_partial_half(p(env), ctypes.c_size_t(n_env), ctypes.c_int32(side), None, None, None, z, None, z, z, p(out))
        assert st == t4a_amd.INVALID_ARGUMENT
    assert lib.t4a_gpu_mpo_partial_half(p(env), ctypes.c_size_t(1), ctypes.c_int32(0), None, None, None, z, None, z, z, p(out)) == t4a_amd.NULL_POINTER
    # a pair count without its array
    assert lib.t4a_gpu_mpo_partial_plan(None, z, None, z, None, ctypes.c_size_t(1), None, z, z, None, None) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_mpo_relabel_site_dims(None, None, z) == t4a_amd.NULL_POINTER


# ------------------------------------------------------------------------------------------------ the restatement
def test_matrix_product_spec_equals_the_existing_restatements():
    from test_gpu_mpo import np_naive
    a = random_tensors([1, 3, 4, 3, 1], 2, 3, SEED)
    b = random_tensors([1, 2, 3, 2, 1], 3, 2, SEED ^ 0xFF)
    plan = pn.plan_for(a, b, contract_pairs=pn.matrix_product_pairs(4))
    for x, y in zip(pn.np_partial_naive(a, b, plan), np_naive(a, b)):
        assert np.array_equal(x, y)
    for o in (Options(1e-12, None), Options(1e-3, 4)):
        # (np_naive's QR / SVD bookkeeping is its own copy of the same steps: the same matrices go into the same LAPACK calls)
        for x, y in zip(pn.np_partial_naive(a, b, plan, o), np_naive(a, b, o)):
            assert x.shape == y.shape and np.abs(x - y).max() <= 1e-13
        for x, y in zip(pn.np_partial_zipup(a, b, plan, o), fit_np.np_zipup(a, b, o)):
            assert x.shape == y.shape and np.abs(x - y).max() <= 1e-13
    o = Options(tolerance=1e-12, max_bond_dim=5, max_sweeps=2, convergence_tol=0.0)
    got, info = pn.np_partial_fit(a, b, plan, o)
    want, winfo = fit_np.np_fit(a, b, o)
    assert info["n_sweeps"] == winfo["n_sweeps"] and np.allclose(info["norms"], winfo["norms"], rtol=1e-13, atol=0)
    assert links(got) == links(want) and np.abs(dense(got) - dense(want)).max() <= 1e-12
    # the patch of fit_np is gone
    assert fit_np.np_half_left.__module__ == "fit_np" and fit_np.np_zipup.__module__ == "fit_np"


def random_chain(rng, n, dims):
    bonds = [1] + [int(x) for x in rng.integers(1, 4, n - 1)] + [1]
    return [rng.standard_normal((l, d[0], d[1], r)) for l, r, d in zip(bonds[:-1], bonds[1:], dims)]


def routes(a, b, plan):
    o = Options(tolerance=1e-13, max_bond_dim=None, max_sweeps=1, convergence_tol=0.0)
    return [pn.np_partial_naive(a, b, plan), pn.np_partial_naive(a, b, plan, o), pn.np_partial_zipup(a, b, plan, o),
            pn.np_partial_fit(a, b, plan, o)[0]]


def test_dense_meaning_of_hadamard_mixed_inner_and_outer():
    rng = np.random.default_rng(5)
    n = 3
    dims = [(2, 3), (3, 2), (2, 2)]
    a, b = random_chain(rng, n, dims), random_chain(rng, n, dims)
    fa, fb = dense(a), dense(b)  # [i1, j1, i2, j2, i3, j3]
    # Hadamard: the elementwise product, site dims (x0 * x1, 1)
    plan = pn.plan_for(a, b, diagonal_pairs=pn.hadamard_pairs(n))
    want = (fa * fb).reshape([6, 1, 6, 1, 4, 1], order="F")
    for ts in routes(a, b, plan):
        assert [t.shape[1:3] for t in ts] == [(6, 1), (6, 1), (4, 1)]
        assert np.abs(dense(ts) - want).max() <= 1e-12
    # all legs contracted: the inner product, site dims (1, 1)
    plan = pn.plan_for(a, b, contract_pairs=[((i, leg), (i, leg)) for i in range(n) for leg in (0, 1)])
    for ts in routes(a, b, plan):
        assert abs(dense(ts).reshape(-1)[0] - (fa * fb).sum()) <= 1e-12 and dense(ts).size == 1
    # nothing paired: the outer product, S = (x0, x1), T = (y0, y1)
    plan = pn.plan_for(a, b)
    want = np.einsum("abcdef,ghijkl->abghcdijefkl", fa, fb)
    want = want.reshape([6, 6, 6, 6, 4, 4], order="F")
    for ts in routes(a, b, plan):
        assert np.abs(dense(ts) - want).max() <= 1e-12
    # mixed: f(x, y) g(y, z); y kept (diagonal) at sites 0 and 2, summed at site 1
    dims_b = [(3, 2), (2, 4), (2, 3)]
    b = random_chain(rng, n, dims_b)
    fb = dense(b)
    plan = pn.plan_for(a, b, contract_pairs=[((1, 1), (1, 0))], diagonal_pairs=[((0, 1), (0, 0)), ((2, 1), (2, 0))])
    assert [(p.S, p.T) for p in plan] == [(6, 2), (3, 4), (4, 3)]
    want = np.einsum("abcdef,bgdhfi->abgchefi", fa, fb).reshape([6, 2, 3, 4, 4, 3], order="F")
    for ts in routes(a, b, plan):
        assert np.abs(dense(ts) - want).max() <= 1e-12
    # a diagonal pair between unlike legs: A.0 - B.1, with A.1 and B.0 kept
    b = random_chain(rng, n, [(4, d[0]) for d in dims])
    fb = dense(b)
    plan = pn.plan_for(a, b, diagonal_pairs=[((i, 0), (i, 1)) for i in range(n)])
    want = np.einsum("abcdef,gaicke->abgcdiefk", fa, fb).reshape([6, 4, 6, 4, 4, 4], order="F")
    for ts in routes(a, b, plan):
        assert np.abs(dense(ts) - want).max() <= 1e-12


def test_half_products_of_the_restatement_agree_with_the_site_product():
    rng = np.random.default_rng(9)
    x, y = rng.standard_normal((2, 2, 3, 3)), rng.standard_normal((3, 3, 2, 2))
    sp = pn.np_plan([(2, 3)], [(3, 2)], diagonal_pairs=[((0, 1), (0, 0))])[0]
    site = pn.np_site(x, y, sp)  # [(a b), s, t, (c d)], b and d fastest
    one_l, one_r = np.eye(6).reshape((6, 2, 3)), np.eye(6).reshape((3, 2, 6))
    p = pn.np_half_left(one_l, x, y, sp)    # n = a * 3 + b = the fused row of the site product
    q = pn.np_half_right(one_r, x, y, sp)   # n = c * 2 + d
    assert np.allclose(np.einsum("nstcd->nstdc", p).reshape((6, 6, 2, 6), order="F"), site.reshape((6, 6, 2, 6), order="F"))
    assert np.allclose(np.einsum("abstn->bastn", q).reshape((6, 6, 2, 6), order="F"), site)


# ------------------------------------------------------------------------------------------------ the gap condition
def run_logged(fn):
    log = pn.GapLog()
    with log.recording():
        fn()
    assert log.splits, "nothing was factorised"
    return log


@pytest.mark.parametrize("name", sorted(pn.CASES))
@pytest.mark.parametrize("tol, cap", pn.TOL_CAP)
def test_gap_condition_of_the_compared_cases(name, tol, cap):
    a, b, spec, plan = pn.case_operands(pn.CASES[name])
    o = Options(tolerance=tol, max_bond_dim=cap)
    for fn in (lambda: pn.np_partial_naive(a, b, plan, o), lambda: pn.np_partial_zipup(a, b, plan, o),
               lambda: pn.np_partial_fit(a, b, plan, pn.fit_options(tol, cap))):
        log = run_logged(fn)
        assert log.ok(), log.violations()


def test_gap_condition_of_the_large_case():
    a, b, spec, plan = pn.case_operands(pn.BIG)
    tol, cap = pn.BIG_OPTIONS
    for fn in (lambda: pn.np_partial_zipup(a, b, plan, Options(tolerance=tol, max_bond_dim=cap)),
               lambda: pn.np_partial_fit(a, b, plan, pn.fit_options(tol, cap))):
        log = run_logged(fn)
        assert log.ok(), log.violations()


def test_gap_log_sees_a_violation():
    log = pn.GapLog()
    with log.recording():
        fit_np.np_factorize(np.diag([1.0, 0.5, 3e-7]), 1e-6, None)   # 3e-7 is within a factor 100 of the cutoff
        fit_np.np_factorize(np.diag([1.0, 0.5, 0.5 * (1 - 1e-9)]), 0.0, 2)  # the cap cuts inside a near-degenerate pair
        fit_np.np_factorize(np.diag([1.0, 0.5, 1e-12]), 1e-6, 2)     # clear on both counts
    assert [(k, kind) for k, kind, _ in log.violations()] == [(0, "tolerance"), (1, "cap")]
