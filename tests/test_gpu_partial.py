"""Partial contraction of two MPOs on the device (t4a_amd.partial) against the numpy restatement of tests/partial_np.py, against dense
elementwise products, and against the composition the matrix product could already run (the copy tensor multiplied into A on the
host, then contract_zipup).  Values are compared with `close` / `assert_matches` of tests/test_gpu_mpo.py at its rel = 1e-10, link
dimensions exactly — on operand sets for which tests/test_cpu_partial.py asserts the gap condition."""
import functools

import numpy as np
import pytest

import t4a_amd
from t4a_amd import (MPO, ContractionOptions, ContractionAlgorithm, FactorizeMethod, FitOptions, PartialContractionSpec as Spec,
                     partial_contract, partial_contract_fit, hadamard)
import partial_np as pn
from partial_np import Options, np_full, links
from test_gpu_mpo import assert_matches, close

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    """(a, b, Spec, plan) of a named operand set; computed once, never written to"""
    a, b, spec, plan = pn.case_operands(pn.BIG if name == "BIG" else pn.CASES[name])
    return a, b, Spec(spec.get("contract_pairs", ()), spec.get("diagonal_pairs", ())), plan


@functools.lru_cache(maxsize=None)
def restated(name, route, tol, cap):
    a, b, _, plan = case(name)
    if route == "naive":
        return pn.np_partial_naive(a, b, plan, Options(tolerance=tol, max_bond_dim=cap))
    if route == "zipup":
        return pn.np_partial_zipup(a, b, plan, Options(tolerance=tol, max_bond_dim=cap))
    return pn.np_partial_fit(a, b, plan, pn.fit_options(tol, cap))


def device_fit_options(tol, cap):
    o = pn.fit_options(tol, cap)
    return FitOptions(tolerance=o.tolerance, max_bond_dim=o.max_bond_dim, max_sweeps=o.max_sweeps, convergence_tol=o.convergence_tol)


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("tol, cap", pn.TOL_CAP)
@pytest.mark.parametrize("name", sorted(pn.CASES))
def test_three_routes_match_the_restatement(name, tol, cap):
    a, b, spec, plan = case(name)
    ma, mb = MPO(a), MPO(b)
    o = ContractionOptions(tolerance=tol, max_bond_dim=cap)
    assert_matches(partial_contract(ma, mb, spec, ContractionAlgorithm.Naive, o), restated(name, "naive", tol, cap))
    assert_matches(partial_contract(ma, mb, spec, ContractionAlgorithm.ZipUp, o), restated(name, "zipup", tol, cap))
    want, winfo = restated(name, "fit", tol, cap)
    r, info = partial_contract_fit(ma, mb, spec, device_fit_options(tol, cap), return_info=True)
    assert info["n_sweeps"] == winfo["n_sweeps"]
    close(info["norms"], winfo["norms"])
    assert_matches(r, want)


@pytest.mark.parametrize("name", sorted(pn.CASES))
def test_uncompressed_naive_is_the_exact_site_product(name):
    a, b, spec, plan = case(name)
    r = partial_contract(MPO(a), MPO(b), spec)
    assert r.site_dims() == [(p.S, p.T) for p in plan]
    for got, want in zip(r.site_tensors(), pn.np_partial_naive(a, b, plan)):
        close(got, want, rel=1e-14)


def test_zipup_at_bonds_17_x_18():
    """MFMA tiles and ragged edges inside the driver"""
    a, b, spec, plan = case("BIG")
    tol, cap = pn.BIG_OPTIONS
    r = partial_contract(MPO(a), MPO(b), spec, ContractionAlgorithm.ZipUp, ContractionOptions(tolerance=tol, max_bond_dim=cap))
    assert_matches(r, restated("BIG", "zipup", tol, cap))


def test_fit_at_bonds_17_x_18():
    a, b, spec, plan = case("BIG")
    tol, cap = pn.BIG_OPTIONS
    want, winfo = restated("BIG", "fit", tol, cap)
    r, info = partial_contract_fit(MPO(a), MPO(b), spec, device_fit_options(tol, cap), return_info=True)
    assert info["n_sweeps"] == winfo["n_sweeps"]
    close(info["norms"], winfo["norms"])
    assert_matches(r, want)


# ------------------------------------------------------------------------------------------------ hadamard
def train_cores(bonds, d, seed):
    return [c[:, :, 0, :] for c in pn.random_tensors(bonds, d, 1, seed)]


def dense_train(cores):
    """values indexed [i1, i2, ...]"""
    return np_full([c[:, :, None, :] for c in cores]).reshape([c.shape[1] for c in cores])


@pytest.mark.parametrize("alg", [ContractionAlgorithm.ZipUp, ContractionAlgorithm.Naive])
def test_hadamard_of_two_operators_is_the_elementwise_product(alg):
    a = pn.random_tensors([1, 3, 4, 2, 1], 2, 3, pn.SEED ^ 0x7)
    b = pn.random_tensors([1, 2, 3, 3, 1], 2, 3, pn.SEED ^ 0x8)
    r = hadamard(MPO(a), MPO(b), alg)
    assert r.site_dims() == [(2, 3)] * 4
    close(r.full_tensor(), np_full(a) * np_full(b))


def test_hadamard_of_two_trains_and_of_a_train_with_itself():
    n, chi = 8, 3
    bonds = [1, 2] + [chi] * (n - 3) + [2, 1]
    f, g = train_cores(bonds, 2, pn.SEED ^ 0x9), train_cores(bonds, 2, pn.SEED ^ 0xA)
    tf, tg = t4a_amd.SimpleTensorTrain(f), t4a_amd.SimpleTensorTrain(g)
    df, dg = dense_train(f), dense_train(g)
    r = hadamard(tf, tg)
    assert isinstance(r, t4a_amd.SimpleTensorTrain) and r.site_dims() == [2] * n
    close(np.asarray(r.full_tensor()), (df * dg).reshape(-1, order="F"))
    # f * f: the bond pair (a, b) enters symmetrically, the true bond is chi (chi + 1) / 2 = 6 < chi^2 = 9: the rank rule cuts exact zeros
    sq = hadamard(tf, tf)
    close(np.asarray(sq.full_tensor()), (df * df).reshape(-1, order="F"))
    assert sq.link_dims()[:3] == [2, 4, 6] and max(sq.link_dims()) == chi * (chi + 1) // 2
    sq = hadamard(tf, tf, ContractionAlgorithm.Naive, ContractionOptions())
    close(np.asarray(sq.full_tensor()), (df * df).reshape(-1, order="F"))
    assert sq.link_dims() == [2, 4, 6, 6, 6, 4, 2]
    with pytest.raises(t4a_amd.T4aError) as e:
        hadamard(tf, MPO.from_tensor_train(tg))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ the composition the parent could run
def copy_tensor_composition(a, b, plan):
    """(A', B') whose matrix product is the partial contraction: B' = B with its paired legs (in leg order) in front of its free ones,
    A'[a, S, K', c] = A times delta(s, s') for every diagonal pair, K' the legs B' shows in front"""
    out_a, out_b = [], []
    for x, y, sp in zip(a, b, plan):
        la, lb = ["p", "q"], ["u", "v"]
        eyes, ops = [], []
        for xa, yb in sp.k_pairs:
            lb[yb] = la[xa]
        for xa, yb in sp.diag.items():
            lb[yb] = la[xa].upper()  # a copy of A's leg
            eyes.append(np.eye(x.shape[1 + xa]))
            ops.append(la[xa] + la[xa].upper())
        paired = "".join(lb[k] for k in (0, 1) if k not in sp.t_legs)
        free = "".join(lb[k] for k in sp.t_legs)
        s = "".join(la[k] for k in sp.s_legs)
        xa_ = np.einsum(",".join(["apqc"] + ops) + "->a" + s + paired + "c", x, *eyes)
        yb_ = np.einsum("b" + "".join(lb) + "d->b" + paired + free + "d", y)
        kk = int(np.prod(yb_.shape[1:1 + len(paired)], dtype=np.int64))
        out_a.append(xa_.reshape((x.shape[0], sp.S, kk, x.shape[3]), order="F"))
        out_b.append(yb_.reshape((y.shape[0], kk, sp.T, y.shape[3]), order="F"))
    return out_a, out_b


@pytest.mark.parametrize("name", sorted(pn.CASES))
def test_diagonal_specs_equal_the_copy_tensor_composition(name):
    a, b, spec, plan = case(name)
    ca, cb = copy_tensor_composition(a, b, plan)
    want = t4a_amd.contract_zipup(MPO(ca), MPO(cb), ContractionOptions())
    got = partial_contract(MPO(a), MPO(b), spec, ContractionAlgorithm.ZipUp, ContractionOptions())
    assert got.site_dims() == want.site_dims()
    close(got.full_tensor(), want.full_tensor())


# ------------------------------------------------------------------------------------------------ edge cases
def test_one_site_and_empty_chains():
    x, y = pn.random_tensors([1, 1], 2, 3, pn.SEED), pn.random_tensors([1, 1], 2, 3, pn.SEED ^ 0xFF)
    spec = Spec.hadamard(1)
    want = (x[0] * y[0]).reshape((1, 6, 1, 1), order="F")
    for r in (partial_contract(MPO(x), MPO(y), spec), partial_contract(MPO(x), MPO(y), spec, ContractionAlgorithm.Naive, ContractionOptions()),
              partial_contract(MPO(x), MPO(y), spec, ContractionAlgorithm.ZipUp), partial_contract_fit(MPO(x), MPO(y), spec)):
        assert len(r) == 1 and r.site_dims() == [(6, 1)]
        close(r.site_tensor(0), want, rel=1e-14)
    r, info = partial_contract_fit(MPO(x), MPO(y), spec, return_info=True)
    assert info["n_sweeps"] == 0 and info["norms"] == []
    close(hadamard(MPO(x), MPO(y)).site_tensor(0), x[0] * y[0], rel=1e-14)
    for r in (partial_contract(MPO([]), MPO([]), Spec()), partial_contract(MPO([]), MPO([]), Spec(), ContractionAlgorithm.ZipUp),
              partial_contract_fit(MPO([]), MPO([]), Spec()), hadamard(MPO([]), MPO([]))):
        assert len(r) == 0 and r.link_dims() == []


def test_error_answers():
    two, one = MPO.constant([(2, 2), (2, 2)], 1.0), MPO.constant([(2, 2)], 1.0)
    ok = Spec.matrix_product(2)

    def answer(fn, code, needle):
        with pytest.raises(t4a_amd.T4aError) as e:
            fn()
        assert e.value.code == code and needle in e.value.message, e.value.message

    inv, nimp = t4a_amd.INVALID_ARGUMENT, t4a_amd.NOT_IMPLEMENTED
    for run in (lambda s, a=two, b=two: partial_contract(a, b, s), lambda s, a=two, b=two: partial_contract(a, b, s, ContractionAlgorithm.ZipUp),
                lambda s, a=two, b=two: partial_contract_fit(a, b, s)):
        answer(lambda: run(Spec(), b=one), inv, "length mismatch: expected 2, got 1")
        answer(lambda: run(Spec(contract_pairs=[((0, 1), (1, 0))])), nimp, "joins two sites")
        answer(lambda: run(Spec(output_order=[(0, 0)])), nimp, "output_order is not implemented")
        answer(lambda: run(Spec(contract_pairs=[((0, 0), (0, 0))], diagonal_pairs=[((0, 0), (0, 1))])), inv,
               "first MPO index (site 0, leg 0) appears in multiple pairs")
        answer(lambda: run(Spec(diagonal_pairs=[((0, 0), (0, 0)), ((0, 1), (0, 0))])), inv,
               "second MPO index (site 0, leg 0) appears in multiple pairs")
        answer(lambda: run(Spec(contract_pairs=[((2, 0), (0, 0))])), inv, "(site 2, leg 0) from contract_pairs not found in first MPO")
        answer(lambda: run(Spec(diagonal_pairs=[((0, 0), (0, 3))])), inv, "(site 0, leg 3) from diagonal_pairs not found in second MPO")
    wide = MPO.constant([(2, 3), (2, 3)], 1.0)
    answer(lambda: partial_contract(wide, two, Spec(diagonal_pairs=[((0, 1), (0, 1))])), inv, "diagonal_pairs index shape mismatch: 3 != 2")
    answer(lambda: hadamard(wide, two), inv, "diagonal_pairs index shape mismatch: 3 != 2")
    # Fit through partial_contract and RSVD keep the answers of `contract`
    answer(lambda: partial_contract(two, two, ok, ContractionAlgorithm.Fit), nimp, "fitting is not implemented")
    for alg in (ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp):
        answer(lambda: partial_contract(two, two, ok, alg, ContractionOptions(factorize_method=FactorizeMethod.RSVD)), nimp,
               "RSVD factorization not yet implemented")
    answer(lambda: partial_contract_fit(two, two, ok, FitOptions(factorize_method=FactorizeMethod.RSVD)), nimp,
           "RSVD factorization not yet implemented")
    answer(lambda: partial_contract(two, two, ok, 7), inv, "unknown contraction algorithm")
    # initial of the fit: the site dims of the result, (|S|, |T|) = (4, 1) for the Hadamard product
    had = Spec.hadamard(2)
    answer(lambda: partial_contract_fit(two, two, had, initial=MPO.constant([(2, 2), (2, 2)], 1.0)), inv,
           "initial has site dims (2, 2) at site 0, the product has (4, 1)")
    answer(lambda: partial_contract_fit(two, two, had, initial=MPO.constant([(4, 1)], 1.0)), inv, "initial has 1 sites, the product has 2")
    r = partial_contract_fit(two, two, had, initial=MPO.constant([(4, 1), (4, 1)], 0.5))
    close(r.full_tensor(), np.ones((4, 1, 4, 1)))
