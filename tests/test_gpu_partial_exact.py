"""The two kernels of the partial contraction (csrc/kernels_partial.hip) exactly, as tests/test_gpu_fit_exact.py tests the half
product of the fit: operand entries come from {-1, 0, 1}, every product and partial sum is an integer far below 2^53 (the largest
possible sum is 32 * 24 * 3), so the result must EQUAL the int64 einsum whatever arithmetic a tile takes and in whatever order a
correct kernel sums.  On the matrix-product spec both kernels must give the bytes of the kernels they generalise."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, PartialContractionSpec as Spec, partial_contract
from t4a_amd.mpo import _fit_half
from t4a_amd.partial import _partial_half
import partial_np as pn
from test_gpu_fit_exact import SHAPES, int_draw

pytestmark = pytest.mark.gpu

N_SITES = 3  # the chains of the half-product tests: the middle site carries the bonds under test


def all_sites(contract=(), diagonal=()):
    return ([((i, la), (i, lb)) for i in range(N_SITES) for la, lb in contract], [((i, la), (i, lb)) for i in range(N_SITES) for la, lb in diagonal])


# name -> (leg dims of A, leg dims of B, contract (leg_a, leg_b), diagonal (leg_a, leg_b)); None: the dims of the shape itself.
# Leg dims 2 and 3 mixed: S, K and T differ wherever the plan has more than one group of more than one element.
LEG_PLANS = {
    "matrix_product": (None, None, [(1, 0)], []),
    "diag0_contract1": ((2, 3), (2, 3), [(1, 1)], [(0, 0)]),          # S = 2, K = 3, T = 1
    "both_diagonal": ((2, 3), (2, 3), [], [(0, 0), (1, 1)]),            # S = 6, K = 1, T = 1
    "diag1_keep0": ((2, 3), (2, 3), [], [(1, 1)]),                      # S = 6 of two legs, only the slower drives B; T = 2
    "nothing_paired": ((2, 3), (2, 2), [], []),                         # S = 6, T = 4
}


def chain(left, dims, right, draw):
    return [draw((1, dims[0], dims[1], left)), draw((left, dims[0], dims[1], right)), draw((right, dims[0], dims[1], 1))]


def operands(shape, leg_plan, draw):
    n, la, lb, s, k, t, ra, rb = shape
    da, db, contract, diagonal = LEG_PLANS[leg_plan]
    da, db = da or (s, k), db or (k, t)
    a, b = chain(la, da, ra, draw), chain(lb, db, rb, draw)
    cp, dp = all_sites(contract, diagonal)
    env_l, env_r = draw((n, la, lb)), draw((ra, rb, n))
    for env in (env_l, env_r):  # a one-element environment may be drawn as 0, which would test nothing
        if not env.any():
            env.flat[0] = 1.0
    return a, b, env_l, env_r, Spec(cp, dp), pn.plan_for(a, b, cp, dp)[1]


@pytest.mark.parametrize("leg_plan", list(LEG_PLANS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_products_equal_the_integer_einsum(shape, leg_plan):
    a, b, env_l, env_r, spec, sp = operands(shape, leg_plan, int_draw((hash(shape) ^ len(leg_plan)) & 0xFFFF))
    ma, mb = MPO(a), MPO(b)
    ia, ib = a[1].astype(np.int64), b[1].astype(np.int64)
    n, la, lb, _, _, _, ra, rb = shape
    got = _partial_half(env_l, 0, ma, mb, spec, 1)
    want = pn.np_half_left(env_l.astype(np.int64), ia, ib, sp)
    assert got.shape == want.shape == (n, sp.S, sp.T, ra, rb)
    assert np.abs(want).max() > 0
    assert np.array_equal(got, want.astype(np.float64))
    got = _partial_half(env_r, 1, ma, mb, spec, 1)
    want = pn.np_half_right(env_r.astype(np.int64), ia, ib, sp)
    assert got.shape == want.shape == (la, lb, sp.S, sp.T, n)
    assert np.array_equal(got, want.astype(np.float64))


# a different plan on every site, mixed bonds; site 2 has K of two pairs and site dims (1, 1)
NAIVE_A = ([1, 3, 17, 2, 1], [(2, 3), (2, 3), (2, 3), (3, 2)])
NAIVE_B = ([1, 17, 2, 3, 1], [(3, 2), (2, 3), (3, 2), (3, 2)])
NAIVE_CONTRACT = [((0, 1), (0, 0)), ((2, 0), (2, 1)), ((2, 1), (2, 0))]
NAIVE_DIAGONAL = [((1, 0), (1, 0)), ((1, 1), (1, 1)), ((3, 1), (3, 1))]


def test_naive_site_tensors_of_a_chain_with_a_plan_per_site():
    draw = int_draw(21)
    a = [draw((l, d[0], d[1], r)) for l, r, d in zip(NAIVE_A[0][:-1], NAIVE_A[0][1:], NAIVE_A[1])]
    b = [draw((l, d[0], d[1], r)) for l, r, d in zip(NAIVE_B[0][:-1], NAIVE_B[0][1:], NAIVE_B[1])]
    plan = pn.plan_for(a, b, NAIVE_CONTRACT, NAIVE_DIAGONAL)
    assert [(p.S, p.T) for p in plan] == [(2, 2), (6, 1), (1, 1), (6, 3)]
    r = partial_contract(MPO(a), MPO(b), Spec(NAIVE_CONTRACT, NAIVE_DIAGONAL))
    assert r.site_dims() == [(p.S, p.T) for p in plan]
    assert r.link_dims() == [x * y for x, y in zip(NAIVE_A[0][1:-1], NAIVE_B[0][1:-1])]
    for got, x, y, sp in zip(r.site_tensors(), a, b, plan):
        want = pn.np_site(x.astype(np.int64), y.astype(np.int64), sp)
        assert np.abs(want).max() > 0
        assert np.array_equal(got, want.astype(np.float64))


def test_matrix_product_spec_gives_the_bytes_of_contract_naive():
    rng = np.random.default_rng(3)
    a = [rng.standard_normal((l, 2, 3, r)) for l, r in zip(NAIVE_A[0][:-1], NAIVE_A[0][1:])]
    b = [rng.standard_normal((l, 3, 2, r)) for l, r in zip(NAIVE_B[0][:-1], NAIVE_B[0][1:])]
    ma, mb = MPO(a), MPO(b)
    got = partial_contract(ma, mb, Spec.matrix_product(4))
    want = t4a_amd.contract_naive(ma, mb)
    assert got.site_dims() == want.site_dims() and got.link_dims() == want.link_dims()
    for x, y in zip(got.site_tensors(), want.site_tensors()):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matrix_product_spec_gives_the_bytes_of_the_fit_half_product(shape):
    rng = np.random.default_rng(hash(shape) & 0xFFFF)
    a, b, env_l, env_r, spec, _ = operands(shape, "matrix_product", lambda sh: rng.standard_normal(sh))
    ma, mb = MPO(a), MPO(b)
    for env, side in ((env_l, 0), (env_r, 1)):
        assert _partial_half(env, side, ma, mb, spec, 1).tobytes() == _fit_half(env, side, ma, mb, 1).tobytes()


@pytest.mark.parametrize("leg_plan", ["diag0_contract1", "diag1_keep0"])
def test_two_runs_give_the_same_bits(leg_plan):
    """real-valued operands: no summed index is split across workgroups, nothing is added atomically"""
    rng = np.random.default_rng(11)
    shape = (33, 5, 17, 3, 2, 3, 4, 33)
    a, b, env_l, env_r, spec, sp = operands(shape, leg_plan, lambda sh: rng.standard_normal(sh))
    ma, mb = MPO(a), MPO(b)
    for env, side, ref in ((env_l, 0, pn.np_half_left), (env_r, 1, pn.np_half_right)):
        first = _partial_half(env, side, ma, mb, spec, 1)
        second = _partial_half(env, side, ma, mb, spec, 1)
        assert first.tobytes() == second.tobytes()
        want = ref(env, a[1], b[1], sp)
        # the standard bound of a sum of `terms` products of three factors, (terms + 2) eps sum |e a b|, once for the kernel and
        # once for numpy's own rounding
        terms = sp.K * (5 * 17 if side == 0 else 4 * 33)
        bound = 2 * (terms + 2) * np.finfo(np.float64).eps * ref(np.abs(env), np.abs(a[1]), np.abs(b[1]), sp)
        assert np.all(np.abs(first - want) <= bound)
