"""The kernels of csrc/kernels_apply.hip, exactly.  Environments hold integers of {-3..3}, state cores and operators of {-1, 0, 1}, so
every product and partial sum is an integer far below 2^53 and a result must EQUAL int64 arithmetic whatever the order of a sum.

apply_gap_half_kernel runs through its hook on both mirrors,
  left   P[n, x, a, d] = sum_b L[n, a, b] X[b, x, d]        right   Q[a, b, x, n] = sum_d X[b, x, d] R[a, d, n]
at the smallest shapes that reach every path: the environment rows n and the output state bond over 1, 15, 16, 17, 33 (a tile on the
matrix cores needs 16 of both inside the matrix: full tiles, ragged tiles beside full ones, and launches with no full tile at all),
the summed bond over 1, 3, 4, 5, 16, 18 (chunks of four with and without a remainder), the pass-through bond over 1, 2, 3 (1 is an
outside site), the site dim over 2, 3, and one shape with several row tiles and two column strips.  Every launch runs twice and must
give the same bytes; the output buffer is pre-filled and a guard of 64 doubles behind it must come back untouched.

apply_site_kernel runs through apply_linear_operator(naive, fused) on chains that mix operator, bridge and outside sites with bonds
1 - 5 in one launch; with full coverage its bits are those of contract_naive on the state as an MPO.

Real operands: the half against the float64 restatement within 2 (L + 2) 2^-53 sum_b |E| |X| (L the summed bond: the bound of a
length-L dot product in any order, once for each side), and naive fused against naive composed bit for bit."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import ApplyOptions, LinearOperator, MPO, SimpleTensorTrain
from t4a_amd.linop import _gap_half

import apply_np as A

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
# (environment rows, output state bond, summed bond, pass-through bond, site dim)
SHAPES = [
    (1, 1, 1, 1, 2),      # one element per thread only
    (15, 15, 3, 2, 3),    # one ragged tile
    (16, 16, 4, 1, 2),    # one full tile, one chunk
    (16, 16, 5, 3, 2),    # one full tile, a chunk and a remainder
    (17, 17, 16, 2, 3),   # a full tile with ragged tiles below, beside and across
    (33, 33, 18, 3, 2),   # four full tiles and the ragged edges
    (16, 33, 1, 2, 2),
    (33, 16, 3, 1, 3),
    (17, 1, 5, 2, 2),
    (1, 17, 18, 3, 3),
    (33, 15, 16, 2, 2),
    (15, 33, 4, 1, 2),
    (35, 70, 5, 2, 2),    # three row tiles, two column strips of 64
]


def half_operands(rng, shape, right, real=False):
    n, out, k, m, d = shape
    lb, rb = (out, k) if right else (k, out)
    es = (m, rb, n) if right else (n, m, lb)
    if real:
        return rng.uniform(-1, 1, es), rng.uniform(-1, 1, (lb, d, rb))
    return rng.integers(-3, 4, es).astype(np.float64), rng.integers(-1, 2, (lb, d, rb)).astype(np.float64)


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
def test_gap_half_equals_int64_arithmetic(shape, right):
    rng = np.random.default_rng(hash(shape) % 2 ** 31 + right)
    env, x = half_operands(rng, shape, right)
    want = A.np_gap_half(env.astype(np.int64), x.astype(np.int64), right).astype(np.float64)
    res, guard = _gap_half(env, x, right, fill=SENTINEL)
    again, _ = _gap_half(env, x, right, fill=SENTINEL)
    assert res.shape == want.shape
    assert res.tobytes() == again.tobytes()
    assert np.all(guard == SENTINEL)
    assert np.array_equal(res, want)


def test_shapes_cover_every_value_the_kernel_branches_on():
    for col, values in ((0, {1, 15, 16, 17, 33}), (1, {1, 15, 16, 17, 33}), (2, {1, 3, 4, 5, 16, 18}), (3, {1, 2, 3}), (4, {2, 3})):
        assert values <= {s[col] for s in SHAPES}


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("shape", [(17, 33, 18, 3, 2), (33, 17, 5, 2, 3), (15, 15, 16, 1, 2)])
def test_gap_half_real_operands_within_the_dot_product_bound(shape, right):
    rng = np.random.default_rng(41 + right)
    env, x = half_operands(rng, shape, right, real=True)
    got = _gap_half(env, x, right)
    assert got.tobytes() == _gap_half(env, x, right).tobytes()
    ref = A.np_gap_half(env, x, right)
    bound = 2 * (shape[2] + 2) * 2.0 ** -53 * A.np_gap_half(np.abs(env), np.abs(x), right)
    assert np.all(np.abs(got - ref) <= bound)


# ------------------------------------------------------------------------------------------------ the site kernel
def int_chain(rng, dims, bonds, sites, od, ob, real=False):
    draw = (lambda s: rng.uniform(-1, 1, s)) if real else (lambda s: rng.integers(-1, 2, s).astype(np.float64))
    x = [draw((l, d, r)) for d, l, r in zip(dims, bonds[:-1], bonds[1:])]
    op = [draw((l, s1, s2, r)) for (s1, s2), l, r in zip(od, ob[:-1], ob[1:])]
    return op, x


CHAINS = {
    # outside, op, bridge, bridge, op, op, outside: every kind, bonds 1 - 5, site dims 2 and 3, an operator with s1 != s2
    "mixed": ((2, 3, 2, 3, 2, 2, 3), (1, 2, 5, 3, 4, 1, 2, 1), (1, 4, 5), ((2, 3), (3, 2), (3, 2)), (1, 3, 2, 1)),
    "interleaved": ((2,) * 8, (1, 2, 3, 5, 4, 5, 3, 2, 1), (0, 2, 4, 6), ((2, 2),) * 4, (1, 2, 3, 2, 1)),
    "k1_last": ((2, 2, 3), (1, 2, 4, 1), (2,), ((2, 3),), (1, 1)),
    "n1": ((3,), (1, 1), (0,), ((2, 3),), (1, 1)),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_site_kernel_equals_int64_arithmetic(name):
    dims, bonds, sites, od, ob = CHAINS[name]
    rng = np.random.default_rng(7 + len(dims))
    op, x = int_chain(rng, dims, bonds, sites, od, ob)
    want = A.np_naive([t.astype(np.int64) for t in op], sites, [c.astype(np.int64) for c in x])
    lin = LinearOperator(MPO(op), sites)
    state = SimpleTensorTrain(x)
    got, info = t4a_amd.apply_linear_operator(lin, state, ApplyOptions.naive(), route="fused", return_info=True)
    assert info["route"] == "fused"
    again = t4a_amd.apply_linear_operator(lin, state, ApplyOptions.naive(), route="fused")
    for g, a, w in zip(got.site_tensors(), again.site_tensors(), want):
        assert g.shape == w.shape and np.array_equal(g, w.astype(np.float64))
        assert g.tobytes() == a.tobytes()
    # the operands are untouched
    for c, h in zip(x, state.site_tensors()):
        assert np.array_equal(c, h)


def test_full_coverage_has_the_bits_of_contract_naive():
    rng = np.random.default_rng(3)
    op, x = int_chain(rng, (2, 3, 2, 2), (1, 3, 5, 2, 1), (0, 1, 2, 3), ((2, 2), (2, 3), (3, 2), (2, 2)), (1, 2, 4, 3, 1), real=True)
    m, state = MPO(op), SimpleTensorTrain(x)
    got = t4a_amd.apply_linear_operator(m, state, ApplyOptions.naive(), route="fused")
    want = t4a_amd.contract_naive(m, MPO.from_tensor_train(state)).to_tensor_train()
    assert got.link_dims() == want.link_dims() == [6, 20, 6]
    for g, w in zip(got.site_tensors(), want.site_tensors()):
        assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_naive_fused_against_naive_composed_bit_for_bit(name):
    """real operands; a gap site of the composed route adds products with the zeros of the identity, so a zero may come out with the
    other sign: finite values everywhere, compared by value"""
    dims, bonds, sites, od, ob = CHAINS[name]
    rng = np.random.default_rng(19 + len(dims))
    op, x = int_chain(rng, dims, bonds, sites, od, ob, real=True)
    lin, state = LinearOperator(MPO(op), sites), SimpleTensorTrain(x)
    fused = t4a_amd.apply_linear_operator(lin, state, ApplyOptions.naive(), route="fused")
    composed, info = t4a_amd.apply_linear_operator(lin, state, ApplyOptions.naive(), route="composed", return_info=True)
    assert info["route"] == "composed"
    for f, c in zip(fused.site_tensors(), composed.site_tensors()):
        assert f.shape == c.shape and np.isfinite(f).all() and np.isfinite(c).all()
        assert np.array_equal(f, c)
