"""The half-product kernel of the variational MPO fit (csrc/kernels_mpo_fit.hip) through t4a_gpu_mpo_fit_half, exactly: operand
entries come from {-1, 0, 1}, so every product and every partial sum is an integer far below 2^53 (the largest possible sum is
32 * 24 * 2) and the result must EQUAL the int64 einsum whatever arithmetic a tile takes (matrix cores or one element per thread)
and in whatever order a correct kernel sums.  Both orientations are run for every shape."""
import numpy as np
import pytest

from t4a_amd import MPO
from t4a_amd.mpo import _fit_half

pytestmark = pytest.mark.gpu

# (N, La, Lb, S, K, T, Ra, Rb): environment index, bonds of the A site, the B site, and the three site dimensions
SHAPES = [
    (3, 2, 3, 2, 2, 2, 3, 2),          # everything per thread
    (16, 16, 16, 2, 2, 2, 16, 16),     # exact 16-tiles
    (17, 16, 3, 2, 3, 2, 18, 5),       # ragged edges, both arithmetics inside one call
    (33, 5, 17, 3, 2, 3, 4, 33),       # ragged edges, both arithmetics inside one call
    (1, 1, 1, 4, 4, 1, 7, 3),          # first site of operator x state
    (48, 32, 24, 2, 2, 2, 32, 24),     # several workgroups, several (k, b) panels
]


def chain(left, s1, s2, right, draw):
    """a three-site MPO whose middle site is [left, s1, s2, right]"""
    return [draw((1, s1, s2, left)), draw((left, s1, s2, right)), draw((right, s1, s2, 1))]


def operands(shape, draw):
    n, la, lb, s, k, t, ra, rb = shape
    a, b = chain(la, s, k, ra, draw), chain(lb, k, t, rb, draw)
    return a, b, draw((n, la, lb)), draw((ra, rb, n))


def int_draw(seed):
    rng = np.random.default_rng(seed)
    return lambda shape: rng.integers(-1, 2, shape).astype(np.float64)


def einsum_left(env, x, y):
    return np.einsum("nbskc,bktd->nstcd", np.einsum("nab,askc->nbskc", env, x), y)


def einsum_right(env, x, y):
    return np.einsum("askdn,bktd->abstn", np.einsum("askc,cdn->askdn", x, env), y)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_products_equal_the_integer_einsum(shape):
    a, b, env_l, env_r = operands(shape, int_draw(hash(shape) & 0xFFFF))
    ma, mb = MPO(a), MPO(b)
    ia, ib = a[1].astype(np.int64), b[1].astype(np.int64)
    n, la, lb, s, k, t, ra, rb = shape
    got = _fit_half(env_l, 0, ma, mb, 1)
    want = einsum_left(env_l.astype(np.int64), ia, ib)
    assert got.shape == want.shape == (n, s, t, ra, rb)
    assert np.abs(want).max() > 0
    assert np.array_equal(got, want.astype(np.float64))
    got = _fit_half(env_r, 1, ma, mb, 1)
    want = einsum_right(env_r.astype(np.int64), ia, ib)
    assert got.shape == want.shape == (la, lb, s, t, n)
    assert np.array_equal(got, want.astype(np.float64))


def test_first_and_last_site_of_a_chain():
    """the sites the sweeps reach with the trivial environments [[[1]]]"""
    draw = int_draw(5)
    a, b = chain(5, 2, 3, 17, draw), chain(18, 3, 2, 4, draw)
    ma, mb = MPO(a), MPO(b)
    one = np.ones((1, 1, 1))
    ia, ib = [x.astype(np.int64) for x in a], [x.astype(np.int64) for x in b]
    assert np.array_equal(_fit_half(one, 0, ma, mb, 0), einsum_left(one.astype(np.int64), ia[0], ib[0]).astype(np.float64))
    assert np.array_equal(_fit_half(one, 1, ma, mb, 2), einsum_right(one.astype(np.int64), ia[2], ib[2]).astype(np.float64))


def test_two_runs_give_the_same_bits():
    """real-valued operands: no summed index is split across workgroups, nothing is added atomically"""
    rng = np.random.default_rng(11)
    shape = (33, 5, 17, 3, 2, 3, 4, 33)
    a, b, env_l, env_r = operands(shape, lambda sh: rng.standard_normal(sh))
    ma, mb = MPO(a), MPO(b)
    for env, side, ref in ((env_l, 0, einsum_left), (env_r, 1, einsum_right)):
        first = _fit_half(env, side, ma, mb, 1)
        second = _fit_half(env, side, ma, mb, 1)
        assert first.tobytes() == second.tobytes()
        want = ref(env, a[1], b[1])
        # the standard bound of a sum of `terms` products of three factors, (terms + 2) eps sum |e a b|, once for the kernel and
        # once for numpy's own rounding
        terms = 2 * (5 * 17 if side == 0 else 4 * 33)
        bound = 2 * (terms + 2) * np.finfo(np.float64).eps * ref(np.abs(env), np.abs(a[1]), np.abs(b[1]))
        assert np.all(np.abs(first - want) <= bound)
