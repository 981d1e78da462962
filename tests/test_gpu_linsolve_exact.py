"""The kernels of the linear solver (csrc/kernels_linsolve.hip) and the launches around them, exactly: every operand is integer-valued
and small enough that every product and every partial sum is an integer far below 2^53, so the device must EQUAL the int64 einsum
whatever arithmetic a tile takes (matrix cores, split-K, one element per thread) and in whatever order a correct kernel sums.
The projected apply on caller-supplied environments draws from {-2, ..., 2}: its largest sum has w_l chi_l d W d chi_r w_r < 2^21
terms of magnitude at most 2^5."""
import numpy as np
import pytest

import linsolve_np as ln
from t4a_amd import MPO, SimpleTensorTrain, ProjectedOperator
from t4a_amd.linsolve import _apply_env, _orth

pytestmark = pytest.mark.gpu

CHIS = (1, 3, 16, 17, 33)                               # below, on and past the 16-row tile edges of the GEMM
BONDS = ((1, 1, 1), (2, 5, 1), (1, 17, 2), (5, 2, 5))   # (w_l, w_m, w_r); 17 * d * 33 reaches the split-K path of the second product
SITES = ((2, 2), (2, 3), (3, 2))                        # (d_i, d_{i+1})


def int_draw(seed, lo=-2, hi=2):
    rng = np.random.default_rng(seed)
    return lambda shape: rng.integers(lo, hi + 1, shape).astype(np.float64)


def operator(wl, wm, wr, d1, d2, draw):
    """four sites; the region under test is (1, 2)"""
    return [draw((1, 2, 2, wl)), draw((wl, d1, d1, wm)), draw((wm, d2, d2, wr)), draw((wr, 2, 2, 1))]


def i64(a):
    return np.asarray(a).astype(np.int64)


def exact_apply(left, right, op1, op2, v):
    """the int64 contraction in the four-step order of a CPU implementation, which is not the order of the device"""
    y = ln.np_projected_apply_steps(i64(left), i64(right), i64(op1), i64(op2), i64(v))
    assert y.dtype == np.int64
    return y


@pytest.mark.parametrize("dims", SITES, ids=lambda d: "d%dx%d" % d)
@pytest.mark.parametrize("bonds", BONDS, ids=lambda b: "w%d_%d_%d" % b)
def test_apply_env_equals_the_integer_einsum(bonds, dims):
    wl, wm, wr = bonds
    d1, d2 = dims
    draw = int_draw(1000 * wl + 100 * wm + 10 * wr + d1 + 3 * d2)
    ops = operator(wl, wm, wr, d1, d2, draw)
    mpo = MPO(ops)
    nonzero = 0
    for chi_l in CHIS:
        for chi_r in CHIS:
            left, right, v = draw((chi_l, wl, chi_l)), draw((chi_r, wr, chi_r)), draw((chi_l, d1, d2, chi_r))
            want = exact_apply(left, right, ops[1], ops[2], v)
            assert np.abs(want).max() < 2 ** 26
            got = _apply_env(left, right, mpo, 1, v)
            assert got.shape == want.shape
            assert np.array_equal(got, want.astype(np.float64)), (chi_l, chi_r)
            nonzero += int(np.abs(want).max() > 0)
    assert nonzero >= 20


@pytest.mark.parametrize("bonds", BONDS, ids=lambda b: "w%d_%d_%d" % b)
def test_half_operators_equal_the_integer_einsum(bonds):
    wl, wm, wr = bonds
    draw = int_draw(77 + wm)
    nonzero = 0
    for d1, d2 in SITES:
        ops = operator(wl, wm, wr, d1, d2, draw)
        mpo = MPO(ops)
        for chi_l, chi_r in ((1, 33), (17, 3), (16, 16), (33, 17)):
            left, right, v = draw((chi_l, wl, chi_l)), draw((chi_r, wr, chi_r)), draw((chi_l, d1, d2, chi_r))
            _, hl, hr = _apply_env(left, right, mpo, 1, v, return_half_operators=True)
            want_l, want_r = ln.np_half_operators(i64(left), i64(right), i64(ops[1]), i64(ops[2]))
            assert hl.shape == want_l.shape == (wm * chi_l * d1, chi_l * d1) and hr.shape == want_r.shape == (wm * d2 * chi_r, d2 * chi_r)
            assert np.array_equal(hl, want_l.astype(np.float64)) and np.array_equal(hr, want_r.astype(np.float64))
            nonzero += int(np.abs(want_l).max() > 0) + int(np.abs(want_r).max() > 0)
    assert nonzero >= 20


def test_environments_after_one_and_after_three_sites():
    draw2, draw1 = int_draw(5), int_draw(8, -1, 1)
    d = 2
    for draw, bonds_x, bonds_w in ((draw2, [1, 3, 17, 5, 1], [1, 2, 5, 3, 1]), (draw1, [1, 2, 4, 3, 1], [1, 2, 3, 2, 1])):
        ops = [draw((bonds_w[k], d, d, bonds_w[k + 1])) for k in range(4)]
        xs = [draw((bonds_x[k], d, bonds_x[k + 1])) for k in range(4)]
        po = ProjectedOperator(MPO(ops), SimpleTensorTrain(xs))
        left = np.ones((1, 1, 1), dtype=np.int64)
        right = np.ones((1, 1, 1), dtype=np.int64)
        depth = 3 if draw is draw1 else 1  # {-2..2} stays exact over one site, {-1, 0, 1} over three
        for k in range(depth):
            left = ln.np_left_env(left, i64(ops[k]), i64(xs[k]))
            got = po.environment("left", k + 1)
            assert got.shape == left.shape and np.array_equal(got, left.astype(np.float64)), ("left", k + 1)
            right = ln.np_right_env(right, i64(ops[3 - k]), i64(xs[3 - k]))
            got = po.environment("right", 3 - k)
            assert got.shape == right.shape and np.array_equal(got, right.astype(np.float64)), ("right", 3 - k)
        assert np.abs(left).max() > 0 and np.abs(right).max() > 0 and np.abs(left).max() < 2 ** 40
        assert np.array_equal(po.environment("left", 0), np.ones((1, 1, 1))) and np.array_equal(po.environment("right", 4), np.ones((1, 1, 1)))


def exact_orth(basis, w):
    """the two passes in int64: every coefficient of a pass from the same w (classical Gram-Schmidt), then the update"""
    b, w = i64(basis), i64(w)
    h1 = b.T @ w
    w1 = w - b @ h1
    h2 = b.T @ w1
    w2 = w1 - b @ h2
    n2 = int(w2 @ w2)
    assert n2 < 2 ** 53 and np.abs(w2).max() < 2 ** 26
    return h1, h2, w2, n2


@pytest.mark.parametrize("nb", (1, 2, 31))
@pytest.mark.parametrize("length", (1, 63, 64, 65, 4097))
def test_orth_step_is_exact_on_integers(length, nb):
    """At most eight entries of a basis vector are nonzero, which bounds |w| after both passes by 2 + 31 * 16 + 31 * 8 * 498 and its
    squared norm by 4097 * 1.3e5^2 < 2^53."""
    rng = np.random.default_rng(31 * length + nb)
    basis = np.zeros((length, nb))
    for i in range(nb):
        where = rng.choice(length, size=min(length, 8), replace=False)
        basis[where, i] = rng.choice([-1.0, 1.0], size=len(where))
    w = rng.integers(-2, 3, length).astype(np.float64)
    h1, h2, w2, n2 = exact_orth(basis, w)
    got_w, got_h1, got_h2, got_norm = _orth(basis, w)
    assert np.array_equal(got_h1, h1.astype(np.float64)) and np.array_equal(got_h2, h2.astype(np.float64))
    assert got_norm == np.sqrt(np.float64(n2))
    if n2 > 0:
        assert np.array_equal(got_w, w2.astype(np.float64) * (1.0 / np.sqrt(np.float64(n2))))


def test_two_runs_of_each_hook_give_the_same_bits():
    rng = np.random.default_rng(11)
    ops = [rng.standard_normal(s) for s in ((1, 2, 2, 5), (5, 2, 2, 17), (17, 3, 3, 2), (2, 2, 2, 1))]
    mpo = MPO(ops)
    left, right, v = rng.standard_normal((33, 5, 33)), rng.standard_normal((17, 2, 17)), rng.standard_normal((33, 2, 3, 17))
    first = _apply_env(left, right, mpo, 1, v, return_half_operators=True)
    second = _apply_env(left, right, mpo, 1, v, return_half_operators=True)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    want = ln.np_projected_apply_steps(left, right, ops[1], ops[2], v)
    assert np.abs(first[0] - want).max() <= 1e-11 * np.abs(want).max()
    basis, w = rng.standard_normal((4097, 31)), rng.standard_normal(4097)
    a, b = _orth(basis, w), _orth(basis, w)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
