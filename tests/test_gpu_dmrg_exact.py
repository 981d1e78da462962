"""The kernels Lanczos adds to a local solve (csrc/kernels_dmrg.hip), exactly: on integer operands every product and every partial sum
is an integer far below 2^53, so the device must EQUAL int64 arithmetic in whatever order a correct kernel sums.  The lengths are the
edges of the partition (256 threads, 1024 elements per workgroup up to 128 workgroups): one workgroup, two, all 128, and the second
round of the grid stride.  On Gaussian operands the sums are compared with math.fsum at the bound of a recursive sum of len terms,
and two calls must give the same bits."""
import math

import numpy as np
import pytest

from t4a_amd.dmrg import _krylov_combine, _eig_residual

pytestmark = pytest.mark.gpu

LENGTHS = (1, 255, 256, 257, 1023, 1024, 1025, 131072, 131073)
NBS = (1, 2, 64, 65)


@pytest.mark.parametrize("length", LENGTHS)
def test_krylov_combine_equals_int64_arithmetic(length):
    """|out| <= 65 * 3 * 4 = 780 and |out|^2 <= 131073 * 780^2 < 2^37"""
    nonzero = 0
    for nb in NBS:
        rng = np.random.default_rng(1000 * nb + length)
        basis = rng.integers(-3, 4, (length, nb))
        coef = rng.integers(-4, 5, nb)
        want = basis.astype(np.int64) @ coef.astype(np.int64)
        out, norm2 = _krylov_combine(basis.astype(np.float64), coef.astype(np.float64))
        assert out.shape == (length,) and np.array_equal(out, want.astype(np.float64)), nb
        assert norm2 == float(int(want @ want)), nb
        nonzero += int(np.abs(want).max() > 0)
    assert nonzero >= 2  # a coefficient may be drawn as 0


@pytest.mark.parametrize("length", LENGTHS)
def test_eig_residual_equals_int64_arithmetic(length):
    rng = np.random.default_rng(77 + length)
    v, hv = rng.integers(-3, 4, length), rng.integers(-3, 4, length)
    for lam in (-2, 0, 3):
        r = hv.astype(np.int64) - lam * v.astype(np.int64)
        want = np.array([int(r @ r), int(v @ hv), int(v @ v)], dtype=np.float64)
        got_r, sums = _eig_residual(v.astype(np.float64), hv.astype(np.float64), float(lam))
        assert np.array_equal(got_r, r.astype(np.float64)), lam
        assert np.array_equal(sums, want), lam
        none, sums_only = _eig_residual(v.astype(np.float64), hv.astype(np.float64), float(lam), with_residual=False)
        assert none is None and np.array_equal(sums_only, want), lam


def within_recursive_sum_bound(got, terms):
    """a sum of len terms in any order is within (len - 1) u sum|terms| of the exact sum to first order; len 2^-52 sum|terms| covers it"""
    exact = math.fsum(terms)
    bound = len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms))
    return abs(got - exact) <= bound


@pytest.mark.parametrize("length", (257, 1025, 131073))
def test_gaussian_sums_stay_within_the_bound_of_a_recursive_sum_and_repeat(length):
    rng = np.random.default_rng(5 + length)
    v, hv, lam = rng.standard_normal(length), rng.standard_normal(length), 0.37
    r, sums = _eig_residual(v, hv, lam)
    assert np.array_equal(r, hv - lam * v)  # a separately rounded multiply and subtract
    for got, terms in zip(sums, (r * r, v * hv, v * v)):
        assert within_recursive_sum_bound(got, terms)
    r2, sums2 = _eig_residual(v, hv, lam)
    none, sums3 = _eig_residual(v, hv, lam, with_residual=False)
    assert r.tobytes() == r2.tobytes() and sums.tobytes() == sums2.tobytes() == sums3.tobytes()
    for nb in (2, 65):
        basis, coef = rng.standard_normal((length, nb)), rng.standard_normal(nb)
        out, norm2 = _krylov_combine(basis, coef)
        want = coef[0] * basis[:, 0]
        for i in range(1, nb):
            want = want + coef[i] * basis[:, i]  # i ascending, every term rounded
        assert np.array_equal(out, want)
        assert within_recursive_sum_bound(norm2, out * out)
        out2, norm2b = _krylov_combine(basis, coef)
        assert out.tobytes() == out2.tobytes() and norm2 == norm2b
