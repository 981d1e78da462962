"""Quantics transform operators (tensor4all-quanticstransform: shift.rs, flip.rs, cumsum.rs, common.rs, affine.rs) without a GPU.

The operators are built on the host, so everything here runs with no device visible.  The host site tensors are contracted to the
dense matrix M[y, x] and compared with what the operator is defined to do.  Every entry is an integer: every comparison is
np.array_equal, there is no tolerance."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import t4a_amd
from t4a_amd import quanticstransform as qt
from t4a_amd.quanticstransform import BoundaryCondition as BC, TriangleType, AffineParams

P, AP, OPEN = BC.Periodic, BC.AntiPeriodic, BC.Open
ALL_BC = (P, AP, OPEN)
BC_BY_NAME = {"Periodic": P, "AntiPeriodic": AP, "Open": OPEN}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quanticstransform_cases.json")) as _f:
    AFFINE_CASES = json.load(_f)["affine"]


def dense(tensors, r):
    """M[y, x] of site tensors (left, out, in, right), site 0 the most significant bit.  A site index holds one bit per variable,
    var0 + 2 var1 + ...; the flat index of several variables is v0 + 2^r v1 + ... (as affine_transform_matrix)."""
    assert len(tensors) == r
    env = np.ones((1, 1, 1))
    yflat = np.zeros(1, dtype=np.int64)
    xflat = np.zeros(1, dtype=np.int64)

    def offsets(dim, k):
        nvar = dim.bit_length() - 1
        assert 1 << nvar == dim
        return np.array([sum(((s >> v) & 1) << (r * v + r - 1 - k) for v in range(nvar)) for s in range(dim)], dtype=np.int64)

    for k, t in enumerate(tensors):
        left, so, si, right = t.shape
        assert left == env.shape[2]
        env = np.einsum("yxl,loir->yoxir", env, t).reshape(env.shape[0] * so, env.shape[1] * si, right)
        yflat = (yflat[:, None] + offsets(so, k)[None, :]).reshape(-1)
        xflat = (xflat[:, None] + offsets(si, k)[None, :]).reshape(-1)
    assert env.shape[2] == 1
    out = np.zeros((yflat.size, xflat.size))
    out[np.ix_(yflat, xflat)] = env[:, :, 0]
    return out


def dense_op(op):
    return dense(op.site_tensors(), len(op))


def shift_matrix(r, offset, bc):
    n = 1 << r
    m = np.zeros((n, n))
    for x in range(n):
        q, y = divmod(x + offset, n)
        m[y, x] = 1.0 if bc == P else (-1.0) ** (q % 2) if bc == AP else float(q == 0)
    return m


def flip_matrix(r, bc):
    n = 1 << r
    m = np.zeros((n, n))
    for x in range(1, n):
        m[(n - x) % n, x] = 1.0
    m[0, 0] = {P: 1.0, AP: -1.0, OPEN: 0.0}[bc]
    return m


def embed(single, r, nvariables, target_var):
    """kron of `single` on target_var with identities, flat index v0 + 2^r v1 + ... (variable 0 fastest)"""
    eye = np.eye(1 << r)
    out = np.ones((1, 1))
    for v in range(nvariables):  # the later variable is the slower index: kron(later, earlier)
        out = np.kron(single if v == target_var else eye, out)
    return out


# ------------------------------------------------------------------------------------------------ shift
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("bc", ALL_BC)
def test_shift_every_offset(r, bc):
    lim = (1 << (r + 1)) + 1
    for offset in range(-lim, lim + 1):
        op = qt.shift_operator(r, offset, bc)
        assert np.array_equal(dense_op(op), shift_matrix(r, offset, bc)), (r, offset, bc)
        # (M g)[x] = g[x - offset]
        if bc == P:
            g = np.arange(1.0, (1 << r) + 1)
            assert np.array_equal(dense_op(op) @ g, np.array([g[(x - offset) % (1 << r)] for x in range(1 << r)]))


# ------------------------------------------------------------------------------------------------ flip
@pytest.mark.parametrize("r", [2, 3, 4, 5])
@pytest.mark.parametrize("bc", ALL_BC)
def test_flip(r, bc):
    assert np.array_equal(dense_op(qt.flip_operator(r, bc)), flip_matrix(r, bc))


# ------------------------------------------------------------------------------------------------ triangle / cumsum
@pytest.mark.parametrize("r", [2, 3, 4, 5])
def test_triangle_and_cumsum(r):
    n = 1 << r
    i, j = np.indices((n, n))
    lower = dense_op(qt.triangle_operator(r, TriangleType.Lower))
    upper = dense_op(qt.triangle_operator(r, TriangleType.Upper))
    assert np.array_equal(lower, (i > j).astype(float))
    assert np.array_equal(upper, (i < j).astype(float))
    assert np.array_equal(dense_op(qt.cumsum_operator(r)), lower)
    assert np.array_equal(lower + upper + np.eye(n), np.ones((n, n)))


# ------------------------------------------------------------------------------------------------ several variables
@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("nvariables", [2, 3])
def test_multivar_shift_and_flip(r, nvariables):
    for target in range(nvariables):
        for bc in ALL_BC:
            for offset in (1, -3, (1 << r) + 2):
                op = qt.shift_operator_multivar(r, offset, bc, nvariables, target)
                assert op.site_dims() == [(1 << nvariables, 1 << nvariables)] * r
                assert np.array_equal(dense_op(op), embed(shift_matrix(r, offset, bc), r, nvariables, target)), (target, bc, offset)
            op = qt.flip_operator_multivar(r, bc, nvariables, target)
            assert np.array_equal(dense_op(op), embed(flip_matrix(r, bc), r, nvariables, target)), (target, bc)


# ------------------------------------------------------------------------------------------------ affine
def case_params(case):
    def rat(v):
        return Fraction(v[0], v[1]) if isinstance(v, list) else v
    return AffineParams([rat(v) for v in case["a"]], [rat(v) for v in case["b"]], case["m"], case["n"])


def affine_by_solving(r, params, bc):
    """A second statement of affine_transform_matrix: for every x form v = A x + b exactly and solve for y.  Open: y = v must be
    an integer in range.  Periodic / AntiPeriodic: with A and b cleared of denominators, scale * y = v_int (mod 2^r), solved with
    the modular inverse: g = gcd(scale, 2^r) must divide v_int, and there are g solutions y0 + k 2^r / g; the number of wraps is
    (v_int - scale * y) / 2^r."""
    m, n, size = params.m, params.n, 1 << r
    scale = 1
    for v in params.a + params.b:
        scale = np.lcm(scale, v.denominator)
    scale = int(scale)
    out = np.zeros((1 << (r * m), 1 << (r * n)))
    for x_flat in range(1 << (r * n)):
        x = [(x_flat >> (r * j)) % size for j in range(n)]
        per_var = []
        for i in range(m):
            v = params.b[i] + sum(params.a[i + m * j] * x[j] for j in range(n))  # a Fraction
            sols = []
            if bc[i] == OPEN:
                if v.denominator == 1 and 0 <= v.numerator < size:
                    sols.append((v.numerator, 1.0))
            else:
                v_int = v * scale
                assert v_int.denominator == 1
                v_int = v_int.numerator
                g = int(np.gcd(scale, size))
                if v_int % g == 0:
                    period = size // g
                    y0 = (v_int // g) * pow(scale // g, -1, period) % period if period > 1 else 0
                    for k in range(g):
                        y = y0 + k * period
                        wraps, rem = divmod(v_int - scale * y, size)
                        assert rem == 0
                        sols.append((y, -1.0 if bc[i] == AP and wraps % 2 else 1.0))
            per_var.append(sols)
        rows = [(0, 1.0)]
        for i, sols in enumerate(per_var):
            rows = [(yf + (y << (r * i)), w * wi) for yf, w in rows for y, wi in sols]
        for yf, w in rows:
            out[yf, x_flat] += w
    return out


def affine_runs():
    for case in AFFINE_CASES:
        for r in case["r"]:
            for bc in case["bc"]:
                yield pytest.param(case, r, bc, id=f"{case['name']}-r{r}-{bc}")


@pytest.mark.parametrize("case, r, bc", list(affine_runs()))
def test_affine_operator_against_the_brute_force_matrix(case, r, bc):
    params = case_params(case)
    conditions = [BC_BY_NAME[bc]] * params.m
    want = qt.affine_transform_matrix(r, params, conditions)
    op = qt.affine_operator(r, params, conditions)
    assert op.site_dims() == [(1 << params.m, 1 << params.n)] * r
    assert np.array_equal(dense_op(op), want)


@pytest.mark.parametrize("case, r, bc", list(affine_runs()))
def test_affine_transform_matrix_against_solving_for_y(case, r, bc):
    params = case_params(case)
    conditions = [BC_BY_NAME[bc]] * params.m
    want = affine_by_solving(r, params, conditions)
    assert np.array_equal(qt.affine_transform_matrix(r, params, conditions), want)


def test_affine_matrix_known_entries():
    # antiperiodic full cycles: +-2^r is minus the identity, 2 * 2^r the identity; the difference delta flips sign for x < x'
    for shift, sign in ((8, -1.0), (-8, -1.0), (16, 1.0)):
        m = qt.affine_transform_matrix(3, AffineParams.from_integers([1], [shift], 1, 1), [AP])
        assert np.array_equal(m, sign * np.eye(8))
    m = qt.affine_transform_matrix(3, AffineParams.from_integers([1, -1], [0], 1, 2), [AP])
    for x in range(8):
        for xp in range(8):
            col = np.zeros(8)
            col[(x - xp) % 8] = 1.0 if x >= xp else -1.0
            assert np.array_equal(m[:, x | (xp << 3)], col)


@pytest.mark.parametrize("bc", ALL_BC)
def test_affine_is_shift_and_flip(bc):
    for r in (1, 3, 4):
        for k in (0, 1, -3, 5, (1 << r), -(1 << r) - 1, 3 * (1 << r) + 2):
            op = qt.affine_operator(r, AffineParams.from_integers([1], [k], 1, 1), [bc])
            assert np.array_equal(dense_op(op), dense_op(qt.shift_operator(r, k, bc))), (r, k)
    for r in (2, 3, 5):
        op = qt.affine_operator(r, AffineParams.from_integers([-1], [0], 1, 1), [P])
        assert np.array_equal(dense_op(op), dense_op(qt.flip_operator(r, P)))


def test_bond_dimensions_and_reproducible_carries():
    for r in (2, 3, 6):
        for op in (qt.shift_operator(r, 3, AP), qt.flip_operator(r, OPEN), qt.triangle_operator(r, TriangleType.Upper), qt.cumsum_operator(r),
                   qt.affine_operator(r, AffineParams.from_integers([1, -1], [0], 1, 2), [P])):
            assert op.link_dims() == [2] * (r - 1)
    params = AffineParams([Fraction(1, 2), Fraction(1, 2), Fraction(1, 2), Fraction(-1, 2)], [2, 3], 2, 2)
    one = qt.affine_operator(4, params, [P, OPEN]).site_tensors()
    two = qt.affine_operator(4, params, [P, OPEN]).site_tensors()
    assert len(one) == len(two) == 4
    for x, y in zip(one, two):
        assert x.shape == y.shape and np.array_equal(x, y)


def test_affine_params():
    p = AffineParams([Fraction(1, 2), Fraction(1, 3)], [Fraction(5, 4)], 1, 2)
    assert p.to_integer_scaled() == ([6, 4], [15], 12)
    q = AffineParams.from_integers([1, 0, 0, 1], [1, 2], 2, 2)
    assert (q.m, q.n) == (2, 2) and q.to_integer_scaled() == ([1, 0, 0, 1], [1, 2], 1)
    assert AffineParams([(1, 3)], [0], 1, 1).a == [Fraction(1, 3)]


# ------------------------------------------------------------------------------------------------ errors
def raises_invalid(call, needle):
    with pytest.raises(t4a_amd.T4aError) as e:
        call()
    assert e.value.code == t4a_amd.INVALID_ARGUMENT, e.value
    assert needle in e.value.message, e.value.message


def test_errors():
    ident = AffineParams.from_integers([1], [0], 1, 1)
    raises_invalid(lambda: qt.shift_operator(0, 1, P), "Number of sites must be positive")
    raises_invalid(lambda: qt.shift_operator(64, 1, P), "at most 63")
    raises_invalid(lambda: qt.shift_operator_multivar(0, 1, P, 2, 0), "Number of sites must be positive")
    raises_invalid(lambda: qt.flip_operator(0, P), "Number of sites must be positive")
    raises_invalid(lambda: qt.flip_operator(1, P), "MPO with one tensor is not supported for flip operator")
    raises_invalid(lambda: qt.flip_operator_multivar(1, P, 2, 0), "MPO with one tensor is not supported for flip operator")
    raises_invalid(lambda: qt.cumsum_operator(1), "Number of sites must be at least 2, got 1")
    raises_invalid(lambda: qt.cumsum_operator(0), "Number of sites must be at least 2, got 0")
    raises_invalid(lambda: qt.triangle_operator(1, TriangleType.Upper), "Number of sites must be at least 2, got 1")
    raises_invalid(lambda: qt.shift_operator_multivar(3, 1, P, 2, 2), "target_var 2 must be less than nvariables 2")
    raises_invalid(lambda: qt.flip_operator_multivar(3, P, 3, 5), "target_var 5 must be less than nvariables 3")
    raises_invalid(lambda: qt.shift_operator_multivar(3, 1, P, 1, 0), "nvariables must be at least 2, got 1")
    raises_invalid(lambda: qt.flip_operator_multivar(3, P, 0, 0), "nvariables must be at least 2, got 0")
    raises_invalid(lambda: qt.affine_operator(0, ident, [P]), "Number of bits must be positive")
    raises_invalid(lambda: qt.affine_operator(3, ident, [P, P]), "Boundary conditions length 2 doesn't match output dimensions 1")
    raises_invalid(lambda: qt.affine_transform_matrix(3, ident, []), "Boundary conditions length 0 doesn't match output dimensions 1")
    raises_invalid(lambda: AffineParams.from_integers([1, 2, 3], [0], 1, 2), "Matrix A has 3 elements but expected 1×2=2")
    raises_invalid(lambda: AffineParams.from_integers([1, 2], [0, 1], 1, 2), "Vector b has 2 elements but expected 1")
    raises_invalid(lambda: AffineParams([(1, 0)], [0], 1, 1), "affine matrix[0] has zero denominator")
    raises_invalid(lambda: AffineParams([1], [(3, 0)], 1, 1), "affine translation[0] has zero denominator")
    raises_invalid(lambda: qt.affine_operator(2, AffineParams.from_integers([1] * 16, [0], 1, 16), [P]), "m + n = 17 exceeds 15")
    raises_invalid(lambda: qt.affine_operator(2, AffineParams.from_integers([1] * 64, [0] * 8, 8, 8), [P] * 8), "m + n = 16 exceeds 15")
    raises_invalid(lambda: qt.affine_operator(8, AffineParams.from_integers([1 << 62] * 4, [0], 1, 4), [P]), "overflows int64")
    raises_invalid(lambda: qt.affine_operator(8, AffineParams.from_integers([1 << 70], [0], 1, 1), [P]), "does not fit int64")
    raises_invalid(lambda: qt.affine_transform_matrix(7, AffineParams.from_integers([1, 0, 0, 1], [0, 0], 2, 2), [P, P]), "exceeds 20")


def test_abi_checks_lengths_itself():
    import ctypes
    a = np.array([1, 2, 3], dtype=np.int64)
    b = np.array([0], dtype=np.int64)
    bc = np.array([0], dtype=np.int32)
    h = ctypes.c_void_p()
    st = t4a_amd._lib.t4a_gpu_qt_affine_operator(ctypes.c_size_t(3), t4a_amd._p(a), ctypes.c_size_t(3), t4a_amd._p(b), ctypes.c_size_t(1),
                                                 ctypes.c_int64(1), ctypes.c_size_t(1), ctypes.c_size_t(2), t4a_amd._p(bc), ctypes.c_size_t(1),
                                                 ctypes.byref(h))
    assert st == t4a_amd.INVALID_ARGUMENT and "Matrix A has 3 elements" in t4a_amd.last_error_message()
    st = t4a_amd._lib.t4a_gpu_qt_affine_operator(ctypes.c_size_t(3), t4a_amd._p(a), ctypes.c_size_t(2), t4a_amd._p(b), ctypes.c_size_t(1),
                                                 ctypes.c_int64(0), ctypes.c_size_t(1), ctypes.c_size_t(2), t4a_amd._p(bc), ctypes.c_size_t(1),
                                                 ctypes.byref(h))
    assert st == t4a_amd.INVALID_ARGUMENT and "common denominator must be positive" in t4a_amd.last_error_message()


class _StateShape:
    """what apply reads of a state before it touches the device"""

    def __init__(self, dims):
        self._dims = dims

    def site_dims(self):
        return list(self._dims)


def test_apply_checks_shapes_first():
    op = qt.shift_operator(3, 1, P)
    raises_invalid(lambda: qt.apply(op, _StateShape([2, 2])), "operator has 3 sites, the state has 2")
    raises_invalid(lambda: qt.apply(op, _StateShape([2, 4, 2])), "Shared shape mismatch at site 1")


def test_device_steps_without_gpu_are_no_device():
    if t4a_amd.device_count() > 0:
        pytest.skip("a GPU is visible: the loud-failure path is covered on the CPU builder")
    op = qt.shift_operator(3, 1, P)
    assert len(op.site_tensors()) == 3  # building and reading back needs no device
    cores = [np.ones((1, 2, 1))] * 3
    for call in (op.mpo, lambda: qt.apply(op, _StateShape([2, 2, 2])), lambda: qt.identity_mpo(3),
                 lambda: qt.difference_kernel_mpo(t4a_amd.SimpleTensorTrain(cores), P)):
        with pytest.raises(t4a_amd.T4aError) as e:
            call()
        assert e.value.code == t4a_amd.NO_DEVICE and "no CPU fallback" in e.value.message
