"""What two-site TDVP adds below its solver, exactly.  gs_dots_wide (csrc/kernels_tdvp.hip) must give the BITS of the serial gs_dots: the
same element partition, summation order and reduction tree, so the whole orthogonalisation step agrees bit for bit whichever launch
forms the projections — and, so that this does not lean on the existing kernel alone, on small-integer operands every product and
partial sum is an integer far below 2^53 and the coefficients must EQUAL int64 arithmetic.  The one-site projected apply
(ProjectedOperator::apply_one_site) on integer environments and operators must equal the int64 einsum, on mixed bonds and on bonds
of 1, and the half operator reused from a bond step must give the bits of a fresh one."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, SimpleTensorTrain, ProjectedOperator
from t4a_amd.linsolve import _orth
from t4a_amd.tdvp import _krylov_orth, _apply_one_site, ROUTE_SERIAL, ROUTE_WIDE, ROUTE_AUTO

pytestmark = pytest.mark.gpu

# the edges of the element partition (256 threads, 1024 elements per workgroup up to 128 workgroups, the second round of the grid stride),
# of GS_WIDE = 8, and of the 32-vector batch of the serial kernel
LENGTHS = (1, 255, 256, 257, 1023, 1024, 1025, 4097, 131073)
NBS = (1, 7, 8, 9, 16, 30, 33, 65)


def same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("length", LENGTHS)
def test_wide_route_gives_the_bits_of_the_serial_route(length):
    for nb in NBS:
        rng = np.random.default_rng(7000 * nb + length)
        basis, w = rng.standard_normal((length, nb)), rng.standard_normal(length)
        serial = _krylov_orth(basis, w, ROUTE_SERIAL)
        wide = _krylov_orth(basis, w, ROUTE_WIDE)
        assert same_bits(wide, serial), nb
        assert same_bits(_krylov_orth(basis, w, ROUTE_WIDE), wide), nb  # two calls
        assert same_bits(_orth(basis, w), serial), nb                   # what GMRES and Lanczos launch
        assert same_bits(_krylov_orth(basis, w, ROUTE_AUTO), serial), nb
        assert np.isfinite(serial[3]) and serial[3] > 0


@pytest.mark.parametrize("route", (ROUTE_SERIAL, ROUTE_WIDE), ids=("serial", "wide"))
@pytest.mark.parametrize("length", LENGTHS)
def test_coefficients_equal_int64_arithmetic(length, route):
    """Entries in [-3, 3]: |c1| <= 9 len < 2^21, the updated w is an integer of at most 3 + 65 * 3 * 9 len < 2^28, the second-pass
    coefficients at most 3 len * 2^28 < 2^47: every sum stays below 2^53."""
    for nb in NBS:
        rng = np.random.default_rng(9000 * nb + length)
        basis, w = rng.integers(-3, 4, (length, nb)), rng.integers(-3, 4, length)
        c1 = basis.T.astype(np.int64) @ w.astype(np.int64)
        w1 = w.astype(np.int64) - basis.astype(np.int64) @ c1
        c2 = basis.T.astype(np.int64) @ w1
        w2 = w1 - basis.astype(np.int64) @ c2
        assert max(np.abs(c1).max(), np.abs(c2).max(), np.abs(w2).max()) < 2 ** 53
        _, h1, h2, _ = _krylov_orth(basis.astype(np.float64), w.astype(np.float64), route)
        assert np.array_equal(h1, c1.astype(np.float64)), nb
        assert np.array_equal(h2, c2.astype(np.float64)), nb


# ------------------------------------------------------------------------------------------------ the one-site apply
def integer_chain(dims, bonds, wbonds, seed):
    """integer site tensors and operator sites (square) with entries in {-2, -1, 1, 2}: no zeros, so that bonds of 1 do not give zero
    environments"""
    rng = np.random.default_rng(seed)

    def draw(shape):
        t = rng.integers(-2, 3, shape)
        return np.where(t == 0, 1, t).astype(np.float64)
    x = [draw((bonds[k], d, bonds[k + 1])) for k, d in enumerate(dims)]
    ops = [draw((wbonds[k], d, d, wbonds[k + 1])) for k, d in enumerate(dims)]
    return x, ops


def int_envs(ops, x, c):
    """L_c and R_{c+1} in int64"""
    xi, oi = [t.astype(np.int64) for t in x], [t.astype(np.int64) for t in ops]
    left = np.ones((1, 1, 1), dtype=np.int64)
    for k in range(c):
        left = np.einsum("bwa,bsc,wstv,atd->cvd", left, xi[k], oi[k], xi[k])
    right = np.ones((1, 1, 1), dtype=np.int64)
    for k in range(len(ops) - 1, c, -1):
        right = np.einsum("bsc,wstv,atd,cvd->bwa", xi[k], oi[k], xi[k], right)
    return left, right


CHAINS = {  # name: (site dimensions, state bonds, operator bonds)
    "mixed": ((2, 3, 2, 2), (1, 2, 3, 2, 1), (1, 2, 3, 2, 1)),   # at site 1: chi_l = 2, chi_r = 3, W_l = 2, W_r = 3, d = 3
    "ones": ((2, 3, 2), (1, 1, 1, 1), (1, 1, 1, 1)),              # chi_l = chi_r = W = 1
    "wide": ((3, 3, 3), (1, 3, 5, 1), (1, 4, 2, 1)),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_apply_one_site_equals_the_int64_einsum(name):
    dims, bonds, wbonds = CHAINS[name]
    x, ops = integer_chain(dims, bonds, wbonds, 31 + len(name))
    po = ProjectedOperator(MPO(ops), SimpleTensorTrain(x))
    rng = np.random.default_rng(5)
    for c in range(len(dims)):
        left, right = int_envs(ops, x, c)
        v = rng.integers(-3, 4, x[c].shape)
        want = np.einsum("bwa,wstv,atd,cvd->bsc", left, ops[c].astype(np.int64), v.astype(np.int64), right)
        assert np.abs(want).max() < 2 ** 53 and np.abs(want).max() > 0
        y, reused = _apply_one_site(po, c, v.astype(np.float64))
        assert not reused
        assert y.shape == x[c].shape and np.array_equal(y, want.astype(np.float64)), c


@pytest.mark.parametrize("name", ("mixed", "wide"))
def test_the_half_operator_of_a_bond_step_is_reused_with_the_same_bits(name):
    dims, bonds, wbonds = CHAINS[name]
    x, ops = integer_chain(dims, bonds, wbonds, 77)
    rng = np.random.default_rng(6)
    c = 1
    v = rng.standard_normal(x[c].shape)
    fresh, reused = _apply_one_site(ProjectedOperator(MPO(ops), SimpleTensorTrain(x)), c, v)
    assert not reused
    po = ProjectedOperator(MPO(ops), SimpleTensorTrain(x))
    po.apply(c, rng.standard_normal(po.local_dimension(c)))  # the bond step (c, c + 1) builds HL = L_c A_c
    again, reused = _apply_one_site(po, c, v)
    assert reused and again.tobytes() == fresh.tobytes()
    # a left-moving split replaces x_c and x_{c+1}: HL of the step still serves, the right environment is rebuilt
    k = min(x[c].shape[0] * x[c].shape[1], x[c + 1].shape[1] * x[c + 1].shape[2], 2)
    a = rng.integers(-2, 3, (x[c].shape[0], x[c].shape[1], k)).astype(np.float64)
    b = rng.integers(-2, 3, (k, x[c + 1].shape[1], x[c + 1].shape[2])).astype(np.float64)
    po.apply(c, rng.standard_normal(po.local_dimension(c)))
    po.set_site_tensors(c, a, b)
    x2 = x[:c] + [a, b] + x[c + 2:]
    v2 = rng.standard_normal(a.shape)
    moved, reused = _apply_one_site(po, c, v2)
    fresh2, reused2 = _apply_one_site(ProjectedOperator(MPO(ops), SimpleTensorTrain(x2)), c, v2)
    assert reused and not reused2 and moved.tobytes() == fresh2.tobytes()
    # a change to the left of c makes it stale
    po.apply(c, rng.standard_normal(po.local_dimension(c)))
    po.invalidate(0)
    _, reused = _apply_one_site(po, c, v2)
    assert not reused


def test_apply_one_site_refuses_a_site_outside_the_chain():
    dims, bonds, wbonds = CHAINS["ones"]
    x, ops = integer_chain(dims, bonds, wbonds, 3)
    po = ProjectedOperator(MPO(ops), SimpleTensorTrain(x))
    with pytest.raises(t4a_amd.T4aError) as e:
        _apply_one_site(po, 3, np.ones((1, 2, 1)))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "site 3 is out of range" in e.value.message
