"""The single-XCD rrLU kernel carries its column maxima and early keys as HIGH WORDS of the magnitudes (kernels_rrlu_xcd2.hip):
the exact candidate is known only behind the position search, and everything the high words do not single out goes to the exact
paths.  Inputs built to sit on those seams — many entries on one high word (inside a lane, between lanes, between the columns of
one agent, between agents), one-ulp neighbours, the edges of the mid range, overflowing / underflowing scores, non-finite
values — against the oracle, bitwise, in both orthogonalities.

Shapes: the smallest that reach the single-XCD kernel with at least three row slots per lane (rows i, i + 64 and i + 128 share a
lane).  As the kernel sees them: 200 x 260 is four row slots and TWO columns per agent (columns j and j + 136 share an agent),
260 x 200 is six row slots and one column per agent; a right-orthogonal factorisation runs on the transpose, so both shapes meet
both plans.  One 1 100 x 900 case runs the multi-XCD form (rank capped at 16 so that the oracle stays fast)."""
import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

SHAPES = [(200, 260), (260, 200)]
BIG = (1100, 900)
EXACT = dict(rel_tol=0.0, abs_tol=0.0)


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def _same_outcome(t4a, a, **opts):
    """Device and oracle either both refuse (NaN in L / U: MatrixCIError::NaNEncountered) or agree bitwise."""
    try:
        f, rp, cp, npiv, err = ob.rrlu(a, **opts)
    except ob.OracleError:
        with pytest.raises(t4a.T4aError) as e:
            t4a.rrlu(a, **opts)
        assert e.value.code == t4a.NAN_ENCOUNTERED
        return None
    lu = t4a.rrlu(a, **opts)
    assert lu.npivots() == npiv
    assert np.array_equal(lu.row_permutation, rp) and np.array_equal(lu.col_permutation, cp)
    assert np.array_equal(lu.factored.view(np.uint64), f.view(np.uint64))
    assert lu.error == err or (np.isnan(lu.error) and np.isnan(err))
    return lu


def _hi(a):
    return (np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32) & np.uint32(0x7FFFFFFF)


def _tie_values(rng, count):
    """+-(1 + k 2^-40) with distinct k: one high word (0x3FF00000), distinct low words."""
    k = rng.permutation(count) + 1
    v = (1.0 + k * 2.0 ** -40) * rng.choice([-1.0, 1.0], size=count)
    assert np.all(_hi(v) == 0x3FF00000) and len(np.unique(np.abs(v))) == count
    return v


def _signed_permutation(rng, m, n):
    mn = min(m, n)
    a = np.zeros((m, n))
    a[rng.permutation(m)[:mn], rng.permutation(n)[:mn]] = _tie_values(rng, mn)
    return a


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_step_ties_on_the_high_word(t4a, left, shape):
    """A signed permutation-like matrix: at every step all remaining non-zeros share one high word and differ in the low word, so no
    step is decided on high words — collisions inside a lane, between lanes, between the columns of an agent and between agents.
    The zero fill keeps the later steps the same kind (the rank-1 update touches nothing but the pivot row)."""
    m, n = shape
    rng = np.random.default_rng(6100 + m)
    lu = _same_outcome(t4a, _signed_permutation(rng, m, n), left_orthogonal=left, **EXACT)
    assert lu.npivots() == min(m, n)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_dense_near_ties(t4a, left, shape):
    """c (1 + eps_ij), |eps| < 2^-30, random signs: step 0 finds all entries on one high word, the steps behind it are ordinary."""
    m, n = shape
    rng = np.random.default_rng(6200 + m)
    a = 1.3 * (1.0 + rng.uniform(-1, 1, size=(m, n)) * 2.0 ** -31) * rng.choice([-1.0, 1.0], size=(m, n))
    assert np.all(_hi(a) == _hi(np.float64(1.3)))   # (1.3 sits in the middle of its high word)
    _same_outcome(t4a, a, max_bond_dim=24, left_orthogonal=left, **EXACT)
    _same_outcome(t4a, np.abs(a), max_bond_dim=8, left_orthogonal=left)  # (numerically rank one: the default tolerances stop it)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_two_entries_one_ulp_apart(t4a, left, shape):
    """The two largest magnitudes share the high word and differ by one ulp: in one lane (64 / 128 rows apart), in different lanes, in
    the two columns of one agent (136 apart), in different agents; the larger one first or second in tie order, either sign; the
    background holds exact zeros of both signs."""
    m, n = shape
    rng = np.random.default_rng(6300 + m)
    base = rng.uniform(-1, 1, size=(m, n))
    base[rng.random((m, n)) < 0.05] = 0.0
    base[rng.random((m, n)) < 0.02] = -0.0
    assert np.signbit(base[base == 0.0]).any()
    i, j = 5, 9
    big = 3.0 + 2.0 ** -30
    big_up = np.nextafter(big, np.inf)
    assert _hi(np.float64(big)) == _hi(np.float64(big_up))
    for off in (1, 64, 128, 136):
        for (di, dj) in ((off, 0), (0, off)):
            for (v0, v1) in ((big, -big_up), (-big_up, big), (-big, -big)):
                a = base.copy()
                a[i, j] = v0
                a[i + di, j + dj] = v1
                _same_outcome(t4a, a, max_bond_dim=4, left_orthogonal=left, **EXACT)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_edges_of_the_mid_ranges(t4a, left, shape):
    """Maxima just inside and just outside the ranges the fast paths are proven for: 2^+-300 (the shared-reciprocal division) and
    biased exponents 600 / 1500 (hi_mid: where a decision on high words is allowed); whole matrices at those scales, and one entry
    outside above a matrix inside."""
    m, n = shape
    rng = np.random.default_rng(6400 + m)
    u = rng.uniform(0.5, 1.0, size=(m, n)) * rng.choice([-1.0, 1.0], size=(m, n))   # biased exponent 1022 everywhere
    for e in (-302, -300, -298, 298, 300, 302, -425, -423, -422, -421, 476, 477, 478, 479):
        _same_outcome(t4a, np.ldexp(u, e), max_bond_dim=5, left_orthogonal=left, **EXACT)
    for e in (301, 478, -299):
        a = np.ldexp(u, -10 if e > 0 else -320)
        a[m // 2, n // 3] = np.ldexp(0.75, e)
        a[m // 3, n // 2] = -np.ldexp(0.75, e)       # (and a tie on it)
        _same_outcome(t4a, a, max_bond_dim=5, left_orthogonal=left, **EXACT)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_special_values(t4a, left, shape):
    """The cases of test_rrlu_special_values_on_multi_workgroup_shapes (test_gpu_fuzz.py) at these shapes: scores that overflow
    (hand-over to the chip-wide kernels) or underflow, subnormals, zeros, NaN / inf — and finite entries so large that their high
    word reads as an f32 NaN pattern."""
    m, n = shape
    rng = np.random.default_rng(6500 + m)
    kw = dict(left_orthogonal=left)
    a = rng.uniform(-1, 1, size=(m, n))
    a[m // 2, n // 3] = 1e200
    _same_outcome(t4a, a, max_bond_dim=6, **EXACT, **kw)
    for (i, j, v) in [(7, 100, 1e200), (60, 3, -3e199), (61, 3, 2e180), (2, 2, 9e170)]:
        a[i, j] = v
    _same_outcome(t4a, a, max_bond_dim=12, **EXACT, **kw)
    for v in (1e307, -1.7e308, 2.0 ** 1017, np.nextafter(2.0 ** 512, 0.0), 2.0 ** 512):
        b = rng.uniform(-1, 1, size=(m, n))
        b[m - 3, n - 2] = v
        _same_outcome(t4a, b, max_bond_dim=4, **EXACT, **kw)
    grow = rng.uniform(-1, 1, size=(m, n)) * 2.0 ** 505   # finite scores at first; the trailing block may grow past 2^512 on the way
    _same_outcome(t4a, grow, max_bond_dim=40, **EXACT, **kw)
    tiny = rng.uniform(0.5, 1, size=(m, n)) * 1e-200
    _same_outcome(t4a, tiny, max_bond_dim=9, **EXACT, **kw)
    _same_outcome(t4a, tiny, **kw)
    few = rng.uniform(-1, 1, size=(m, n))
    few[::3, ::2] = 1e-200
    _same_outcome(t4a, few, max_bond_dim=20, **EXACT, **kw)
    sub = rng.integers(1, 1000, size=(m, n)).astype(float) * 5e-324 * 1e10
    _same_outcome(t4a, sub, max_bond_dim=6, **EXACT, **kw)
    sub2 = rng.integers(1, 1000, size=(m, n)).astype(float) * 5e-324       # (high word 0 everywhere: only low words differ)
    _same_outcome(t4a, sub2, max_bond_dim=6, **EXACT, **kw)
    mixed = rng.uniform(-1, 1, size=(m, n))
    mixed[:, ::7] *= 1e-180
    mixed[::5, :] *= 1e150
    _same_outcome(t4a, mixed, max_bond_dim=20, **EXACT, **kw)
    _same_outcome(t4a, np.zeros((m, n)), **kw)
    _same_outcome(t4a, np.zeros((m, n)), max_bond_dim=7, **EXACT, **kw)
    _same_outcome(t4a, -np.zeros((m, n)), max_bond_dim=3, **EXACT, **kw)
    lowrank = np.outer(np.arange(1, m + 1), np.arange(1, n + 1)).astype(float)
    _same_outcome(t4a, lowrank, **EXACT, **kw)
    for (i, j, v) in [(0, 0, np.nan), (m // 2, n // 2, np.nan), (m - 1, n - 1, np.nan), (11, 13, np.inf), (0, n - 1, -np.inf)]:
        bad = rng.uniform(-1, 1, size=(m, n))
        bad[i, j] = v
        _same_outcome(t4a, bad, max_bond_dim=5, **kw)


@pytest.mark.parametrize("left", [True, False])
def test_high_word_ties_beyond_one_xcd(t4a, left):
    """The multi-XCD form (agents on several XCDs, finalists built from full keys): ties on the high word at every step, dense
    near-ties, one-ulp neighbours on one XCD and on two, a score that overflows."""
    m, n = BIG
    rng = np.random.default_rng(6600)
    kw = dict(max_bond_dim=16, left_orthogonal=left, **EXACT)
    _same_outcome(t4a, _signed_permutation(rng, m, n), **kw)
    a = 1.3 * (1.0 + rng.uniform(-1, 1, size=(m, n)) * 2.0 ** -31) * rng.choice([-1.0, 1.0], size=(m, n))
    assert np.all(_hi(a) == _hi(np.float64(1.3)))
    _same_outcome(t4a, a, **kw)
    base = rng.uniform(-1, 1, size=(m, n))
    big = 3.0 + 2.0 ** -30
    for (di, dj) in ((64, 0), (0, 1), (0, 450), (500, 0)):
        b = base.copy()
        b[700, 300] = -big
        b[700 - di, 300 + dj] = np.nextafter(big, np.inf)
        _same_outcome(t4a, b, **kw)
    base[m // 2, n // 3] = 1e200
    _same_outcome(t4a, base, **kw)
