"""The half launch of fit_sum (csrc/kernels_fit_sum.hip), exactly.  Environments hold integers of {-3..3} and cores of {-1, 0, 1}, so
every product and partial sum is an integer far below 2^53 and the result must EQUAL int64 arithmetic whatever the order of a sum:
  left   P[c, s, off_k + b] = sum_a EL[c, offL_k + a] T_k[a, s, b]        right   Q[off_k + a, s, c] = sum_b T_k[a, s, b] ER[offR_k + b, c]
in both orientations, on the fused launch and on the GEMM composition.  The result bond and the targets' bonds run over the edges of
the 16-wide tiles of the matrix-core path (1, 2, 15, 16, 17, 33), S over 1, 2, 3, the number of targets over 1, 3 ragged, 8 ragged and
40 (the job table lives in device memory and the tile lookup crosses many jobs); a target of bond 1 sits between targets of bond >= 16,
so both arithmetics run in one launch; one shape has several row tiles and column strips per job.  Every launch runs twice and must give
the same bytes, a sentinel behind the output stays untouched, and the block of a target has the same bytes alone and among the others."""
import numpy as np
import pytest

from t4a_amd.fitsum import _half

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 15, 16, 17, 33)
RAGGED = {1: ((17, 15),), 3: ((1, 17), (17, 2), (2, 1)), 8: ((1, 17), (17, 1), (1, 17), (17, 33), (33, 15), (15, 16), (16, 2), (2, 1))}
SENTINEL = -7.5


def operands(rng, chi, S, bonds, right, real=False):
    A, B = sum(a for a, _ in bonds), sum(b for _, b in bonds)
    shape = (B, chi) if right else (chi, A)
    if real:
        return rng.uniform(-1, 1, shape), [rng.uniform(-1, 1, (a, S, b)) for a, b in bonds]
    return rng.integers(-3, 4, shape).astype(np.float64), [rng.integers(-1, 2, (a, S, b)).astype(np.float64) for a, b in bonds]


def expected(env, cores, right):
    """int64 einsum, block by block"""
    e = env.astype(np.int64)
    out, oa, ob = [], 0, 0
    for t in cores:
        a, _, b = t.shape
        ti = t.astype(np.int64)
        out.append(np.einsum("asb,bc->asc", ti, e[ob:ob + b]) if right else np.einsum("ca,asb->csb", e[:, oa:oa + a], ti))
        oa, ob = oa + a, ob + b
    return np.concatenate(out, axis=0 if right else 2)


def check(env, cores, right):
    want = expected(env, cores, right).astype(np.float64)
    got = {}
    for route in ("fused", "gemm"):
        res, guard = _half(env, cores, right, route, fill=SENTINEL)
        again, _ = _half(env, cores, right, route, fill=SENTINEL)
        assert res.tobytes() == again.tobytes(), route
        assert np.all(guard == SENTINEL), route
        assert np.array_equal(res, want), (route, right)
        got[route] = res
    return got["fused"]


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("S", (1, 2, 3))
@pytest.mark.parametrize("chi", SIZES)
def test_every_pair_of_bonds_in_one_launch(chi, S, right):
    """36 targets, (a_k, b_k) over SIZES x SIZES: |P| <= 3 * 33, |Q| <= 3 * 33"""
    rng = np.random.default_rng(1000 * chi + 10 * S + right)
    bonds = [(a, b) for a in SIZES for b in SIZES]
    check(*operands(rng, chi, S, bonds, right), right)


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("K", (1, 3, 8, 40))
def test_target_counts(K, right):
    rng = np.random.default_rng(77 + K + right)
    bonds = RAGGED[K] if K in RAGGED else tuple((SIZES[k % 6], SIZES[(k // 6 + 2 * k) % 6]) for k in range(K))
    for chi in (2, 16, 33):
        check(*operands(rng, chi, 2, bonds, right), right)


@pytest.mark.parametrize("right", (False, True))
def test_a_target_of_bond_one_between_targets_on_the_matrix_cores(right):
    rng = np.random.default_rng(5 + right)
    for chi in (16, 33):
        check(*operands(rng, chi, 3, ((17, 33), (1, 1), (16, 16), (1, 1), (33, 17)), right), right)


@pytest.mark.parametrize("right", (False, True))
def test_several_row_tiles_and_column_strips_per_job(right):
    """left: 70 rows (five row tiles) by 3 * 33 = 99 columns (two strips of 64); right: 33 * 3 = 99 rows by 70 columns"""
    rng = np.random.default_rng(11 + right)
    check(*operands(rng, 70, 3, ((33, 33), (17, 33), (33, 16)), right), right)


@pytest.mark.parametrize("right", (False, True))
def test_a_block_has_the_same_bytes_alone_and_among_the_others(right):
    """real operands: the bits of a block depend on its operands and its shape alone, not on the other jobs of the launch"""
    rng = np.random.default_rng(31 + right)
    bonds = RAGGED[8]
    for chi in (2, 17):
        env, cores = operands(rng, chi, 2, bonds, right, real=True)
        whole = _half(env, cores, right, "fused")
        oa = ob = 0
        for t in cores:
            a, _, b = t.shape
            alone = _half(env[ob:ob + b] if right else env[:, oa:oa + a], [t], right, "fused")
            block = whole[oa:oa + a] if right else whole[:, :, ob:ob + b]
            assert np.ascontiguousarray(block).tobytes() == np.ascontiguousarray(alone).tobytes()
            oa, ob = oa + a, ob + b
        ref = np.concatenate([np.einsum("asb,bc->asc", t, env[o:o + t.shape[2]]) if right else np.einsum("ca,asb->csb", env[:, o:o + t.shape[0]], t)
                              for t, o in zip(cores, np.cumsum([0] + [t.shape[2 if right else 0] for t in cores[:-1]]))], axis=0 if right else 2)
        # a sum of n <= 33 terms below 1 in magnitude is off by at most n u n, u = 2^-53, on either side
        assert np.abs(whole - ref).max() <= 2 * 33 * 33 * 2.0 ** -53
