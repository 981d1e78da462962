"""Dense solves and the SVD on every launch route, against answers that are exact by construction.

test_gpu_dense.py compares solve / trsm / SVD with the oracle or LAPACK on random matrices at a few shapes.  Here the inputs are built
so that the right answer is known without a reference implementation:

- triangular solve: small-integer triangular factors with power-of-two diagonals and integer solutions, every intermediate an integer
  (or a multiple of a small power of two) below 2^53, so every summation order returns X bit for bit;
- LU solve: A = P L U with |l| <= 1/2 off the diagonal (partial pivoting must reproduce P) and a power-of-two diagonal of U, so the
  elimination is exact; and the same construction with multipliers of 1e-9, where any pivot other than the column maximum inflates the
  error by 1e9;
- SVD: blocks on disjoint rows and columns (their singular values are those of the blocks), column norms between 1e-150 and 2e-154
  inside a matrix whose largest entry is far from the 2^+-200 band that is rescaled: the squared norms of the pair test underflow there.

Every shape names the launch route it targets (the launchers pick kernels by size: kernels_dense.hip trsm_left_batched_launch,
lu_solve_blocked_launch, lu_forward_blocked_launch; capi.hip t4a_gpu_solve_f64; engine.hip Engine::svd / svd_plain).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from fill_exact_np import _pivot_rows, _plu  # noqa: F401  (the matrices of the LU solves; shared with test_gpu_fill_exact.py)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


# ----------------------------------------------------------------------------------------------------------- triangular solve
FLAGS = [(side, lower, trans, unit) for side in (True, False) for lower in (True, False) for trans in (False, True)
         for unit in (False, True)]


def _tri_problem(rng, n, nrhs, left_side, lower, trans, unit):
    """T (n x n, the stored triangle `lower`), B and the exact X of op(T) X = B (left) or X op(T) = B (right); `nrhs` counts the
    right-hand sides the kernel sees (rows of B for a right-side solve)."""
    t = rng.integers(-2, 3, size=(n, n)).astype(np.float64)
    t = np.tril(t, -1) if lower else np.triu(t, 1)
    d = rng.choice([1.0, -1.0, 2.0, -2.0, 4.0, -0.5, 0.25], size=n)
    t_eff = t + np.diag(np.ones(n) if unit else d)
    # the unit case stores a diagonal the solve must not read
    t_stored = t + np.diag(np.full(n, 3.0) if unit else d)
    op = t_eff.T if trans else t_eff
    x = rng.integers(-8, 9, size=(n, nrhs) if left_side else (nrhs, n)).astype(np.float64)
    b = op @ x if left_side else x @ op  # every partial sum is a multiple of 1/4 below 2^20: exact in any order
    return t_stored, b, x


def _check_tri(t4a, n, nrhs, flags, seed):
    rng = np.random.default_rng(seed)
    for left_side, lower, trans, unit in flags:
        t, b, x = _tri_problem(rng, n, nrhs, left_side, lower, trans, unit)
        got = t4a.triangular_solve_matrix(t, b, left_side, lower, trans, unit)
        assert np.array_equal(got, x), (n, nrhs, left_side, lower, trans, unit, np.abs(got - x).max())


@pytest.mark.parametrize("n,nrhs,route", [
    (1, 1, "scalar kernel, cw 4"),
    (17, 16, "scalar kernel (n < 64), cw 4: a partial last chunk"),
    (65, 17, "matrix-core kernel, cw 16: a one-row last diagonal block, a one-column last chunk"),
    (1264, 5, "scalar kernel, cw 12 -> 3: odd chunks"),
])
def test_trsm_exact_all_flag_combinations(t4a, n, nrhs, route):
    _check_tri(t4a, n, nrhs, FLAGS, seed=n * 31 + nrhs)


@pytest.mark.parametrize("n,route", [
    (1, "scalar"), (15, "scalar"), (16, "scalar"), (17, "scalar"), (63, "scalar (n < 64 with any nrhs)"),
    (64, "matrix core from 16 rhs on"), (65, "matrix core from 16 rhs on"),
    (1263, "matrix core at its LDS limit (cw 16) from 16 rhs on; scalar cw 3 below"),
    (1264, "scalar cw 3 at every nrhs: one row past the matrix-core LDS limit"),
])
def test_trsm_exact_on_both_sides_of_every_switch(t4a, n, route):
    """nrhs 15 / 16 / 17 straddle the matrix-core threshold; 1 and 61 give one-column and odd last chunks (61 = 20 x 3 + 1)."""
    flags = [FLAGS[0], FLAGS[7], FLAGS[10], FLAGS[13]]  # left L N nonunit, left U T unit, right L T nonunit, right U N unit
    for nrhs in (1, 15, 16, 17, 61):
        _check_tri(t4a, n, nrhs, flags, seed=n * 131 + nrhs)


@pytest.mark.parametrize("nrhs", [1, 20])
def test_trsm_exact_ill_conditioned(t4a, nrhs):
    """Unit upper triangular with -1 above the diagonal: kappa ~ 2^n, inverse entries 2^(j - i - 1).  With b in {0, +-1} every |x_i| and
    every partial sum stays below 2^53 (n = 52): the exact answer, from Python integers, is representable and must come back bit for bit
    — through both kernels (nrhs 20: matrix cores) and every orientation of the same matrix."""
    n = 52
    rng = np.random.default_rng(5 + nrhs)
    u = np.triu(-np.ones((n, n)), 1) + np.eye(n)
    b = rng.integers(-1, 2, size=(n, nrhs)).astype(np.float64)
    x_left = _exact_unit_triangular(u, b, lower=False)     # U X = B
    x_right = _exact_unit_triangular(u.T, b, lower=True).T  # X U = B^T  <=>  U^T X^T = B
    assert np.abs(x_left).max() > 2.0 ** 40
    for unit in (False, True):
        for left_side in (True, False):
            for trans in (False, True):
                # op(T) is U in every case: stored as U (upper) or as U^T (lower, transposed)
                t = u.T if trans else u
                got = t4a.triangular_solve_matrix(t, b if left_side else b.T.copy(), left_side, trans, trans, unit)
                assert np.array_equal(got, x_left if left_side else x_right), (unit, left_side, trans)


def _exact_unit_triangular(t, b, lower):
    """Substitution in Python integers for a unit triangular integer t; asserts the answer is representable."""
    n, nrhs = b.shape
    ti = t.astype(np.int64).tolist()
    out = np.zeros((n, nrhs))
    order = range(n) if lower else range(n - 1, -1, -1)
    for c in range(nrhs):
        xs = [0] * n
        for i in order:
            xs[i] = int(b[i, c]) - sum(ti[i][j] * xs[j] for j in (range(i) if lower else range(i + 1, n)))
        assert max(abs(v) for v in xs) < 2 ** 53
        out[:, c] = xs
    return out


# ------------------------------------------------------------------------------------------------------------------ LU solve
SOLVE_ROUTES = [
    (1, 1, "blocked LU nb 32 + trsm"),
    (2, 3, "blocked LU nb 32 + trsm"),
    (31, 16, "blocked LU nb 32 + trsm (n < 32: not fused)"),
    (32, 15, "blocked LU nb 32 + trsm (nrhs < 16)"),
    (32, 16, "fused LU + solve nb 32"),
    (33, 17, "fused nb 32"),
    (255, 16, "fused nb 32"),
    (256, 20, "fused nb 32"),
    (257, 16, "fused nb 16"),
    (256, 15, "blocked nb 32 + trsm"),
    (257, 15, "blocked nb 16 + trsm"),
    (511, 17, "fused nb 16"),
    (512, 16, "fused nb 16"),
    (512, 15, "blocked nb 16 + trsm"),
    (513, 16, "blocked nb 8 + matrix-core trsm"),
    (513, 1, "blocked nb 8 + scalar trsm"),
    (1023, 17, "blocked nb 8"),
    (1024, 16, "blocked nb 8"),
    (1025, 16, "lu_kernel + two trsm"),
    (1025, 1, "lu_kernel + two scalar trsm"),
    (1500, 20, "lu_kernel + two trsm"),
]


@pytest.mark.parametrize("n,nrhs,route", SOLVE_ROUTES)
def test_solve_exact_on_every_route(t4a, n, nrhs, route):
    rng = np.random.default_rng(n * 7 + nrhs)
    a = _plu(rng, n, small=False)
    x = rng.integers(-4, 5, size=(n, nrhs)).astype(np.float64)
    b = a @ x  # multiples of 1/4 below 2^26: exact
    got = t4a.solve_matrix(a, b)
    assert np.array_equal(got, x), (route, np.abs(got - x).max())


@pytest.mark.parametrize("n,nrhs,route", SOLVE_ROUTES)
def test_solve_pivot_sensitive_on_every_route(t4a, n, nrhs, route):
    rng = np.random.default_rng(n * 11 + nrhs + 1)
    a = _plu(rng, n, small=True)
    x = rng.uniform(-1, 1, size=(n, nrhs))
    b = a @ x
    got = t4a.solve_matrix(a, b)
    kappa = np.linalg.cond(a, np.inf)
    assert kappa < 1e3
    fwd = np.abs(got - x).max() / np.abs(x).max()
    assert fwd <= 4 * n * EPS * kappa, (route, fwd, kappa)
    al, gl, bl = a.astype(np.longdouble), got.astype(np.longdouble), b.astype(np.longdouble)
    res = np.abs(bl - al @ gl).max()
    norm_a = np.abs(al).sum(axis=1).max()
    back = float(res / (norm_a * np.abs(gl).max() + np.abs(bl).max()))
    assert back <= 2 * n * EPS, (route, back)


# ----------------------------------------------------------------------------------------------------------------------- SVD
# Column norms of the pairs and the cosines between them.  alpha * beta (the product of two squared norms in the pair test) underflows
# for every pair; the inner product gamma = cos * norm^2 is subnormal from cos ~ 2e-8 on at 1e-150 and for every cosine at 2e-154.
PAIR_NORMS = [1e-150, 1e-151, 3e-152, 1e-153, 2e-154]
PAIR_COSINES = [1e-3, 1e-6, 1e-8, 1e-10, 1e-12]
PAIRS = [(s, c) for s in PAIR_NORMS for c in PAIR_COSINES]


def _scaled_svdvals(blk):
    """LAPACK singular values of a block after an exact power-of-two rescale to unit size."""
    e = int(np.frexp(np.abs(blk).max())[1])
    return np.ldexp(np.linalg.svd(np.ldexp(blk, -e), compute_uv=False), e)


def _mixed_scale_matrix(rng, m, n, pairs):
    """m x n (m >= n) with blocks on disjoint rows and columns (rows and columns then shuffled): one column of norm 1e-57, two-column
    blocks with the given (norm, cosine) — the second column 1.25 times longer than the first — and a graded block Q diag(d) whose d spans
    98 decades down to 1e-153 (every one of its columns live: above 1.49e-154 and 1e-100 sigma_max).  Returns the matrix and, per block, its
    columns and reference singular values."""
    a = np.zeros((m, n))
    blocks = []
    r = c = 0
    a[r, c] = 1e-57
    blocks.append(([c], np.array([1e-57])))
    r += 1
    c += 1
    for s, cos in pairs:
        q, _ = np.linalg.qr(rng.standard_normal((2, 2)))
        blk = np.column_stack([s * q[:, 0], 1.25 * s * (cos * q[:, 0] + np.sqrt(1.0 - cos * cos) * q[:, 1])])
        a[r:r + 2, c:c + 2] = blk
        blocks.append(([c, c + 1], _scaled_svdvals(blk)))
        r += 2
        c += 2
    g = n - c
    assert g >= 2 and r + g <= m
    q, _ = np.linalg.qr(rng.standard_normal((g, g)))
    d = np.logspace(-55, -153, g)
    a[r:r + g, c:c + g] = q * d
    blocks.append((list(range(c, c + g)), d))
    rp, cp = rng.permutation(m), rng.permutation(n)
    inv_c = np.argsort(cp)
    return a[rp][:, cp], [([int(inv_c[j]) for j in cols], sv) for cols, sv in blocks]


# (m, n, route): m x n with m >= n; every case runs in both orientations
SVD_ROUTES = [
    (40, 12, "one launch (jacobi_groups_kernel, V of 32 rows)"),
    (120, 40, "one launch (V of 64 rows, W of 128)"),
    (90, 90, "one launch (96 x 96 instantiation)"),
    (300, 12, "jacobi_small_kernel (n <= 16, m > 224)"),
    (300, 40, "blocked tournament (m > 224, n < 64)"),
    (200, 80, "QR-preconditioned, one launch on the 80 x 80 factor"),
    (260, 110, "QR-preconditioned, blocked tournament on the 110 x 110 factor"),
]
# Known defect, kept visible: behind the Householder QR, the blocked tournament on the 110 x 110 factor L = R^T does not converge within
# 60 sweeps and the right factor comes back far from orthonormal (|V^T V - I| ~ 0.9) — with or without the tiny pairs, i.e. for the graded
# block alone.  The same blocks without the QR in front (300 x 40) and behind it on an 80 x 80 factor (one launch) are fine.
QR_BLOCKED_DEFECT = (260, 110)


def _route_cases(m, n):
    """The matrices of one route: PAIRS spread over as many matrices as needed (at most (n - 3) / 2 pairs per matrix: the graded block
    keeps at least two columns)."""
    per = (n - 3) // 2
    return [PAIRS[i:i + per] for i in range(0, len(PAIRS), per)]


def _check_svd(t4a, a, blocks, label, wide):
    """wide: `a` is the transpose of the matrix _mixed_scale_matrix built (the blocks' columns are rows of `a`)."""
    m, n = a.shape
    k = min(m, n)
    u, s, vt = t4a.svd_backend(a)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(s)) and np.all(np.isfinite(vt)), label
    smax = max(sv.max() for _, sv in blocks)
    sref = np.sort(np.concatenate([sv for _, sv in blocks] + [np.zeros(k - sum(len(sv) for _, sv in blocks))]))[::-1]
    assert np.abs(s - sref).max() <= 1e-12 * smax, label
    assert np.abs(u.T @ u - np.eye(k)).max() < 1e-10, (label, np.abs(u.T @ u - np.eye(k)).max())
    assert np.abs(vt @ vt.T - np.eye(k)).max() < 1e-10, (label, np.abs(vt @ vt.T - np.eye(k)).max())
    assert np.abs((u * s) @ vt - a).max() <= 1e-12 * smax * k, label
    # each block on its own: the singular values whose right singular vectors (left ones in the wide orientation) live on a block's
    # columns are that block's, to 1e-10 relative
    v = u if wide else vt.T
    for cols, sv in blocks:
        weight = (v[cols, :] ** 2).sum(axis=0)
        mine = np.sort(s[weight > 0.5])[::-1]
        assert len(mine) == len(sv), (label, cols, len(mine), len(sv))
        rel = np.abs(mine - np.sort(sv)[::-1]) / np.sort(sv)[::-1]
        assert rel.max() <= 1e-10, (label, cols, rel.max(), sv)


@pytest.mark.parametrize("m,n,route", [
    pytest.param(m, n, r, marks=pytest.mark.xfail(strict=True, reason="QR-preconditioned route: no convergence on a 98-decade graded "
                                                                       "factor (QR_BLOCKED_DEFECT)"))
    if (m, n) == QR_BLOCKED_DEFECT else (m, n, r) for m, n, r in SVD_ROUTES])
def test_svd_mixed_column_scales_inside_the_unscaled_band(t4a, m, n, route):
    rng = np.random.default_rng(m * 1009 + n)
    for i, pairs in enumerate(_route_cases(m, n)):
        a, blocks = _mixed_scale_matrix(rng, m, n, pairs)
        assert 2.0 ** -200 <= np.abs(a).max() <= 2.0 ** 200  # (the band Engine::svd does not rescale)
        _check_svd(t4a, a, blocks, (route, i, "tall"), wide=False)
        # the wide orientation: the blocks' columns become rows; the per-block check reads U instead of V
        _check_svd(t4a, a.T.copy(), blocks, (route, i, "wide"), wide=True)


def test_svd_mixed_column_scales_converge_on_every_route():
    """The iteration must stop because no pair needs a rotation, not because it ran out of sweeps: every decomposition above, in a child
    process with T4A_SVD_DEBUG=1, reports convergence (one line per Jacobi iteration, engine.hip svd_plain).  QR_BLOCKED_DEFECT aside."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys
sys.path.insert(0, os.path.join(%r, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, t4a_amd
import test_gpu_dense_exact as t
calls = 0
for m, n, route in t.SVD_ROUTES:
    if (m, n) == t.QR_BLOCKED_DEFECT:
        continue
    rng = np.random.default_rng(m * 1009 + n)
    for pairs in t._route_cases(m, n):
        a, _ = t._mixed_scale_matrix(rng, m, n, pairs)
        for x in (a, a.T.copy()):
            t4a_amd.svd_backend(x)
            calls += 1
print("CALLS", calls)
""" % (root, root)
    env = dict(os.environ)
    env["T4A_SVD_DEBUG"] = "1"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    calls = int(re.search(r"CALLS (\d+)", out.stdout).group(1))
    lines = [l for l in out.stderr.splitlines() if l.startswith("[t4a svd]")]
    bad = [l for l in lines if "converged within" not in l]
    assert not bad, bad[:10]
    sweeps = [int(re.search(r"within (\d+) sweeps", l).group(1)) for l in lines]
    assert len(lines) == calls, (len(lines), calls, out.stderr[-3000:])
    assert all(0 < w < 60 for w in sweeps), sweeps
