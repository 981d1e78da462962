"""Numpy restatement of the gauge forms of tensor4all-simplett — SiteTensorTrain / center_canonicalize (canonical.rs:118-393, :439-544),
VidalTensorTrain (vidal.rs:215-493) and InverseTensorTrain (vidal.rs:551-767) — and the fixtures of tests/test_cpu_canonical.py and
tests/test_gpu_canonical.py.

The reference's `qr_decomp` is rrlu(matrix, {max_bond_dim: min(m, n), rel_tol: 0, abs_tol: 0, left_orthogonal: true}) followed by
lu.left(true) / lu.right(true) (canonical.rs:17-29): the rrLU goes through the CPU oracle, the factors are built from the factored
matrix and the permutations as matrixlu.rs:263-326 does.  Cores are numpy arrays (l, s, r); every function returns new arrays.
"""
from fractions import Fraction

import numpy as np

import oracle_binding as ob

SEED = 20260417
GUARD = 1e-15


# ------------------------------------------------------------------------------------------------ matrices of a core
def left_matrix(core):  # tensor3_to_left_matrix: row l * S + s (canonical.rs:39-55)
    l, s, r = core.shape
    return np.ascontiguousarray(core.reshape(l * s, r))


def right_matrix(core):  # tensor3_to_right_matrix: column s * R + r (canonical.rs:58-74)
    l, s, r = core.shape
    return np.ascontiguousarray(core.reshape(l, s * r))


def lu_for_qr(mat):
    """qr_decomp (canonical.rs:17-29): (left(true), right(true)) of the rrLU that stops only at an exactly zero pivot."""
    m, n = mat.shape
    f, rp, cp, k, _ = ob.rrlu(mat, max_bond_dim=min(m, n), rel_tol=0.0, abs_tol=0.0, left_orthogonal=True)
    lo = np.tril(f[:, :k]).copy()
    lo[np.arange(k), np.arange(k)] = 1.0
    up = np.triu(f[:k, :]).copy()
    left = np.zeros_like(lo)
    left[rp, :] = lo
    right = np.zeros_like(up)
    right[:, cp] = up
    return left, right


def left_step(core_i, core_next):
    """make_left_orthogonal (canonical.rs:191-241): (new core i, new core i + 1)"""
    l, s, _ = core_i.shape
    q, r = lu_for_qr(left_matrix(core_i))
    k = q.shape[1]
    _, ns, nr = core_next.shape
    return q.reshape(l, s, k), (r @ right_matrix(core_next)).reshape(k, ns, nr)


def right_step(core_prev, core_i):
    """make_right_orthogonal (canonical.rs:244-291), lq_decomp literally (:32-36): (new core i - 1, new core i)"""
    _, s, r = core_i.shape
    qt, lt = lu_for_qr(np.ascontiguousarray(right_matrix(core_i).T))
    lmat, q = lt.T, qt.T
    k = q.shape[0]
    pl, ps, _ = core_prev.shape
    return (left_matrix(core_prev) @ lmat).reshape(pl, ps, k), np.ascontiguousarray(q).reshape(k, s, r)


def step_factors(core, left):
    """the two factors of one gauge step on their own: (left(true), right(true)) of the matrix the step factorises"""
    return lu_for_qr(left_matrix(core) if left else np.ascontiguousarray(right_matrix(core).T))


# ------------------------------------------------------------------------------------------------ whole objects
def site_form(cores, center):
    """SiteTensorTrain::new / center_canonicalize (canonical.rs:172-188, :439-544)"""
    t = [np.array(c, dtype=np.float64) for c in cores]
    n = len(t)
    if n <= 1 or center >= n:
        return t
    for i in range(center):
        t[i], t[i + 1] = left_step(t[i], t[i + 1])
    for i in range(n - 1, center, -1):
        t[i - 1], t[i] = right_step(t[i - 1], t[i])
    return t


def np_svd(a):
    u, s, vt = np.linalg.svd(a, full_matrices=False)
    return u, s, vt


def vidal_form(cores, start=0, end=None, svd=np_svd):
    """from_tensor_train_with_partition (vidal.rs:229-395): (tensors, singular value vectors)"""
    t = [np.array(c, dtype=np.float64) for c in cores]
    n = len(t)
    end = n if end is None else end
    sv = [np.zeros(0) for _ in range(max(n - 1, 0))]
    if n == 0:
        return t, sv
    for i in range(start, max(end - 1, 0)):
        t[i], t[i + 1] = left_step(t[i], t[i + 1])
    for i in range(end - 1, start, -1):
        _, s, r = t[i].shape
        u, sing, vt = svd(right_matrix(t[i]))
        sv[i - 1] = np.array(sing)
        k = vt.shape[0]
        pl, ps, _ = t[i - 1].shape
        t[i - 1] = (left_matrix(t[i - 1]) @ (u * sing[None, :])).reshape(pl, ps, k)
        t[i] = np.ascontiguousarray(vt).reshape(k, s, r)
    for i in range(start, max(end - 1, 0)):
        if len(sv[i]):
            t[i] = scale_right(t[i], sv[i], divide=True)
    return t, sv


def _factors(vec, dim, divide=False):
    f = np.ones(dim)
    k = min(len(vec), dim)
    v = np.asarray(vec, dtype=np.float64)[:k]
    f[:k] = np.where(v > GUARD, v, 1.0) if divide else v
    return f


def scale_right(core, vec, divide=False):
    """val * sv[r] (vidal.rs:476-481) or val / (sv[r] > 1e-15 ? sv[r] : 1.0) (:378-383); r beyond the vector: 1.0"""
    f = _factors(vec, core.shape[2], divide)[None, None, :]
    return core / f if divide else core * f


def scale_left(core, vec):
    return core * _factors(vec, core.shape[0])[:, None, None]


def vidal_to_tt(tensors, sv):  # vidal.rs:456-492
    n = len(tensors)
    return [scale_right(tensors[i], sv[i]) if i + 1 < n else tensors[i].copy() for i in range(n)]


def inverse_from_vidal(tensors, sv):
    """from_vidal (vidal.rs:551-663): (val * sv[i-1][l]) * sv[i][r] in that order; inverse values 1/v if |v| > 1e-15 else 0"""
    n = len(tensors)
    out = []
    for i, t in enumerate(tensors):
        x = t.copy()
        if i > 0:
            x = scale_left(x, sv[i - 1])
        if i + 1 < n:
            x = scale_right(x, sv[i])
        out.append(x)
    with np.errstate(divide="ignore", over="ignore"):
        inv = [np.where(np.abs(v) > GUARD, 1.0 / np.where(v == 0.0, 1.0, v), 0.0) for v in (np.asarray(v, dtype=np.float64) for v in sv)]
    return out, inv


def inverse_to_tt(tensors, inv):  # vidal.rs:730-766
    return vidal_to_tt(tensors, inv)


# ------------------------------------------------------------------------------------------------ values
def dense(cores):
    """all values, shape = site dims"""
    cur = np.ones((1, 1))
    for c in cores:
        l, s, r = c.shape
        cur = (cur @ c.reshape(l, s * r)).reshape(-1, r)
    return cur.reshape([c.shape[1] for c in cores])


def evaluate_seq(cores, idx):
    """AbstractTensorTrain::evaluate (traits.rs:146-212) with its summation order: the bond index ascending from 0.0, multiply and add
    rounded separately — bit for bit what t4a_gpu_tt_evaluate and the oracle compute."""
    out = np.zeros(len(idx))
    for p, point in enumerate(idx):
        cur = cores[0][0, point[0], :].copy()
        for c, i in zip(cores[1:], point[1:]):
            nxt = np.zeros(c.shape[2])
            for r in range(c.shape[2]):
                acc = 0.0
                for l in range(c.shape[0]):
                    acc = acc + cur[l] * c[l, i, r]
                nxt[r] = acc
            cur = nxt
        out[p] = cur[0]
    return out


def lcg_points(n_pts, site_dims, seed):
    x = (seed * 2862933555777941757 + 3037000493) % (1 << 64)
    pts = np.zeros((n_pts, len(site_dims)), dtype=np.int64)
    for p in range(n_pts):
        for k, d in enumerate(site_dims):
            x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            pts[p, k] = (x >> 33) % d
    return pts


def all_points(site_dims):
    return np.array(list(np.ndindex(*site_dims)), dtype=np.int64).reshape(-1, len(site_dims))


def rows_orthonormal_defect(tensors, sv, start=0, end=None):
    """max over the sites start < i < end of |M M^T - 1| for M the right matrix of Gamma_i lambda_i (the last site: Gamma itself)"""
    worst = 0.0
    n = len(tensors)
    for i in range(start + 1, n if end is None else end):
        m = right_matrix(scale_right(tensors[i], sv[i]) if i + 1 < n else tensors[i])
        worst = max(worst, float(np.abs(m @ m.T - np.eye(m.shape[0])).max()))
    return worst


# ------------------------------------------------------------------------------------------------ fixtures
def random_train(site_dims, bonds, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((bonds[i], d, bonds[i + 1])) for i, d in enumerate(site_dims)]


def fixture_a():
    return random_train([2, 3, 2, 4, 3], [1, 2, 5, 6, 3, 1], SEED)


def fixture_b():
    return random_train([2, 2, 2, 2], [1, 4, 7, 4, 1], SEED + 1)


def fixture_c(index=3):
    t = fixture_a()
    t[1][:, :, index] = 0.0  # one index of bond 2 (dimension 5) zeroed on both neighbours
    t[2][index, :, :] = 0.0
    return t


def monomial_chain(powers):
    """D1 (powers=True: values +-2^e, e distinct within a matrix and their running sums distinct along the left sweep) and D2 (all +-1):
    every core's left matrix has one nonzero per column, in distinct rows"""
    site_dims, bonds = [2, 3, 2, 3], [1, 2, 4, 3, 1]
    rng = np.random.default_rng(SEED + (2 if powers else 3))
    cores, base = [], 1
    for i, d in enumerate(site_dims):
        l, r = bonds[i], bonds[i + 1]
        c = np.zeros((l, d, r))
        rows = rng.permutation(l * d)[:r]
        for col, row in enumerate(rows):
            sign = -1.0 if rng.integers(0, 2) else 1.0
            c[row // d, row % d, col] = sign * (2.0 ** (col * base) if powers else 1.0)
        base *= r
        cores.append(c)
    return cores


def fixture_d1():
    return monomial_chain(True)


def fixture_d2():
    return monomial_chain(False)


def fixture_e():
    """6 sites of dimension 2, bonds [1, 2, 4, 40, 4, 2, 1]: 8 x 40 and 40 x 8 matrices at the middle bond, which the sweeps cut to 8"""
    return random_train([2, 2, 2, 2, 2, 2], [1, 2, 4, 40, 4, 2, 1], SEED + 4)


def fixture_e2():
    """Sites of dimension 2 cannot hold a bond of 40 six sites from an end, so the 80 x 40 and 40 x 80 matrices of E are embedded between
    two sites of dimension 40: site dims [40, 2, 2, 40], bonds [1, 40, 40, 40, 1].  The left step at site 1 factorises an 80 x 40 left
    matrix, the right step at site 2 the transpose of a 40 x 80 right matrix — beyond the one-wavefront rrLU and the scalar GEMM."""
    return random_train([40, 2, 2, 40], [1, 40, 40, 40, 1], SEED + 9)


def fixture_f():
    return [random_train([3], [1, 1], SEED + 5), random_train([2, 3], [1, 4, 1], SEED + 6)]


G_VALUES = [0.0, 1e-15, float(np.nextafter(1e-15, 1.0)), -3.0, 1e-300, 1e300]


def fixture_g():
    """(cores, vectors) for the scale kernel alone: cores (1,2,3), (3,3,5), (5,1,2), (2,4,1); vectors of lengths 3 (exact), 3 (SHORTER
    than its bond 5) and 4 (LONGER than its bond 2) holding the guard cases"""
    rng = np.random.default_rng(SEED + 7)
    cores = [rng.standard_normal(s) for s in ((1, 2, 3), (3, 3, 5), (5, 1, 2), (2, 4, 1))]
    vecs = [np.array([0.0, 1e-15, G_VALUES[2]]), np.array([-3.0, 1e-300, 1e300]), np.array([2.5, 0.0, 7.0, -1.0])]
    return cores, vecs


def fixture_g_large(min_items):
    """one core with more items than the scale kernel launches workgroups: (256, 2, r) has r / 2 items of 4 columns of 256 lanes"""
    r = 2 * min_items + 6
    rng = np.random.default_rng(SEED + 8)
    cores = [rng.standard_normal((1, 2, 256)), rng.standard_normal((256, 2, r)), rng.standard_normal((r, 1, 1))]
    vecs = [rng.standard_normal(256), np.concatenate([rng.standard_normal(r - 4), G_VALUES[:4]])]
    return cores, vecs


# ------------------------------------------------------------------------------------------------ exact expectation (D1, D2)
def _exact_rrlu(a):
    """Full-pivot LU in rational arithmetic with the reference's scan (column-major, the first strictly larger magnitude wins,
    matrixlu.rs:742-791) and its swaps; stops at an exactly zero pivot.  Returns (left(true), right(true)) as Fraction arrays."""
    m, n = len(a), len(a[0])
    a = [row[:] for row in a]
    rp, cp = list(range(m)), list(range(n))
    k = 0
    while k < min(m, n):
        best, br, bc = a[k][k] * a[k][k], k, k
        for col in range(k, n):
            for row in range(k, m):
                v = a[row][col] * a[row][col]
                if v > best:
                    best, br, bc = v, row, col
        if best == 0:
            break
        a[k], a[br] = a[br], a[k]
        rp[k], rp[br] = rp[br], rp[k]
        for row in a:
            row[k], row[bc] = row[bc], row[k]
        cp[k], cp[bc] = cp[bc], cp[k]
        piv = a[k][k]
        for row in range(k + 1, m):
            a[row][k] = a[row][k] / piv
        for row in range(k + 1, m):
            for col in range(k + 1, n):
                a[row][col] = a[row][col] - a[row][k] * a[k][col]
        k += 1
    left = [[Fraction(0)] * k for _ in range(m)]
    right = [[Fraction(0)] * n for _ in range(k)]
    for i in range(m):
        for j in range(min(i + 1, k)):
            left[rp[i]][j] = Fraction(1) if i == j else a[i][j]
    for i in range(k):
        for j in range(i, n):
            right[i][cp[j]] = a[i][j]
    return left, right


def _fr(mat):
    return [[Fraction(float(x)) for x in row] for row in mat]


def _fl(rows, shape):
    return np.array([[float(x) for x in row] for row in rows], dtype=np.float64).reshape(shape)


def _mul(a, b):
    return [[sum((a[i][k] * b[k][j] for k in range(len(b))), Fraction(0)) for j in range(len(b[0]))] for i in range(len(a))]


def exact_site_form(cores, center):
    """The site form in exact rational arithmetic, independent of the oracle and of any rounding: what the reference computes when no
    operation rounds (the monomial chains D1 and D2).  Raises if a value is not a double."""
    t = [np.array(c, dtype=np.float64) for c in cores]
    n = len(t)

    def back(rows, shape):
        out = _fl(rows, shape)
        assert all(Fraction(float(v)) == x for v, x in zip(out.reshape(-1), (x for row in rows for x in row))), "not exact in double"
        return out

    for i in range(center):
        l, s, _ = t[i].shape
        _, ns, nr = t[i + 1].shape
        q, r = _exact_rrlu(_fr(left_matrix(t[i])))
        k = len(r)
        t[i] = back(q, (l * s, k)).reshape(l, s, k)
        t[i + 1] = back(_mul(r, _fr(right_matrix(t[i + 1]))), (k, ns * nr)).reshape(k, ns, nr)
    for i in range(n - 1, center, -1):
        _, s, r = t[i].shape
        pl, ps, _ = t[i - 1].shape
        qt, lt = _exact_rrlu(_fr(right_matrix(t[i]).T))
        k = len(lt)
        lmat = [[lt[b][a] for b in range(k)] for a in range(len(lt[0]))]
        t[i - 1] = back(_mul(_fr(left_matrix(t[i - 1])), lmat), (pl * ps, k)).reshape(pl, ps, k)
        t[i] = np.ascontiguousarray(back(qt, (s * r, k)).T).reshape(k, s, r)
    return t
