"""Matrices whose LUCI factors are exact by construction (numpy + the standard library only).

A0 (M x N, exact rank R = sum r_t) is made of blocks on disjoint rows and columns; block t is L_t diag(d_t) U_t with L_t (m_t x r_t) unit
lower trapezoidal, U_t (r_t x n_t) unit upper trapezoidal, every other entry from {0, +-1/4, +-1/2}, and d_t[k] = c_t 2^(-2k),
c_t = +-(64 - t)/64 (c_0 = 1).  All |d| are distinct, the largest is 1, and after any number of pivots the largest entry of what is
left is strictly the next d (inside a block every other entry is below 5/6 of the block's next d: at most 1/2 from the term of that d,
at most 1/4 + 1/16 + ... = 1/3 from the later ones), so full pivoting has no ties and takes the (t, k) by |d| descending.
A = A0[rp][:, cp] with random permutations.

Every multiplier is then an exact quotient and every Schur update exact, the factorisation stops at rank R (or at max_bond_dim), and

    left-orthogonal:   right == A[I, :] bit for bit,  left == A[:, J] A[I, J]^-1
    right-orthogonal:  left == A[:, J] bit for bit,   right == A[I, J]^-1 A[I, :]

with the inverse halves computed here in fractions.Fraction, block by block, and asserted to be representable in binary64.

bit_budget() is the condition under which ANY summation order (scalar loops, blocked substitution, matrix-core accumulation, split-K)
returns those bits: for every sum the kernels form, the sum of the absolute terms, counted in the terms' common power-of-two unit, stays
below 2^52.

route_of() mirrors the launchers (kernels_dense.hip luci_factors_small_launch, trsm_left_batched_launch, gemm_launch; engine.hip
Engine::build_factors_from); CASES names the route each case is there for, and test_cpu_luci_exact.py holds the two together.
"""
from fractions import Fraction

import numpy as np

REL_TOL = 1e-15  # the smallest pivot of a rank-24 block is 2^-46 ~ 1.4e-14 of the largest
ABS_TOL = 0.0
ENTRIES = (0, 0, 1, -1, 2, -2)  # quarters: {0, +-1/4, +-1/2}


class Fixture:
    """a: the matrix; rows / cols: the pivots in the order full pivoting takes them (all R of them)."""

    def __init__(self, a, rows, cols, blocks):
        self.a = a
        self.rows = rows
        self.cols = cols
        self._blocks = blocks  # per block: (rows of A of its m_t block rows, columns of A of its n_t block columns, Fraction entries)

    def expected(self, left_orthogonal, max_bond_dim=None):
        """(rank, rows, cols, left, right) under an optional rank cap."""
        r = len(self.rows) if max_bond_dim is None else min(len(self.rows), max_bond_dim)
        rows, cols = self.rows[:r], self.cols[:r]
        m, n = self.a.shape
        if left_orthogonal:
            right = self.a[rows, :].copy()
            left = np.zeros((m, r))
        else:
            left = self.a[:, cols].copy()
            right = np.zeros((r, n))
        pos = {(int(i), int(j)): q for q, (i, j) in enumerate(zip(rows, cols))}
        for brow, bcol, f in self._blocks:
            # this block's pivots among the first r, in block order k = 0, 1, ...: the leading k x k minor of the block
            qs = [pos[(brow[k], bcol[k])] for k in range(min(len(brow), len(bcol))) if (brow[k], bcol[k]) in pos]
            k = len(qs)
            if k == 0:
                continue
            p = [row[:k] for row in f[:k]]
            if left_orthogonal:  # X P = F[:, :k]
                x = _solve_xp(p, [row[:k] for row in f])
                for i, xi in enumerate(x):
                    for c, v in enumerate(xi):
                        left[brow[i], qs[c]] = _to_double(v)
            else:  # P Y = F[:k, :]  <=>  Y^T P^T = F[:k, :]^T
                pt = [[p[j][i] for j in range(k)] for i in range(k)]
                ncol = len(bcol)
                yt = _solve_xp(pt, [[f[i][j] for i in range(k)] for j in range(ncol)])
                for j, yj in enumerate(yt):
                    for c, v in enumerate(yj):
                        right[qs[c], bcol[j]] = _to_double(v)
        return r, rows, cols, left, right


def _to_double(v):
    x = float(v)
    assert Fraction(x) == v, "a reference entry is not representable in binary64"
    return x


def _solve_xp(p, b):
    """X with X P = B (Fractions; P k x k with non-singular leading minors, B rows of length k): eliminate the columns of [P; B]."""
    k = len(p)
    p = [row[:] for row in p]
    b = [row[:] for row in b]
    for c in range(k):  # column operations: col_j -= col_c * p[c][j] / p[c][c] for j > c, on P and B alike
        piv = p[c][c]
        assert piv != 0
        fac = [p[c][j] / piv for j in range(k)]
        for rows in (p, b):
            for row in rows:
                rc = row[c]
                if rc != 0:
                    for j in range(c + 1, k):
                        if fac[j] != 0:
                            row[j] -= rc * fac[j]
    # P is now lower triangular: X P = B by back substitution from the last column
    out = []
    for row in b:
        x = [Fraction(0)] * k
        for j in range(k - 1, -1, -1):
            s = row[j]
            for q in range(j + 1, k):
                if x[q] != 0 and p[q][j] != 0:
                    s -= x[q] * p[q][j]
            x[j] = s / p[j][j]
        out.append(x)
    return out


def _split(total, ranks):
    """Block sizes: each block its rank, the remaining rows (columns) dealt round robin."""
    assert total >= sum(ranks)
    sizes = list(ranks)
    extra = total - sum(ranks)
    for q in range(extra):
        sizes[q % len(ranks)] += 1
    return sizes


def build(m, n, ranks, seed):
    """The fixture for an m x n matrix with blocks of the given ranks."""
    rng = np.random.default_rng(seed)
    assert 1 <= len(ranks) <= 16 and max(ranks) <= 24
    ms, ns = _split(m, ranks), _split(n, ranks)
    a0 = np.zeros((m, n))
    blocks0 = []
    pivots = []  # (|d|, A0 row, A0 column)
    r0 = c0 = 0
    for t, r in enumerate(ranks):
        mt, nt = ms[t], ns[t]
        lq = np.tril(rng.choice(ENTRIES, size=(mt, r)), -1)  # quarters
        uq = np.triu(rng.choice(ENTRIES, size=(r, nt)), 1)
        for k in range(r):
            lq[k, k] = 4
            uq[k, k] = 4
        sign = int(rng.choice((-1, 1))) if t else 1  # (c_0 = +1: the largest entry of A is 1 itself)
        d = [Fraction(sign * (64 - t), 64) / 4 ** k for k in range(r)]
        f = []
        for i in range(mt):
            li = [int(v) for v in lq[i]]
            row = []
            for j in range(nt):
                s = Fraction(0)
                for k in range(min(i, j, r - 1) + 1):
                    if li[k] and uq[k, j]:
                        s += li[k] * int(uq[k, j]) * d[k]
                row.append(s / 16)
            f.append(row)
            a0[r0 + i, c0:c0 + nt] = [_to_double(v) for v in row]
        blocks0.append((r0, mt, c0, nt, f))
        pivots += [(abs(d[k]), r0 + k, c0 + k) for k in range(r)]
        r0 += mt
        c0 += nt
    assert len({p[0] for p in pivots}) == len(pivots) and max(p[0] for p in pivots) == 1
    rp, cp = rng.permutation(m), rng.permutation(n)
    inv_r, inv_c = np.argsort(rp), np.argsort(cp)  # A[i, j] = A0[rp[i], cp[j]]: row g of A0 is row inv_r[g] of A
    pivots.sort(key=lambda p: -p[0])
    rows = np.array([inv_r[p[1]] for p in pivots], dtype=np.int64)
    cols = np.array([inv_c[p[2]] for p in pivots], dtype=np.int64)
    blocks = [([int(inv_r[r0 + i]) for i in range(mt)], [int(inv_c[c0 + j]) for j in range(nt)], f) for r0, mt, c0, nt, f in blocks0]
    return Fixture(np.ascontiguousarray(a0[rp][:, cp]), rows, cols, blocks)


# ------------------------------------------------------------------------------------------------------------------ bit budget
_INF = 1 << 20


def _lsb_exponent(x):
    """e with x = odd * 2^e, elementwise (_INF for zero)."""
    mant, ex = np.frexp(x)
    mi = np.ldexp(np.abs(mant), 53).astype(np.int64)  # exact: 53-bit integers
    low = mi & -mi
    tz = np.zeros(x.shape, dtype=np.int64)
    nz = mi != 0
    tz[nz] = np.round(np.log2(low[nz].astype(np.float64))).astype(np.int64)
    return np.where(nz, ex.astype(np.int64) - 53 + tz, _INF)


def _budget(a, b, extra=None):
    """Bits needed by the sums sum_k a[i, k] b[k, j] (+ extra[i, j]): log2 of (sum of |terms| / the terms' common unit), maximised over
    (i, j).  Structural zeros of a and b are terms that no kernel's rounding can see (0 * x = 0, s + 0 = s)."""
    absum = np.abs(a) @ np.abs(b)  # rounded upwards below by a relative 1e-9
    la, lb = _lsb_exponent(a), _lsb_exponent(b)
    unit = np.full(absum.shape, _INF, dtype=np.int64)
    for k in range(a.shape[1]):
        np.minimum(unit, np.minimum(la[:, k, None] + lb[None, k, :], _INF), out=unit)
    if extra is not None:
        absum = absum + np.abs(extra)
        np.minimum(unit, _lsb_exponent(extra), out=unit)
    live = (unit < _INF) & (absum > 0)
    if not live.any():
        return 0.0
    return float(np.max(np.log2(absum[live] * (1 + 1e-9)) - unit[live]))


def bit_budget(factored, row_perm, col_perm, rank, left_orthogonal, left, right):
    """The largest bit count over every sum the factor kernels form, from the factored buffer of rrlu (permuted coordinates) and the
    exact factors `left`, `right` (original coordinates):
    left-orthogonal:  x L11 = L21(i, :) -> terms L21(i, j) and x_k L11(k, j), k > j;   (L11 U)(i, j) -> terms L11(i, k) U(k, j)
    right-orthogonal: U11 x = U12(:, j) -> terms U12(i, j) and U11(i, k) x_k, k > i;   (L U11)(i, j) -> terms L(i, k) U11(k, j)."""
    m, n = factored.shape
    r = rank
    if left_orthogonal:
        l11 = np.tril(factored[:r, :r], -1)
        x = left[row_perm[r:], :]  # the solved rows, permuted order
        sub = _budget(x, l11, extra=factored[r:, :r]) if m > r else 0.0
        prod = _budget(l11 + np.eye(r), np.triu(factored[:r, :]))
    else:
        u11 = np.triu(factored[:r, :r], 1)
        x = right[:, col_perm[r:]]
        sub = _budget(u11, x, extra=factored[:r, r:]) if n > r else 0.0
        prod = _budget(np.tril(factored[:, :r]), u11 + np.eye(r))
    return max(sub, prod)


# ---------------------------------------------------------------------------------------------------------------------- routes
def _gemm_ksplit(m, n, k):
    """gemm_launch (kernels_dense.hip): GBM = 64, GBK = 32."""
    tiles64 = ((m + 63) // 64) * ((n + 63) // 64)
    narrow = tiles64 < 512 and n > 32
    tiles = ((m + 63) // 64) * ((n + (31 if narrow else 63)) // (32 if narrow else 64))
    ktiles = (k + 31) // 32
    if tiles < 256 and ktiles >= 8:
        return max(1, min(16, ktiles // 2, (512 + tiles - 1) // tiles))
    return 1


def route_of(m, n, rank, left_orthogonal):
    """The launch route of Engine::build_factors_from for an m x n factorisation of the given rank."""
    if rank < 1:
        return "none"
    if rank <= 16 and m <= 1024 and n <= 1024:  # luci_factors_small_launch
        return "one launch, %d workgroup%s" % ((max(m, n) + 255) // 256, "" if max(m, n) <= 256 else "s")
    nrhs = (m if left_orthogonal else n) - rank
    if nrhs == 0:
        trsm = "no trsm"
    elif rank >= 64 and nrhs >= 16:  # trsm_left_batched_launch (its LDS limit, 1263 rows, is far away)
        trsm = "matrix-core trsm"
    else:
        trsm = "scalar trsm"
    ks = _gemm_ksplit(rank, n, rank) if left_orthogonal else _gemm_ksplit(m, rank, rank)
    return "general, %s, %s" % (trsm, "split-K gemm" if ks > 1 else "gemm")


# (m, n, block ranks, max_bond_dim, route left-orthogonal, route right-orthogonal)
G, S, MC = "general, ", "scalar trsm, gemm", "matrix-core trsm, gemm"
CASES = [
    (8, 6, [4], None, "one launch, 1 workgroup", "one launch, 1 workgroup"),
    (33, 20, [1], None, "one launch, 1 workgroup", "one launch, 1 workgroup"),
    (40, 50, [16], None, "one launch, 1 workgroup", "one launch, 1 workgroup"),  # rk = 16, the last rank of the kernel
    (12, 30, [12], None, "one launch, 1 workgroup", "one launch, 1 workgroup"),  # rk == M: no L21 rows
    (30, 12, [12], None, "one launch, 1 workgroup", "one launch, 1 workgroup"),  # rk == N: no U12 columns
    (1024, 40, [3, 2], None, "one launch, 4 workgroups", "one launch, 4 workgroups"),
    (40, 1024, [3, 2], None, "one launch, 4 workgroups", "one launch, 4 workgroups"),
    (1025, 40, [3, 2], None, G + S, G + S),  # general by size
    (40, 1025, [3, 2], None, G + S, G + S),
    (64, 64, [17], None, G + S, G + S),  # general by rank
    (70, 90, [24], None, G + S, G + S),
    (20, 20, [20], None, G + "no trsm, gemm", G + "no trsm, gemm"),  # rk == M == N
    (79, 100, [8] * 8, None, G + S, G + MC),  # rk = 64, M - rk = 15 | N - rk = 36
    (80, 100, [8] * 8, None, G + MC, G + MC),  # M - rk = 16
    (100, 79, [8] * 8, None, G + MC, G + S),  # N - rk = 15
    (100, 80, [8] * 8, None, G + MC, G + MC),  # N - rk = 16
    (100, 100, [8] * 7 + [7], None, G + S, G + S),  # rk = 63
    (120, 110, [16] * 5, None, G + MC, G + MC),  # rk = 80: the last diagonal block of the blocked substitution is whole, nrhs is not
    (100, 90, [8] * 8, None, G + MC, G + MC),
    (130, 150, [8] * 12, None, G + MC, G + MC),  # rk = 96
    (120, 110, [12, 5, 16, 1, 9, 16, 3], None, G + S, G + S),  # rk = 62, mixed block ranks
    (200, 180, [16] * 6, None, G + MC, G + MC),  # rk = 96
    (300, 310, [15] * 16, None, G + "matrix-core trsm, split-K gemm", G + "matrix-core trsm, split-K gemm"),  # rk = 240
    (40, 50, [16], 10, "one launch, 1 workgroup", "one launch, 1 workgroup"),
    (70, 90, [24], 16, "one launch, 1 workgroup", "one launch, 1 workgroup"),  # a rank-24 matrix cut to the kernel's last rank
    (100, 90, [8] * 8, 20, G + S, G + S),
]


def case_id(case):
    m, n, ranks, cap = case[:4]
    return "%dx%d-r%d%s" % (m, n, sum(ranks), "" if cap is None else "-cap%d" % cap)


def case_seed(case):
    m, n, ranks, _ = case[:4]
    return 1000003 * m + 1009 * n + 7 * sum(ranks) + len(ranks)


_cache = {}


def fixture(case):
    """The fixture of a case (built once per process; the expected factors are cached per orientation as well)."""
    key = (case[0], case[1], tuple(case[2]))
    if key not in _cache:
        _cache[key] = (build(case[0], case[1], case[2], case_seed(case)), {})
    return _cache[key][0]


def expected(case, left_orthogonal):
    fx = fixture(case)
    memo = _cache[(case[0], case[1], tuple(case[2]))][1]
    k = (left_orthogonal, case[3])
    if k not in memo:
        memo[k] = fx.expected(left_orthogonal, case[3])
    return memo[k]


# ------------------------------------------------------------------------------------------------- the same matrices through TensorCI2
# (m, n, block ranks) per form: "MN" is local dims [M, N] with f(i) = A[i0, i1]; "MN1" and "1MN" add a trivial site behind / in front
TCI_CASES = [("MN", (8, 6, [4])), ("MN", (40, 50, [16])), ("MN", (64, 64, [17])), ("MN", (100, 90, [8] * 8)),
             ("MN1", (30, 28, [8, 8, 3])), ("1MN", (30, 28, [8, 8, 3]))]


def tci_case_id(tc):
    form, (m, n, ranks) = tc
    return "%s-%dx%d-r%d" % (form, m, n, sum(ranks))


def tci_fixture(tc):
    m, n, ranks = tc[1]
    return fixture((m, n, ranks, None))


def tci_check(tci, opts, fx, form):
    """Drive `tci` (a TensorCI2 of the product or of the oracle, already constructed on tci_dims(fx, form)) through the 2-site sweeps,
    fill_site_tensors, both 1-site sweeps and make_canonical; `opts` are its TCI2Options (tolerance 1e-15, no global search).  The bond
    sets must be the constructed pivot lists in order and the two non-trivial cores the exact factors; the trivial core is 1."""
    a = fx.a
    m, n = a.shape
    nsites = len(form)
    s = form.index("M")
    rank, rows, cols, left_fwd, right_fwd = fx.expected(True)
    _, _, _, left_bwd, right_bwd = fx.expected(False)

    def f(idx):
        return float(a[idx[s], idx[s + 1]])

    f.batched = lambda idx: a[idx[:, s], idx[:, s + 1]]
    tci.set_function(f)
    pivot = [0] * nsites
    pivot[s], pivot[s + 1] = int(rows[0]), int(cols[0])
    tci.add_global_pivots([pivot])
    tci.sweep2site(True, opts)
    if nsites == 3:
        tci.sweep2site(False, opts)

    def check_sets():
        lead, trail = [0] * s, [0] * (nsites - 2 - s)
        assert np.array_equal(tci.i_set(s + 1), np.array([lead + [int(i)] for i in rows]).reshape(rank, s + 1)), "row pivots"
        assert np.array_equal(tci.j_set(s), np.array([[int(j)] + trail for j in cols]).reshape(rank, nsites - 1 - s)), "column pivots"
        if form == "MN1":
            assert np.array_equal(tci.i_set(2), [pivot[:2]]) and np.array_equal(tci.j_set(1), [[0]])
        if form == "1MN":
            assert np.array_equal(tci.i_set(1), [[0]]) and np.array_equal(tci.j_set(0), [pivot[1:]])

    def check_cores(left, right, what):
        t0, t1 = tci.site_tensor(s), tci.site_tensor(s + 1)
        assert t0.shape == (1, m, rank) and t1.shape == (rank, n, 1), (what, t0.shape, t1.shape)
        assert np.array_equal(t0[0], left), what + ": left core"
        assert np.array_equal(t1[:, :, 0], right), what + ": right core"
        if nsites == 3:
            assert np.array_equal(tci.site_tensor(2 if s == 0 else 0), np.ones((1, 1, 1))), what + ": trivial core"

    check_sets()
    tci.fill_site_tensors()
    check_cores(left_fwd, right_fwd, "fill_site_tensors")
    tci.sweep1site(True, 1e-15, 0.0, None, True)
    check_sets()
    check_cores(left_fwd, right_fwd, "sweep1site forward")
    tci.sweep1site(False, 1e-15, 0.0, None, True)
    check_sets()
    check_cores(left_bwd, right_bwd, "sweep1site backward")
    tci.make_canonical(1e-15, 0.0)
    check_sets()
    check_cores(left_fwd, right_fwd, "make_canonical")


def tci_dims(fx, form):
    m, n = fx.a.shape
    return {"MN": [m, n], "MN1": [m, n, 1], "1MN": [1, m, n]}[form]


# ------------------------------------------------------------------------------------------- componentwise bounds on random matrices
U_ROUND = 2.0 ** -53  # unit roundoff of binary64 (Higham's u)


def gamma(n):
    return n * U_ROUND / (1.0 - n * U_ROUND)


def _exact_ints(a, p=None):
    """Python integers a * 2^p (object array) and p, exactly; p is the smallest that makes every entry an integer unless given."""
    mant, ex = np.frexp(a)
    mi = np.ldexp(mant, 53).astype(np.int64)  # exact: |mant| 2^53 is a 53-bit integer
    nz = mi != 0
    need = int((53 - ex[nz]).max()) if nz.any() else 0
    p = max(need, 0) if p is None else p
    assert p >= need
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(*a.shape):
        out[idx] = (int(mi[idx]) << (int(ex[idx]) - 53 + p)) if mi[idx] else 0
    return out, p


def _unit_lower_solve_rows(b, l11):
    """X with X L11 = B for the unit lower triangle of l11 (its diagonal and upper part are not read), in integers: returns the object
    array of numerators and the list of scales s_j, X[:, j] = numerators[:, j] / 2^s_j.  No division occurs: X is a dyadic rational."""
    r = l11.shape[0]
    p = max(_exact_ints(b)[1], _exact_ints(l11)[1])
    bi, li = _exact_ints(b, p)[0], _exact_ints(l11, p)[0]
    x = np.empty(b.shape, dtype=object)
    scales = [p * (r - j) for j in range(r)]
    for j in range(r - 1, -1, -1):  # x_j = b_j - sum_{k > j} x_k l_kj, every term brought to the scale p (r - j)
        col = bi[:, j] * (1 << (p * (r - j - 1)))
        for k in range(j + 1, r):
            if li[k, j]:
                col = col - x[:, k] * (li[k, j] << (p * (k - j - 1)))
        x[:, j] = col
    return x, scales


def _abs_diff(dev, num, scale):
    """|dev - num / 2^scale| for a double and an exact dyadic rational: formed exactly, rounded once."""
    mant, ex = np.frexp(dev)
    mi, ex = int(np.ldexp(mant, 53)), int(ex)
    q = max(0, 53 - ex)
    d = (mi << (scale + ex - 53 + q)) - (num << q)
    return abs(d) / (1 << (scale + q))  # (int / int is correctly rounded)


def _ratio_to_solve_bound(dev, tri, rhs):
    """max over entries of |dev - X| / (2 gamma_{r+2} (|dev| |T| |T^-1|)) for X T = rhs, T the unit lower triangle of `tri`
    (Higham, Accuracy and Stability of Numerical Algorithms, Thm 8.5: (T + dT) x^ = b with |dT| <= gamma_r |T|, hence
    |x^ - x| <= gamma_r |x^| |T| |T^-1|; the factor 2 and the r + 2 leave room for blocked accumulation)."""
    r = tri.shape[0]
    num, scales = _unit_lower_solve_rows(rhs, tri)
    inum, iscales = _unit_lower_solve_rows(np.eye(r), tri)
    tinv = np.array([[abs(inum[i, j]) / (1 << iscales[j]) for j in range(r)] for i in range(r)])
    bound = 2 * gamma(r + 2) * (np.abs(dev) @ (np.abs(np.tril(tri, -1)) + np.eye(r)) @ tinv)
    worst = 0.0
    for i in range(dev.shape[0]):
        for j in range(r):
            e = _abs_diff(dev[i, j], num[i, j], scales[j])
            if e > 0.0:
                worst = max(worst, e / bound[i, j] if bound[i, j] > 0 else np.inf)
    return worst


def _ratio_to_product_bound(dev, a, b):
    """max over entries of |dev - a b| / (2 gamma_{k+2} |a| |b|), the product a b formed in integers."""
    k = a.shape[1]
    ai, pa = _exact_ints(a)
    bi, pb = _exact_ints(b)
    prod = ai.dot(bi)
    bound = 2 * gamma(k + 2) * (np.abs(a) @ np.abs(b))
    worst = 0.0
    for i in range(dev.shape[0]):
        for j in range(dev.shape[1]):
            e = _abs_diff(dev[i, j], prod[i, j], pa + pb)
            if e > 0.0:
                worst = max(worst, e / bound[i, j] if bound[i, j] > 0 else np.inf)
    return worst


def componentwise_ratios(factored, row_perm, col_perm, rank, left_orthogonal, left, right):
    """(solve half, product half): the largest error of the factors `left`, `right` (original coordinates) relative to their
    componentwise bounds, from the factored buffer of rrlu (permuted coordinates).  At most 1 for a correct kernel.
    left-orthogonal:   |left - L21 L11^-1| <= 2 gamma_{rk+2} |left| |L11| |L11^-1|,   |right - L11 U| <= 2 gamma_{rk+2} |L11| |U|
    right-orthogonal:  |right - U11^-1 U12| <= 2 gamma_{rk+2} |U11^-1| |U11| |right|,  |left - L U11| <= 2 gamma_{rk+2} |L| |U11|."""
    r = rank
    lp, rq = left[row_perm, :], right[:, col_perm]  # permuted coordinates
    if left_orthogonal:
        assert np.array_equal(lp[:r], np.eye(r))
        solve = _ratio_to_solve_bound(lp[r:], factored[:r, :r], factored[r:, :r]) if lp.shape[0] > r else 0.0
        prod = _ratio_to_product_bound(rq, np.tril(factored[:r, :r], -1) + np.eye(r), np.triu(factored[:r, :]))
    else:
        assert np.array_equal(rq[:, :r], np.eye(r))
        # U11 y = U12(:, j)  <=>  y^T U11^T = U12(:, j)^T
        solve = _ratio_to_solve_bound(rq[:, r:].T, factored[:r, :r].T, factored[:r, r:].T) if rq.shape[1] > r else 0.0
        prod = _ratio_to_product_bound(lp, np.tril(factored[:, :r]), np.triu(factored[:r, :r], 1) + np.eye(r))
    return solve, prod
