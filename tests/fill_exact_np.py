"""Index sets and functions whose fill_site_tensors cores are known by construction (numpy only).

fill_site_tensors solves, for every site b < n - 1, solve(P_b^T, Pi1_b^T) with P_b = f(I_{b+1} + J_b) and Pi1_b = f(kron(I_b, d_b) + J_b),
all sites as ONE batch of ragged problems.  Two constructions make the answer known without a reference implementation.

Callback chain, build(dims, bonds, seed, zero_site, small): bonds[b] = |J_b| = |I_{b+1}|.
  I sets   I_{b+1} is bonds[b] rows drawn from kron(I_b, d_b) (nested; I_0 is the empty prefix).
  J sets   J_b is bonds[b] distinct suffixes over the sites b+1 .. n-1 whose last coordinate is = b (mod n-1): the evaluation points of
           different bonds are disjoint, so one table serves the whole chain.
  A_b      P_b^T = _plu(rng, bonds[b], small), the matrix the device factors (all zeros at zero_site).
  X_b      bonds[b] x ni_b (ni_b = |I_b| d_b), integers in [-4, 4] (small: uniform(-1, 1)); column l d_b + s is the unit vector e_k
           wherever (I_b[l], s) = I_{b+1}[k]: a nested row of Pi1 is a row of P.
  B_b      A_b X_b.  At zero_site B_b is X_b with zeros in the nested columns instead: the reference returns a zero core for a pivot
           matrix of zeros whatever Pi1 holds (tensorci2.rs:1154-1157), and a right-hand side that is not zero shows a solve that did
           not skip the flagged problem or a packing that did not read the flag.
  f        f(I_{b+1}[k] + J_b[j]) = A_b[j, k], f(I_b[l] + s + J_b[j]) = B_b[j, l d_b + s], 0.0 everywhere else.
  cores    T_b[l, s, r] = X_b[r, l d_b + s] for b < n-1 (zeros at zero_site), and the last core is f on kron(I_{n-1}, d_{n-1}).
With small=False every entry of A, B and X and every partial sum of the elimination and of both substitutions is a multiple of 1/4
below 2^53 (assert_bit_budget): no summation order, scalar or on the matrix cores, can change a bit.  With small=True the multipliers
are about 1e-9, so that a pivot other than the column maximum inflates the error by about 1e9; X is then the answer within
4 n eps kappa_inf(A_b).

Built-in chain, linear_chain(dims, seed): f = sum_s w_s[i_s] (FN_LINEAR) with signed integer tables, w_s[0] = 0 on every site,
w_0[1] = -1, w_last[1] = +1, and I_b = {(0, .., 0), (1, 0, .., 0)}, J_b = {(0, .., 0, 1), (0, .., 0)}.  Every pivot matrix is
[[1, 0], [0, -1]] and the cores are small integers: T_b[l, s, :] = [a_l + w_b[s] + 1, -(a_l + w_b[s])] with a = [0] at site 0 and
[0, -1] behind it, T_{n-1}[l, s, 0] = a_l + w_last[s].

fill_route() restates the launchers (tci2_fill.hip fill_issue; kernels_dense.hip lu_solve_blocked_launch, lu_forward_blocked_launch,
lu_batched_launch, trsm_left_batched_launch), which choose ONE route for the whole batch from the largest site; PROFILES names the route
each profile is there for, and test_cpu_fill_exact.py holds the two together.
"""
import numpy as np

EPS = np.finfo(np.float64).eps


# --------------------------------------------------------------------------------------------- matrices with known row swaps
def _pivot_rows(rng, n):
    """ipiv[k] >= k, the row the partial pivoting must swap with k at step k: no swap, the edges of the panel around k for every panel
    width (kb + nb - 1, kb + nb), the last row, or anywhere beyond."""
    ipiv = np.empty(n, dtype=np.int64)
    for k in range(n):
        cand = [k, n - 1, int(rng.integers(k, n))]
        for nb in (8, 16, 32):
            kb = k - k % nb
            cand += [kb + nb - 1, kb + nb, kb + 2 * nb]
        cand = [c for c in cand if k <= c < n]
        ipiv[k] = cand[int(rng.integers(0, len(cand)))]
    return ipiv


def _plu_parts(rng, n, small):
    """(A, ipiv) of _plu."""
    if small:
        l = np.tril(rng.uniform(0.5, 1.0, size=(n, n)) * rng.choice([-1.0, 1.0], size=(n, n)) * 1e-9, -1) + np.eye(n)
        u = np.triu(rng.uniform(-1, 1, size=(n, n)) / n, 1) + np.diag(rng.choice([1.0, -1.0, 2.0, -2.0], size=n))
    else:
        l = np.tril(rng.choice([0.0, 0.25, -0.25, 0.5, -0.5], size=(n, n)), -1) + np.eye(n)
        u = np.triu(rng.integers(-3, 4, size=(n, n)).astype(np.float64), 1) + np.diag(
            rng.choice([1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 8.0], size=n))
    a = l @ u  # exact for the integer construction: multiples of 1/4 below 2^16
    ipiv = _pivot_rows(rng, n)
    for k in range(n - 1, -1, -1):  # A = P_0 P_1 ... P_{n-1} L U: partial pivoting swaps k and ipiv[k] at step k
        p = ipiv[k]
        if p != k:
            a[[k, p], :] = a[[p, k], :]
    return a, ipiv


def _plu(rng, n, small):
    """A = P L U (P from _pivot_rows).  small=False: |l| in {0, 1/4, 1/2}, U small integers with a power-of-two diagonal, every step of
    the elimination exact.  small=True: l ~ 1e-9 and a diagonally dominant U (kappa of a few)."""
    return _plu_parts(rng, n, small)[0]


def partial_pivot_lu(a):
    """(L, U, ipiv) of the partial-pivoting elimination of `a` in binary64, row by row as lu_kernel does it: the first largest entry of
    the column, separately rounded multiply and subtract."""
    a = a.copy()
    n = a.shape[0]
    ipiv = np.empty(n, dtype=np.int64)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        ipiv[k] = p
        if p != k:
            a[[k, p], :] = a[[p, k], :]
        a[k + 1:, k] /= a[k, k]
        a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k, k + 1:])
    return np.tril(a, -1) + np.eye(n), np.triu(a), ipiv


# ------------------------------------------------------------------------------------------------------------- callback chain
class Chain:
    """dims, bonds; i_sets[b] (|I_b| x b), j_sets[b] (|J_b| x n-1-b); A[b], X[b], B[b], ipiv[b] for b < n-1; f; cores[b]."""

    def n_points(self):
        return sum(self.B[b].size + self.A[b].size for b in range(len(self.dims) - 1)) + self.cores[-1].size

    def max_n(self):
        return max(self.bonds)

    def max_nrhs(self):
        return max(x.shape[1] for x in self.X)


class TableFunction:
    """f as a sorted table of (mixed-radix key of the full index, value); 0.0 off the table.  Callable on one index; `batched` on an
    (n_pts, n_sites) array."""

    def __init__(self, dims, keys, vals):
        self.strides = np.array([int(np.prod(dims[s + 1:], dtype=np.int64)) for s in range(len(dims))], dtype=np.int64)
        order = np.argsort(keys, kind="stable")
        keys, vals = keys[order], vals[order]
        same = keys[1:] == keys[:-1]
        # a point reached twice (a nested row of Pi1 is a row of P) carries one value
        assert np.array_equal(vals[1:][same], vals[:-1][same]), "two values for one evaluation point"
        first = np.concatenate([[True], ~same])
        self.keys, self.vals = keys[first], vals[first]
        self.n_duplicates = int(same.sum())
        self._dict = None
        self.batched = self._batched

    def key(self, idx):
        return np.asarray(idx).astype(np.int64) @ self.strides

    def _batched(self, idx):
        k = self.key(idx)
        pos = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
        return np.where(self.keys[pos] == k, self.vals[pos], 0.0)

    def __call__(self, idx):
        if self._dict is None:
            self._dict = dict(zip(self.keys.tolist(), self.vals.tolist()))
        k = 0
        for v, s in zip(idx, self.strides.tolist()):
            k += int(v) * s
        return self._dict.get(k, 0.0)


def _cross(rows, cols):
    """Every row followed by every column, column index fastest: (len(rows) * len(cols), width)."""
    r = np.repeat(rows, len(cols), axis=0)
    c = np.tile(cols, (len(rows), 1))
    return np.concatenate([r, c], axis=1)


def kron_i(i_set, d):
    """kron(I_b, d_b): row l d + s is I_b[l] followed by s."""
    return _cross(i_set, np.arange(d, dtype=np.int64).reshape(d, 1))


def build(dims, bonds, seed, zero_site=None, small=False):
    dims = [int(d) for d in dims]
    bonds = [int(b) for b in bonds]
    n = len(dims)
    assert n >= 2 and len(bonds) == n - 1 and (zero_site is None or 0 <= zero_site < n - 1)
    rng = np.random.default_rng(seed)
    c = Chain()
    c.dims, c.bonds, c.zero_site, c.small = dims, bonds, zero_site, small
    c.i_sets = [np.zeros((1, 0), dtype=np.int64)]
    c.j_sets, c.A, c.X, c.B, c.ipiv, c.nested_cols = [], [], [], [], [], []
    keys, vals = [], []
    strides = np.array([int(np.prod(dims[s + 1:], dtype=np.int64)) for s in range(n)], dtype=np.int64)
    for b in range(n - 1):
        r = bonds[b]
        kron = kron_i(c.i_sets[b], dims[b])
        ni = len(kron)
        assert 1 <= r <= ni, (b, r, ni)
        rows = rng.choice(ni, size=r, replace=False)  # unsorted: I_{b+1}[k] = kron[rows[k]]
        c.i_sets.append(kron[rows])
        # suffixes over b+1 .. n-1, the last coordinate = b (mod n-1)
        last = np.arange(b % (n - 1), dims[-1], n - 1, dtype=np.int64)
        mid = dims[b + 1:n - 1]
        space = int(np.prod(mid, dtype=np.int64)) * len(last)
        assert r <= space, "the last local dimension is too small for bond %d" % b
        pick = rng.choice(space, size=r, replace=False)
        js = np.empty((r, n - 1 - b), dtype=np.int64)
        js[:, -1] = last[pick % len(last)]
        pick = pick // len(last)
        for q in range(len(mid) - 1, -1, -1):
            js[:, q] = pick % mid[q]
            pick = pick // mid[q]
        c.j_sets.append(js)
        a, ipiv = _plu_parts(rng, r, small)
        if zero_site == b:
            a = np.zeros((r, r))
        x = rng.uniform(-1, 1, size=(r, ni)) if small else rng.integers(-4, 5, size=(r, ni)).astype(np.float64)
        x[:, rows] = np.eye(r)
        bm = a @ x
        if zero_site == b:
            bm = x.copy()  # (nothing may be solved here: a right-hand side that is not zero shows a solve or a packing that went on)
        bm[:, rows] = a  # (bit for bit what the product gives: one term per entry)
        c.A.append(a)
        c.ipiv.append(ipiv)
        c.X.append(x)
        c.B.append(bm)
        c.nested_cols.append(rows)
        # f(I_{b+1}[k] + J_b[j]) = A[j, k];  f(kron[q] + J_b[j]) = B[j, q]
        keys.append(_cross(c.i_sets[b + 1], js) @ strides)
        vals.append(a.T.ravel())
        keys.append(_cross(kron, js) @ strides)
        vals.append(bm.T.ravel())
    c.j_sets.append(np.zeros((1, 0), dtype=np.int64))
    c.f = TableFunction(dims, np.concatenate(keys), np.concatenate(vals))
    c.cores = []
    for b in range(n - 1):
        l = len(c.i_sets[b])
        t = np.zeros((l, dims[b], bonds[b])) if zero_site == b else c.X[b].T.reshape(l, dims[b], bonds[b]).copy()
        c.cores.append(t)
    lastk = kron_i(c.i_sets[n - 1], dims[n - 1])
    c.cores.append(c.f.batched(lastk).reshape(len(c.i_sets[n - 1]), dims[n - 1], 1))
    return c


def assert_bit_budget(c):
    """small=False only.  Every entry of A, B, X, L and U is a multiple of 1/4 (U and X are integers), the multipliers are the
    constructed {0, +-1/4, +-1/2}, and for every sum the kernels form — the Schur updates a_ij - sum_k l_ik u_kj, the forward
    substitution b_i - sum_k l_ik y_k with Y = U X and the backward substitution y_i - sum_k u_ik x_k — the sum of the absolute terms,
    counted in quarters, stays below 2^53: every partial sum in any order is then a representable multiple of 1/4.  Returns the
    largest bit count."""
    assert not c.small
    worst = 0.0
    for b, a in enumerate(c.A):
        if c.zero_site == b:
            assert not a.any() and not c.B[b][:, c.nested_cols[b]].any()
            assert c.B[b].any() or c.B[b].shape[1] == len(a)  # (every column nested: nothing else to put there)
            continue
        l, u, ipiv = partial_pivot_lu(a)
        x, bm = c.X[b], c.B[b]
        for m in (4 * a, 4 * bm, 4 * l, u, x):
            assert np.array_equal(m, np.rint(m))
        ls = np.abs(np.tril(l, -1))
        assert set(np.unique(ls)) <= {0.0, 0.25, 0.5}
        d = np.abs(np.diag(u))
        assert np.array_equal(np.exp2(np.round(np.log2(d))), d), "the diagonal of U is not a power of two"
        y = np.abs(u) @ np.abs(x)  # >= |U X| and >= every backward sum
        sums = [(ls + np.eye(len(a))) @ np.abs(u), (ls + np.eye(len(a))) @ y, y]
        top = 4.0 * max(float(s.max()) for s in sums)
        assert top < 2.0 ** 53
        worst = max(worst, float(np.log2(top)))
    return worst


def chain_sets(c):
    """[(which, site, entries)] for set_index_set."""
    out = []
    for s in range(len(c.dims)):
        out.append((0, s, c.i_sets[s]))
        out.append((1, s, c.j_sets[s]))
    return out


def apply_sets(tci, c):
    for which, s, e in chain_sets(c):
        tci.set_index_set(which, s, np.ascontiguousarray(e))


# --------------------------------------------------------------------------------------------------- the pivot-sensitive bounds
def _slices(m, axis, q=20, count=3):
    """m = s_0 + .. + s_{count-1} + rest, slice t a multiple of 2^(-q (t + 1)) of the power of two above the largest entry along
    `axis`, with at most q + 1 bits: products of two slices summed over fewer than 2^(52 - 2 q) terms are exact in binary64."""
    mu = np.abs(m).max(axis=axis, keepdims=True)
    tau = np.exp2(np.ceil(np.log2(np.where(mu > 0, mu, 1.0))))
    out = []
    rest = m.copy()
    for t in range(count):
        unit = tau * 2.0 ** (-q * (t + 1))
        s = np.rint(rest / unit) * unit
        out.append(s)
        rest = rest - s  # exact
    return out, rest


def residual_longdouble(a, g, bm):
    """B - A G as longdouble.  Small products are formed in longdouble directly; large ones (numpy's longdouble product of the 1030-site
    takes 13 s) from slices of A's rows and G's columns whose binary64 products are exact (test_cpu_fill_exact.py holds the two
    together): what is left out is below 2^-60 of (row maximum of A) x (column maximum of G) per term."""
    n = a.shape[0]
    if n * n * g.shape[1] <= 2e7:
        return bm.astype(np.longdouble) - a.astype(np.longdouble) @ g.astype(np.longdouble)
    assert n < 4096
    sa, ra = _slices(a, 1)
    sg, rg = _slices(g, 0)
    r = bm.astype(np.longdouble)
    for p in sa:
        for q in sg:
            r = r - (p @ q).astype(np.longdouble)
    return r - (ra @ g).astype(np.longdouble) - ((a - ra) @ rg).astype(np.longdouble)


def pivot_sensitive_ratios(c, cores, sites=None):
    """small=True.  Per solved site (forward error / (4 n eps kappa_inf(A_b)), backward error / (2 n eps)), n = bonds[b], both at most 1
    for a correct solve; kappa_inf(A_b) < 1e3 is asserted.  The bounds of test_gpu_dense_exact.py
    test_solve_pivot_sensitive_on_every_route."""
    assert c.small
    out = {}
    for b in (range(len(c.dims) - 1) if sites is None else sites):
        if b == len(c.dims) - 1 or c.zero_site == b:
            continue
        a, x, bm, n = c.A[b], c.X[b], c.B[b], c.bonds[b]
        got = cores[b].reshape(-1, n).T  # X^T[r, l d + s] = T[l, s, r]
        assert got.shape == x.shape
        kappa = np.linalg.cond(a, np.inf)
        assert kappa < 1e3, (b, kappa)
        fwd = np.abs(got - x).max() / np.abs(x).max()
        res = np.abs(residual_longdouble(a, got, bm)).max()
        back = float(res / (np.abs(a).sum(axis=1).max() * np.abs(got).max() + np.abs(bm).max()))
        out[b] = (float(fwd / (4 * n * EPS * kappa)), back / (2 * n * EPS))
    return out


# -------------------------------------------------------------------------------------------------------------------- routes
def fill_route(max_n, max_nrhs):
    """The route family fill_issue takes for a batch whose largest problem has max_n rows and whose widest has max_nrhs right-hand
    sides (general route: host callback, or a built-in functor with a site beyond FILL_SMALL_MAX_N / FILL_SMALL_MAX_RHS)."""
    mc = max_n >= 64 and max_nrhs >= 16 and max_n <= 1263  # trsm_left_batched_launch: matrix cores inside their LDS limit
    trsm = "matrix-core trsm" if mc else "scalar trsm"
    if 32 <= max_n <= 512 and max_nrhs >= 16:  # lu_solve_blocked_launch (16 * 4 * SV_MAXS = 512)
        return "fused lu_solve_kernel, nb %d" % (32 if max_n <= 256 else 16)
    if max_n <= 1024:  # lu_forward_blocked_launch
        return "blocked LU nb %d, upper %s" % (32 if max_n <= 256 else 16 if max_n <= 512 else 8, trsm)
    return "lu_kernel, two %s" % trsm


FILL_SMALL_MAX_N, FILL_SMALL_MAX_RHS = 32, 64  # kernels.hpp


def linear_route(dims):
    """The route of a linear_chain fill: every site has 2 rows and at most 2 d_b right-hand sides."""
    if 2 * max(dims[:-1]) <= FILL_SMALL_MAX_RHS:
        return "fill_small_kernel"
    return "pi_eval_batched_kernel, " + fill_route(2, 2 * max(dims[:-1]))


# (dims, bonds, route family of the whole batch, checked against the oracle on the CPU)
PROFILES = [
    ([3, 2, 2, 12], [3, 5, 2], "blocked LU nb 32, upper scalar trsm", True),  # max_nrhs 10 < 16
    ([8, 6, 4, 3, 80], [3, 17, 9, 5], "blocked LU nb 32, upper scalar trsm", True),  # max_n 17 < 32 with 68 right-hand sides
    ([8, 6, 4, 3, 80], [3, 17, 40, 5], "fused lu_solve_kernel, nb 32", True),  # 40: one full and one partial panel beside 3, 5, 17
    ([40, 12, 4, 4, 160], [33, 300, 64, 7], "fused lu_solve_kernel, nb 16", True),
    ([64, 64, 8, 6, 64], [9, 530, 40, 2], "blocked LU nb 8, upper matrix-core trsm", False),
    ([64, 20, 40, 120], [60, 1030, 20], "lu_kernel, two matrix-core trsm", False),
]
P40 = PROFILES[2]
P5 = PROFILES[0]
LINEAR_DIMS = [[3, 5, 7, 4, 2, 6], [3, 5, 300, 4, 2, 6]]


def profile_id(p):
    return "n" + "-".join(str(b) for b in p[1])


def profile_seed(p):
    return 1009 * sum(p[0]) + 7 * sum(p[1]) + len(p[0])


_cache = {}


def chain(p, zero_site=None, small=False):
    """The chain of a profile (built once per process)."""
    key = (tuple(p[0]), tuple(p[1]), zero_site, small)
    if key not in _cache:
        _cache[key] = build(p[0], p[1], profile_seed(p), zero_site, small)
    return _cache[key]


def assert_cores_exact(tci, c, sites=None):
    for s in (range(len(c.dims)) if sites is None else sites):
        got = tci.site_tensor(s)
        assert got.shape == c.cores[s].shape, (s, got.shape, c.cores[s].shape)
        assert np.array_equal(got, c.cores[s]), "site %d: %d entries differ, largest by %.3g" % (
            s, int((got != c.cores[s]).sum()), np.abs(got - c.cores[s]).max())


# ----------------------------------------------------------------------------------------------------------- built-in chain
class LinearChain:
    """spec (FnSpec), dims, i_sets, j_sets, cores."""


def linear_chain(dims, seed):
    from t4a_amd.functions import FN_LINEAR, FnSpec
    dims = [int(d) for d in dims]
    n = len(dims)
    assert n >= 3 and min(dims) >= 2
    rng = np.random.default_rng(seed)
    w = [rng.integers(-40, 41, size=d) for d in dims]
    for t in w:
        t[0] = 0
    w[0][1] = -1
    w[-1][1] = 1
    c = LinearChain()
    c.dims = dims
    c.spec = FnSpec(FN_LINEAR, [1.0, 0.0], np.concatenate(w).astype(np.int64).astype(np.uint64).reshape(1, -1), dims)
    c.weights = w
    c.i_sets, c.j_sets, c.cores = [np.zeros((1, 0), dtype=np.int64)], [], []
    for b in range(1, n):
        i = np.zeros((2, b), dtype=np.int64)
        i[1, 0] = 1
        c.i_sets.append(i)
    for b in range(n - 1):
        j = np.zeros((2, n - 1 - b), dtype=np.int64)
        j[0, -1] = 1
        c.j_sets.append(j)
    c.j_sets.append(np.zeros((1, 0), dtype=np.int64))
    for b in range(n):
        a = np.array([0.0]) if b == 0 else np.array([0.0, -1.0])
        v = a[:, None] + w[b][None, :].astype(np.float64)  # a_l + w_b[s]
        c.cores.append(v[:, :, None] if b == n - 1 else np.stack([v + 1.0, -v], axis=2))
    return c
