"""numpy restatement of tensor4all-simplett's Contraction (src/mpo/contraction.rs:60-383) — the checker of tests/test_cpu_contraction.py and
tests/test_gpu_contraction.py, and with integer-valued operands on int64 the exact reference of tests/test_gpu_mpo_exact.py and
tests/soak/soak_mpo.py.  Site tensors are numpy arrays [left, s1, s2, right]; an index tuple is [(i_1, j_1), ...] with i_k indexing s1
of A and j_k indexing s2 of B."""
import numpy as np

SEED = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def random_tensors(bonds, s1, s2, seed):
    """random_mpo (test_support.rs:8-44): an LCG fills every site tensor column-major (as in tests/test_gpu_mpo.py)."""
    state = seed
    out = []
    for left, right in zip(bonds[:-1], bonds[1:]):
        vals = []
        for _ in range(left * s1 * s2 * right):
            state = (state * 6364136223846793005 + 1442695040888963407) & MASK
            vals.append((state >> 33) / float(1 << 31) - 0.5)
        out.append(np.array(vals).reshape((left, s1, s2, right), order="F"))
    return out


def integer_tensors(bonds, s1, s2, seed):
    """random_tensors with every entry drawn from {-1, 0, 1} by the same LCG, column-major: float64 arrays that hold integers, so
    that every product and every partial sum of a contraction is exact in f64 while it stays below 2^53 (exact_bound)."""
    state = seed
    out = []
    for left, right in zip(bonds[:-1], bonds[1:]):
        vals = []
        for _ in range(left * s1 * s2 * right):
            state = (state * 6364136223846793005 + 1442695040888963407) & MASK
            vals.append(float((state >> 33) % 3) - 1.0)
        out.append(np.array(vals).reshape((left, s1, s2, right), order="F"))
    return out


def exact_bound(a, b):
    """The element of A·B with every entry of both operands replaced by 1: prod_s K_s * prod_{inner bonds} (ra_s * rb_s), a Python
    int.  For entries of absolute value <= 1 every partial sum of an environment, a pairing or a site product, in any order, is a
    subset sum of that total of absolute values: below 2^53 all of them are exact in f64."""
    total = 1
    for x in a:
        total *= int(x.shape[2])
    for x, y in zip(a[:-1], b[:-1]):
        total *= int(x.shape[3]) * int(y.shape[3])
    return total


# Operands of the exact tests (tests/test_cpu_contraction.py, tests/test_gpu_mpo_exact.py): name -> (bonds of A, bonds of B, (s1, k, s2)).
# The mixed profiles put a bond below 16 beside one of 16 or more, and summed dimensions 3, 5, 17, 18, 31, 33, on both walks.
MIXED_1 = [1, 17, 33, 16, 5, 20, 1]
MIXED_2 = [1, 3, 16, 31, 18, 2, 1]
EXACT_PROFILES = {
    "P1": (MIXED_1, MIXED_2, (2, 2, 2)),
    "P2": (MIXED_2, MIXED_1, (2, 2, 2)),
    "P1_k3": (MIXED_1, MIXED_2, (2, 3, 2)),
    "P1_k1": (MIXED_1, MIXED_2, (3, 1, 2)),
    "scratch": ([1, 64, 64, 1], [1, 33, 33, 1], (2, 2, 2)),          # working set 4 * 64 * 33 = 8448 doubles: beyond the LDS
    "stride": ([1] + [2] * 6 + [1], [1] + [3] * 6 + [1], (2, 2, 2)),  # 4^7 = 16384 index tuples
    "naive27": ([1, 27, 27, 1], [1, 27, 27, 1], (2, 2, 2)),           # a middle site of 729 * 4 * 729 output elements
}
# bond pairs (A, B) at the cut of a two-site product: K = 31, 32, 33, 37, 64, 65 around the 32-wide panels of the pairing kernel
PAIR_SEAMS = [(31, 1), (4, 8), (3, 11), (37, 1), (8, 8), (5, 13)]
for _ba, _bb in PAIR_SEAMS:
    EXACT_PROFILES[f"seam{_ba * _bb}"] = ([1, _ba, 1], [1, _bb, 1], (3, 2, 3))


def exact_operands(name, seed=SEED):
    """the integer-valued operands of a profile"""
    bonds_a, bonds_b, (s1, k, s2) = EXACT_PROFILES[name]
    return integer_tensors(bonds_a, s1, k, seed), integer_tensors(bonds_b, k, s2, seed ^ 0x5555)


def lcg_points(n_pts, dims, seed):
    """n_pts multi-indices below `dims` (any shape prefix: the result is (n_pts,) + dims.shape), drawn from the same LCG."""
    dims = np.asarray(dims, dtype=np.int64)
    flat = dims.reshape(-1)
    state = seed
    out = np.zeros((n_pts, flat.size), dtype=np.int64)
    for p in range(n_pts):
        for k, d in enumerate(flat):
            state = (state * 6364136223846793005 + 1442695040888963407) & MASK
            out[p, k] = (state >> 33) % int(d)
    return out.reshape((n_pts,) + dims.shape)


def np_site(a, b):
    """contract_site_tensors (environment.rs:37-80): C[(la*Lb+lb), s1, t, (ra*Rb+rb)] = sum_k A[la,s1,k,ra] B[lb,k,t,rb]"""
    la, s1, _, ra = a.shape
    lb, _, t, rb = b.shape
    return np.einsum("askr,bktq->bastqr", a, b).reshape((lb * la, s1, t, rb * ra), order="F")


def np_full(ts):
    """dense operator indexed [i1, j1, i2, j2, ...]"""
    acc = ts[0][0]
    for t in ts[1:]:
        acc = np.tensordot(acc, t, axes=([-1], [0]))
    return acc[..., 0]


def dense_product(a, b):
    """every element of A·B, indexed [i1, j1, i2, j2, ...]: the product of the site-wise contractions"""
    return np_full([np_site(x, y) for x, y in zip(a, b)])


class ContractionNP:
    """Contraction<f64> for batches of index tuples: `pairs` is (n_pts, >= needed, 2).  With exact=True the same steps run on
    astype(np.int64) site tensors (which must hold integers) and every result is int64: the reference of the exact device tests."""

    def __init__(self, a, b, exact=False):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.shape[2] == y.shape[1]
        self.a, self.b = list(a), list(b)
        self.dtype = np.float64
        if exact:
            assert all(np.array_equal(t, np.rint(t)) for t in self.a + self.b), "exact=True needs integer-valued site tensors"
            self.a, self.b = [t.astype(np.int64) for t in self.a], [t.astype(np.int64) for t in self.b]
            self.dtype = np.int64
        self.n = len(a)
        self.site_dims = [(x.shape[1], y.shape[2]) for x, y in zip(a, b)]

    # A site step as two batched matrix products (the five-deep loop of contraction.rs:288-308 / :357-377 regrouped: the sum over the
    # shared index k is taken last), so that a few thousand points at bonds of a few dozen stay a matter of seconds
    def _step_left(self, env, s, pairs):
        ai = self.a[s].transpose(1, 0, 2, 3)[pairs[:, s, 0]]          # [p, la, k, ra]
        bj = self.b[s].transpose(2, 0, 1, 3)[pairs[:, s, 1]]          # [p, lb, k, rb]
        t = np.matmul(ai.transpose(0, 2, 3, 1), env[:, None])          # [p, k, ra, lb] = sum_la A[la, i, k, ra] L[la, lb]
        return np.matmul(t, bj.transpose(0, 2, 1, 3)).sum(axis=1)      # [p, ra, rb]

    def _step_right(self, env, s, pairs):
        ai = self.a[s].transpose(1, 0, 2, 3)[pairs[:, s, 0]]
        bj = self.b[s].transpose(2, 0, 1, 3)[pairs[:, s, 1]]
        t = np.matmul(ai.transpose(0, 2, 1, 3), env[:, None])          # [p, k, la, rb] = sum_ra A[la, i, k, ra] R[ra, rb]
        return np.matmul(t, bj.transpose(0, 2, 3, 1)).sum(axis=1)      # [p, la, lb]

    def evaluate_left(self, n, pairs):
        pairs = np.asarray(pairs, dtype=np.int64)
        env = np.ones((pairs.shape[0], 1, 1), dtype=self.dtype)
        for s in range(n):
            env = self._step_left(env, s, pairs)
        return env

    def evaluate_right(self, n, pairs):
        pairs = np.asarray(pairs, dtype=np.int64)
        env = np.ones((pairs.shape[0], 1, 1), dtype=self.dtype)
        for s in range(self.n - 1, n - 1, -1):
            env = self._step_right(env, s, pairs)
        return env

    def evaluate(self, pairs):
        return self.evaluate_left(self.n, pairs)[:, 0, 0]

    def evaluate_many(self, pairs, split):
        """TTCache::evaluate_many (cache.rs:558-685) restated for the contraction: every unique left half of `split` sites and every unique
        right half once, then value[p] = sum_{a, b} L[il[p]][a, b] R[ir[p]][a, b]"""
        pairs = np.asarray(pairs, dtype=np.int64)
        p = len(pairs)
        ul, il = np.unique(pairs[:, :split].reshape(p, -1), axis=0, return_inverse=True)
        ur, ir = np.unique(pairs[:, split:].reshape(p, -1), axis=0, return_inverse=True)
        full_l = np.zeros((len(ul), self.n, 2), dtype=np.int64)
        full_l[:, :split] = ul.reshape(len(ul), split, 2)
        full_r = np.zeros((len(ur), self.n, 2), dtype=np.int64)
        full_r[:, split:] = ur.reshape(len(ur), self.n - split, 2)
        left = self.evaluate_left(split, full_l).reshape(len(ul), -1)
        right = self.evaluate_right(split, full_r).reshape(len(ur), -1)
        il, ir = il.reshape(-1), ir.reshape(-1)
        if len(ul) * len(ur) == p:  # a full outer product: one matrix product
            return (left @ right.T)[il, ir]
        return np.einsum("pe,pe->p", left[il], right[ir])

    def evaluate_matrix(self, cut, rows, cols):
        """the candidate matrix of `rows` (n_rows, cut, 2) and `cols` (n_cols, n - cut, 2): left environments times right environments"""
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        full_l = np.zeros((len(rows), self.n, 2), dtype=np.int64)
        full_l[:, :cut] = rows
        full_r = np.zeros((len(cols), self.n, 2), dtype=np.int64)
        full_r[:, cut:] = cols
        left = self.evaluate_left(cut, full_l).reshape(len(rows), -1)
        right = self.evaluate_right(cut, full_r).reshape(len(cols), -1)
        return left @ right.T

    def fused_dims(self):
        return [s1 * s2 for s1, s2 in self.site_dims]

    def decode(self, fused):
        """fused site index f = i + s1_a * j -> (n_pts, n, 2)"""
        fused = np.asarray(fused, dtype=np.int64).reshape(-1, self.n)
        s1 = np.array([d[0] for d in self.site_dims], dtype=np.int64)
        return np.stack([fused % s1, fused // s1], axis=2)

    def fused_function(self):
        """f(list of fused indices) -> float, with a `batched` twin over an (n_pts, n) array: the function a TensorCI2 interpolates"""
        def f(idx):
            return float(self.evaluate(self.decode([idx]))[0])
        f.batched = lambda arr: self.evaluate(self.decode(arr))
        return f


def find_split(pairs):
    """find_split_heuristic (cache.rs:690-744): of n/4, n/2, 3n/4 inside [1, n) the first with the fewest unique left + right halves"""
    pairs = np.asarray(pairs, dtype=np.int64)
    n = pairs.shape[1]
    if n <= 1:
        return max(n, 1)
    best = None
    for p in (n // 4, n // 2, n * 3 // 4):
        if p < 1 or p >= n:
            continue
        cost = len({tuple(r) for r in pairs[:, :p].reshape(len(pairs), -1)}) + len({tuple(r) for r in pairs[:, p:].reshape(len(pairs), -1)})
        if best is None or cost < best[1]:
            best = (p, cost)
    return best[0]


def fused_dense(dense, site_dims):
    """the dense product over the fused site index i + s1 * j: shape (s1*s2, ...) per site"""
    return dense.reshape([s1 * s2 for s1, s2 in site_dims], order="F")
