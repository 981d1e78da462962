"""The GEMM descriptor (csrc/kernels.hpp GemmDesc, include/t4a_gpu.h t4a_gpu_gemm_desc) restated on flat numpy buffers, and the
cases the tests and the soak draw from its option space.

A descriptor is a dict with the fields of t4a_gpu_gemm_desc.  Product j < batch is
    C_j = alpha op(A_j) op(B_j) + beta C_j
with A_j stored column-major at a[off_a + j stride_a + row + lda col] as m x k (k x m when trans_a), B_j likewise, C_j at
c[off_c + j stride_c + row + ldc col].  gemm_desc_ref returns the WHOLE c buffer: what the product must not touch comes back as it went in.

Two modes:
  exact: operands that are small integers, int64 arithmetic scaled by the common power of two of alpha and beta -- the one right
         answer of every summation order, slice split and MFMA association as long as every partial sum stays below 2^53;
  tight: real operands.  Every product a b is formed in np.longdouble (64-bit significand) and split into two doubles, all 2k parts
         are summed by math.fsum (correctly rounded), the rounding error of that sum is recovered by a second fsum, and alpha, beta
         are applied in longdouble: the value is good to about k 2^-64 of the magnitude, a thousandth of one double rounding.  Returned
         with the componentwise magnitude |alpha| (|op A| |op B|) + |beta| |C| that error bounds are stated in.
(test infrastructure: numpy is the checker)"""
import math

import numpy as np

# a quiet NaN with a payload no arithmetic produces: padding, gaps and (for beta == 0) the result region itself are preset to it
SENTINEL_BITS = np.uint64(0x7FF8DEADBEEF1234)
ALPHAS = (1.0, -1.0, 2.0, 0.5)
BETAS = (0.0, 1.0, -1.0, 0.25)
ALPHA_BETA = ((1.0, 0.0), (-1.0, 1.0), (2.0, -1.0), (0.5, 0.25))  # every alpha and every beta once
TRANS = ((0, 0), (1, 0), (0, 1), (1, 1))
PADS = (False, True)
STRIDE_MODES = ("dense", "a0", "b0", "ab0", "cpad")  # zero stride_a, zero stride_b, both, padded strides (batched cases)


def sentinel(count):
    return np.full(count, SENTINEL_BITS, dtype=np.uint64).view(np.float64)


def _index(off, stride, j, rows, cols, ld):
    """flat indices of the stored rows x cols matrix of problem j"""
    return off + j * stride + np.arange(rows, dtype=np.int64)[:, None] + ld * np.arange(cols, dtype=np.int64)[None, :]


def a_index(d, j):
    return _index(d["off_a"], d["stride_a"], j, d["k"] if d["trans_a"] else d["m"], d["m"] if d["trans_a"] else d["k"], d["lda"])


def b_index(d, j):
    return _index(d["off_b"], d["stride_b"], j, d["n"] if d["trans_b"] else d["k"], d["k"] if d["trans_b"] else d["n"], d["ldb"])


def c_index(d, j):
    return _index(d["off_c"], d["stride_c"], j, d["m"], d["n"], d["ldc"])


def c_mask(d, nc):
    """True where the product writes"""
    mask = np.zeros(nc, dtype=bool)
    for j in range(d["batch"]):
        mask[c_index(d, j).ravel()] = True
    return mask


def _ops(d, a, b, j):
    A = a[a_index(d, j)]
    B = b[b_index(d, j)]
    return (A.T if d["trans_a"] else A), (B.T if d["trans_b"] else B)


def _pow2_scale(alpha, beta):
    for e in range(0, 11):  # (a float that needs more is no multiple of a small power of two: 1 / 3 is an integer times 2^-54)
        s = float(2 ** e)
        if alpha * s == math.floor(alpha * s) and beta * s == math.floor(beta * s):
            return 2 ** e, int(alpha * s), int(beta * s)
    raise ValueError("alpha and beta have no common power-of-two scale up to 2^10")


def _as_int(x, what):
    xi = np.rint(x).astype(np.int64)
    if not np.array_equal(xi.astype(np.float64), x):
        raise ValueError(f"exact mode: {what} is not integer-valued")
    return xi


def _tight_product(A, B):
    """sum_p A[i, p] B[p, j] as longdouble, good to ~k 2^-64 of sum |A| |B|"""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("tight mode needs a long double with a 64-bit significand")
    m, k = A.shape
    n = B.shape[1]
    out = np.zeros((m, n), dtype=np.longdouble)
    if k == 0:
        return out
    P = A.astype(np.longdouble)[:, None, :] * B.T.astype(np.longdouble)[None, :, :]  # (m, n, k)
    hi = P.astype(np.float64)
    lo = (P - hi).astype(np.float64)
    parts = np.concatenate([hi, lo], axis=2).reshape(m * n, 2 * k).tolist()
    flat = out.reshape(-1)
    for e, p in enumerate(parts):
        s = math.fsum(p)
        p.append(-s)
        flat[e] = np.longdouble(s) + np.longdouble(math.fsum(p))
    return out


def gemm_desc_ref(d, a, b, c, mode="exact"):
    """exact: the c buffer after the product.  tight: (the c buffer as longdouble, the magnitude buffer as longdouble, zero where the
    product does not write)."""
    alpha, beta = float(d["alpha"]), float(d["beta"])
    if mode == "exact":
        out = np.array(c, dtype=np.float64, copy=True)
        scale, ai, bi = _pow2_scale(alpha, beta)
        for j in range(d["batch"]):
            A, B = _ops(d, a, b, j)
            r = ai * (_as_int(A, "A") @ _as_int(B, "B"))
            ci = c_index(d, j)
            if bi != 0:  # beta == 0: C is not read (it may hold the sentinel)
                r = r + bi * _as_int(c[ci], "C")
            if r.size and np.abs(r).max() >= 2 ** 52:
                raise ValueError("exact mode: the result leaves the integer range of a double")
            out[ci] = r.astype(np.float64) / float(scale)
        return out
    if mode != "tight":
        raise ValueError(mode)
    out = np.array(c, dtype=np.longdouble)
    mag = np.zeros(c.size, dtype=np.longdouble)
    for j in range(d["batch"]):
        A, B = _ops(d, a, b, j)
        ci = c_index(d, j)
        v = np.longdouble(alpha) * _tight_product(A, B)
        g = abs(np.longdouble(alpha)) * (np.abs(A).astype(np.longdouble) @ np.abs(B).astype(np.longdouble))
        if beta != 0.0:
            v = v + np.longdouble(beta) * c[ci].astype(np.longdouble)
            g = g + abs(np.longdouble(beta)) * np.abs(c[ci]).astype(np.longdouble)
        out[ci] = v
        mag[ci] = g
    return out, mag


def make_desc(m, n, k, batch, trans_a, trans_b, alpha, beta, pad, stride_mode):
    """The descriptor of one case and the sizes (na, nb, nc) of its buffers.  pad: leading dimensions padded by the odd amounts 3, 5, 7
    (rows are no 16-byte multiples), offsets 3, 5, 7 into the buffers and 9 elements behind the last result.  stride_mode (batch > 1):
    dense strides, stride_a = 0, stride_b = 0, both, or every stride padded by an odd gap."""
    a_rows, a_cols = (k, m) if trans_a else (m, k)
    b_rows, b_cols = (n, k) if trans_b else (k, n)
    lda, ldb, ldc = max(a_rows, 1) + (3 if pad else 0), max(b_rows, 1) + (5 if pad else 0), max(m, 1) + (7 if pad else 0)
    gap = (5, 3, 11) if stride_mode == "cpad" else (0, 0, 0)
    stride_a = 0 if stride_mode in ("a0", "ab0") else lda * a_cols + gap[0]
    stride_b = 0 if stride_mode in ("b0", "ab0") else ldb * b_cols + gap[1]
    stride_c = ldc * n + gap[2]
    off = (3, 5, 7) if pad else (0, 0, 0)
    d = dict(m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=ldc, trans_a=trans_a, trans_b=trans_b, alpha=alpha, beta=beta, batch=batch,
             stride_a=stride_a, stride_b=stride_b, stride_c=stride_c, off_a=off[0], off_b=off[1], off_c=off[2])
    na = off[0] + (batch - 1) * stride_a + lda * a_cols
    nb = off[1] + (batch - 1) * stride_b + ldb * b_cols
    nc = off[2] + (batch - 1) * stride_c + ldc * n + (9 if pad else 0)
    return d, (na, nb, nc)


def fill_case(rng, d, sizes, real=False):
    """Buffers of a case: operands are integers in [-3, 3] and C integers in [-8, 8] (real: all uniform in [-1, 1]); everything outside
    the stored matrices is the sentinel, and with beta == 0 so is the result region: the product must not read C then."""
    na, nb, nc = sizes
    a, b, c = sentinel(na), sentinel(nb), sentinel(nc)

    def draw(shape, bound):
        return rng.uniform(-1.0, 1.0, size=shape) if real else rng.integers(-bound, bound + 1, size=shape).astype(np.float64)

    for j in range(d["batch"] if d["stride_a"] else 1):
        ia = a_index(d, j)
        a[ia] = draw(ia.shape, 3)
    for j in range(d["batch"] if d["stride_b"] else 1):
        ib = b_index(d, j)
        b[ib] = draw(ib.shape, 3)
    if d["beta"] != 0.0:
        for j in range(d["batch"]):
            ic = c_index(d, j)
            c[ic] = draw(ic.shape, 8)
    return a, b, c


def check_exact(d, c_before, got, want):
    """What the exact tests assert of a result buffer: the written region finite and equal to the restatement, everything else bit for bit
    what went in.  Returns None or a description of the first difference."""
    mask = c_mask(d, c_before.size)
    if not np.array_equal(got.view(np.uint64)[~mask], c_before.view(np.uint64)[~mask]):
        bad = np.flatnonzero(~mask & (got.view(np.uint64) != c_before.view(np.uint64)))
        return f"{bad.size} elements outside the result changed, first at flat index {bad[0]}"
    if not np.all(np.isfinite(got[mask])):
        bad = np.flatnonzero(mask & ~np.isfinite(got))
        return f"{bad.size} non-finite results, first at flat index {bad[0]} (C read with beta == 0, or padding of A / B read)"
    if not np.array_equal(got[mask], want[mask]):  # (by value: a sum of zero may come back as -0.0)
        bad = np.flatnonzero(mask & (got != want))
        e = int(bad[0])
        rel = e - d["off_c"]
        j = rel // d["stride_c"] if d["batch"] > 1 else 0
        rel -= j * d["stride_c"]
        return f"{bad.size} wrong results, first at problem {j} row {rel % d['ldc']} column {rel // d['ldc']}: {got[e]} against {want[e]}"
    return None


# ------------------------------------------------------------------------------------------------ the rows of the exact tests
# The smallest shapes that reach each route of gemm_launch: (m, n, k, batch) -> (bn, ksplit, grid_m, grid_n, remapped), worked out by
# hand from the rule (64 x 64 tiles unless fewer than 512 of them and n > 32; split-K below 256 tiles from 8 k-tiles of 32 on:
# min(16, ktiles / 2, ceil(512 / tiles)) slices of ceil(ktiles / ksplit) k-tiles).  Every test asserts its row against gemm_route, so a
# change of the rule fails loudly instead of silently dropping a route from the coverage.
GPU_ROWS = [
    ((5, 3, 7, 1), (64, 1, 1, 1, False), "wide, one tile, checked path: the half of the tile past n"),
    ((70, 40, 33, 1), (32, 1, 2, 2, False), "narrow 2 x 2, ragged m and n, partial second k-tile, no interior tile"),
    ((70, 40, 33, 3), (32, 1, 2, 2, False), "the same, three problems"),
    ((128, 64, 40, 1), (32, 1, 2, 2, False), "narrow, every tile interior: pointer-stepped, then the checked last k-tile"),
    ((256, 128, 70, 1), (32, 1, 4, 4, True), "narrow, 16 tiles in the remapped order, interior"),
    ((128, 128, 40, 128), (64, 1, 2, 2, False), "wide interior tiles: 512 tiles of 64 x 64, reachable only batched"),
    ((256, 128, 40, 64), (64, 1, 4, 2, True), "wide, remapped, batched"),
    # n <= 32 is the only way wide tiles meet split-K (n > 32 below 256 tiles is always narrow), and such a tile is never interior:
    # split-K never meets a wide interior tile
    ((64, 32, 256, 1), (64, 4, 1, 1, False), "wide, 4 even slices of 2 k-tiles on the checked path"),
    ((64, 32, 257, 1), (64, 4, 1, 1, False), "wide, 9 k-tiles in slices of 3: the last slice is empty"),
    ((64, 64, 512, 1), (32, 8, 1, 2, False), "narrow interior, 8 slices: kt0 > 0 on the pointer-stepped path"),
    ((70, 70, 321, 5), (32, 5, 2, 3, False), "narrow, 11 k-tiles in slices of 3 (the fifth empty), five problems"),
    ((100, 100, 289, 1), (32, 5, 2, 4, True), "narrow, split and remapped"),
    ((30, 20, 1000, 1), (64, 16, 1, 1, False), "the cap of 16 slices"),
]
ROUTE_KEYS = ("bn", "ksplit", "grid_m", "grid_n", "remapped")
# rows whose buffers are megabytes: twenty cases each; the other batched rows forty; an unbatched row runs its full cube
BIG_ROWS = {(128, 128, 40, 128): 20, (256, 128, 40, 64): 20}
N_BATCHED = 40


def row_cases(shape):
    """The (trans, (alpha, beta), pad, stride_mode) cases of a row.  Unbatched: the full cube (stride_mode dense).  Batched: a fixed
    selection -- each option is a column that cycles through its values (so each occurs as evenly as the count allows), and the four
    columns are shuffled independently by a generator seeded with the shape.  That guarantees every value of every option on every
    row (asserted below) and nothing about pairings: it is no Latin square, and a given pair, say stride_a = 0 with trans_a = 1, may be
    missing from a row."""
    if shape[3] == 1:
        return [(t, ab, p, "dense") for t in TRANS for ab in ALPHA_BETA for p in PADS]
    count = BIG_ROWS.get(shape, N_BATCHED)
    rng = np.random.default_rng(list(shape))

    def column(values):
        seq = [values[i % len(values)] for i in range(count)]
        return [seq[i] for i in rng.permutation(count)]

    cols = [column(TRANS), column(ALPHA_BETA), column(PADS), column(STRIDE_MODES)]
    return list(zip(*cols))


# thinning must not drop a value: every value of every option on every row (and a beta != 0 beside beta == 0)
for _shape, _, _ in GPU_ROWS:
    _cases = row_cases(_shape)
    assert {c[0] for c in _cases} == set(TRANS), _shape
    assert {c[1] for c in _cases} == set(ALPHA_BETA), _shape
    assert {c[2] for c in _cases} == set(PADS), _shape
    assert {c[3] for c in _cases} == (set(STRIDE_MODES) if _shape[3] > 1 else {"dense"}), _shape
