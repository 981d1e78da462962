"""The blocked Householder QR of csrc/kernels_linalg.hip (Engine::qr, entry t4a_amd.qr_backend) restated in numpy, the inputs
its exact and eps-tight tests run on, and the constants the device is held to.

  reference(a)        unblocked Householder in np.longdouble with the device's sign convention: the answer a dense case is compared to;
  blocked(a, dtype)   what the device does, step by step: panels of QR_NB columns, the explicit reflector matrix V, the compact-WY factor T
                      column by column, three products per panel for the trailing matrix, Q from the identity with the panels in reverse;
  panel_routes(m, n)  which panel kernel (and which of its instantiations) factors each panel: a function of the shape alone;
  exact_case(...)     A = P U with U upper trapezoidal and dyadic: every reflector has ONE non-zero at or below its head, so every norm,
                      tau, T entry and GEMM operand is a small dyadic rational, no operation rounds in any summation order, with or without
                      FMA, and the device must return the restatement's doubles;
  dense_case(...)     Gaussian and column-graded matrices, measured in the units res and orth below.

Units (eps = 2^-52, products formed in longdouble):
    res  = |Q R - A|_F / (eps |A|_F)            orth = |Q^T Q - I|_F / (eps sqrt(k))
QR_RESTATEMENT_RES / QR_RESTATEMENT_ORTH are the largest values blocked(., float64) itself reaches over every dense case of SHAPES with
seeds 0..19 (tests/test_cpu_qr_exact.py recomputes and asserts them); the device gets C_QR = 8 times that, the margin restructure_np.py
(C_SPLIT) and swap_np.py (C_DENSE) give a second Householder implementation that rounds differently.  Nothing here comes from the
device's output.
(test infrastructure: numpy is the checker)"""
import os

import numpy as np

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble has to carry a 64-bit significand (x87 extended or wider)"

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tensor4all-rs_amd", "csrc")

# ------------------------------------------------------------------------------------------------ what the sources fix
QR_NB = 32               # columns per panel
QR_LDS_MAX_ROWS = 560    # a panel of at most this many rows is factored in the LDS, a taller one in global memory
QR_RPL_LADDER = (1, 2, 3, 4, 6, 9)  # rows per lane the LDS kernel is instantiated for
LDS_KERNEL = "qr_panel_lds2_kernel"
GLOBAL_KERNEL = "qr_panel_kernel"
ROUTES = tuple((LDS_KERNEL, r) for r in QR_RPL_LADDER) + ((GLOBAL_KERNEL, None),)  # the seven kernels


def panel_routes(m, n):
    """(kernel, RPL or None, rows, w) per panel, as qr_factor_launch chooses"""
    k = min(m, n)
    out = []
    for j0 in range(0, k, QR_NB):
        w = min(QR_NB, k - j0)
        rows = m - j0
        if rows <= QR_LDS_MAX_ROWS:
            need = (rows + 63) // 64
            out.append((LDS_KERNEL, next(r for r in QR_RPL_LADDER if need <= r), rows, w))
        else:
            out.append((GLOBAL_KERNEL, None, rows, w))
    return out


def route_rows(route):
    """(smallest, largest) number of panel rows that take the route"""
    kernel, rpl = route
    if kernel == GLOBAL_KERNEL:
        return QR_LDS_MAX_ROWS + 1, None
    i = QR_RPL_LADDER.index(rpl)
    return (64 * QR_RPL_LADDER[i - 1] + 1 if i else 1), min(64 * rpl, QR_LDS_MAX_ROWS)


def route_name(route):
    return f"{route[0]}<{route[1]}>" if route[1] else route[0]


# ------------------------------------------------------------------------------------------------ units and constants
EPS = 2.0 ** -52
C_QR = 8
QR_RESTATEMENT_RES = 5.46    # measured: tests/test_cpu_qr_exact.py::test_the_restatement_constants_are_the_measured_ones (257 x 257 graded, seed 8)
QR_RESTATEMENT_ORTH = 5.08   # (257 x 257 graded, seed 5)
MIN_HEAD_RATIO = 1e-6        # |x0| / |x| of every column of a dense case: a sign of R_jj that 1e9 roundings cannot turn
CONSTANT_SEEDS = range(20)


def _norm_f(x):
    return np.sqrt((np.asarray(x, dtype=np.longdouble) ** 2).sum())


def res_units(q, r, a):
    q, r, a = (np.asarray(x, dtype=np.longdouble) for x in (q, r, a))
    na = _norm_f(a)
    return float(_norm_f(q @ r - a) / (EPS * na)) if na != 0 else float(_norm_f(q @ r))


def orth_units(q):
    q = np.asarray(q, dtype=np.longdouble)
    k = q.shape[1]
    return float(_norm_f(q.T @ q - np.eye(k, dtype=np.longdouble)) / (EPS * np.sqrt(np.longdouble(k))))


# ------------------------------------------------------------------------------------------------ reference
def reference(a):
    """Unblocked Householder QR in longdouble, the device's convention: alpha = -|x| for x0 >= 0, else +|x|; v = x - alpha e1;
    tau = 2 / v.v; a column whose norm is 0 gets R_jj = 0 and H = I.  Returns thin Q, R and per column |x0| / |x| (inf for a zero column)."""
    ld = np.longdouble
    w = np.array(a, dtype=ld)
    m, n = w.shape
    k = min(m, n)
    vs, taus = [], []
    ratio = np.full(k, np.inf)
    r = np.zeros((k, n), dtype=ld)
    for j in range(k):
        x = w[j:, j]
        nrm = np.sqrt((x * x).sum())
        if nrm == 0:
            vs.append(None)
            taus.append(ld(0))
        else:
            ratio[j] = float(abs(x[0]) / nrm)
            alpha = -nrm if x[0] >= 0 else nrm
            v = x.copy()
            v[0] = x[0] - alpha
            tau = ld(2) / (v * v).sum()
            w[j:, j + 1:] -= np.outer(v, tau * (v @ w[j:, j + 1:]))
            r[j, j] = alpha
            vs.append(v)
            taus.append(tau)
        r[:j, j] = w[:j, j]
    r[:, k:] = w[:k, k:]
    q = np.eye(m, k, dtype=ld)
    for j in range(k - 1, -1, -1):
        if vs[j] is not None:
            q[j:, j:] -= np.outer(vs[j], taus[j] * (vs[j] @ q[j:, j:]))
    return q, r, ratio


# ------------------------------------------------------------------------------------------------ the device, restated
def grain_exponent(x):
    """the largest e with every entry of x an integer multiple of 2^e (None for an all-zero x)"""
    x = np.asarray(x, dtype=np.float64).ravel()
    x = x[x != 0]
    if x.size == 0:
        return None
    mant, exp = np.frexp(x)
    bits = np.abs(mant * 2.0 ** 53).astype(np.int64)
    low = (bits & -bits).astype(np.float64)  # the lowest set bit, a power of two
    return int((exp.astype(np.int64) - 53 + (np.frexp(low)[1] - 1)).min())


class Record:
    """Per dot product and GEMM of one blocked() run: the largest entry of |X| |Y| (+ |C| where the product is added to C) — no partial
    sum of any order exceeds it — and the grain of the operands (see grain_exponent)."""

    def __init__(self):
        self.rows = []  # (what, panel, bound, operand grain exponent or None)

    def note(self, what, panel, x, y, c=None):
        x, y = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(y, dtype=np.float64))
        x = x.reshape(1, -1) if x.ndim < 2 else x  # a vector on the left is a row, on the right a column
        y = y.reshape(-1, 1) if y.ndim < 2 else y
        if x.size == 0 or y.size == 0:
            return
        bound = x @ y
        grains = [grain_exponent(x), grain_exponent(y)]
        if c is not None:
            bound = bound + np.abs(np.asarray(c, dtype=np.float64))
            grains.append(grain_exponent(c))
        grains = [g for g in grains if g is not None]
        self.rows.append((what, panel, float(bound.max()), min(grains) if grains else None))

    def largest_bound(self):
        return max((r[2] for r in self.rows), default=0.0)

    def finest_grain(self):
        return min((r[3] for r in self.rows if r[3] is not None), default=0)


def _mm(x, y):
    """x y without a BLAS: the products formed elementwise, every sum taken by numpy's own reduction.  A BLAS picks its order of summation
    by CPU model and thread count, which moved QR_RESTATEMENT_RES between 4.9 and 5.3; this gives the same doubles everywhere."""
    return (x[:, :, None] * y[None, :, :]).sum(axis=1)


class Blocked:
    """q, r and what the panels did: pivot[j] = row of the largest |entry| at or below the head of column j when its reflector is built
    (-1 for a zero column), below[j] = how many non-zeros it had there, t = the compact-WY factors"""


def blocked(a, dtype=np.float64, record=None):
    dt = np.dtype(dtype).type
    w = np.array(a, dtype=dt, order="F")
    m, n = w.shape
    k = min(m, n)
    vall = np.zeros((m, k), dtype=dt)
    diag = np.zeros(k, dtype=dt)
    ts = []
    out = Blocked()
    out.pivot = np.full(k, -1)
    out.below = np.zeros(k, dtype=int)
    zero, two = dt(0), dt(2)
    for pi, j0 in enumerate(range(0, k, QR_NB)):
        wd = min(QR_NB, k - j0)
        t = np.zeros((QR_NB, QR_NB), dtype=dt)
        for jj in range(wd):
            j = j0 + jj
            x = w[j:, j]
            out.below[j] = np.count_nonzero(x)
            if out.below[j]:
                out.pivot[j] = j + int(np.argmax(np.abs(x)))
            x0 = x[0]
            tail = (x[1:] * x[1:]).sum() if x.size > 1 else zero
            nrm = np.sqrt(x0 * x0 + tail)
            alpha = -nrm if x0 >= 0 else nrm
            v0 = x0 - alpha
            vv = v0 * v0 + tail
            tau = zero if nrm == 0 else two / vv
            diag[j] = zero if nrm == 0 else alpha
            v = vall[j:, j]
            v[:] = x
            v[0] = v0
            if record is not None:
                record.note("norm", pi, x, x)
                record.note("v.v", pi, v, v)
                record.note("tau v.v", pi, tau, vv)
            if tau != 0:
                if jj + 1 < wd:  # H_j on the remaining columns of the panel
                    y = w[j:, j + 1:j0 + wd]
                    dots = _mm(v[None, :], y)[0]
                    f = tau * dots
                    if record is not None:
                        record.note("panel v.y", pi, v, y)
                        record.note("panel tau dot", pi, tau, dots[None, :])
                        record.note("panel y -= f v", pi, v[:, None], f[None, :], y)
                    y -= np.outer(v, f)
                if jj:           # T(0:jj, jj) = -tau T(0:jj, 0:jj) (V^T v)
                    z = _mm(vall[j:, j0:j].T, v[:, None])[:, 0]
                    tz = _mm(t[:jj, :jj], z[:, None])[:, 0]
                    if record is not None:
                        record.note("T z = V^T v", pi, vall[j:, j0:j].T, v)
                        record.note("T column", pi, t[:jj, :jj], z)
                        record.note("T tau column", pi, tau, tz[None, :])
                    t[:jj, jj] = -tau * tz
            t[jj, jj] = tau
        ts.append(t)
        n2 = n - j0 - wd
        if n2 > 0:  # the trailing matrix: W = Vp^T A2, W2 = T^T W, A2 -= Vp W2
            vp = vall[j0:, j0:j0 + wd]
            a2 = w[j0:, j0 + wd:]
            w1 = _mm(vp.T, a2)
            w2 = _mm(t[:wd, :wd].T, w1)
            if record is not None:
                record.note("trailing Vp^T A2", pi, vp.T, a2)
                record.note("trailing T^T W", pi, t[:wd, :wd].T, w1)
                record.note("trailing A2 -= Vp W2", pi, vp, w2, a2)
            a2 -= _mm(vp, w2)
    r = np.zeros((k, n), dtype=dt)
    for j in range(n):
        r[:min(j, k), j] = w[:min(j, k), j]
    r[np.arange(k), np.arange(k)] = diag
    q = np.eye(m, k, dtype=dt)
    for pi in range(len(ts) - 1, -1, -1):  # Q <- (I - V T V^T) Q, panels in reverse: columns left of j0 are still unit vectors
        j0 = pi * QR_NB
        wd = min(QR_NB, k - j0)
        vp = vall[j0:, j0:j0 + wd]
        qs = q[j0:, j0:]
        w1 = _mm(vp.T, qs)
        w2 = _mm(ts[pi][:wd, :wd], w1)
        if record is not None:
            record.note("form Vp^T Q", pi, vp.T, qs)
            record.note("form T W", pi, ts[pi][:wd, :wd], w1)
            record.note("form Q -= Vp W2", pi, vp, w2, qs)
        qs -= _mm(vp, w2)
    out.q, out.r, out.t = q, r, ts
    return out


# ------------------------------------------------------------------------------------------------ shapes
TALL_M = (33, 63, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 560, 561, 593)  # both sides of every RPL rung and of LDS / global
TALL = tuple((m, 33) for m in TALL_M) + ((592, 65),)                              # a full panel and a one-column panel; 593: two global panels
WIDTHS = tuple((100, n) for n in (1, 2, 16, 17, 18, 31, 32, 34, 48, 49, 50, 63, 64))  # last panels of 1, 2, 16, 17, 18, 31, 32 columns, first and later
WIDE = ((1, 4), (2, 2), (33, 200), (40, 100), (64, 129), (96, 96), (257, 257))    # k = m: no tail under the last column, wide trailing updates
SHAPES = TALL + WIDTHS + WIDE
TWICE_SHAPES = ((592, 65), (593, 33), (600, 100))  # global panels followed by LDS panels, global panels alone, both with full panels


# ------------------------------------------------------------------------------------------------ the exact family
DIAGONAL = (0.5, 1.0, 2.0, 4.0)
SPECIAL_OFFSETS = (0, 1, 2, 63, 64, 65)  # rows (below the head) the register code of the LDS kernel treats specially


def perm_identity(m):
    return np.arange(m)


def perm_reversal(m):
    return np.arange(m)[::-1].copy()


def perm_rotation(m, s):
    return (np.arange(m) + s) % m


def perm_random(m, seed):
    return np.random.default_rng([seed, m, 7]).permutation(m)


def perm_from_offsets(m, offsets):
    """The permutation under which column j of an exact case (without zero columns) finds its single non-zero offsets[j] rows below its
    head: a reflector with a single non-zero off its head swaps the two rows (up to sign), so the arrangement that ends as the identity
    is the identity with those swaps undone, last first."""
    at = np.arange(m)  # at[position] = row of U
    for j in range(len(offsets) - 1, -1, -1):
        p = j + offsets[j]
        assert j <= p < m
        at[j], at[p] = at[p], at[j]
    perm = np.empty(m, dtype=int)
    perm[at] = np.arange(m)
    return perm


def special_offsets(m, n):
    """per column: the first column of every panel takes the panel's last row, the others walk through SPECIAL_OFFSETS and the last row"""
    out = []
    for j in range(min(m, n)):
        jj = j % QR_NB
        last = m - 1 - j
        out.append(last if jj == 0 else min((SPECIAL_OFFSETS + (last,))[(jj - 1) % (len(SPECIAL_OFFSETS) + 1)], last))
    return out


def perm_special(m, n):
    return perm_from_offsets(m, special_offsets(m, n))


def default_zero_cols(m, n):
    """first, inner, the one after a zero column and last of the first panel, first of the second, last of all"""
    k = min(m, n)
    return tuple(sorted({j for j in (0, 5, 6, QR_NB - 1, QR_NB, k - 1) if j < k})) if k > 2 else (k - 1,)


def exact_case(m, n, perm, zero_cols=(), seed=0):
    """A = P U: U (k x n, zero rows below) has integers of -3..3 above its diagonal and +-{1/2, 1, 2, 4} on it; row i of U becomes row
    perm[i] of A; for j in zero_cols column j AND row j of U are zero (a zero column alone would leave the next pivot two non-zeros)."""
    k = min(m, n)
    rng = np.random.default_rng([seed, m, n, 11])
    u = np.triu(rng.integers(-3, 4, size=(k, n)).astype(np.float64), 1)
    u[np.arange(k), np.arange(k)] = rng.choice(DIAGONAL, size=k) * rng.choice((-1.0, 1.0), size=k)
    for j in zero_cols:
        u[:, j] = 0.0
        u[j, :] = 0.0
    a = np.zeros((m, n), order="F")
    a[np.asarray(perm)[:k], :] = u
    return a


def exact_cases():
    """(m, n, permutation name, zero columns) of every exact input the GPU test runs"""
    out = []
    for (m, n) in SHAPES:
        for pname in ("identity", "reversal", "special", "random0"):
            out.append((m, n, pname, ()))
        out.append((m, n, "special", default_zero_cols(m, n)))
        out.append((m, n, "random1", default_zero_cols(m, n)))
        if m > 2:
            out.append((m, n, "rotation1", ()))
    return out


def named_perm(m, n, pname):
    if pname == "identity":
        return perm_identity(m)
    if pname == "reversal":
        return perm_reversal(m)
    if pname == "special":
        return perm_special(m, n)
    if pname.startswith("rotation"):
        return perm_rotation(m, int(pname[8:]))
    assert pname.startswith("random")
    return perm_random(m, int(pname[6:]))


def exact_input(m, n, pname, zero_cols):
    return exact_case(m, n, named_perm(m, n, pname), zero_cols)


# ------------------------------------------------------------------------------------------------ the dense family
KINDS = ("gauss", "graded")
SEED_OVERRIDES = {}  # (m, n, kind) -> two seeds, where seed 0 or 1 has a column with |x0| / |x| < MIN_HEAD_RATIO


def dense_case(m, n, kind, seed):
    rng = np.random.default_rng([seed, m, n, KINDS.index(kind)])
    a = rng.standard_normal((m, n))
    if kind == "graded":
        a = a * 2.0 ** rng.integers(-40, 41, size=n)[None, :]
    return np.asfortranarray(a)


def dense_seeds(m, n, kind):
    return SEED_OVERRIDES.get((m, n, kind), (0, 1))


def dense_cases():
    return [(m, n, kind, seed) for (m, n) in SHAPES for kind in KINDS for seed in dense_seeds(m, n, kind)]


# gauss matrices with columns set to zero: first, inner, the one after a zero column, last of a panel, first of the next, last of all
ZERO_DENSE = (
    (100, 50, 0, (0, 5, 6, 31, 32, 40, 41, 49)),   # two LDS panels
    (593, 40, 0, (0, 5, 6, 31, 32, 39)),           # two global panels
    (40, 100, 0, (0, 5, 6, 31, 32, 39)),           # wide: the trailing update carries the zero columns' rows of R
)
REPEATED_DENSE = (100, 50, 0, ((20, 3), (40, 31)))  # column 20 repeats column 3 (same panel), column 40 repeats column 31 (the panel before)


def zero_dense_case(m, n, seed, zero_cols):
    a = dense_case(m, n, "gauss", seed)
    a[:, list(zero_cols)] = 0.0
    return a


def repeated_dense_case():
    m, n, seed, pairs = REPEATED_DENSE
    a = dense_case(m, n, "gauss", seed)
    for dst, src in pairs:
        a[:, dst] = a[:, src]
    return a
