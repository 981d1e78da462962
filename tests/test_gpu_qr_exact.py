"""The blocked Householder QR (Engine::qr, entry t4a_amd.qr_backend) on every panel route, with a known answer.

Exact family (tests/qr_np.py exact_case): A = P U with one non-zero at or below the head of every reflector.  Nothing rounds in any
order of summation, fused or not (tests/test_cpu_qr_exact.py proves it for every input used here), so the device must return the
doubles of the restatement, and no tolerance appears.  An off-diagonal pivot has x0 == 0 exactly, which is the only input that tells
`x0 >= 0.0` from `x0 > 0.0`; the permutations put the pivot on row 0, 1, 2, 63, 64, 65 below the head and on the last row of the panel,
the rows the register code of qr_panel_lds2_kernel treats specially.

Dense family: Gaussian and column-graded matrices, held to C_QR = 8 times what the float64 restatement itself reaches (QR_RESTATEMENT_RES,
QR_RESTATEMENT_ORTH: measured on the CPU, asserted by the CPU test, never taken from the device), with an exactly zero strict lower
triangle of R and the signs of R's diagonal of the longdouble reference.  A's QR is unique once those signs are fixed, so residual,
orthogonality, triangularity and signs together pin the factors; the forward differences to the reference scale with the conditioning
of A and are printed, not asserted."""
import functools

import numpy as np
import pytest

import qr_np as qn
import t4a_amd

pytestmark = pytest.mark.gpu

WORST = {}  # route -> [res, orth] of the device, the largest over the dense cases whose shape has a panel on the route


def equal_values(a, b):  # equal doubles, the sign of a zero left open
    a, b = np.ascontiguousarray(np.asarray(a) + 0.0), np.ascontiguousarray(np.asarray(b) + 0.0)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def blame(m, n, dev, want):
    """the first differing column and the route of the panel that owns it"""
    cols = np.nonzero((np.asarray(dev) + 0.0 != np.asarray(want) + 0.0).any(axis=0))[0]
    if cols.size == 0:
        return "no differing column"
    j = int(cols[0])
    routes = qn.panel_routes(m, n)
    pi = min(j // qn.QR_NB, len(routes) - 1)
    kern, rpl, rows, w = routes[pi]
    own = "" if j < min(m, n) else " (a trailing column: last panel named)"
    i = int(np.nonzero(np.asarray(dev)[:, j] + 0.0 != np.asarray(want)[:, j] + 0.0)[0][0])
    return f"column {j} row {i}: {dev[i, j]!r} for {want[i, j]!r}; panel {pi} = {qn.route_name((kern, rpl))}, {rows} rows, w = {w}{own}; " \
           f"all routes {[(qn.route_name((p[0], p[1])), p[2], p[3]) for p in routes]}"


@functools.lru_cache(maxsize=None)
def reference(key):
    """(a, q, r, ratio) of a dense input, computed once"""
    kind = key[0]
    if kind == "dense":
        a = qn.dense_case(*key[1:])
    elif kind == "zero":
        a = qn.zero_dense_case(*key[1:])
    else:
        a = qn.repeated_dense_case()
    q, r, ratio = qn.reference(a)
    for x in (a, q, r, ratio):
        x.setflags(write=False)
    return a, q, r, ratio


def units(m, n, a, q, r, qref, rref, label):
    res, orth = qn.res_units(q, r, a), qn.orth_units(q)
    scale = np.maximum(np.abs(rref).max(axis=0), np.finfo(np.float64).tiny)  # per column: graded columns differ by 2^80
    dq = float(np.abs(q - qref).max() / qn.EPS)
    dr = float((np.abs(r - rref) / scale).max() / qn.EPS)
    print(f"{label}: res {res:.2f} orth {orth:.2f} (restatement {qn.QR_RESTATEMENT_RES}, {qn.QR_RESTATEMENT_ORTH}; bound x{qn.C_QR}) | "
          f"forward, not asserted: |Q - Qref| {dq:.1f} eps, |R - Rref| {dr:.1f} eps of the column")
    for (kern, rpl, _, _) in qn.panel_routes(m, n):
        w = WORST.setdefault((kern, rpl), [0.0, 0.0])
        w[0], w[1] = max(w[0], res), max(w[1], orth)
    return res, orth


@pytest.fixture(scope="module", autouse=True)
def worst_per_route():
    yield
    for route in qn.ROUTES:
        if route in WORST:
            print(f"\ndevice, worst over the dense cases with a panel on {qn.route_name(route)}: res {WORST[route][0]:.2f} orth {WORST[route][1]:.2f}", end="")
    print()


def _exact_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}-z{len(c[3])}"


@pytest.mark.parametrize("case", qn.exact_cases(), ids=_exact_id)
def test_exact_family_bit_for_bit(case):
    m, n, pname, zero_cols = case
    a = qn.exact_input(m, n, pname, zero_cols)
    want = qn.blocked(a)
    q, r = t4a_amd.qr_backend(a)
    assert equal_values(q, want.q), f"Q: {blame(m, n, q, want.q)}"
    assert equal_values(r, want.r), f"R: {blame(m, n, r, want.r)}"
    # the device-side rescaling around an exact factorisation: 2^e A has the same Q and 2^e R
    for e in (300, -300):
        qs, rs = t4a_amd.qr_backend(np.ldexp(a, e))
        assert equal_values(qs, want.q), f"Q of 2^{e} A: {blame(m, n, qs, want.q)}"
        assert equal_values(rs, np.ldexp(want.r, e)), f"R of 2^{e} A: {blame(m, n, rs, np.ldexp(want.r, e))}"


@pytest.mark.parametrize("case", qn.dense_cases(), ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-s{c[3]}")
def test_dense_within_the_margin_of_the_restatement(case):
    m, n, kind, seed = case
    a, qref, rref, ratio = reference(("dense",) + case)
    assert ratio.min() >= qn.MIN_HEAD_RATIO
    q, r = t4a_amd.qr_backend(a)
    res, orth = units(m, n, a, q, r, qref, rref, f"{m} x {n} {kind} seed {seed}")
    assert res <= qn.C_QR * qn.QR_RESTATEMENT_RES, f"res {res}: routes {qn.panel_routes(m, n)}"
    assert orth <= qn.C_QR * qn.QR_RESTATEMENT_ORTH, f"orth {orth}: routes {qn.panel_routes(m, n)}"
    assert not np.tril(r, -1).any(), "strict lower triangle of R"
    signs = np.sign(np.diag(r)) == np.sign(np.diag(rref))
    assert signs.all(), f"sign of R_jj in columns {np.nonzero(~signs)[0]}: routes {qn.panel_routes(m, n)}"


@pytest.mark.parametrize("case", qn.ZERO_DENSE, ids=lambda c: f"{c[0]}x{c[1]}")
def test_zero_and_dependent_columns(case):
    """Gaussian matrices with exactly zero columns: first, inner, after a zero column and last of a panel, first of the next panel, last
    of all.  A zero column stays exactly zero under every earlier reflector, so its column of R is exactly zero, diagonal included, and
    its reflector is the identity; the other columns keep the reference's signs."""
    m, n, seed, zero_cols = case
    a, qref, rref, ratio = reference(("zero",) + case)
    q, r = t4a_amd.qr_backend(a)
    res, orth = units(m, n, a, q, r, qref, rref, f"{m} x {n} zero columns {zero_cols}")
    assert not r[:, list(zero_cols)].any(), "R in the zero columns"
    assert res <= qn.C_QR * qn.QR_RESTATEMENT_RES and orth <= qn.C_QR * qn.QR_RESTATEMENT_ORTH, (res, orth)
    assert not np.tril(r, -1).any()
    live = np.array([j for j in range(min(m, n)) if j not in zero_cols])
    assert np.array_equal(np.sign(np.diag(r))[live], np.sign(np.diag(rref))[live]) and ratio[live].min() >= qn.MIN_HEAD_RATIO


def test_a_repeated_column():
    """Columns 20 and 40 repeat columns 3 and 31.  What is left of a dependent column below its head is rounding noise: its direction,
    hence the sign of R_jj and that column of Q, is arbitrary, so only residual, orthogonality and triangularity are asserted."""
    m, n = qn.REPEATED_DENSE[:2]
    a, qref, rref, _ = reference(("repeated",))
    q, r = t4a_amd.qr_backend(a)
    res, orth = qn.res_units(q, r, a), qn.orth_units(q)
    print(f"{m} x {n} repeated columns: res {res:.2f} orth {orth:.2f}")
    assert res <= qn.C_QR * qn.QR_RESTATEMENT_RES and orth <= qn.C_QR * qn.QR_RESTATEMENT_ORTH, (res, orth)
    assert not np.tril(r, -1).any()


@pytest.mark.parametrize("shape", qn.TWICE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_call_twice_gives_the_same_bits(shape):
    """the two-task schedule of the panel kernels is static: nothing depends on which wave arrives first"""
    m, n = shape
    a = qn.dense_case(m, n, "gauss", 5)
    q1, r1 = t4a_amd.qr_backend(a)
    q2, r2 = t4a_amd.qr_backend(a)
    assert np.array_equal(q1.view(np.uint64), q2.view(np.uint64)) and np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
    assert qn.res_units(q1, r1, a) <= qn.C_QR * qn.QR_RESTATEMENT_RES
