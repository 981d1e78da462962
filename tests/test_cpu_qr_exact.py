"""Holds tests/qr_np.py to the sources and to itself, without a device: the panel width, the LDS limit and the ladder of instantiations
stand in kernels_linalg.hip where panel_routes assumes them, the shape list reaches every panel kernel at both ends of its range, the
exact family is exact (float64 and longdouble runs of the restatement agree bit for bit, no sum can round), its permutations put the
pivot on every row the register code treats specially, the dense cases pin the signs of R's diagonal, and QR_RESTATEMENT_RES / _ORTH
are what the restatement measures.  tests/test_gpu_qr_exact.py relies on every one of these."""
import functools
import os
import re

import numpy as np
import pytest

import qr_np as qn

# Every operand of every product of an exact case is an integer multiple of 2^EXACT_GRAIN (entries of A: halves; v: halves; tau down to
# 1/32; f = tau (v.y), T: multiples of 1/32), so every product and every partial sum is an integer multiple of EXACT_STEP, and a sum
# whose absolute-sum bound stays below 2^50 steps is exact in any order, fused or not.
EXACT_GRAIN = -5
EXACT_STEP = 2.0 ** (2 * EXACT_GRAIN)


def _source():
    with open(os.path.join(qn.CSRC, "kernels_linalg.hip")) as f:
        return f.read()


def _shapes_on(route):
    return sorted({(m, n) for (m, n) in qn.SHAPES for (kern, rpl, _, _) in qn.panel_routes(m, n) if (kern, rpl) == route})


# ------------------------------------------------------------------------------------------------ constants and routes
def test_the_literals_of_panel_routes_stand_in_the_sources():
    src = _source()
    moved = "the shapes of tests/qr_np.py sized against it must move: "
    assert re.search(r"constexpr\s+int\s+QR_NB\s*=\s*%d\s*;" % qn.QR_NB, src), \
        moved + f"QR_NB is no longer {qn.QR_NB}: WIDTHS {qn.WIDTHS} and every n = 33 of TALL"
    assert re.search(r"constexpr\s+int\s+QR_LDS_MAX_ROWS\s*=\s*%d\s*;" % qn.QR_LDS_MAX_ROWS, src), \
        moved + f"QR_LDS_MAX_ROWS is no longer {qn.QR_LDS_MAX_ROWS}: {_shapes_on((qn.GLOBAL_KERNEL, None))} and (560, 33)"
    assert re.search(r"if\s*\(\s*m\s*-\s*j0\s*<=\s*QR_LDS_MAX_ROWS\s*\)", src), "qr_factor_launch no longer switches on m - j0 <= QR_LDS_MAX_ROWS"
    assert re.search(r"const\s+int\s+rpl\s*=\s*\(\s*m\s*-\s*j0\s*\+\s*63\s*\)\s*/\s*64\s*;", src), "rows per lane are no longer ceil((m - j0) / 64)"
    ladder = [(int(a), int(b)) for a, b in re.findall(r"if\s*\(\s*rpl\s*<=\s*(\d+)\s*\)\s*go\(&qr_panel_lds2_kernel<(\d+)>\)", src)]
    last = re.findall(r"else\s+go\(&qr_panel_lds2_kernel<(\d+)>\)", src)
    assert all(a == b for a, b in ladder) and len(last) == 1
    found = tuple(a for a, _ in ladder) + (int(last[0]),)
    assert found == qn.QR_RPL_LADDER, moved + f"the ladder is {found}, not {qn.QR_RPL_LADDER}: " \
        + "; ".join(f"{qn.route_name(r)}: {_shapes_on(r)}" for r in qn.ROUTES[:-1])
    assert 64 * qn.QR_RPL_LADDER[-1] >= qn.QR_LDS_MAX_ROWS
    assert re.search(r"__launch_bounds__\(QR_T\)\s+qr_panel_kernel\(", src) and re.search(r"__launch_bounds__\(QR_T\)\s+qr_panel_lds2_kernel\(", src)


def test_the_shape_list_reaches_every_kernel_at_both_ends():
    panels = [(kern, rpl, rows, w, first) for (m, n) in qn.SHAPES
              for first, (kern, rpl, rows, w) in ((i == 0, p) for i, p in enumerate(qn.panel_routes(m, n)))]
    assert {(p[0], p[1]) for p in panels} == set(qn.ROUTES) and len(qn.ROUTES) == 7
    for route in qn.ROUTES:
        mine = [p for p in panels if (p[0], p[1]) == route]
        lo, hi = qn.route_rows(route)
        assert any(p[2] == lo for p in mine), f"{qn.route_name(route)}: no panel of {lo} rows, its smallest"
        if route[0] == qn.LDS_KERNEL:
            assert any(p[2] == hi for p in mine), f"{qn.route_name(route)}: no panel of {hi} rows, its largest"
            assert any(p[4] for p in mine) and any(not p[4] for p in mine), f"{qn.route_name(route)}: first and later panel"
        else:
            assert {p[3] for p in mine} >= {1, qn.QR_NB}, "the global kernel with w = 32 and w = 1"
    # the last panel in every width at which the two-task schedule changes, as a first and as a later panel
    for first in (True, False):
        assert {p[3] for p in panels if p[4] == first and p[0] == qn.LDS_KERNEL} >= {1, 2, 16, 17, 18, 31, 32}
    assert qn.panel_routes(592, 65) == [(qn.GLOBAL_KERNEL, None, 592, 32), (qn.LDS_KERNEL, 9, 560, 32), (qn.LDS_KERNEL, 9, 528, 1)]
    for (m, n) in qn.TWICE_SHAPES:
        assert qn.panel_routes(m, n)[0][0] == qn.GLOBAL_KERNEL


# ------------------------------------------------------------------------------------------------ the exact family
@functools.lru_cache(maxsize=None)
def _exact_run(m, n, pname, zero_cols):
    a = qn.exact_input(m, n, pname, zero_cols)
    rec = qn.Record()
    return a, qn.blocked(a, np.float64, rec), rec


@pytest.mark.parametrize("shape", qn.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_family_is_exact(shape):
    cases = [c for c in qn.exact_cases() if (c[0], c[1]) == shape]
    assert len(cases) >= 6
    m, n = shape
    k = min(m, n)
    for (_, _, pname, zero_cols) in cases:
        what = f"{m} x {n} {pname} zero columns {zero_cols}"
        a, b, rec = _exact_run(m, n, pname, zero_cols)
        assert np.array_equal(np.sort(qn.named_perm(m, n, pname)), np.arange(m)), what
        wide = qn.blocked(a, np.longdouble)
        for name, x, y in [("Q", b.q, wide.q), ("R", b.r, wide.r)] + [(f"T{i}", s, t) for i, (s, t) in enumerate(zip(b.t, wide.t))]:
            assert np.array_equal(x.astype(np.longdouble), y), f"{what}: {name} differs between float64 and longdouble"
        assert b.below.max() <= 1, f"{what}: a reflector with more than one non-zero at or below its head"
        assert rec.finest_grain() >= EXACT_GRAIN, f"{what}: an operand finer than 2^{EXACT_GRAIN}"
        assert rec.largest_bound() < 2.0 ** 50 * EXACT_STEP, f"{what}: {rec.largest_bound()}"
        assert max(np.abs(t).max() for t in b.t) <= 4.0
        assert np.array_equal(b.q @ b.r, a) and np.array_equal(b.q.T @ b.q, np.eye(k)), what
        assert np.count_nonzero(np.abs(b.q) == 1.0) == k and np.count_nonzero(b.q) == k, what
        assert np.array_equal(np.tril(b.r, -1), np.zeros_like(b.r))
        for j in zero_cols:
            assert not b.r[:, j].any() and b.pivot[j] == -1, f"{what}: column {j} of R"
        # the reference, which shares no code with the restatement, finds the same factors: one convention in both
        qr, rr, _ = qn.reference(a)
        assert np.array_equal(qr, wide.q) and np.array_equal(rr, wide.r), what


def _offsets_by_route():
    seen = {r: set() for r in qn.ROUTES}
    last_row = {r: False for r in qn.ROUTES}
    for (m, n, pname, zero_cols) in qn.exact_cases():
        _, b, _ = _exact_run(m, n, pname, zero_cols)
        for pi, (kern, rpl, rows, w) in enumerate(qn.panel_routes(m, n)):
            for jj in range(w):
                j = pi * qn.QR_NB + jj
                if b.pivot[j] >= 0:
                    seen[(kern, rpl)].add(int(b.pivot[j]) - j)
                    last_row[(kern, rpl)] |= jj == 0 and b.pivot[j] == m - 1
    return seen, last_row


def test_the_pivot_meets_every_special_row_on_every_route():
    """offset = rows below the reflector's head = lane + 64 q of the LDS kernel: 0 is the substituted v0, 1 the shuffled head of the next
    column, 2 the first row of its tail, 63 / 64 / 65 the step between two registers of a lane, rows - 1 the last masked row.
    qr_panel_lds2_kernel<1> holds at most 64 rows, so offsets 64 and 65 cannot occur there, and 63 only as the last row of a 64-row panel."""
    seen, last_row = _offsets_by_route()
    for route in qn.ROUTES:
        tallest = max(p[2] for (m, n) in qn.SHAPES for p in qn.panel_routes(m, n) if (p[0], p[1]) == route)
        need = {o for o in qn.SPECIAL_OFFSETS if o <= tallest - 1}
        if route == (qn.LDS_KERNEL, 1):
            assert need == {0, 1, 2, 63}
        else:
            assert need == set(qn.SPECIAL_OFFSETS)
        assert seen[route] >= need, f"{qn.route_name(route)}: offsets {sorted(need - seen[route])} never occur"
        assert last_row[route], f"{qn.route_name(route)}: no first column of a panel with its pivot in the panel's last row"
        assert len(seen[route] - {0}) >= 4  # x0 == 0 exactly: the x0 >= 0.0 branch decides the sign of R_jj


def _zero_positions(m, n, zero_cols):
    """per kernel kind: positions (first, inner, after a zero column, last of a full panel) the zero columns take"""
    out = {qn.LDS_KERNEL: set(), qn.GLOBAL_KERNEL: set()}
    for j in zero_cols:
        pi, jj = divmod(j, qn.QR_NB)
        kern, _, _, w = qn.panel_routes(m, n)[pi]
        if jj == 0:
            out[kern].add("first")
        if 0 < jj < w - 1:
            out[kern].add("inner")
        if jj == w - 1 and w > 1:
            out[kern].add("last")
        if jj > 0 and j - 1 in zero_cols:
            out[kern].add("after a zero column")
    return out


def test_zero_columns_sit_at_every_panel_position_on_both_kernels():
    want = {"first", "inner", "after a zero column", "last"}
    exact = {qn.LDS_KERNEL: set(), qn.GLOBAL_KERNEL: set()}
    for (m, n, _, zero_cols) in qn.exact_cases():
        for kern, s in _zero_positions(m, n, zero_cols).items():
            exact[kern] |= s
    dense = {qn.LDS_KERNEL: set(), qn.GLOBAL_KERNEL: set()}
    for (m, n, _, zero_cols) in qn.ZERO_DENSE:
        for kern, s in _zero_positions(m, n, zero_cols).items():
            dense[kern] |= s
    for kern in (qn.LDS_KERNEL, qn.GLOBAL_KERNEL):
        assert exact[kern] == want, (kern, exact[kern])
        assert dense[kern] == want, (kern, dense[kern])


# ------------------------------------------------------------------------------------------------ the dense family
def test_dense_cases_pin_the_signs_of_the_diagonal():
    for (m, n) in qn.SHAPES:
        for kind in qn.KINDS:
            seeds = qn.dense_seeds(m, n, kind)
            assert len(set(seeds)) >= 2 and set(seeds) <= set(qn.CONSTANT_SEEDS), (m, n, kind)
    for (m, n, kind, seed) in qn.dense_cases():
        _, _, ratio = qn.reference(qn.dense_case(m, n, kind, seed))
        assert ratio.min() >= qn.MIN_HEAD_RATIO, f"{m} x {n} {kind} seed {seed}: |x0| / |x| = {ratio.min()} in column {ratio.argmin()}"
    for (m, n, seed, zero_cols) in qn.ZERO_DENSE:
        a = qn.zero_dense_case(m, n, seed, zero_cols)
        _, r, ratio = qn.reference(a)
        assert not a[:, list(zero_cols)].any() and not r[:, list(zero_cols)].any()
        assert np.all(np.isinf(ratio[list(zero_cols)])) and ratio.min() >= qn.MIN_HEAD_RATIO
    a = qn.repeated_dense_case()
    for dst, src in qn.REPEATED_DENSE[3]:
        assert np.array_equal(a[:, dst], a[:, src]) and src < dst


def test_reference_and_restatement_agree_on_dense_input():
    """two codes, one convention: the longdouble run of the blocked restatement is the reference to longdouble rounding"""
    for (m, n, kind) in ((100, 50, "gauss"), (40, 100, "graded"), (65, 33, "gauss")):
        a = qn.dense_case(m, n, kind, 0)
        q, r, _ = qn.reference(a)
        b = qn.blocked(a, np.longdouble)
        scale = np.abs(r).max(axis=0)  # per column: graded columns differ by 2^80
        assert np.abs(b.q - q).max() < 1e-15 and (np.abs(b.r - r) / scale).max() < 1e-15
        assert np.array_equal(np.sign(np.diag(b.r)), np.sign(np.diag(r)))


def test_the_restatement_constants_are_the_measured_ones():
    """QR_RESTATEMENT_RES and QR_RESTATEMENT_ORTH: the largest res and orth of blocked(., float64) over every dense case, seeds 0..19"""
    res = orth = 0.0
    where = [None, None]
    for (m, n) in qn.SHAPES:
        for kind in qn.KINDS:
            for seed in qn.CONSTANT_SEEDS:
                a = qn.dense_case(m, n, kind, seed)
                b = qn.blocked(a)
                r, o = qn.res_units(b.q, b.r, a), qn.orth_units(b.q)
                if r > res:
                    res, where[0] = r, (m, n, kind, seed)
                if o > orth:
                    orth, where[1] = o, (m, n, kind, seed)
    print(f"restatement: res {res:.4f} at {where[0]}, orth {orth:.4f} at {where[1]}")
    assert round(res, 2) == qn.QR_RESTATEMENT_RES and round(orth, 2) == qn.QR_RESTATEMENT_ORTH, (res, orth)
    assert qn.C_QR == 8
