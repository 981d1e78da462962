"""The exact LUCI fixtures of luci_exact_np.py, pinned on the CPU: for every case of its table and both orientations the oracle returns the
constructed rank, pivot lists and factors bit for bit, the rational references are representable (asserted while they are built), every
sum the factor kernels form stays inside the bit budget, and the route named for the case is the one the launchers' conditions give.
test_gpu_luci_exact.py takes its expected values from the construction alone, never from the oracle.
"""
import numpy as np
import pytest

import luci_exact_np as lx
import oracle_binding as ob

IDS = [lx.case_id(c) for c in lx.CASES]


def test_the_table_holds_every_required_case():
    have = {(c[0], c[1], tuple(c[2]), c[3]) for c in lx.CASES}
    need = [(8, 6, [4], None), (33, 20, [1], None), (40, 50, [16], None), (12, 30, [12], None), (30, 12, [12], None),
            (1024, 40, [3, 2], None), (40, 1024, [3, 2], None), (1025, 40, [3, 2], None), (40, 1025, [3, 2], None), (64, 64, [17], None),
            (70, 90, [24], None), (20, 20, [20], None), (100, 100, [8] * 7 + [7], None), (120, 110, [16] * 5, None),
            (300, 310, [15] * 16, None), (40, 50, [16], 10), (70, 90, [24], 16), (100, 90, [8] * 8, 20), (100, 90, [8] * 8, None),
            (130, 150, [8] * 12, None), (120, 110, [12, 5, 16, 1, 9, 16, 3], None), (200, 180, [16] * 6, None)]
    for m, n, ranks, cap in need:
        assert (m, n, tuple(ranks), cap) in have, (m, n, ranks, cap)
    # rk = 64 with 15, then 16 right-hand sides, in each orientation
    for m, n in ((79, 100), (80, 100), (100, 79), (100, 80)):
        assert (m, n, (8,) * 8, None) in have


@pytest.mark.parametrize("case", lx.CASES, ids=IDS)
def test_route_named_in_the_table_is_the_launchers(case):
    m, n, ranks, cap, route_l, route_r = case
    rank = sum(ranks) if cap is None else min(cap, sum(ranks))
    assert lx.route_of(m, n, rank, True) == route_l
    assert lx.route_of(m, n, rank, False) == route_r


def test_split_k_case_splits_both_products():
    # (300, 310), rank 240: L11 U is 240 x 310 over k = 240, L U11 is 300 x 240 over k = 240
    assert lx._gemm_ksplit(240, 310, 240) > 1 and lx._gemm_ksplit(300, 240, 240) > 1
    assert lx._gemm_ksplit(96, 180, 96) == 1  # (three k-tiles: never split)


@pytest.mark.parametrize("left", [True, False], ids=["left", "right"])
@pytest.mark.parametrize("case", lx.CASES, ids=IDS)
def test_oracle_returns_the_constructed_factors(case, left):
    fx = lx.fixture(case)
    cap = case[3]
    rank, rows, cols, exp_l, exp_r = lx.expected(case, left)
    assert np.abs(fx.a).max() == 1.0
    ref = ob.luci(fx.a, max_bond_dim=cap, rel_tol=lx.REL_TOL, abs_tol=lx.ABS_TOL, left_orthogonal=left)
    assert ref["rank"] == rank
    assert np.array_equal(ref["rows"], rows)
    assert np.array_equal(ref["cols"], cols)
    assert np.array_equal(ref["left"], exp_l)
    assert np.array_equal(ref["right"], exp_r)
    # the selection half is a slice of A, the other half the identity on the pivots
    if left:
        assert np.array_equal(exp_r, fx.a[rows, :]) and np.array_equal(exp_l[rows, :], np.eye(rank))
    else:
        assert np.array_equal(exp_l, fx.a[:, cols]) and np.array_equal(exp_r[:, cols], np.eye(rank))
    # condition (2), in full: every sum of the factor kernels, from the factored buffer (bitwise the device's)
    fac, rp, cp, npiv, _ = ob.rrlu(fx.a, max_bond_dim=cap, rel_tol=lx.REL_TOL, abs_tol=lx.ABS_TOL, left_orthogonal=left)
    assert npiv == rank and np.array_equal(rp[:rank], rows) and np.array_equal(cp[:rank], cols)
    bits = lx.bit_budget(fac, rp, cp, rank, left, exp_l, exp_r)
    assert bits < 52, bits


def test_bit_budget_sees_an_overflowing_sum():
    """The check itself: 1 + 2^-60 needs 61 bits; with equal units it needs 2."""
    one = np.array([[1.0]])
    assert 60 < lx._budget(one, one, extra=np.array([[2.0 ** -60]])) < 62
    assert 0.9 < lx._budget(one, one, extra=one) < 1.1


@pytest.mark.parametrize("tc", lx.TCI_CASES, ids=[lx.tci_case_id(t) for t in lx.TCI_CASES])
def test_oracle_tci2_returns_the_constructed_cores(tc):
    """The same matrices as a two-site (or padded three-site) function through the oracle's TensorCI2: bond sets and cores are the
    constructed ones after every step that test_gpu_luci_exact.py takes."""
    from t4a_amd import TCI2Options
    fx = lx.tci_fixture(tc)
    tci = ob.OracleTCI2(lx.tci_dims(fx, tc[0]))
    lx.tci_check(tci, TCI2Options(tolerance=1e-15, nsearch=0, max_nglobal_pivot=0), fx, tc[0])


def test_block_rook_takes_other_pivots():
    """Why matrix_luci_factors_from_blocks has no exact test: the block-rook search accepts any entry that is the largest of its row and
    its column.  On one block it finds the constructed pivots in another order; on several it ends early (every row and column it
    visits from a found block has a zero residual)."""
    one = next(c for c in lx.CASES if c[:4] == (64, 64, [17], None))
    fx = lx.fixture(one)
    ref = ob.luci_rook(fx.a, rel_tol=lx.REL_TOL, abs_tol=lx.ABS_TOL)
    assert ref["rank"] == 17 and sorted(ref["row_indices"]) == sorted(fx.rows) and not np.array_equal(ref["row_indices"], fx.rows)
    many = next(c for c in lx.CASES if c[:4] == (100, 90, [8] * 8, None))
    assert ob.luci_rook(lx.fixture(many).a, rel_tol=lx.REL_TOL, abs_tol=lx.ABS_TOL)["rank"] < 64


@pytest.mark.parametrize("left", [True, False], ids=["left", "right"])
@pytest.mark.parametrize("shape,maxb", [((8, 6), 4), ((40, 50), 16), ((33, 20), 8)])
def test_componentwise_bound_holds_for_the_oracle_and_sees_a_small_entry(shape, maxb, left):
    """The check that test_gpu_dense.py test_luci_factors applies to the device, on the oracle's factors: inside the bound, and one
    entry of the solved half off by 1e-9 of ITSELF is outside it, which 1e-10 of the largest entry does not notice."""
    rng = np.random.default_rng(11)
    a = rng.uniform(-1, 1, size=shape)
    ref = ob.luci(a, max_bond_dim=maxb, left_orthogonal=left)
    fac, rp, cp, npiv, _ = ob.rrlu(a, max_bond_dim=maxb, left_orthogonal=left)
    solve, prod = lx.componentwise_ratios(fac, rp, cp, npiv, left, ref["left"], ref["right"])
    assert solve <= 1.0 and prod <= 1.0
    half = (ref["left"] if left else ref["right"]).copy()
    live = np.argwhere((half != 0) & (half != 1))
    i, j = live[np.argmin(np.abs(half[live[:, 0], live[:, 1]]))]
    half[i, j] *= 1 + 1e-9
    assert np.abs(half - (ref["left"] if left else ref["right"])).max() <= 1e-10 * max(1.0, np.abs(half).max())
    solve, _ = lx.componentwise_ratios(fac, rp, cp, npiv, left, half if left else ref["left"], ref["right"] if left else half)
    assert solve > 1.0
