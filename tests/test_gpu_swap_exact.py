"""Exact tests of the step kernel of swap_site_indices (csrc/kernels_swap.hip, through the hook swap_theta) and of
LegTrain.reorder_legs.  The entries of both cores come from {-1, 0, 1} and the bond is at most 33, so every sum is an integer of
magnitude at most 33 and is exact in f64 whatever the summation order: the kernel must EQUAL the int64 einsum.

The kernel has three thresholds.  A 16 x 16 tile of (l, r) that lies inside runs on the matrix cores, every other tile per thread:
l and r from {1, 2, 15, 16, 17, 33} straddle it (15: no matrix-core tile, 16: only such tiles, 17 and 33: both routes in one launch,
l != r, l = 1, r = 1).  The matrix-core route sums m in chunks of 4 and loads 4 chunks per trip: m from {1, 3, 4, 5, 16, 17, 33}
straddles both.  A workgroup holds four wavefronts: shapes with fewer and with more than four work items occur."""
import numpy as np
import pytest

import swap_np as sn
import t4a_amd
from t4a_amd import swap as swap_mod

pytestmark = pytest.mark.gpu

MS = (1, 3, 4, 5, 16, 17, 33)
LR = ((1, 1), (2, 2), (15, 15), (16, 16), (17, 17), (33, 33), (1, 16), (16, 1), (1, 33), (33, 2), (15, 17), (17, 16), (16, 33), (33, 16))

# name -> (legs_left, legs_right, a_side, b_side, left_moving); leg dims 2 and 3 mixed
PLANS = {
    "nothing_moves": ([(0, 2), (1, 3)], [(2, 3)], {0, 1}, {2}, False),
    "full_exchange": ([(1, 3), (0, 2)], [(2, 3), (3, 2)], {2, 3}, {0, 1}, False),  # (the left site not in key order)
    "all_to_a": ([(0, 2), (1, 3)], [(2, 2)], {0, 1, 2}, set(), False),
    "all_to_b": ([(0, 3), (1, 2)], [(2, 2)], set(), {0, 1, 2}, False),
    "site_without_leg": ([], [(0, 2), (1, 3)], {1}, {0}, False),
    "three_legs_on_a_site": ([(0, 2), (1, 3), (2, 2)], [(3, 3)], {1, 3}, {0, 2}, False),
    "left_moving": ([(0, 3)], [(1, 2), (2, 2)], {0, 2}, {1}, True),
}


def cores(rng, l, x, m, y, r):
    return rng.integers(-1, 2, size=(l, x, m)), rng.integers(-1, 2, size=(m, y, r))


def expected_route(l, r):
    return (swap_mod.ROUTE_MFMA if l >= 16 and r >= 16 else 0) | (swap_mod.ROUTE_SCALAR if l % 16 or r % 16 else 0)


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_swap_theta_equals_the_integer_einsum(plan):
    legs_left, legs_right, a_side, b_side, left_moving = PLANS[plan]
    x = int(np.prod([d for _, d in legs_left], dtype=np.int64))
    y = int(np.prod([d for _, d in legs_right], dtype=np.int64))
    to_left, to_right = (b_side, a_side) if left_moving else (a_side, b_side)
    rng = np.random.default_rng(sorted(PLANS).index(plan))
    routes = set()
    for m in MS:
        for l, r in LR:
            a, b = cores(rng, l, x, m, y, r)
            want, _, _ = sn.theta_np(a, b, legs_left, legs_right, to_left, to_right)  # int64 throughout
            assert want.dtype == np.int64 and np.abs(want).max() <= 33
            got, route = t4a_amd.swap_theta(a, b, legs_left, legs_right, a_side, b_side, left_moving=left_moving)
            assert got.shape == want.shape
            assert np.array_equal(got, want.astype(np.float64)), (plan, l, m, r)
            assert route == expected_route(l, r), (l, r, route)
            routes.add(route)
            if plan == "nothing_moves":  # the plain two-site contraction
                plain = np.einsum("lxm,myr->lxyr", a, b).reshape(l * x, y * r, order="F")
                assert np.array_equal(got, plain.astype(np.float64))
    # both routes ran alone and together
    assert routes == {swap_mod.ROUTE_SCALAR, swap_mod.ROUTE_MFMA, swap_mod.ROUTE_SCALAR | swap_mod.ROUTE_MFMA}


def test_shapes_straddle_every_threshold():
    ls = {l for l, _ in LR} | {r for _, r in LR}
    assert {15, 16, 17} <= ls and {1, 33} <= ls            # the tile edge, a bond of one, more than one tile with a ragged one
    assert {3, 4, 5} <= set(MS) and {16, 17} <= set(MS)    # the chunk of four and the trip of four chunks
    assert any(l != r for l, r in LR) and any(l == 1 for l, _ in LR) and any(r == 1 for _, r in LR)
    assert expected_route(15, 33) == swap_mod.ROUTE_SCALAR and expected_route(16, 16) == swap_mod.ROUTE_MFMA


def test_swap_theta_refuses_what_is_no_step():
    a, b = np.zeros((2, 2, 3)), np.zeros((3, 3, 2))
    for args in (([(0, 2)], [(1, 3)], {0}, {0, 1}), ([(0, 2)], [(1, 3)], {0}, set()), ([(0, 2)], [(0, 3)], {0}, set())):
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.swap_theta(a, b, *args)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT


@pytest.mark.parametrize("bonds", [(1, 2, 1), (2, 17, 3), (3, 5, 16)])
def test_reorder_legs_is_the_exact_axis_permutation(bonds):
    rng = np.random.default_rng(sum(bonds))
    legs = [[(0, 2), (1, 3), (2, 2)], [(3, 3)], [(4, 3), (5, 2)], [(6, 2), (7, 2), (8, 3), (9, 3)]]
    b = [1] + list(bonds) + [1]
    cs = [rng.integers(-1, 2, size=(b[i], int(np.prod([d for _, d in s])), b[i + 1])).astype(np.float64) for i, s in enumerate(legs)]
    lt = t4a_amd.LegTrain(t4a_amd.SimpleTensorTrain(cs), legs)
    dense = lt.to_dense()
    orders = {0: [2, 0, 1], 2: [5, 4], 3: [9, 6, 8, 7]}  # site 1 is not named and stays
    assert lt.reorder_legs(orders) is lt
    new = lt._tt.site_tensors()
    for i, site in enumerate(legs):
        want = cs[i]
        if i in orders:
            dims = [d for _, d in site]
            keys = [k for k, _ in site]
            t = cs[i].reshape([cs[i].shape[0]] + dims + [cs[i].shape[2]], order="F")
            t = np.transpose(t, [0] + [1 + keys.index(k) for k in orders[i]] + [len(dims) + 1])
            want = t.reshape(cs[i].shape, order="F")
            assert [k for k, _ in lt.legs[i]] == orders[i]
        assert np.array_equal(new[i], want)
    assert np.array_equal(lt.to_dense(keys=sn.keys_of(legs)), dense)
    with pytest.raises(t4a_amd.T4aError):
        lt.reorder_legs({1: [3, 3]})
