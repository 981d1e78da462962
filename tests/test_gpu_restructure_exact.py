"""The fuse kernel and fuse_to on the device against exact answers: operands with integer entries in -2 .. 2, so that every product
and every partial sum of a contraction is an integer far below 2^53 and the result must equal int64 arithmetic bit for bit, whatever
route an element takes.  One fuse_round call holds jobs that together straddle every threshold of the kernel: (l, r) below the tile,
equal to it, one past it in l, two tiles with an edge in r; the bond m below a chunk of four, no multiple of it, a whole pass of
sixteen, one past it."""
import itertools

import numpy as np
import pytest

import restructure_np as rn
import swap_np as sn
from t4a_amd import LegTrain, SimpleTensorTrain, fuse_round, fuse_to, swap_theta
from t4a_amd import restructure as rmod

pytestmark = pytest.mark.gpu

SCALAR, MFMA = rmod.ROUTE_SCALAR, rmod.ROUTE_MFMA
LR = [(3, 5), (16, 16), (17, 16), (32, 33)]
MS = [1, 5, 16, 18]
ROUTE = {(3, 5): SCALAR, (16, 16): MFMA, (17, 16): SCALAR | MFMA, (32, 33): SCALAR | MFMA}


def ints(rng, shape):
    return rng.integers(-2, 3, size=shape).astype(np.float64)


def exact_pair(a, b, dims=None, order=None):
    """int64 arithmetic: A[l, x, m] B[m, y, r] -> [l, x + X y, r], the legs (dims, chain order) then in the order `order`"""
    t = np.einsum("lxm,myr->lxyr", a.astype(np.int64), b.astype(np.int64))
    l, r = a.shape[0], b.shape[2]
    t = t.reshape(l, -1, r, order="F")
    if dims:
        t = t.reshape([l] + list(dims) + [r], order="F")
        t = np.transpose(t, [0] + [1 + p for p in order] + [len(dims) + 1]).reshape(l, -1, r, order="F")
    return t


_JOBS = {}


def threshold_jobs():
    """the jobs of the one call, made once: every (l, r) x m, X and Y in 1 .. 3, and a member without legs (X = 1, Y = 1)"""
    if not _JOBS:
        rng = np.random.default_rng(0)
        jobs, shapes = [], []
        for k, ((l, r), m) in enumerate(itertools.product(LR, MS)):
            x, y = 1 + k % 3, 1 + (k // 3) % 3
            jobs.append((ints(rng, (l, x, m)), ints(rng, (m, y, r))))
            shapes.append((l, r))
        jobs.append((ints(rng, (17, 1, 18)), ints(rng, (18, 1, 16))))  # the accumulated core of sites without legs
        shapes.append((17, 16))
        _JOBS["jobs"], _JOBS["shapes"] = jobs, shapes
        _JOBS["out"] = fuse_round(jobs)
    return _JOBS["jobs"], _JOBS["shapes"], _JOBS["out"]


def test_one_call_over_every_threshold_is_exact_and_takes_the_predicted_routes():
    jobs, shapes, out = threshold_jobs()
    assert len(out) == len(LR) * len(MS) + 1
    for (a, b), lr, (res, route) in zip(jobs, shapes, out):
        assert route == ROUTE[lr], (lr, route)
        assert res.shape == (a.shape[0], a.shape[1] * b.shape[1], b.shape[2])
        assert np.array_equal(res, exact_pair(a, b).astype(np.float64)), (a.shape, b.shape)
    assert {ROUTE[s] for s in shapes} == {SCALAR, MFMA, SCALAR | MFMA}


def test_two_runs_give_the_same_bits_and_a_job_does_not_depend_on_the_others():
    jobs, _, out = threshold_jobs()
    again = fuse_round(jobs)
    for (r1, _), (r2, _) in zip(out, again):
        assert np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
    rng = np.random.default_rng(1)
    for k in (0, 6, 9, 15):  # one job of every (l, r) alone, on generic operands
        a, b = rng.standard_normal(jobs[k][0].shape), rng.standard_normal(jobs[k][1].shape)
        alone = fuse_round([(a, b)])[0][0]
        others = [(rng.standard_normal(x.shape), rng.standard_normal(y.shape)) for x, y in jobs[:5]]
        among = fuse_round(others[:2] + [(a, b)] + others[2:])[2][0]
        assert np.array_equal(alone.view(np.uint64), among.view(np.uint64))


@pytest.mark.parametrize("l,m,r", [(3, 5, 5), (16, 16, 16), (17, 18, 16), (32, 7, 33)])
def test_a_pair_in_chain_order_has_the_bits_of_swap_theta_with_every_leg_left(l, m, r):
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((l, 6, m)), rng.standard_normal((m, 2, r))
    legs_left, legs_right = [(0, 2), (1, 3)], [(2, 2)]
    theta, route = swap_theta(a, b, legs_left, legs_right, [0, 1, 2], [])
    out, froute = fuse_round([(a, b)])[0]
    assert froute == route
    assert theta.shape == (l * 12, r)
    assert np.array_equal(out.reshape(l * 12, r, order="F").view(np.uint64), theta.view(np.uint64))
    # the table of the chain order itself is the same launch
    tabled = fuse_round([(a, b, [2, 3, 2], [0, 1, 2])])[0][0]
    assert np.array_equal(tabled.view(np.uint64), out.view(np.uint64))


def test_every_permutation_of_three_legs_on_the_last_round():
    rng = np.random.default_rng(3)
    dims = [2, 3, 2]
    a, b = ints(rng, (17, 6, 5)), ints(rng, (5, 2, 18))
    perms = list(itertools.permutations(range(3)))
    out = fuse_round([(a, b, dims, list(p)) for p in perms])  # one launch for all six
    for p, (res, route) in zip(perms, out):
        assert route == SCALAR | MFMA
        assert np.array_equal(res, exact_pair(a, b, dims, p).astype(np.float64)), p


_TRAIN = {}


def mixed_train():
    """groups of 1, 2 and 3 sites at once; a site without legs at the left end (joins group 0), between groups 0 and 1 (joins the
    smaller index) and inside group 1; a group of one site in another order; bonds on both sides of the tile"""
    if not _TRAIN:
        rng = np.random.default_rng(4)
        legs = [[], [("a", 2), ("b", 3)], [], [("c", 2)], [], [("d", 3)], [("e", 2)], [("f", 2)], [("g", 3), ("h", 2)]]
        bonds = [3, 17, 16, 16, 18, 33, 32, 17]
        target = [["b", "a"], ["d", "c"], ["f", "e"], ["h", "g"]]
        cores = rn.int_train(rng, legs, bonds)
        _TRAIN.update(legs=legs, target=target, cores=cores)
    return _TRAIN["cores"], _TRAIN["legs"], _TRAIN["target"]


def test_fuse_to_with_groups_of_one_two_and_three_sites_is_exact():
    cores, legs, target = mixed_train()
    fp = rn.fuse_plan(legs, target)
    assert sorted(len(m) for m in fp["members"]) == [1, 2, 3, 3]
    assert fp["members"] == [[0, 1, 2], [3, 4, 5], [6, 7], [8]]
    ref_cores, ref_legs = rn.fuse([c.astype(np.int64) for c in cores], legs, target)
    lt = LegTrain(SimpleTensorTrain(cores), legs, center=6)
    out, launches = fuse_to(lt, target, as_legs=True, counted=True)
    assert out.legs == ref_legs
    assert out.center == 2  # the group that holds site 6
    got = out._tt.site_tensors()
    assert len(got) == 4
    for g, r in zip(got, ref_cores):
        assert g.shape == r.shape and np.array_equal(g, r.astype(np.float64))
    # k_max - 1 rounds for all groups together, plus the one reorder launch of the group of one site
    assert launches == (3 - 1) + 1 == fp["launches"]
    again = fuse_to(lt, target, as_legs=True)._tt.site_tensors()
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(got, again))


def test_a_groups_bits_do_not_depend_on_the_other_groups_of_the_call():
    rng = np.random.default_rng(5)
    legs = sn.train_legs([2, 3, 2, 2, 3, 2, 2])
    cores = sn.random_train(rng, legs, [2, 6, 17, 16, 6, 2])
    k = [(i, 0) for i in range(7)]
    full = fuse_to(LegTrain(SimpleTensorTrain(cores), legs), [[k[0]], [k[2], k[1], k[3]], [k[4], k[5]], [k[6]]], as_legs=True)
    alone = fuse_to(LegTrain(SimpleTensorTrain(cores), legs), [[k[0]], [k[2], k[1], k[3]], [k[4]], [k[5]], [k[6]]], as_legs=True)
    a, b = full._tt.site_tensors()[1], alone._tt.site_tensors()[1]
    assert a.shape == b.shape == (2, 12, 16)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
