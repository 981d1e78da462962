"""swap_site_indices on the device against the exact dense axis permutation and the numpy restatement (tests/swap_np.py): chains of
2 to 6 sites, leg dims 2 and 3, bonds up to 17, at most 4096 dense elements.

Dense tolerance: C_DENSE * n_steps * eps * |T|_F with C_DENSE = 67 = 8 * 8.35: 8.35 is the restatement's own largest deviation from the
exact permutation on these cases (seeds 0 .. 19, in units of n_steps eps |T|_F; 3.6 at the seed used here), 8 the margin for a Jacobi
SVD that rounds differently from LAPACK's.  See tests/swap_np.py; the number was not tuned to the device's output."""
import numpy as np
import pytest

import swap_np as sn
import t4a_amd
from t4a_amd import LegTrain, MPO, SimpleTensorTrain, SwapOptions, swap_site_indices, swap_site_indices_legs

pytestmark = pytest.mark.gpu

CASES = sn.driver_cases()
_INPUTS = {}


def inputs(name, low_rank=False):
    """(cores, legs, target, kind, dense) of a case, made once and left unchanged"""
    key = (name, low_rank)
    if key not in _INPUTS:
        legs, bonds, target, kind = CASES[name]
        rng = np.random.default_rng(0)
        cores = sn.low_rank_train(rng, legs, 3) if low_rank else sn.random_train(rng, legs, bonds)
        _INPUTS[key] = (cores, legs, target, kind, sn.to_dense(cores, legs))
    return _INPUTS[key]


def leg_train(cores, legs):
    return LegTrain(SimpleTensorTrain(cores), legs)


def dense_tol(n_steps, dense):
    return sn.C_DENSE * n_steps * sn.EPS * np.linalg.norm(dense)


def check_isometries(out):
    """sites left of the centre are orthonormal over (left, site), sites right of it over (site, right)"""
    cores = out._tt.site_tensors()
    for i, c in enumerate(cores):
        if i == out.center:
            continue
        m = c.reshape(-1, c.shape[2], order="F") if i < out.center else c.reshape(c.shape[0], -1, order="F").T
        gram = m.T @ m
        assert np.abs(gram - np.eye(gram.shape[0])).max() <= 64 * sn.EPS * max(m.shape), (i, out.center)


@pytest.mark.parametrize("name", sorted(CASES))
def test_swap_equals_the_axis_permuted_dense_input(name):
    cores, legs, target, kind, dense = inputs(name)
    _, ref_legs, ref_center, info = sn.swap(cores, legs, target)
    out = swap_site_indices_legs(leg_train(cores, legs), target)
    # every leg on its target, in ascending key order on the sites a step touched, untouched sites as they were
    assert out.legs == ref_legs
    where = out.assignment()
    assert all(where[k] == v for k, v in target.items())
    assert out.center == ref_center == info["steps"][-1][2]
    exact = sn.permuted(dense, sn.keys_of(legs), out.keys())
    err = np.linalg.norm(out.to_dense() - exact)
    print(f"{name}: |out - exact| = {err / (info['n_steps'] * sn.EPS * np.linalg.norm(dense)):.3f} n_steps eps |T|")
    assert err <= dense_tol(info["n_steps"], dense)
    check_isometries(out)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bonds_equal_the_restatement_at_rtol(name):
    cores, legs, target, _, dense = inputs(name, low_rank=True)
    ref_cores, _, _, info = sn.swap(cores, legs, target, rtol=1e-10)
    assert info["margin"] >= 1e4  # the gap: no decision of the rank rule is near its threshold
    out = swap_site_indices_legs(leg_train(cores, legs), target, SwapOptions(rtol=1e-10))
    assert out.link_dims() == [c.shape[2] for c in ref_cores[:-1]]
    exact = sn.permuted(dense, sn.keys_of(legs), out.keys())
    # what rtol cuts is below 1e-10 s_max per value, at most min(M, N) <= 36 values per step
    assert np.linalg.norm(out.to_dense() - exact) <= dense_tol(info["n_steps"], dense) + info["n_steps"] * 6 * 1e-10 * np.linalg.norm(dense)
    check_isometries(out)


@pytest.mark.parametrize("name,cap", [("mpo_n4", 5), ("reversal_6", 3), ("quantics_r3", 2), ("partial_target", 4)])
def test_max_bond_dim_caps_every_bond_and_the_error_is_the_discarded_weight(name, cap):
    cores, legs, target, _, dense = inputs(name)
    _, _, _, info = sn.swap(cores, legs, target, max_bond_dim=cap)
    out = swap_site_indices_legs(leg_train(cores, legs), target, SwapOptions(max_bond_dim=cap))
    touched = {min(st[1], st[2]) for st in info["steps"]}
    bonds = out.link_dims()
    assert all(bonds[i] <= cap for i in touched)
    assert any(d > 0.0 for d in info["discarded"])  # the cap did cut
    exact = sn.permuted(dense, sn.keys_of(legs), out.keys())
    err = np.linalg.norm(out.to_dense() - exact)
    # the centre is on the bond of every step, so a step's error is the norm of what it cut; the steps add up by the triangle inequality
    bound = sum(np.sqrt(d) for d in info["discarded"])
    print(f"{name}: truncation error {err:.6e}, discarded weight of the restatement {bound:.6e}")
    assert err <= bound * (1.0 + 1e-8) + dense_tol(info["n_steps"], dense)
    check_isometries(out)


def test_mpo_in_and_mpo_out():
    cores, legs, target, kind, dense = inputs("mpo_n4")
    m = MPO([c.reshape(c.shape[0], legs[i][0][1], legs[i][1][1], c.shape[2], order="F") for i, c in enumerate(cores)])
    _, ref_legs, _, info = sn.swap(cores, legs, target)
    out = swap_site_indices(m, target)
    assert isinstance(out, MPO) and kind == "mpo"
    # site j ends with the legs (j, 0) and (3 - j, 1), in ascending key order: (1, 1) before (2, 0) on site 2
    assert [sorted(k for k, _ in s) for s in ref_legs] == [sorted([(j, 0), (3 - j, 1)]) for j in range(4)]
    assert out.site_dims() == [(s[0][1], s[1][1]) for s in ref_legs]
    full = out.full_tensor()  # one axis per leg in train order
    assert np.linalg.norm(full - sn.permuted(dense, sn.keys_of(legs), sn.keys_of(ref_legs))) <= dense_tol(info["n_steps"], dense)


def test_train_in_and_train_out_and_regroup_quantics_there_and_back():
    cores, legs, target, kind, dense = inputs("quantics_r3")
    tt = SimpleTensorTrain(cores)
    seq = t4a_amd.regroup_quantics(tt, 2, to="sequential")
    assert isinstance(seq, SimpleTensorTrain) and kind == "train"
    got = LegTrain.from_train(seq).to_dense()  # axes: x1 x2 x3 y1 y2 y3
    assert np.linalg.norm(got - np.transpose(dense, [0, 2, 4, 1, 3, 5])) <= dense_tol(4, dense)
    back = t4a_amd.regroup_quantics(seq, 2, to="interleaved")
    assert isinstance(back, SimpleTensorTrain)
    assert np.linalg.norm(LegTrain.from_train(back).to_dense() - dense) <= 2 * dense_tol(4, dense)
    out = swap_site_indices(tt, target)  # the same through the general entry
    assert isinstance(out, SimpleTensorTrain) and out.site_dims() == [2] * 6


def test_partial_target_stays_a_leg_train_with_its_centre():
    cores, legs, target, kind, _ = inputs("partial_target")
    out = swap_site_indices(leg_train(cores, legs), target)
    assert isinstance(out, LegTrain) and kind == "legs"
    assert [len(s) for s in out.legs] == [1, 2, 3, 2] and out.center == 2
    with pytest.raises(t4a_amd.T4aError):
        out.as_mpo()


def test_empty_target_and_satisfied_target_return_the_input_unchanged():
    cores, legs, _, _, _ = inputs("n3_exchange")
    tt = SimpleTensorTrain(cores)
    assert swap_site_indices(tt, {}) is tt
    assert swap_site_indices(tt, {(1, 0): 1}) is tt
    assert all(np.array_equal(a, b) for a, b in zip(tt.site_tensors(), cores))  # not canonicalised
    with pytest.raises(t4a_amd.T4aError, match="not in the network"):
        swap_site_indices(tt, {(9, 0): 0})
    with pytest.raises(t4a_amd.T4aError, match="max_bond_dim must be positive"):
        swap_site_indices(tt, {(0, 0): 2}, SwapOptions(max_bond_dim=0))
