"""swap_site_indices without a device: the schedule of SwapSchedule.build against the cases of the reference restated by hand and
against tests/swap_np.py, every error message, the refusals at plan time, the numpy restatement of the driver against the exact
dense axis permutation, the gap condition of the rank tests, and the empty-target no-op."""
import numpy as np
import pytest

import swap_np as sn
import t4a_amd
from t4a_amd import SwapSchedule, T4aError
from t4a_amd import swap as swap_mod

INVALID = t4a_amd.INVALID_ARGUMENT

RESTATEMENT_DEVIATION = sn.RESTATEMENT_DEVIATION  # measured and explained in tests/swap_np.py


def one_leg(n):
    return {k: k for k in range(n)}


def steps_of(s):
    return [st.as_tuple() for st in s.steps]


def test_schedule_n5_last_to_first():
    s = SwapSchedule.build(5, one_leg(5), {4: 0})
    assert steps_of(s) == [([0, 1, 2, 3], 3, 4, {3, 4}, set()), ([4, 3], 3, 2, {3}, {2, 4}), ([], 2, 1, {2}, {1, 4}), ([], 1, 0, {1}, {0, 4})]
    assert s.root == 0


def test_schedule_n5_first_to_last():
    s = SwapSchedule.build(5, one_leg(5), {0: 4})
    assert steps_of(s) == [([], 0, 1, set(), {0, 1}), ([], 1, 2, {1}, {0, 2}), ([], 2, 3, {2}, {0, 3}), ([], 3, 4, {3}, {0, 4})]


def test_schedule_n3_exchange():
    s = SwapSchedule.build(3, one_leg(3), {0: 2, 2: 0})
    assert steps_of(s) == [([], 0, 1, set(), {0, 1}), ([], 1, 2, {1, 2}, {0}), ([2, 1], 1, 0, {1}, {2})]


def most_legs(s):
    return max(max(len(st.a_side_sites), len(st.b_side_sites)) for st in s.steps)


@pytest.mark.parametrize("r,n_steps,legs", [(3, 4, 2), (4, 8, 2), (8, 24, 4)])
def test_schedule_interleaved_to_variable_major(r, n_steps, legs):
    n = 2 * r
    target = {k[0]: v for k, v in swap_mod.quantics_target(n, 2, "sequential").items()}
    s = SwapSchedule.build(n, one_leg(n), target)
    assert (len(s), most_legs(s)) == (n_steps, legs)
    ref = sn.schedule(n, one_leg(n), target)
    assert steps_of(s) == [tuple(x) for x in ref]
    assert len(ref) <= 2 * (n - 1)  # one pass over the edges


def test_schedule_reversal_and_mpo():
    s = SwapSchedule.build(6, one_leg(6), {k: 5 - k for k in range(6)})
    assert (len(s), most_legs(s)) == (9, 3)
    n = 4
    current = {(i, leg): i for i in range(n) for leg in (0, 1)}
    target = {(i, 1): n - 1 - i for i in range(n)}
    m = SwapSchedule.build(n, current, target)
    assert (len(m), most_legs(m)) == (5, 3) and m.steps[3].transport_path == [3, 2]
    assert steps_of(m) == [tuple(x) for x in sn.schedule(n, current, target)]


@pytest.mark.parametrize("seed", range(6))
def test_schedule_matches_the_restatement_on_random_assignments(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 8))
    keys = list(range(int(rng.integers(1, 10))))
    current = {k: int(rng.integers(0, n)) for k in keys}
    target = {k: int(rng.integers(0, n)) for k in keys if rng.random() < 0.6}
    root = int(rng.integers(0, n)) if seed % 2 else 0
    s = SwapSchedule.build(n, current, target, root=root)
    assert steps_of(s) == [tuple(x) for x in sn.schedule(n, current, target, root=root)]
    # replaying the steps puts every targeted leg on its target and leaves the centre on node_b of the last step
    position = dict(current)
    for st in s.steps:
        assert abs(st.node_a - st.node_b) == 1
        position.update({k: st.node_a for k in st.a_side_sites})
        position.update({k: st.node_b for k in st.b_side_sites})
    assert all(position[k] == v for k, v in target.items())


def message(fn):
    with pytest.raises(T4aError) as e:
        fn()
    assert e.value.code == INVALID
    return str(e.value)


def test_every_error_message():
    assert "SwapSchedule::build: root 3 not in topology" in message(lambda: SwapSchedule.build(3, {0: 0}, {0: 1}, root=3))
    assert "target_assignment contains index 7 which is not in the network" in message(lambda: SwapSchedule.build(3, {0: 0}, {7: 1}))
    assert "target node 5 for index 0 is not in the topology" in message(lambda: SwapSchedule.build(3, {0: 0}, {0: 5}))
    assert "current node 4 for index 0 is not in the topology" in message(lambda: SwapSchedule.build(3, {0: 4}, {}))
    assert "did not converge within 0 passes" in message(lambda: SwapSchedule.build(3, {0: 0}, {0: 2}, max_passes=0))
    # the same texts from the restatement
    for fn, text in ((lambda: sn.schedule(3, {0: 0}, {0: 1}, root=3), "root 3 not in topology"),
                     (lambda: sn.schedule(3, {0: 0}, {7: 1}), "index 7 which is not in the network"),
                     (lambda: sn.schedule(3, {0: 0}, {0: 5}), "target node 5 for index 0 is not in the topology"),
                     (lambda: sn.schedule(3, {0: 0}, {0: 2}, max_passes=0), "did not converge within 0 passes")):
        with pytest.raises(ValueError, match=text):
            fn()


def test_plan_refuses_more_than_eight_legs_in_a_pair():
    current = {k: (0 if k < 5 else 1) for k in range(9)}
    dims = {k: 2 for k in current}
    assert len(SwapSchedule.build(2, {k: v for k, v in current.items() if k != 8}, {0: 1}, dims=dims)) == 1  # eight legs pass
    assert "at most 8" in message(lambda: SwapSchedule.build(2, current, {0: 1}, dims=dims))
    assert len(SwapSchedule.build(2, current, {0: 1})) == 1  # the schedule alone has no such limit


def test_plan_refuses_a_side_above_the_fused_dimension_limit():
    current, dims = {0: 0, 1: 1}, {0: 256, 1: 256}
    assert "above 65535" in message(lambda: SwapSchedule.build(2, current, {0: 1}, dims=dims))
    assert len(SwapSchedule.build(2, current, {0: 1}, dims={0: 255, 1: 257})) == 1  # 65535 itself passes


def test_plan_refuses_a_work_matrix_above_int_max():
    # {1 -> 2} is one step on the edge (1, 2): M = bond(0, 1) * 1 rows and N = (2 * 2) * bond(2, 3) columns
    current, dims = {k: k for k in range(4)}, {k: 2 for k in range(4)}
    assert "INT_MAX" in message(lambda: SwapSchedule.build(4, current, {1: 2}, dims=dims, link_dims=[60000, 2, 60000]))
    assert len(SwapSchedule.build(4, current, {1: 2}, dims=dims, link_dims=[6, 2, 6])) == 1
    assert len(SwapSchedule.build(4, current, {1: 2}, dims=dims)) == 1  # without bonds there is nothing to multiply
    assert "link_dims needs dims" in message(lambda: SwapSchedule.build(4, current, {1: 2}, link_dims=[2, 2, 2]))


def test_options_defaults_and_alias():
    assert t4a_amd.SwapOptions().max_bond_dim is None and t4a_amd.SwapOptions().rtol is None
    assert t4a_amd.swap_site_indices_by_index is t4a_amd.swap_site_indices


@pytest.mark.parametrize("name", sorted(sn.driver_cases()))
def test_restatement_equals_the_exact_axis_permutation(name):
    legs, bonds, target, _ = sn.driver_cases()[name]
    cores = sn.random_train(np.random.default_rng(0), legs, bonds)
    dense = sn.to_dense(cores, legs)
    out, out_legs, center, info = sn.swap(cores, legs, target)
    exact = sn.permuted(dense, sn.keys_of(legs), sn.keys_of(out_legs))
    dev = np.linalg.norm(sn.to_dense(out, out_legs) - exact) / (info["n_steps"] * sn.EPS * np.linalg.norm(dense))
    print(f"{name}: restatement deviates by {dev:.3f} n_steps eps |T|")
    assert dev <= RESTATEMENT_DEVIATION
    where = {k: i for i, site in enumerate(out_legs) for k, _ in site}
    assert all(where[k] == v for k, v in target.items())
    assert center == info["steps"][-1][2]
    touched = {x for st in info["steps"] for x in (st[1], st[2])}
    for i, site in enumerate(out_legs):
        if i in touched:
            assert [k for k, _ in site] == sorted(k for k, _ in site)
        else:
            assert site == legs[i]


@pytest.mark.parametrize("name", sorted(sn.driver_cases()))
def test_gap_condition_of_the_rank_tests(name):
    """the operands of the rank tests: every singular value a step decides on is at least 1e4 away from rtol * s_max, so that a
    Jacobi SVD and LAPACK's cannot decide differently"""
    legs, _, target, _ = sn.driver_cases()[name]
    cores = sn.low_rank_train(np.random.default_rng(0), legs, 3)
    _, _, _, info = sn.swap(cores, legs, target, rtol=1e-10)
    assert info["margin"] >= 1e4


def test_retained_rank_is_the_rule_of_the_library():
    rng = np.random.default_rng(1)
    for _ in range(20):
        s = np.sort(np.abs(rng.standard_normal(6)) * 10.0 ** rng.integers(-14, 1, 6))[::-1].copy()
        for thr in (0.0, 1e-10, 1e-3):
            pol = t4a_amd.SvdTruncationPolicy(threshold=thr)
            assert sn.retained_rank(s, thr, None) == t4a_amd.svd_retained_rank(s, pol)


def test_quantics_targets_are_inverse_to_each_other():
    there = swap_mod.quantics_target(8, 2, "sequential")
    back = swap_mod.quantics_target(8, 2, "interleaved")
    assert there == sn.quantics_target(8, 2, "sequential") and back == sn.quantics_target(8, 2, "interleaved")
    assert all(back[(there[k], 0)] == k[0] for k in there)
    assert "equally many bits" in message(lambda: swap_mod.quantics_target(7, 2, "sequential"))


def test_empty_target_is_a_no_op_of_the_restatement():
    legs, bonds, _, _ = sn.driver_cases()["n3_exchange"]
    cores = sn.random_train(np.random.default_rng(0), legs, bonds)
    out, out_legs, center, info = sn.swap(cores, legs, {})
    assert center is None and info["n_steps"] == 0 and out_legs == legs
    assert all(np.array_equal(a, b) for a, b in zip(out, cores))  # not canonicalised
    assert len(SwapSchedule.build(3, one_leg(3), {})) == 0 and len(SwapSchedule.build(3, one_leg(3), {1: 1})) == 0
