"""fuse_to, split_to and restructure_to without a device: every plan kind and the precedence of build_plan, the reference's own cases
(treetn/restructure/mod.rs tests, restated by position), the absorption of sites without legs, the swap-then-fuse assignment, every
message and plan-time refusal, the launch counts of fuse_plan, and the numpy restatement (tests/restructure_np.py) against dense
reshapes and transposes, with the constant the device's split tolerance is derived from."""
import itertools

import numpy as np
import pytest

import restructure_np as rn
import swap_np as sn
import t4a_amd
from t4a_amd import T4aError, fuse_plan, restructure_plan, split_plan
from t4a_amd import restructure as rmod

INVALID, NOT_IMPLEMENTED = t4a_amd.INVALID_ARGUMENT, t4a_amd.NOT_IMPLEMENTED


def one(dims, keys=None):
    """one leg per site"""
    keys = list(range(len(dims))) if keys is None else keys
    return [[(k, d)] for k, d in zip(keys, dims)]


def raises(code, text, fn, *args, **kw):
    with pytest.raises(T4aError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def same_plan(legs, target, link_dims=None):
    """the library's plan, checked against the restatement's"""
    p = restructure_plan(legs, target, link_dims)
    ref = rn.plan(legs, target, link_dims)
    for k in ("kind", "legs", "fuse_rounds", "fuse_launches", "n_qr", "swap_target"):
        assert p[k] == ref[k], (k, p[k], ref[k])
    return p


# ------------------------------------------------------------------------------------------------ kinds, the reference's cases
def test_two_node_fuse():
    p = same_plan(one([2, 2], ["left", "right"]), [["left", "right"]])
    assert (p["kind"], p["fuse_rounds"], p["fuse_launches"]) == ("FuseOnly", 1, 1)
    assert p["legs"] == [[("left", 2), ("right", 2)]]


def test_dangling_and_internal_sites_without_legs_are_absorbed():
    # A(left) - B(right) - C(): the dangling leaf joins B; A(left) - M() - B(right): M has two neighbouring groups, the smaller index
    p = same_plan([[("left", 2)], [("right", 2)], []], [["left"], ["right"]])
    assert (p["kind"], p["fuse_rounds"]) == ("FuseOnly", 1)
    assert rn.fuse_plan([[("left", 2)], [("right", 2)], []], [["left"], ["right"]])["members"] == [[0], [1, 2]]
    p = same_plan([[("left", 2)], [], [("right", 2)]], [["left"], ["right"]])
    assert p["kind"] == "FuseOnly"
    assert rn.fuse_plan([[("left", 2)], [], [("right", 2)]], [["left"], ["right"]])["members"] == [[0, 1], [2]]


def test_absorption_runs_to_a_fixed_point():
    legs = [[], [], [("a", 2)], [], [("b", 2)], [], [], [], [("c", 3)], []]
    target = [["b", "a"], ["c"]]
    fp = rn.fuse_plan(legs, target)
    # step 4: site 3 between a and b; step 4b: 1 then 0 join group 0, 5 joins 0, 7 joins 1, then 6 lies between both: the smaller
    assert fp["members"] == [[0, 1, 2, 3, 4, 5, 6], [7, 8, 9]]
    p = fuse_plan(legs, target)
    assert (p["rounds"], p["launches"], p["legs"]) == (6, 6, [[("b", 2), ("a", 2)], [("c", 3)]])


def test_groups_of_two_split_then_fuse_and_swap_only():
    legs = [[("x0", 2), ("x1", 2)], [("y0", 2), ("y1", 2)]]
    p = same_plan(legs, [["x0"], ["x1", "y0"], ["y1"]])
    assert (p["kind"], p["n_qr"], p["fuse_rounds"]) == ("SplitThenFuse", 2, 1)
    p = same_plan(legs, [["x0", "y0"], ["x1", "y1"]])  # the cross pairing of two nodes
    assert p["kind"] == "SwapOnly" and p["swap_target"] == {"x0": 0, "y0": 0, "x1": 1, "y1": 1}


def test_four_node_interleaved_is_swap_then_fuse_with_the_block_assignment():
    legs = one([2, 2, 2, 2], ["x0", "x1", "y0", "y1"])
    p = same_plan(legs, [["x0", "y0"], ["x1", "y1"]])
    assert p["kind"] == "SwapThenFuse"
    # groups in target order take consecutive blocks of as many sites as contribute; ascending keys to block[min(position, len - 1)]
    assert p["swap_target"] == {"x0": 0, "y0": 1, "x1": 2, "y1": 3}
    assert (p["fuse_rounds"], p["fuse_launches"]) == (1, 1)
    # more keys than contributing sites: the tail shares the block's last site
    legs = [[("a", 2), ("b", 2)], [("c", 2)], [("d", 2), ("e", 2)], [("f", 2)]]
    p = same_plan(legs, [["d", "e", "a", "b"], ["c", "f"]])
    assert p["kind"] == "SwapThenFuse" and p["swap_target"] == {"a": 0, "b": 1, "d": 1, "e": 1, "c": 2, "f": 3}


def test_three_node_swap_only_and_split_only():
    legs = [[("s0", 2), ("s1", 2)], [("s2", 2)], [("s3", 2)]]
    p = same_plan(legs, [["s0"], ["s1", "s2"], ["s3"]])
    assert p["kind"] == "SwapOnly" and p["swap_target"] == {"s0": 0, "s1": 1, "s2": 1, "s3": 2}
    p = same_plan([[("left", 2), ("right", 2)]], [["left"], ["right"]])
    assert (p["kind"], p["n_qr"]) == ("SplitOnly", 1)


def test_a_whole_site_permutation_is_swap_then_fuse_not_swap_only():
    p = same_plan(one([2, 3, 2, 3]), [[3], [1], [0], [2]])
    assert p["kind"] == "SwapThenFuse" and p["swap_target"] == {3: 0, 1: 1, 0: 2, 2: 3}
    assert p["fuse_rounds"] == 0


@pytest.mark.parametrize("name", sorted(rn.restructure_cases()))
def test_the_shared_cases_have_the_kind_they_are_named_for(name):
    legs, bonds, target, kind = rn.restructure_cases()[name]
    assert same_plan(legs, target, bonds)["kind"] == kind


def test_widened_split_then_fuse_and_what_still_gets_the_placeholder():
    # 2-bit sites into 3-bit sites: site 1 holds two fragments shared with neighbours, which the reference gives up on
    bits2 = [[((2 * s, 0), 2), ((2 * s + 1, 0), 2)] for s in range(3)]
    p = same_plan(bits2, [[(0, 0), (1, 0), (2, 0)], [(3, 0), (4, 0), (5, 0)]])
    assert (p["kind"], p["n_qr"], p["fuse_rounds"]) == ("SplitThenFuse", 1, 1)
    # fragments that would have to cross: site 0 holds groups 0 and 1, site 2 group 0 again
    legs = [[("a", 2), ("b", 2)], [("c", 2), ("d", 2)], [("e", 2)]]
    raises(NOT_IMPLEMENTED, rn.PLACEHOLDER, restructure_plan, legs, [["a", "e"], ["b", "c", "d"]])
    with pytest.raises(NotImplementedError):
        rn.plan(legs, [["a", "e"], ["b", "c", "d"]])


# ------------------------------------------------------------------------------------------------ messages and refusals
def test_target_refusals():
    legs = one([2, 2, 2])
    for op, fn in (("restructure_to", restructure_plan), ("fuse_to", fuse_plan), ("split_to", split_plan)):
        raises(INVALID, f"{op}: target node 1 has no site indices", fn, legs, [[0, 1, 2], []])
        raises(INVALID, f"{op}: site index 1 appears in both target nodes 0 and 1", fn, legs, [[0, 1], [1, 2]])
    raises(INVALID, "restructure_to: current and target must contain the same site indices", restructure_plan, legs, [[0, 1]])
    raises(INVALID, "restructure_to: current and target must contain the same site indices", restructure_plan, legs, [[0, 1, 2, 3]])
    raises(INVALID, "fuse_to: missing target for current node 2", fuse_plan, legs, [[0, 1]])
    raises(INVALID, "fuse_to: incompatible target structure: target node 0", fuse_plan, legs, [[0, 1, 2, 7]])
    raises(INVALID, "split_to: target site index 7 is missing from the current network", split_plan, legs, [[0], [1], [2, 7]])
    raises(INVALID, "in current node 2 has no corresponding target node", split_plan, legs, [[0], [1]])


def test_fuse_messages():
    raises(INVALID, "fuse_to: ambiguous mapping: current node 0 maps to multiple target nodes", fuse_plan, [[("a", 2), ("b", 2)], [("c", 2)]],
           [["a"], ["b", "c"]])
    raises(INVALID, "Nodes to contract do not form a connected subtree", fuse_plan, one([2, 2, 2]), [[0, 2], [1]])
    raises(INVALID, "restructure_to can move them", fuse_plan, one([2, 2, 2]), [[2], [0, 1]])
    for text, args in (("ambiguous mapping", ([[("a", 2), ("b", 2)], [("c", 2)]], [["a"], ["b", "c"]])),
                       ("connected subtree", (one([2, 2, 2]), [[0, 2], [1]])), ("restructure_to can move them", (one([2, 2, 2]), [[2], [0, 1]]))):
        with pytest.raises(ValueError, match=text):
            rn.fuse_plan(*args)


def test_fuse_limits():
    raises(INVALID, "would hold a fused site dimension above 65535", fuse_plan, one([256, 256]), [[0, 1]])
    assert fuse_plan(one([255, 257]), [[0, 1]])["rounds"] == 1  # 65535 itself passes
    raises(INVALID, "holds 17 legs; a fused site holds at most 16", fuse_plan, one([1] * 17), [list(range(17))])
    assert fuse_plan(one([1] * 16), [list(range(16))])["rounds"] == 15
    # 40000 * 4 * 20000 elements in the result, and an accumulated core inside a group that is larger than the result
    raises(INVALID, "the result core would hold more than INT_MAX elements", fuse_plan, one([2, 2, 2, 2]), [[0], [1, 2], [3]],
           link_dims=[40000, 2, 20000])
    raises(INVALID, "the result core would hold more than INT_MAX elements", fuse_plan, one([2, 2, 2]), [[0, 1, 2]], link_dims=[2, 2 ** 30])
    with pytest.raises(ValueError, match="INT_MAX"):
        rn.fuse_plan(one([2, 2, 2]), [[0, 1, 2]], [2, 2 ** 30])
    assert fuse_plan(one([2, 2, 2, 2]), [[0], [1, 2], [3]], link_dims=[40000, 2, 10000])["rounds"] == 1
    raises(INVALID, "above 65535", restructure_plan, one([256, 256]), [[0, 1]])


def test_split_messages_and_options():
    legs = [[("a", 2), ("b", 2)], [("c", 2)]]
    raises(INVALID, "split_to: target node 1 spans multiple current nodes; use restructure_to for mixed regrouping", split_plan, legs,
           [["a"], ["b", "c"]])
    raises(INVALID, "split_to: the target is not in chain order", split_plan, legs, [["c"], ["a"], ["b"]])
    raises(INVALID, "has no site indices and so has no corresponding target node", split_plan, legs + [[]], [["a"], ["b"], ["c"]])
    p = split_plan(legs, [["b"], ["a"], ["c"]])
    assert p == {"legs": [[("b", 2)], [("a", 2)], [("c", 2)]], "n_qr": 1, "launches": 1}
    assert split_plan(legs, [["a"], ["b"], ["c"]])["launches"] == 0
    ref = rn.split_plan(legs, [["b"], ["a"], ["c"]])
    assert (ref["legs"], ref["n_qr"], ref["launches"]) == (p["legs"], 1, 1)
    with pytest.raises(T4aError) as e:
        rmod.SplitOptions(form="qr")._c()
    assert e.value.code == INVALID
    assert rmod.SplitOptions(form="lu")._c()[1][0].value == 1  # refused by the library: NOT_IMPLEMENTED, tests/test_gpu_restructure.py


# ------------------------------------------------------------------------------------------------ launch counts
@pytest.mark.parametrize("sizes", [(1, 1, 1), (2, 2, 2, 2), (1, 2, 3), (5, 1), (3, 1, 3)])
def test_fuse_plan_launches_are_the_largest_group_minus_one(sizes):
    n = sum(sizes)
    legs = one([2] * n)
    target, at = [], 0
    for s in sizes:
        target.append(list(range(at, at + s)))
        at += s
    p = fuse_plan(legs, target)
    assert p["rounds"] == p["launches"] == max(sizes) - 1
    # a group of one site in another order: one reorder launch more, however many such groups there are
    legs2 = [[((i, 0), 2), ((i, 1), 3)] for i in range(n)]
    t2 = [[((i, q)) for i in g for q in ((1, 0) if len(g) == 1 else (0, 1))] for g in target]
    p2 = fuse_plan(legs2, t2)
    assert p2["launches"] == max(sizes) - 1 + (1 if 1 in sizes else 0)
    assert rn.fuse_plan(legs2, t2)["launches"] == p2["launches"]


# ------------------------------------------------------------------------------------------------ the restatement against dense
def test_restated_fuse_equals_the_reshaped_dense_tensor_exactly_on_integers():
    rng = np.random.default_rng(0)
    legs = [[("a", 2)], [("b", 3), ("c", 2)], [], [("d", 2)], [("e", 3)]]
    cores = rn.int_train(rng, legs, [3, 4, 4, 2])
    target = [["c", "a", "b"], ["e", "d"]]
    out, ol = rn.fuse(cores, legs, target)
    assert [k for s in ol for k, _ in s] == ["c", "a", "b", "e", "d"]
    exact = sn.permuted(sn.to_dense(cores, legs), sn.keys_of(legs), sn.keys_of(ol))
    assert np.array_equal(sn.to_dense(out, ol), exact)
    assert [c.shape for c in out] == [(1, 12, 4), (4, 6, 1)]


@pytest.mark.parametrize("name", sorted(rn.split_cases()))
def test_restated_split_deviation_is_the_recorded_constant(name):
    legs, bonds, target = rn.split_cases()[name]
    worst = 0.0
    for seed in range(20):
        cores = sn.random_train(np.random.default_rng(seed), legs, bonds)
        dense = sn.to_dense(cores, legs)
        out, ol, info = rn.split(cores, legs, target)
        assert [[k for k, _ in s] for s in ol] == [list(g) for g in target]
        # bonds equal min(rows, cols) of every unfolding on generic inputs
        assert all(k == min(rows, cols) for rows, cols, k in info["qr_shapes"])
        assert [out[f].shape[2] for f in info["fragments"]] == [k for _, _, k in info["qr_shapes"]]
        exact = sn.permuted(dense, sn.keys_of(legs), sn.keys_of(ol))
        worst = max(worst, np.linalg.norm(sn.to_dense(out, ol) - exact) / (info["n_qr"] * rn.EPS * np.linalg.norm(dense)))
    assert worst <= rn.SPLIT_RESTATEMENT_DEVIATION
    assert rn.C_SPLIT == 8.0 * rn.SPLIT_RESTATEMENT_DEVIATION


@pytest.mark.parametrize("name", sorted(rn.restructure_cases()))
def test_restated_restructure_equals_the_regrouped_dense_tensor(name):
    legs, bonds, target, kind = rn.restructure_cases()[name]
    cores = sn.random_train(np.random.default_rng(0), legs, bonds)
    dense = sn.to_dense(cores, legs)
    out, ol, info = rn.restructure(cores, legs, target)
    assert info["kind"] == kind
    assert [[k for k, _ in s] for s in ol] == [list(g) for g in target]
    exact = sn.permuted(dense, sn.keys_of(legs), sn.keys_of(ol))
    tol = (sn.C_DENSE * info["n_steps"] + rn.C_SPLIT * info["n_qr"] + 8) * rn.EPS * np.linalg.norm(dense)
    assert np.linalg.norm(sn.to_dense(out, ol) - exact) <= tol


def test_exports():
    for name in ("fuse_to", "split_to", "restructure_to", "restructure_plan", "SplitOptions", "RestructureOptions", "fuse_round",
                 "fuse_quantics", "unfuse_quantics"):
        assert hasattr(t4a_amd, name), name
    o = t4a_amd.RestructureOptions()
    assert isinstance(o.split, t4a_amd.SplitOptions) and isinstance(o.swap, t4a_amd.SwapOptions) and o.final_truncation is None
    assert (o.split.form, o.split.policy, o.split.max_bond_dim, o.split.final_sweep) == ("unitary", None, None, False)
    assert all(itertools.starmap(lambda a, b: a == b, zip(rmod.KINDS, rn.KINDS)))
