"""Adaptive patching on the device (t4a_amd.partitioned.truncate_adaptive, add_with_patching, contract_adaptive) against the numpy restatement of
patching.rs (tests/patching_np.py) and against dense arithmetic, on the random operands of tests/patching_cases_np.py: chains of 3 to
6 sites, leg dims 2 and 3, bonds up to 17, MPO patches and train patches (s2 = 1).

tests/test_cpu_patching.py checks for every case used here that no quantity the rank rule compares lies within a relative 1e-8 of its
budget in the restatement, so the bonds are pinned and nothing is skipped.  The dense bound is the one derived there
(patching_cases_np.error_bound): |F - F~| <= 2 (n - 1) rtol |F| + 1e-13 |F| without a cap.  With a cap the device is held to the
restatement's own error: both make the same sequence of best rank-k cuts, and the cut values are simple."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, T4aError, INVALID_ARGUMENT
from t4a_amd import partitioned as P
from t4a_amd.partitioned import PartitionedMPO, PatchingOptions, PatchSplitStrategy

import patching_np as R
import patching_cases_np as C
import pmpo_np as PM

pytestmark = pytest.mark.gpu


def pmpo(patches, projs, sd=None):
    return PartitionedMPO([MPO(t) for t in patches], projs, sd)


def projectors(p):
    return [dict(q.items()) for q in p.projectors()]


def exact_sum(patches, projs):
    return sum(R.dense(R.project(t, p)) for t, p in zip(patches, projs))


@pytest.fixture(scope="module")
def references():
    """the restatement of every case, computed once"""
    out = {}
    for name, *_ in C.ADAPTIVE:
        sd, patches, projs, rtol, cap = C.adaptive_case(name)
        out[name] = R.truncate_adaptive(patches, projs, sd, rtol, cap)
    return out


@pytest.mark.parametrize("route", ["batched", "serial"])
@pytest.mark.parametrize("name", [c[0] for c in C.ADAPTIVE])
def test_truncate_adaptive_against_the_restatement_and_the_dense_bound(name, route, references):
    sd, patches, projs, rtol, cap = C.adaptive_case(name)
    want = references[name]
    got, counts = P._truncate_adaptive(pmpo(patches, projs), rtol, cap, route)
    assert projectors(got) == [p for p, _, _ in want]
    assert got.link_dims() == [R.link_dims(t) for _, t, _ in want]
    for k, (_, _, budget) in enumerate(want):
        assert abs(got.budget_squared(k) - budget) <= 1e-12 * budget
    F = exact_sum(patches, projs)
    err = np.linalg.norm(got.full_tensor() - F)
    err_np = np.linalg.norm(R.dense_sum(want, sd) - F)
    norm = np.linalg.norm(F)
    print(f"{name} {route}: err {err:.3e} restatement {err_np:.3e} bound {C.error_bound(len(sd), rtol, norm):.3e} counts {counts}")
    if cap is None:
        assert err <= C.error_bound(len(sd), rtol, norm)
    else:
        assert err <= err_np * (1.0 + 1e-6) + 1e-10 * norm
    n = len(sd)
    if route == "batched":  # one call: the QR sweep, a read of the norms, both SVD sweeps, a read of the ranks
        assert (counts["truncate_calls"], counts["launches"], counts["syncs"]) == (1, 3 * (n - 1), 2)
    else:
        assert (counts["truncate_calls"], counts["launches"], counts["syncs"]) == (1, 0, 0)


def test_the_doc_example_of_truncate_adaptive():
    sd, patches, projs = C.doc_truncate_example()
    got = P.truncate_adaptive(pmpo(patches, projs), 0.01, 4)
    assert projectors(got) == [{(0, 0): 0}] and got.budget_squared(0) is not None
    assert pmpo(patches, projs).budget_squared(0) is None


def test_rtol_zero_drops_only_the_patches_that_are_exactly_zero():
    sd, patches, projs, _, _ = C.adaptive_case("train6_bond17")
    patches[1] = [np.zeros_like(t) for t in patches[1]]
    got = P.truncate_adaptive(pmpo(patches, projs), 0.0, None, "batched")
    assert projectors(got) == [projs[0], projs[2]]
    assert [got.budget_squared(k) for k in range(2)] == [0.0, 0.0]
    F = exact_sum(patches, projs)
    assert np.linalg.norm(got.full_tensor() - F) <= 1e-13 * np.linalg.norm(F)


def test_empty_input_gives_an_empty_result():
    sd = [C.T2, C.T3]
    assert len(P.truncate_adaptive(PartitionedMPO([], [], sd), 1e-3, 2)) == 0
    assert len(P.add_with_patching(PartitionedMPO([], [], sd), None, PatchingOptions())) == 0


def test_the_doc_example_of_add_with_patching_gives_two_patches_of_bond_one():
    sd, t = C.doc_add_example()
    o = PatchingOptions(1e-12, 1, [(0, 0)], PatchSplitStrategy.Sequential)
    got = P.add_with_patching([MPO(t)], [{}], o)
    assert len(got) == 2 and projectors(got) == [{(0, 0): 0}, {(0, 0): 1}] and max(max(b) for b in got.link_dims()) <= 1
    assert np.linalg.norm(got.full_tensor() - R.dense(t)) <= 1e-11 * np.linalg.norm(R.dense(t))


@pytest.mark.parametrize("route", ["batched", "serial"])
@pytest.mark.parametrize("strategy", [PatchSplitStrategy.Sequential, PatchSplitStrategy.ExactParameterGain])
@pytest.mark.parametrize("name", [c[0] for c in C.SPLIT])
def test_add_with_patching_chooses_the_legs_of_the_restatement(name, strategy, route):
    sd, t, rtol, cap, order = C.split_case(name)
    chosen = []
    want = R.add_with_patching([t], [{}], sd, rtol, cap, order, strategy, chosen=chosen)
    got, counts, legs = P._add_with_patching([MPO(t)], [{}], PatchingOptions(rtol, cap, order, strategy), route)
    assert legs == chosen and counts["splits"] == len(chosen)
    assert projectors(got) == [p for p, _, _ in want]
    assert got.link_dims() == [R.link_dims(x) for _, x, _ in want]
    F = R.dense(t)
    err = np.linalg.norm(got.full_tensor() - F)
    print(f"{name} strategy {strategy} {route}: err {err:.3e} bound {C.error_bound(len(sd), rtol, np.linalg.norm(F)):.3e}")
    assert err <= C.error_bound(len(sd), rtol, np.linalg.norm(F))
    # every leg could be split here, so no patch stays above the cap
    assert max(max(b) for b in got.link_dims()) <= cap
    # all children of all candidates of all over-cap patches of a round go into ONE ranks-only call
    rounds_with_a_split = counts["rounds"] - 1
    assert counts["ranks_only_calls"] == (rounds_with_a_split if strategy == PatchSplitStrategy.ExactParameterGain else 0)
    assert counts["truncate_calls"] == counts["rounds"] + 1


def test_the_loop_ends_when_the_order_is_exhausted():
    sd, t, rtol, cap, _ = C.split_case("train4")
    got, counts, legs = P._add_with_patching([MPO(t)], [{}], PatchingOptions(rtol, 1, [(0, 0)], PatchSplitStrategy.Sequential), "batched")
    want = R.add_with_patching([t], [{}], sd, rtol, 1, [(0, 0)], R.SEQUENTIAL)
    assert legs == [(0, 0)] and projectors(got) == [{(0, 0): 0}, {(0, 0): 1}] == [p for p, _, _ in want]
    # the final truncate_adaptive applies the cap even where no split was left
    assert got.link_dims() == [R.link_dims(x) for _, x, _ in want] and max(max(b) for b in got.link_dims()) == 1


def test_the_doc_example_of_contract_adaptive_gives_one_patch():
    sda, sdb, a, b = C.doc_contract_example()
    o = PatchingOptions(0.0, 1, [(0, 0)], PatchSplitStrategy.Sequential)
    got = P.contract_adaptive(pmpo([a], [{}]), pmpo([b], [{}]), patching_options=o)
    assert len(got) == 1 and max(max(x) for x in got.link_dims()) <= 1
    want = R.contract_adaptive([{}], [a], [{}], [b], sda, sdb, rtol=0.0, cap=1, patch_order=[(0, 0)], strategy=R.SEQUENTIAL)
    assert projectors(got) == [p for p, _, _ in want]
    F = PM.dense_product(R.dense(a), R.dense(b))
    assert np.linalg.norm(got.full_tensor() - F) <= 1e-13 * np.linalg.norm(F)


@pytest.mark.parametrize("route", ["batched", "serial"])
@pytest.mark.parametrize("strategy", [PatchSplitStrategy.Sequential, PatchSplitStrategy.ExactParameterGain])
def test_contract_adaptive_splits_a_saturated_group_as_the_restatement_does(strategy, route):
    sda, sdb, a, b, rtol, cap, order = C.saturating_product()
    want = R.contract_adaptive([{}], [a], [{}], [b], sda, sdb, rtol=rtol, cap=cap, patch_order=order, strategy=strategy)
    got, counts = P._contract_adaptive(pmpo([a], [{}]), pmpo([b], [{}]), 0, None, PatchingOptions(rtol, cap, order, strategy), route)
    assert projectors(got) == [p for p, _, _ in want] and len(got) == 4
    assert got.link_dims() == [R.link_dims(t) for _, t, _ in want] == [[1, 1]] * 4
    F = PM.dense_product(R.dense(a), R.dense(b))
    err = np.linalg.norm(got.full_tensor() - F)
    print(f"saturating product strategy {strategy} {route}: err {err:.3e} bound {C.error_bound(3, rtol, np.linalg.norm(F)):.3e} {counts}")
    assert err <= C.error_bound(3, rtol, np.linalg.norm(F))
    # the root group and its two children split; each split projects ONE operand per value and truncates it at 64 eps: 6 calls, and the
    # final truncate_adaptive is one more
    assert counts["splits"] == 3
    assert counts["truncate_calls"] == 6 + 1
    assert counts["ranks_only_calls"] == (3 if strategy == PatchSplitStrategy.ExactParameterGain else 0)


def test_contract_adaptive_over_several_patches_is_the_restatement():
    sda, sdb, a, b, rtol, cap, order = C.saturating_product(1)
    pa, pb = C.halves(sda, (1, 1)), C.halves(sdb, (2, 1))
    ta, tb = [a, [x * 0.5 for x in a]], [b, [x * 2.0 for x in b]]
    want = R.contract_adaptive(pa, ta, pb, tb, sda, sdb, rtol=rtol, cap=cap, patch_order=order, strategy=R.SEQUENTIAL)
    got = P.contract_adaptive(pmpo(ta, pa), pmpo(tb, pb), patching_options=PatchingOptions(rtol, cap, order, PatchSplitStrategy.Sequential))
    assert projectors(got) == [p for p, _, _ in want]
    assert got.link_dims() == [R.link_dims(t) for _, t, _ in want]
    F = PM.dense_product(exact_sum(ta, pa), exact_sum(tb, pb))
    assert np.linalg.norm(got.full_tensor() - F) <= C.error_bound(3, rtol, np.linalg.norm(F))


def test_contract_adaptive_refusals():
    sda, sdb, a, b, *_ = C.saturating_product()
    x, y = pmpo([a], [{}]), pmpo([b], [{}])
    short = pmpo([b[:1] + [b[2]]], [{}])
    for fn, text in [
        (lambda: P.contract_adaptive(x, y, patching_options=PatchingOptions(rtol=-1.0)), "rtol must be finite and non-negative"),
        (lambda: P.contract_adaptive(x, y, patching_options=PatchingOptions(max_bond_dim=0)), "max_bond_dim must be at least 1"),
        (lambda: P.contract_adaptive(x, y, patching_options=PatchingOptions(patch_order=[(3, 0)])), "outside the chain"),
        (lambda: P.contract_adaptive(x, short), "MPO length mismatch: expected 3, got 2"),
        (lambda: P.contract_adaptive(x, y, algorithm=7), "unknown contraction algorithm"),
    ]:
        with pytest.raises(T4aError) as e:
            fn()
        assert e.value.code == INVALID_ARGUMENT and text in str(e.value), str(e.value)


def test_an_inf_on_the_last_site_names_its_item():
    sd, patches, projs, _, _ = C.adaptive_case("train3")
    bad = [t.copy() for t in patches[1]]
    bad[-1][0, 1, 0, 0] = np.inf
    for route in ("batched", "serial"):
        with pytest.raises(T4aError) as e:
            P.truncate_adaptive(pmpo([patches[0], bad], projs), 1e-3, None, route)
        assert "truncate_many: item 1: SVD computation failed: non-finite input" in str(e.value), (route, str(e.value))


def test_refusals_come_before_the_device_is_touched():
    sd, patches, projs, _, _ = C.adaptive_case("train3")
    p = pmpo(patches, projs)
    for fn, text in [
        (lambda: P.truncate_adaptive(p, -1.0), "rtol must be finite and non-negative"),
        (lambda: P.truncate_adaptive(p, float("nan")), "rtol must be finite and non-negative"),
        (lambda: P.truncate_adaptive(p, 1e-3, 0), "max_bond_dim must be at least 1"),
        (lambda: P.truncate_adaptive(p, 1e-3, 2, "fast"), "unknown compress route"),
        (lambda: P.add_with_patching(p, None, PatchingOptions(max_bond_dim=0)), "max_bond_dim must be at least 1"),
        (lambda: P.add_with_patching(p, None, PatchingOptions(patch_order=[(7, 0)])), "outside the chain"),
        (lambda: P.add_with_patching([MPO(t) for t in patches], [{}, {}], PatchingOptions()), "Projectors overlap"),
    ]:
        with pytest.raises(T4aError) as e:
            fn()
        assert e.value.code == INVALID_ARGUMENT and text in str(e.value), str(e.value)
    bad = [t.copy() for t in patches[0]]
    bad[1][0, 0, 0, 0] = np.inf
    with pytest.raises(T4aError) as e:
        P.truncate_adaptive(pmpo([bad, patches[1]], projs), 1e-3, None, "batched")
    assert "truncate_many: item 0: SVD computation failed: non-finite input" in str(e.value)
