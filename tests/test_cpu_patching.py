"""Host-only checks of adaptive patching (t4a_amd.partitioned) and of the budgeted truncation's plan (t4a_amd.mpo.truncate_many_plan):
the options' defaults and every validation message, the volume and budget arithmetic against the numpy restatement
(tests/patching_np.py), split_candidates, the launch and synchronisation counts of the plan, the restatement itself against dense
arithmetic, and the CPU half of the GPU tests: every exact case of tests/test_gpu_patching_exact.py sits away from its threshold and
its model agrees with the restatement, every random case of tests/test_gpu_patching.py keeps its tail sums away from its budgets.
No device is touched."""
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: see tests/test_cpu_compress_many.py)

import t4a_amd
from t4a_amd import T4aError, INVALID_ARGUMENT
from t4a_amd import mpo as M
from t4a_amd import partitioned as P
from t4a_amd.partitioned import PatchingOptions, PatchSplitStrategy

import patching_np as R
import patching_cases_np as C
import pmpo_np as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD = [(2, 1), (3, 2), (2, 2)]


def refusal(fn, text):
    with pytest.raises(T4aError) as e:
        fn()
    assert e.value.code == INVALID_ARGUMENT and text in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ options
def test_defaults_are_those_of_the_reference():
    o = PatchingOptions()
    assert (o.rtol, o.max_bond_dim, o.patch_order, o.split_strategy) == (1e-12, 100, [], PatchSplitStrategy.ExactParameterGain)
    assert (PatchSplitStrategy.Sequential, PatchSplitStrategy.ExactParameterGain) == (0, 1)
    P.validate_patching_options(o, SD)
    P.validate_patching_options(PatchingOptions(0.0, None, [(2, 1), (0, 0)], PatchSplitStrategy.Sequential), SD)


@pytest.mark.parametrize("options, text", [
    (dict(rtol=-1e-3), "rtol must be finite and non-negative"),
    (dict(rtol=float("nan")), "rtol must be finite and non-negative"),
    (dict(rtol=float("inf")), "rtol must be finite and non-negative"),
    (dict(max_bond_dim=0), "max_bond_dim must be at least 1"),
    (dict(patch_order=[(3, 0)]), "outside the chain"),
    (dict(patch_order=[(0, 2)]), "outside the chain"),
    (dict(split_strategy=2), "unknown patch split strategy"),
])
def test_validation_messages(options, text):
    refusal(lambda: P.validate_patching_options(PatchingOptions(**options), SD), text)


def test_a_zero_dimensional_leg_in_the_order_is_refused():
    refusal(lambda: P.validate_patching_options(PatchingOptions(patch_order=[(1, 1)]), [(2, 1), (3, 0)]),
            "patch_order cannot contain zero-dimensional indices")


def test_volume_is_the_product_of_the_unprojected_leg_dims_and_overflow_is_refused():
    assert P.patch_volume({}, SD) == 2 * 3 * 2 * 2 * 2 == R.volume({}, SD)
    assert P.patch_volume({(1, 0): 2, (2, 1): 0}, SD) == 2 * 2 * 2 == R.volume({(1, 0): 2, (2, 1): 0}, SD)
    big = [(65535, 65535)] * 4
    assert P.patch_volume({}, big[:2]) == 65535 ** 4
    refusal(lambda: P.patch_volume({}, big + [(2, 1)]), "subdomain volume overflowed usize")
    refusal(lambda: P.patch_budgets([2 ** 63, 2 ** 63], [1.0, 1.0], 0.1), "partition volume overflowed usize")


# ------------------------------------------------------------------------------------------------ budgets
@pytest.mark.parametrize("seed", range(6))
def test_budgets_and_drops_equal_the_restatement_bit_for_bit(seed):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 9))
    vols = [int(v) for v in rng.integers(1, 1000, k)]
    n2 = list(rng.random(k) * 10.0 ** rng.integers(-12, 3, k))
    n2[0] = 0.0
    rtol = float(10.0 ** rng.integers(-8, 0))
    want = R.budgets(vols, n2, rtol)
    got = P.patch_budgets(vols, n2, rtol)
    assert np.array_equal(np.array(want[0]), got[0]) and want[1] == got[1] and got[1][0]


def test_budget_edge_cases():
    assert P.patch_budgets([], [], 0.1) is None and P.patch_budgets([0, 0], [1.0, 2.0], 0.1) is None
    b, drop = P.patch_budgets([1, 3], [0.0, 5.0], 0.0)  # rtol = 0 drops exactly the zero patches
    assert list(b) == [0.0, 0.0] and drop == [True, False]
    refusal(lambda: P.patch_budgets([1, 1], [1e308, 1e308], 0.1), "partitioned norm is not finite")
    refusal(lambda: P.patch_budgets([1], [1e300], 1e10), "rtol produced a non-finite truncation budget")
    refusal(lambda: P.patch_budgets([1], [1.0], -1.0), "rtol must be finite and non-negative")


def test_the_doc_example_of_truncate_adaptive_keeps_one_patch():
    sd, patches, projs = C.doc_truncate_example()
    kept = R.truncate_adaptive(patches, projs, sd, 0.01, 4)
    assert [p for p, _, _ in kept] == [{(0, 0): 0}]
    n2 = [R.norm2(R.project(t, p)) for t, p in zip(patches, projs)]
    b, drop = P.patch_budgets([R.volume(p, sd) for p in projs], n2, 0.01)
    assert drop == [False, True] and kept[0][2] == b[0]


# ------------------------------------------------------------------------------------------------ split candidates
def test_split_candidates_with_an_empty_and_with_a_given_order():
    assert P.split_candidates({}, SD, PatchingOptions()) == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)] == R.split_candidates({}, SD, ())
    assert P.split_candidates({(1, 0): 1, (2, 1): 0}, SD, PatchingOptions()) == [(0, 0), (1, 1), (2, 0)]
    order = [(2, 1), (0, 0), (2, 1), (1, 0), (0, 1)]  # a duplicate, a projected leg, a leg of dimension 1 named on purpose
    got = P.split_candidates({(1, 0): 0}, SD, PatchingOptions(patch_order=order))
    assert got == [(2, 1), (0, 0), (0, 1)] == R.split_candidates({(1, 0): 0}, SD, order)
    assert P.split_candidates({(0, 0): 0}, SD, PatchingOptions(patch_order=[(0, 0)])) == []


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_counts_three_launches_per_bond_and_one_or_two_synchronisations():
    def chain(sds, bonds):
        return [(bonds[i], a, b, bonds[i + 1]) for i, (a, b) in enumerate(sds)]
    items = [chain([C.E8] * 4, [1, 64, 64, 64, 1]), chain([C.E9] * 4, [1, 65, 65, 65, 1]), chain([C.T2] * 4, [1, 100, 100, 100, 1])]
    p = M.truncate_many_plan(items, [None, None, 3], "batched")
    assert p["routes"] == ["batched", "serial", "batched"] and (p["launches"], p["syncs"], p["n_batched"]) == (9, 1, 2)
    assert p["qr_bonds"][2] == [1, 2, 4, 8, 1] and p["bonds"][2] == [1, 2, 3, 2, 1] and p["bonds"][0] == [1, 64, 64, 64, 1]
    assert M.truncate_many_plan(items, None, "batched", rules_from_norms=True)["syncs"] == 2
    p = M.truncate_many_plan(items, None, "serial")
    assert p["routes"] == ["serial"] * 3 and (p["launches"], p["syncs"]) == (0, 0)
    # auto follows compress_many until measured otherwise: batched up to bond 16 or from 16 items up
    assert M.truncate_many_plan(items[:1], None, "auto")["routes"] == ["serial"]
    assert M.truncate_many_plan(items[2:], None, "auto")["routes"] == ["batched"]
    assert M.truncate_many_plan(items[:1] * 16, None, "auto")["n_batched"] == 16
    refusal(lambda: M.truncate_many_plan([], None), "truncate_many: the list is empty")
    refusal(lambda: M.truncate_many_plan([items[0], items[0][:3]], None), "truncate_many: item 1 has 3 sites, item 0 has 4")
    refusal(lambda: M.truncate_many_plan(items, [1, 0, 1]), "max_bond_dim must be at least 1")


def test_the_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "t4a_gpu.h")) as f:
        header = f.read()
    for name in ("mpo_truncate_many", "mpo_truncate_many_counted", "mpo_truncate_many_plan", "mpo_truncate_many_trace",
                 "pmpo_validate_patching_options", "pmpo_patch_volume", "pmpo_patch_budgets", "pmpo_split_candidates",
                 "pmpo_truncate_adaptive", "pmpo_add_with_patching", "pmpo_contract_adaptive", "pmpo_budget_squared"):
        assert re.search(r"\bt4a_gpu_%s\(" % name, header), name
        assert hasattr(t4a_amd._lib, "t4a_gpu_" + name), name


# ------------------------------------------------------------------------------------------------ the restatement against dense arithmetic
@pytest.mark.parametrize("policy", [(1e-3,) + smr for smr in C.POLICIES])
def test_restated_rank_rule_equals_the_library_on_random_values(policy):
    rng = np.random.default_rng(7)
    for _ in range(20):
        s = np.sort(rng.random(int(rng.integers(1, 12))) * 10.0 ** rng.integers(-6, 1))[::-1]
        assert R.svd_retained_rank(s, policy) == t4a_amd.svd_retained_rank(s, t4a_amd.SvdTruncationPolicy(*policy))
    assert R.svd_retained_rank(np.zeros(4), policy) == 1 == t4a_amd.svd_retained_rank(np.zeros(4), t4a_amd.SvdTruncationPolicy(*policy))


@pytest.mark.parametrize("name", [c[0] for c in C.ADAPTIVE if c[8] is None])
@pytest.mark.parametrize("rtol", [1e-2, 1e-5, 0.0])
def test_restated_truncate_adaptive_stays_within_the_derived_bound(name, rtol):
    sd, patches, projs, _, _ = C.adaptive_case(name)
    assert np.prod([a * b for a, b in sd]) <= 1296
    F = sum(R.dense(R.project(t, p)) for t, p in zip(patches, projs))
    kept = R.truncate_adaptive(patches, projs, sd, rtol, None)
    err = np.linalg.norm(R.dense_sum(kept, sd) - F)
    assert err <= C.error_bound(len(sd), rtol, np.linalg.norm(F)), (err, C.error_bound(len(sd), rtol, np.linalg.norm(F)))


def test_restated_double_truncation_visits_every_bond_twice():
    sd, patches, _, _, _ = C.adaptive_case("train5_drop")
    log = []
    R.truncate_chain(patches[0], R.budget_policy(1e-6), None, log)
    assert len(log) == 2 * (len(sd) - 1)


# ------------------------------------------------------------------------------------------------ the CPU half of the GPU tests
@pytest.mark.parametrize("smr", C.POLICIES)
@pytest.mark.parametrize("n", [2, 3])
def test_exact_cases_sit_away_from_their_thresholds_and_the_model_is_the_restatement(n, smr):
    for name, tensors, values, policy, cap in C.exact_batch(n, smr):
        norm2, steps = C.model(values, n, policy, cap)
        assert norm2 == R.norm2(tensors), name  # exact in any order
        assert min(s[2] for s in steps) > 0.05, (name, [s[2] for s in steps])
        log = []
        R.truncate_chain(tensors, policy, cap, log)
        assert [s[1] for s in steps] == [s[1] for s in log], name
        for (want, _, _), (got, _, _) in zip(steps, log):
            assert np.allclose(got[:len(want)], want, rtol=1e-12, atol=1e-300) and np.all(got[len(want):] < 1e-12), name  # (LAPACK leaves n eps |A| where the model has zeros)


@pytest.mark.parametrize("name", [c[0] for c in C.ADAPTIVE])
def test_random_cases_keep_every_tail_sum_away_from_its_budget(name):
    sd, patches, projs, rtol, cap = C.adaptive_case(name)
    log = []
    R.truncate_adaptive(patches, projs, sd, rtol, cap, log)
    assert log and min(s[2] for s in log) > 1e-8


@pytest.mark.parametrize("name", [c[0] for c in C.SPLIT])
def test_split_cases_keep_their_margins_and_their_parameter_counts_decide(name):
    sd, t, rtol, cap, order = C.split_case(name)
    for strategy in (R.SEQUENTIAL, R.EXACT_PARAMETER_GAIN):
        log, counts = [], []
        R.add_with_patching([t], [{}], sd, rtol, cap, order, strategy, log, None, counts)
        assert min(s[2] for s in log) > 1e-8
        for decision in counts:
            best = sorted(c for _, c in decision)
            if name == "mpo3":
                continue
            assert len(best) == 1 or best[0] < best[1], decision  # the candidates' counts differ where it matters
    if name == "mpo3":  # ... and this one pins the other rule: a tie keeps the first candidate
        assert any(sorted(c for _, c in d)[0] == sorted(c for _, c in d)[1] for d in counts)


# ------------------------------------------------------------------------------------------------ contract_adaptive, restated
def test_restated_doc_example_of_contract_adaptive_gives_one_patch():
    sda, sdb, a, b = C.doc_contract_example()
    got = R.contract_adaptive([{}], [a], [{}], [b], sda, sdb, rtol=0.0, cap=1, patch_order=[(0, 0)], strategy=R.SEQUENTIAL)
    assert len(got) == 1 and R.max_bond(got[0][1]) <= 1


@pytest.mark.parametrize("strategy", [R.SEQUENTIAL, R.EXACT_PARAMETER_GAIN])
@pytest.mark.parametrize("seed", [0, 1])
def test_restated_saturated_group_splits_twice_and_keeps_its_margins(seed, strategy):
    sda, sdb, a, b, rtol, cap, order = C.saturating_product(seed)
    log, chosen = [], []
    got = R.contract_adaptive([{}], [a], [{}], [b], sda, sdb, rtol=rtol, cap=cap, patch_order=order, strategy=strategy, log=log, chosen=chosen)
    assert chosen == [(0, 0), (0, 1), (0, 1)] and len(got) == 4 and all(R.max_bond(t) == 1 for _, t, _ in got)
    assert min(s[2] for s in log) > 1e-8  # the 64 eps cuts after a projection and the budget cuts are all away from their thresholds
    F = PM.dense_product(R.dense(a), R.dense(b))
    assert np.linalg.norm(R.dense_sum(got, [(2, 2)] * 3) - F) <= C.error_bound(3, rtol, np.linalg.norm(F))
    # the products themselves are cut by the rule of mpo.contract at 1e-12: their spectra have a gap of ten orders there
    for proj_a in ({}, {(0, 0): 0}, {(0, 0): 1}):
        d = R.dense([PM.site_product(u, v) for u, v in zip(PM.mask(a, proj_a), b)])
        for cut in (4, 16):  # the unfoldings at the two bonds
            s = np.linalg.svd(d.reshape((cut, -1), order="F"), compute_uv=False)
            assert all(v > 1e-6 * s[0] or v < 1e-14 * s[0] for v in s), (proj_a, cut, s)
