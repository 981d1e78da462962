"""Host-only checks of the partitioned-MPO layer (t4a_amd.partitioned): the projector algebra of projector.rs on hand-written
cases, the task list of contraction_tasks against the numpy restatement (tests/pmpo_np.py), every INVALID_ARGUMENT message of the
host checks, the restatement itself against dense einsum, and the new symbols in the C ABI.  No device is touched."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import t4a_amd
from t4a_amd import T4aError, INVALID_ARGUMENT
from t4a_amd.partitioned import Projector, contract_plan, _check_patches, _launch_blocks

import pmpo_np as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ projector algebra
def test_projector_from_pairs_keeps_the_last_value_and_orders_the_keys():
    p = Projector([((2, 1), 0), ((0, 0), 1), ((2, 1), 3)])
    assert p.items() == [((0, 0), 1), ((2, 1), 3)]
    assert len(p) == 2 and p.get(2, 1) == 3 and p.get(1, 0) is None
    assert p.is_projected_at(0, 0) and not p.is_projected_at(0, 1)
    assert Projector() == Projector({}) and len(Projector()) == 0
    assert Projector({(0, 0): 1}) == Projector([((0, 0), 1)]) and Projector({(0, 0): 1}) != Projector({(0, 1): 1})
    assert len({Projector({(0, 0): 1}), Projector({(0, 0): 1})}) == 1


def test_a_leg_other_than_0_or_1_is_refused():
    with pytest.raises(T4aError) as e:
        Projector({(3, 2): 0})
    assert e.value.code == INVALID_ARGUMENT and e.value.message == "projector leg 2 at site 3 is neither 0 (s1) nor 1 (s2)"
    with pytest.raises(T4aError):
        Projector({(0, -1): 0})


def test_intersection_and_the_conflict_edge():
    a = Projector({(0, 0): 1, (1, 1): 0})
    b = Projector({(1, 1): 0, (2, 0): 2})
    assert (a & b) == Projector({(0, 0): 1, (1, 1): 0, (2, 0): 2})
    assert a.is_compatible_with(b) and b.is_compatible_with(a)
    c = Projector({(1, 1): 1})
    assert a.intersection(c) is None and not a.is_compatible_with(c)
    # the same site on the other leg is another key: no conflict
    assert a.is_compatible_with({(1, 0): 1})
    assert (a & Projector()) == a and (Projector() & Projector()) == Projector()


def test_common_restriction_keeps_only_agreement():
    a = Projector({(0, 0): 1, (1, 1): 0, (2, 0): 1})
    b = Projector({(0, 0): 1, (1, 1): 1, (3, 0): 0})
    assert (a | b) == Projector({(0, 0): 1})
    assert (a | Projector()) == Projector()
    assert (a | a) == a


def test_subset_edges():
    a = Projector({(0, 0): 1, (1, 1): 0})
    assert a.is_subset_of({(0, 0): 1}) and not Projector({(0, 0): 1}).is_subset_of(a)
    assert a.is_subset_of(a) and a.is_subset_of(Projector()) and not Projector().is_subset_of(a)
    assert not a.is_subset_of({(0, 0): 0})        # same key, other value
    assert not a.is_subset_of({(2, 0): 0})        # a key a does not project
    assert Projector().is_subset_of(Projector())


def test_disjoint_edges():
    assert Projector.are_disjoint([{(0, 0): 0}, {(0, 0): 1}, {(0, 0): 2}])
    assert not Projector.are_disjoint([{(0, 0): 0}, {(1, 0): 1}])           # different keys overlap
    assert not Projector.are_disjoint([{(0, 0): 0}, {(0, 0): 0}])           # equal projectors overlap
    assert not Projector.are_disjoint([{(0, 0): 0}, {}])                    # the empty projector overlaps everything
    assert Projector.are_disjoint([]) and Projector.are_disjoint([{}])
    assert Projector.are_disjoint([{(0, 0): 0, (1, 1): 0}, {(0, 0): 0, (1, 1): 1}, {(0, 0): 1}])


def test_filter_edges():
    a = Projector({(0, 0): 1, (1, 1): 0, (2, 0): 1})
    assert a.filter_indices([(0, 0), (2, 0), (5, 1)]) == Projector({(0, 0): 1, (2, 0): 1})
    assert a.filter_indices([]) == Projector()
    assert a.filter_indices([(1, 0)]) == Projector()  # the other leg of a projected site
    assert a.filter_indices([(1, 1), (1, 1)]) == Projector({(1, 1): 0})


def test_total_order_against_the_restatement():
    ps = [{}, {(0, 0): 0}, {(0, 0): 1}, {(0, 0): 0, (1, 1): 0}, {(0, 0): 0, (1, 0): 1}, {(0, 1): 0}, {(1, 0): 0}, {(0, 0): 0, (1, 1): 1}]
    for p, q in itertools.product(ps, ps):
        assert Projector(p).compare(q) == P.compare(p, q), (p, q)
    # hand-written: a proper prefix first, keys before values
    assert Projector({(0, 0): 0}).compare({(0, 0): 0, (1, 1): 0}) == -1
    assert Projector({(0, 0): 1}).compare({(0, 0): 0, (1, 1): 0}) == 1
    assert Projector({(0, 0): 5}).compare({(0, 1): 0}) == -1
    assert Projector({}).compare({}) == 0 and Projector({}).compare({(0, 0): 0}) == -1


def test_algebra_against_the_restatement_on_random_projectors():
    rng = np.random.default_rng(7)
    ps = []
    for _ in range(40):
        keys = [(int(s), int(l)) for s, l in zip(rng.integers(0, 3, 3), rng.integers(0, 2, 3))][:int(rng.integers(0, 4))]
        ps.append({k: int(rng.integers(0, 2)) for k in keys})
    for p, q in zip(ps[:-1], ps[1:]):
        got = Projector(p).intersection(q)
        want = P.intersection(p, q)
        assert (got is None) == (want is None) and (got is None or got.as_dict() == want)
        assert Projector(p).common_restriction(q).as_dict() == P.common_restriction(p, q)
        assert Projector(p).is_subset_of(q) == P.is_subset_of(p, q)
        assert Projector(p).is_compatible_with(q) == P.compatible(p, q)
    for k in range(0, 36, 4):
        assert Projector.are_disjoint(ps[k:k + 4]) == P.are_disjoint(ps[k:k + 4])


# ------------------------------------------------------------------------------------------------ error messages
def test_projector_validation_messages():
    sd = [(2, 3), (3, 2), (2, 1)]
    assert Projector({(0, 1): 2, (2, 1): 0}).validate(sd) is not None
    with pytest.raises(T4aError) as e:
        Projector({(3, 0): 0}).validate(sd)
    assert e.value.code == INVALID_ARGUMENT and e.value.message == "projector index (site 3, leg 0) is absent from the chain of 3 sites"
    with pytest.raises(T4aError) as e:
        Projector({(1, 1): 2}).validate(sd)
    assert e.value.code == INVALID_ARGUMENT
    assert e.value.message == "projector coordinate 2 is out of range for index (site 1, leg 1) with dimension 2"
    with pytest.raises(T4aError) as e:
        Projector({(2, 1): 1}).validate(sd)
    assert e.value.message == "projector coordinate 1 is out of range for index (site 2, leg 1) with dimension 1"


def test_patch_list_messages():
    sd = [(2, 3), (3, 2)]
    ok = [sd, sd]
    _check_patches(sd, ok, [{(0, 0): 0}, {(0, 0): 1}])
    _check_patches(sd, [], [])
    cases = [
        ((sd, [sd, sd[:1]], [{(0, 0): 0}, {(0, 0): 1}]), "partitioned MPO: patch 1 has 1 sites, the chain has 2"),
        ((sd, [sd, [(2, 3), (2, 3)]], [{(0, 0): 0}, {(0, 0): 1}]),
         "partitioned MPO: patch 1 has site dims (2, 3) at site 1, the chain has (3, 2)"),
        ((sd, ok, [{(2, 0): 0}, {(0, 0): 1}]), "projector index (site 2, leg 0) is absent from the chain of 2 sites"),
        ((sd, ok, [{(0, 0): 0}, {(0, 0): 2}]), "projector coordinate 2 is out of range for index (site 0, leg 0) with dimension 2"),
        ((sd, ok, [{(0, 0): 0}, {(1, 1): 1}]), "Projectors overlap: patches 0 and 1 are not disjoint"),
        ((sd, ok + [sd], [{(0, 0): 0}, {(0, 0): 1}, {(0, 0): 1}]), "Projectors overlap: patches 1 and 2 are not disjoint"),
        ((sd, ok, [{}, {(0, 0): 1}]), "Projectors overlap: patches 0 and 1 are not disjoint"),
    ]
    for args, msg in cases:
        with pytest.raises(T4aError) as e:
            _check_patches(*args)
        assert e.value.code == INVALID_ARGUMENT and e.value.message == msg


def test_plan_capacity_message_and_null_pointers():
    lib = t4a_amd._lib
    e = np.array([0, 1, 0, 0, 0, 0], dtype=np.uintp)
    c = np.array([1], dtype=np.uintp)
    nt, nr, ne = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    buf = np.zeros(8, dtype=np.uintp)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    # A = {(0, 1): 0}, B = {(0, 0): 0}: one task, an empty result projector
    st = lib.t4a_gpu_pmpo_contract_plan(p(e), p(c), ctypes.c_size_t(1), p(e[3:]), p(c), ctypes.c_size_t(1), ctypes.c_size_t(0), ctypes.c_size_t(0),
                                        ctypes.byref(nt), None, None, None, ctypes.byref(nr), None, None, ctypes.byref(ne))
    assert st == 0 and (nt.value, nr.value, ne.value) == (1, 1, 0)
    # A = [{(0, 0): 0}, {(0, 0): 1}], B = [{}]: two tasks with one result entry each do not fit one task slot
    e2 = np.array([0, 0, 0, 0, 0, 1], dtype=np.uintp)
    c2 = np.array([1, 1], dtype=np.uintp)
    c0 = np.array([0], dtype=np.uintp)
    st = lib.t4a_gpu_pmpo_contract_plan(p(e2), p(c2), ctypes.c_size_t(2), p(e2), p(c0), ctypes.c_size_t(1), ctypes.c_size_t(1), ctypes.c_size_t(2),
                                        ctypes.byref(nt), p(buf), p(buf), p(buf), ctypes.byref(nr), p(buf), p(buf), ctypes.byref(ne))
    assert st == INVALID_ARGUMENT and (nt.value, nr.value, ne.value) == (2, 2, 2)
    assert t4a_amd.last_error_message() == "pmpo_contract_plan: 2 tasks and 2 result entries do not fit the capacities 1 and 2"
    st = lib.t4a_gpu_pmpo_contract_plan(p(e), p(c), ctypes.c_size_t(1), p(e), p(c), ctypes.c_size_t(1), ctypes.c_size_t(0), ctypes.c_size_t(0),
                                        None, None, None, None, ctypes.byref(nr), None, None, ctypes.byref(ne))
    assert st == t4a_amd.NULL_POINTER


# ------------------------------------------------------------------------------------------------ the plan
def random_partition(rng, n, legs, depth):
    """disjoint projectors that cover the space: split along `depth` of the given legs, some branches left coarser"""
    out = [{}]
    for key in legs[:depth]:
        nxt = []
        for p in out:
            if p and rng.random() < 0.3:
                nxt.append(p)
                continue
            for v in range(2):
                q = dict(p)
                q[key] = v
                nxt.append(q)
        out = nxt
    return out


def test_contract_plan_against_the_restatement():
    rng = np.random.default_rng(11)
    legs = [(s, l) for s in range(3) for l in range(2)]
    for trial in range(30):
        la = [legs[k] for k in rng.permutation(6)]
        lb = [legs[k] for k in rng.permutation(6)]
        pa = random_partition(rng, 3, la, int(rng.integers(0, 4)))
        pb = random_partition(rng, 3, lb, int(rng.integers(0, 4)))
        assert P.are_disjoint(pa) or len(pa) == 1
        tasks, results = contract_plan(pa, pb)
        want_tasks, want_results = P.contraction_tasks(pa, pb)
        assert tasks == want_tasks, trial
        assert [r.as_dict() for r in results] == want_results, trial


def test_contract_plan_hand_written_cases():
    # the canonical case: A split on a y leg, B split on the same leg: two tasks, one empty result projector
    tasks, results = contract_plan([{(0, 1): 0}, {(0, 1): 1}], [{(0, 0): 0}, {(0, 0): 1}])
    assert tasks == [(0, 0, 0), (1, 1, 0)] and results == [Projector()]
    # external legs: every pair is a task, the result carries A's leg 0 and B's leg 1
    tasks, results = contract_plan([{(0, 0): 0}, {(0, 0): 1}], [{(1, 1): 0}, {(1, 1): 1}])
    assert tasks == [(0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 1, 3)]
    assert results == [Projector({(0, 0): a, (1, 1): b}) for a in range(2) for b in range(2)]
    # A's leg 1 against B's leg 1 is no shared index; only one side projecting the shared leg is compatible
    tasks, results = contract_plan([{(0, 1): 0}], [{(0, 1): 1}, {(0, 0): 1}, {}])
    assert tasks == [(0, 0, 0), (0, 2, 1)] and results == [Projector({(0, 1): 1}), Projector()]
    assert contract_plan([], [{}]) == ([], []) and contract_plan([{}], []) == ([], [])
    assert contract_plan([{}], [{}]) == ([(0, 0, 0)], [Projector()])


# ------------------------------------------------------------------------------------------------ the restatement against einsum
def int_tensors(rng, bonds, sd, lo=-3, hi=4):
    return [rng.integers(lo, hi, size=(bonds[i], sd[i][0], sd[i][1], bonds[i + 1])).astype(np.float64) for i in range(len(sd))]


def test_restatement_contract_equals_the_dense_product():
    rng = np.random.default_rng(3)
    sda, sdb = [(2, 3), (3, 2), (2, 2)], [(3, 2), (2, 4), (2, 3)]
    pa = [{(0, 0): 0}, {(0, 0): 1, (0, 1): 0}, {(0, 0): 1, (0, 1): 1}, {(0, 0): 1, (0, 1): 2}]
    pb = [{(2, 1): 0, (0, 0): 0}, {(2, 1): 0, (0, 0): 1}, {(2, 1): 0, (0, 0): 2}, {(2, 1): 1}, {(2, 1): 2}]
    assert P.are_disjoint(pa) and P.are_disjoint(pb)
    assert len(P.contraction_tasks(pa, pb)[0]) == 14 and len(P.contraction_tasks(pa, pb)[1]) == 6
    ta = [P.mask(int_tensors(rng, [1, 2, 3, 1], sda), p) for p in pa]
    tb = [P.mask(int_tensors(rng, [1, 3, 2, 1], sdb), p) for p in pb]
    want = P.dense_product(P.full_sum(ta), P.full_sum(tb))
    rp, rt = P.contract(pa, ta, pb, tb, do_compress=False)
    assert np.array_equal(P.full_sum(rt), want)
    assert P.are_disjoint(rp)
    for p, t in zip(rp, rt):  # every result patch vanishes outside its projector
        assert np.array_equal(P.full(P.mask(t, p)), P.full(t))
    for kw in (dict(do_compress=True), dict(zip_up=True)):
        _, rt = P.contract(pa, ta, pb, tb, tol=1e-13, **kw)
        assert np.abs(P.full_sum(rt) - want).max() <= 1e-10 * np.abs(want).max()
    # unmasked patches: the projection is applied by contract itself
    raw_a = [int_tensors(rng, [1, 2, 2, 1], sda) for _ in pa]
    raw_b = [int_tensors(rng, [1, 2, 2, 1], sdb) for _ in pb]
    want = P.dense_product(P.full_sum([P.mask(t, p) for t, p in zip(raw_a, pa)]), P.full_sum([P.mask(t, p) for t, p in zip(raw_b, pb)]))
    assert np.array_equal(P.full_sum(P.contract(pa, raw_a, pb, raw_b, do_compress=False)[1]), want)
    # results that overlap without being equal are refused, as PartitionedTT::insert refuses them
    with pytest.raises(ValueError, match="Projectors overlap"):
        P.contract([{(0, 1): 0}, {(0, 1): 1, (1, 0): 0}, {(0, 1): 1, (1, 0): 1}, {(0, 1): 1, (1, 0): 2}], ta, [{}], tb[:1])


def test_restatement_add_to_mpo_project_and_norm():
    rng = np.random.default_rng(5)
    sd = [(2, 2), (3, 1), (2, 2)]
    pa = [{(0, 0): 0}, {(0, 0): 1, (2, 1): 0}, {(0, 0): 1, (2, 1): 1}]
    pb = [{(0, 0): 1, (2, 1): 1}, {(0, 0): 0}]
    ta = [P.mask(int_tensors(rng, [1, 2, 3, 1], sd), p) for p in pa]
    tb = [P.mask(int_tensors(rng, [1, 3, 2, 1], sd), p) for p in pb]
    sp, st = P.add(pa, ta, pb, tb, tol=0.0)
    assert sp == pa and [t[1].shape[0] for t in st] == [5, 2, 5]
    assert np.array_equal(P.full_sum(st), P.full_sum(ta) + P.full_sum(tb))
    _, st = P.add(pa, ta, pb, tb, tol=1e-13)
    assert np.abs(P.full_sum(st) - P.full_sum(ta) - P.full_sum(tb)).max() <= 1e-10 * np.abs(P.full_sum(ta)).max()
    with pytest.raises(ValueError):
        P.add(pa, ta, [{(1, 0): 0}], tb[:1])
    m = P.to_mpo(pa, ta)
    assert [t.shape[0] for t in m[1:]] == [6, 9] and np.array_equal(P.full(m), P.full_sum(ta))
    with pytest.raises(ValueError):
        P.to_mpo([], [])
    qp, qt = P.project(pa, ta, {(2, 1): 1, (1, 0): 2})
    assert qp == [{(0, 0): 0, (1, 0): 2, (2, 1): 1}, {(0, 0): 1, (1, 0): 2, (2, 1): 1}]
    want = P.full_sum(ta).copy()
    want[:, :, :2] = 0
    want[..., 0] = 0
    assert np.array_equal(P.full_sum(qt), want)
    assert P.norm(ta) == pytest.approx(np.sqrt((P.full_sum(ta) ** 2).sum()), rel=1e-14)
    nan = [t.copy() for t in ta[0]]
    nan[0][0, 1, 0, 0] = np.nan
    assert np.isfinite(P.full(P.mask(nan, pa[0]))).all()


# ------------------------------------------------------------------------------------------------ ABI
def test_new_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t4a_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(t4a_gpu_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    names = ["t4a_gpu_projector_" + s for s in ("validate", "is_compatible", "intersection", "common_restriction", "is_subset_of",
                                                "are_disjoint", "filter", "compare")]
    names += ["t4a_gpu_pmpo_" + s for s in ("contract_plan", "check", "new", "from_ptt", "release", "len", "n_sites", "site_dims", "projector",
                                            "patch", "norm", "evaluate", "project", "add", "to_mpo", "to_mpo_route", "contract", "pair_products", "mask_sites",
                                            "launch_blocks", "time_contract")]
    for n in names:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert t4a_amd.PartitionedMPO is t4a_amd.partitioned.PartitionedMPO and t4a_amd.Projector is Projector
    assert hasattr(t4a_amd.PartitionedTT, "as_mpo") and callable(t4a_amd.proj_contract)


def test_launch_shape_is_one_resident_pass():
    assert _launch_blocks(1) == 1 and _launch_blocks(256) == 1 and _launch_blocks(257) == 2
    assert _launch_blocks(2048 * 256) == 2048 and _launch_blocks(2048 * 256 + 1) == 2048 and _launch_blocks(2 ** 40) == 2048
