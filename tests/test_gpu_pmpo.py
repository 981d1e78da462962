"""Partitioned MPOs on the device with random operands (seeds fixed): compressed Naive and zip-up contraction, add with truncation,
proj_contract, project and norm against the numpy restatement tests/pmpo_np.py, and the refusals through the C ABI.

Bookkeeping — task lists, result projectors, patch counts and bonds — must equal the restatement's exactly.  Values are compared
through the exact dense product: the device's error may exceed the restatement's error on the same case by 1e-10 * max(1, |exact|max),
the margin tests/test_gpu_mpo.py (`close`, rel = 1e-10) allows between the device and its restatement.  The spectra have a gap at every
cut: with tolerance 1e-12 the only values cut are the exact rank deficiencies of the products (zero against order one), and a cap cuts
between two generic, well separated singular values, so the restatement itself keeps every case inside that bound."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, T4aError, ContractionAlgorithm, ContractionOptions, FactorizeMethod
from t4a_amd import partitioned as pt
from t4a_amd.partitioned import PartitionedMPO, Projector, proj_contract

import pmpo_np as P

pytestmark = pytest.mark.gpu

MARGIN = 1e-10  # tests/test_gpu_mpo.py: close(..., rel=1e-10)


def operands(n, ys, xs, zs, seed, hi=3):
    sda, sdb = P.SD3 if n == 3 else P.SD4
    pa, pb = P.split_projectors(sda, sdb, ys, xs, zs)
    rng = np.random.default_rng(seed)

    def make(sd):
        bonds = P.random_bonds(rng, n, 2, hi)
        return [rng.uniform(-1, 1, size=(bonds[i], sd[i][0], sd[i][1], bonds[i + 1])) for i in range(n)]
    return sda, sdb, pa, [make(sda) for _ in pa], pb, [make(sdb) for _ in pb]


def device(ts_list, projectors):
    return PartitionedMPO([MPO(t) for t in ts_list], projectors)


def masked_dense(ts_list, projectors):
    return P.full_sum([P.mask(t, p) for t, p in zip(ts_list, projectors)])


def check(got, want_p, want_t, exact_dense, what):
    """bookkeeping equal, the device's error within the restatement's error plus the margin"""
    assert [p.as_dict() for p in got.projectors()] == want_p, what
    assert got.link_dims() == [[t.shape[0] for t in w[1:]] for w in want_t], what
    scale = max(1.0, float(np.abs(exact_dense).max()))
    err_dev = float(np.abs(got.full_tensor() - exact_dense).max())
    err_np = float(np.abs(P.full_sum(want_t, exact_dense.shape) - exact_dense).max())
    print(f"{what}: device error {err_dev:.3e}, restatement error {err_np:.3e}, bound {err_np + MARGIN * scale:.3e}, "
          f"ratio {err_dev / (err_np + MARGIN * scale):.3e}")
    assert err_dev <= err_np + MARGIN * scale, what


CASES = [(3, 0, 1, 2), (3, 1, 0, 0), (4, 3, 1, 1), (4, 2, 0, 3)]
OPTIONS = [(1e-12, None), (1e-12, 3), (1e-8, 4)]


@pytest.mark.parametrize("tol, cap", OPTIONS)
@pytest.mark.parametrize("n, ys, xs, zs", CASES)
@pytest.mark.parametrize("zip_up", [False, True])
def test_compressed_contraction(zip_up, n, ys, xs, zs, tol, cap):
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=100 + 10 * n + ys)
    alg = ContractionAlgorithm.ZipUp if zip_up else ContractionAlgorithm.Naive
    r = device(ta, pa).contract(device(tb, pb), alg, True, ContractionOptions(tolerance=tol, max_bond_dim=cap))
    want_p, want_t = P.contract(pa, ta, pb, tb, zip_up=zip_up, do_compress=True, tol=tol, cap=cap)
    exact_dense = P.dense_product(masked_dense(ta, pa), masked_dense(tb, pb))
    check(r, want_p, want_t, exact_dense, f"contract zip_up={zip_up} n={n} ys={ys} tol={tol} cap={cap}")
    if cap is not None:
        assert max(max(ld) for ld in r.link_dims()) <= cap
    tasks, results = pt.contract_plan(pa, pb)
    assert (tasks, [p.as_dict() for p in results]) == P.contraction_tasks(pa, pb) and len(r) == len(results)
    assert pt.contract(device(ta, pa), device(tb, pb), alg, tolerance=tol, max_bond_dim=cap).link_dims() == r.link_dims()


@pytest.mark.parametrize("tol, cap", OPTIONS[:2])
@pytest.mark.parametrize("n, ys, xs, zs", CASES[1:3])
def test_add_with_truncation(n, ys, xs, zs, tol, cap):
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=200 + n)
    rng = np.random.default_rng(201)
    qa = [pa[2], pa[0]]
    ua = []
    for k in (2, 0):  # a low-rank partner: the patch itself scaled plus a bond-1 term, so the sum has rank bond + 1
        one = [rng.uniform(-1, 1, size=(1, sda[i][0], sda[i][1], 1)) for i in range(n)]
        ua.append(P.direct_sum([t * (0.5 if i == 0 else 1.0) for i, t in enumerate(ta[k])], one))
    s = device(ta, pa).add(device(ua, qa), tolerance=tol, max_bond_dim=cap)
    want_p, want_t = P.add(pa, ta, qa, ua, tol=tol, cap=cap)
    exact_dense = P.full_sum(ta) + P.full_sum(ua)
    if cap is None:
        assert [t.shape[0] for t in want_t[0][1:]] == [t.shape[0] + 1 for t in ta[0][1:]]  # the gap: twice the bond + 1 collapses
    check(s, want_p, want_t, exact_dense, f"add n={n} tol={tol} cap={cap}")
    with pytest.raises(T4aError) as e:
        device(ta, pa).add(device(ua[:1], [{(n - 1, 1): 0}]))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    assert e.value.message == "Incompatible projectors: Projectors must be pairwise disjoint for patch-wise addition"


def test_proj_contract_project_and_norm():
    n, ys, xs, zs = 3, 0, 1, 2
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=300)
    a, b = device(ta, pa), device(tb, pb)
    # norm: sqrt of the sum of the squared patch norms; 1e-12 relative covers the few hundred roundings of an element of the
    # norm recursion (bonds <= 3, three sites) with room to spare
    want = np.sqrt(sum(float((P.full(t) ** 2).sum()) for t in ta))
    assert abs(a.norm() - want) <= 1e-12 * want
    assert PartitionedMPO([], [], site_dims=sda).norm() == 0.0
    # project: masking stores zeros and copies everything else, so every site tensor equals the restatement's exactly; the dense
    # values differ by the summation order of evaluate alone
    proj = {(xs, 0): 1, (2, 1): 0}
    got = a.project(proj)
    want_p, want_t = P.project(pa, ta, proj)
    assert [p.as_dict() for p in got.projectors()] == want_p and len(got) == sda[ys][1]
    for k, w in enumerate(want_t):
        for g, ws in zip(got.patch(k).site_tensors(), w):
            assert np.array_equal(g, ws)
    dense = P.full_sum(want_t)
    assert np.abs(got.full_tensor() - dense).max() <= MARGIN * max(1.0, np.abs(dense).max())
    # proj_contract: the result projector names a's s1 legs and b's s2 legs, `shared` the contracted leg
    rp, shared = {(xs, 0): 1, (zs, 1): 0}, {ys: 1}
    qa = {(xs, 0): 1, (ys, 1): 1}
    qb = {(zs, 1): 0, (ys, 0): 1}
    ap, at = P.project(pa, ta, qa)
    bp, bt = P.project(pb, tb, qb)
    want_p, want_t = P.contract(ap, at, bp, bt, do_compress=True, tol=1e-12)
    got = proj_contract(a, b, rp, shared=shared, tolerance=1e-12)
    assert len(ap) == 1 and len(bp) == 1 and len(got) == 1 and got.projector(0) == Projector(rp)
    fa, fb = P.full_sum(at), P.full_sum(bt)
    check(got, want_p, want_t, P.dense_product(fa, fb), "proj_contract")
    exact_dense = P.dense_product(masked_dense(ta, pa), masked_dense(tb, pb))
    sel = np.zeros(exact_dense.shape, dtype=bool)
    idx = [slice(None)] * (2 * n)
    idx[2 * xs], idx[2 * zs + 1] = 1, 0
    sel[tuple(idx)] = True
    only_y1 = P.dense_product(P.full_sum(P.project(pa, ta, {(ys, 1): 1})[1]), P.full_sum(P.project(pb, tb, {(ys, 0): 1})[1]))
    assert np.abs(got.full_tensor() - np.where(sel, only_y1, 0.0)).max() <= MARGIN * max(1.0, np.abs(only_y1).max())
    # an operand left without a compatible patch gives an empty result
    assert len(proj_contract(a.project({(xs, 0): 0}), b, {(xs, 0): 1})) == 0


def test_not_implemented_and_refusals_through_the_c_abi():
    sda, sdb, pa, ta, pb, tb = operands(3, 0, 1, 2, seed=400)
    a, b = device(ta, pa), device(tb, pb)
    with pytest.raises(T4aError) as e:
        a.contract(b, ContractionAlgorithm.Fit)
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED and "variational MPO fitting is not implemented" in e.value.message
    for alg in (ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp):
        with pytest.raises(T4aError) as e:
            a.contract(b, alg, True, ContractionOptions(factorize_method=FactorizeMethod.RSVD))
        assert e.value.code == t4a_amd.NOT_IMPLEMENTED and "RSVD factorization not yet implemented" in e.value.message
    with pytest.raises(T4aError) as e:
        a.contract(a)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    assert e.value.message == "Shared shape mismatch at site 0: MPO A has site_dim_2=3, MPO B has site_dim_1=2"
    short = device([tb[0][:1] + [tb[0][1][:, :, :, :1]]], [{}])
    with pytest.raises(T4aError) as e:
        a.contract(short)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and e.value.message == "MPO length mismatch: expected 3, got 2"
    # construction: the checks of t4a_gpu_pmpo_new with their messages
    cases = [
        (ta[:2], [pa[0], pa[0]], "Projectors overlap: patches 0 and 1 are not disjoint"),
        (ta[:2], [pa[0], {(0, 1): 0}], "Projectors overlap: patches 0 and 1 are not disjoint"),
        ([ta[0], tb[0]], pa[:2], "partitioned MPO: patch 1 has site dims (3, 2) at site 0, the chain has (2, 3)"),
        ([ta[0], short.patch(0).site_tensors()], pa[:2], "partitioned MPO: patch 1 has 2 sites, the chain has 3"),
        (ta[:1], [{(3, 0): 0}], "projector index (site 3, leg 0) is absent from the chain of 3 sites"),
        (ta[:1], [{(1, 1): 2}], "projector coordinate 2 is out of range for index (site 1, leg 1) with dimension 2"),
    ]
    for ts, ps, msg in cases:
        with pytest.raises(T4aError) as e:
            device(ts, ps)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and e.value.message == msg
    # results that overlap without being equal are refused like PartitionedTT::insert refuses them
    with pytest.raises(T4aError) as e:
        device(ta[:2], [{(0, 1): 0}, {(0, 1): 1, (1, 0): 0}]).contract(device(tb[:1], [{}]), compress=False)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    assert e.value.message == "Projectors overlap: results 0 and 1 of the contraction are not disjoint"
    with pytest.raises(T4aError) as e:
        a.patch(len(a))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    with pytest.raises(T4aError) as e:
        a.evaluate([0, 3, 0, 0, 0, 0])
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "Index out of bounds" in e.value.message
