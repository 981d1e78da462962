"""compress_many on the device: the batched site-step kernels (one workgroup per MPO, 2 (n - 1) launches and one host synchronisation
per call) against the numpy restatement tests/pmpo_np.py (``compress``: right QR sweep, left SVD sweep, the rank rule of factorize) and
against the exact dense operator, MPO.compress (the serial stage made public), and the partitioned contraction on the batched route.

The items come from tests/compress_many_np.py; tests/test_cpu_compress_many.py checks that every cut of every item used here has a
gap (kept values >= 1e3 * cutoff, dropped ones <= 1e-3 * cutoff, or a cap between values a factor 1e3 apart), so ranks are pinned.
Per number of sites (2, 3, 5) the batch of 300 — more items than the device has compute units — holds, 27 times each with different
values: a tall, a square and a wide first step, an all-bond-1 item, an all-zero item, an item cut to rank 1, one where the tolerance
binds at one bond and the cap at another, one at the bound of the kernels (64) and one above it (65, the serial stage inside the same
call), and entries of magnitude 1e+120 and 1e-120.  The batch of 11 holds every kind once; the batches of 1 and 3, which cannot hold
them all, are (wide) and (tall, square, wide).
Pinned exactly: link dims, the bits of a repeated call, the bits of an item whatever the batch around it, the bits of the serial route,
the driver's launch and synchronisation counts.  Pinned to the margin the project allows between the device and its restatement for this
stage (1e-10 * max(1, |exact|max): MARGIN of tests/test_gpu_pmpo.py, close(rel=1e-10) of tests/test_gpu_mpo.py): the error against the
exact dense operator, and the left-orthogonality of the sites 0 .. n-2 against what MPO.compress gives on the same item."""
import ctypes

import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, T4aError, ContractionAlgorithm, ContractionOptions
from t4a_amd import mpo as M
from t4a_amd import partitioned as pt
from t4a_amd.mpo import compress_many, compress_many_plan
from t4a_amd.partitioned import PartitionedMPO

import compress_many_np as H
import pmpo_np as P

pytestmark = pytest.mark.gpu

MARGIN = 1e-10


def sites_of(m):
    return m.site_tensors()


def same_bits(x, y):
    return len(x) == len(y) and all(a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(x, y))


def orth_defect(ts):
    """max |U^T U - I| over the sites 0 .. n-2 as (l s1 s2) x r matrices"""
    worst = 0.0
    for t in ts[:-1]:
        u = t.reshape((-1, t.shape[3]), order="F")
        worst = max(worst, float(np.abs(u.T @ u - np.eye(u.shape[1])).max()))
    return worst


@pytest.mark.parametrize("tol, cap", H.OPTIONS)
@pytest.mark.parametrize("size", H.SIZES)
@pytest.mark.parametrize("n", H.LENGTHS)
def test_batched_against_the_restatement_and_the_exact_dense_operator(n, size, tol, cap):
    names, items = H.batch(n, size)
    ref = H.reference(n, size, tol, cap)
    opt = ContractionOptions(tol, cap)
    ops = [MPO(t) for t in items]
    res, counts = M._compress_many(ops, opt, "batched")
    plan = compress_many_plan([H.shapes_of(t) for t in items], opt, "batched")
    # the driver's own counters are the plan's: one synchronisation, launches that do not know the batch size
    assert (counts["launches"], counts["syncs"], counts["n_batched"]) == (plan["launches"], plan["syncs"], plan["n_batched"])
    assert plan["routes"] == ["serial" if name == "bmax_plus_1" else "batched" for name in names]
    assert counts["launches"] == 2 * (n - 1) and counts["syncs"] == 1 and counts["n_serial"] == names.count("bmax_plus_1")
    worst = (0.0, 0.0)
    for k, (name, item, r, (want, dense, err_np)) in enumerate(zip(names, items, res, ref)):
        what = f"n={n} size={size} item {k} ({name}) tol={tol} cap={cap}"
        got = sites_of(r)
        assert r.link_dims() == [t.shape[0] for t in want[1:]], what
        assert r.site_dims() == ops[k].site_dims(), what
        assert all(b <= p for b, p in zip([1] + r.link_dims() + [1], plan["bonds"][k])), what
        scale = max(1.0, float(np.abs(dense).max()))
        err_dev = float(np.abs(P.full(got) - dense).max())
        assert err_dev <= err_np + MARGIN * scale, (what, err_dev, err_np, scale)
        serial = orth_defect(sites_of(ops[k].compress(opt)))
        mine = orth_defect(got)
        assert mine <= serial + MARGIN, (what, mine, serial)
        worst = (max(worst[0], (err_dev - err_np) / scale), max(worst[1], mine - serial))
        if name == "zero":  # ranks all 1, the dense operator exactly zero, the sites 0 .. n-2 isometries (checked above)
            assert r.link_dims() == [1] * (n - 1) and not P.full(got).any(), what
        if k < 11 or k == size - 1:
            assert same_bits(sites_of(ops[k]), items[k]), what + ": the operand changed"
    print(f"n={n} size={size} tol={tol} cap={cap}: error above the restatement's / scale {worst[0]:.3e}, orthogonality defect above the "
          f"serial route's {worst[1]:.3e} (bound {MARGIN:.0e} each)")


@pytest.mark.parametrize("n", H.LENGTHS)
def test_same_bits_twice_and_whatever_the_batch_around_an_item(n):
    tol, cap = H.OPTIONS[1]
    opt = ContractionOptions(tol, cap)
    names, items = H.batch(n, 300)
    ops = [MPO(t) for t in items]
    first = [sites_of(r) for r in compress_many(ops, opt, "batched")]
    again = [sites_of(r) for r in compress_many(ops, opt, "batched")]
    assert all(same_bits(a, b) for a, b in zip(first, again))
    # items 0 .. 10 (one of every kind): alone, at the front (above), in the middle and at the end of the 300
    middle = compress_many(ops[150:] + ops[:150], opt, "batched")
    end = compress_many(ops[11:] + ops[:11], opt, "batched")
    for j in range(11):
        alone = sites_of(compress_many([ops[j]], opt, "batched")[0])
        assert same_bits(alone, first[j]), (n, j, names[j], "alone / front")
        assert same_bits(alone, sites_of(middle[150 + j])), (n, j, names[j], "alone / middle")
        assert same_bits(alone, sites_of(end[289 + j])), (n, j, names[j], "alone / end")
    assert same_bits(sites_of(end[299]), first[10])


@pytest.mark.parametrize("n", H.LENGTHS)
def test_the_serial_route_gives_the_bits_of_mpo_compress(n):
    names, items = H.batch(n, 300)
    for tol, cap in H.OPTIONS:
        opt = ContractionOptions(tol, cap)
        ops = [MPO(t) for t in items[:11]]
        res, counts = M._compress_many(ops, opt, "serial")
        assert counts == {"launches": 0, "syncs": 0, "n_batched": 0, "n_serial": 11}
        for k, (op, r) in enumerate(zip(ops, res)):
            assert same_bits(sites_of(r), sites_of(op.compress(opt))), (n, k, names[k])
    # auto: the kernels for items whose bonds stay at or below 16, the serial stage for fewer than 16 items with a larger bond
    assert names[0] == "tall" and names[7] == "bmax"
    assert M._compress_many(ops[:1], opt, "auto")[1]["n_batched"] == 1
    assert M._compress_many(ops[7:8], opt, "auto")[1] == {"launches": 0, "syncs": 0, "n_batched": 0, "n_serial": 1}
    assert M._compress_many([ops[7]] * 16, opt, "auto")[1]["n_batched"] == 16


def test_mpo_compress_against_the_restatement_and_short_chains():
    for n in H.LENGTHS:
        names, items = H.batch(n, 300)
        for tol, cap in H.OPTIONS:
            for k in range(11):
                want = P.compress(items[k], tol, cap)
                dense = P.full(items[k])
                op = MPO(items[k])
                r = op.compress(ContractionOptions(tol, cap))
                assert r.link_dims() == [t.shape[0] for t in want[1:]], (n, k, names[k])
                scale = max(1.0, float(np.abs(dense).max()))
                assert float(np.abs(P.full(sites_of(r)) - dense).max()) <= float(np.abs(P.full(want) - dense).max()) + MARGIN * scale
                assert same_bits(sites_of(op), items[k])
    # fewer than two sites: a copy, on every route
    one = [np.arange(6.0).reshape((1, 2, 3, 1), order="F")]
    assert same_bits(sites_of(MPO(one).compress()), one)
    for route in ("auto", "batched", "serial"):
        res = compress_many([MPO(one), MPO([2 * one[0]])], route=route)
        assert same_bits(sites_of(res[0]), one) and same_bits(sites_of(res[1]), [2 * one[0]])
    assert len(MPO([]).compress()) == 0


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_item_is_named_and_nothing_is_returned(value):
    names, items = H.batch(3, 300)
    five = [[t.copy() for t in item] for item in items[:5]]
    five[2][1][0, 1, 0, 1] = value
    five[4][0][0, 0, 0, 0] = value
    ops = [MPO(t) for t in five]
    with pytest.raises(T4aError) as e:
        compress_many(ops, ContractionOptions(1e-8, None), "batched")
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    assert e.value.message == "compress_many: item 2: SVD computation failed: non-finite input"
    # no outputs: through the C ABI every handle stays null
    arr = (ctypes.c_void_p * 5)(*[m._h for m in ops])
    out = (ctypes.c_void_p * 5)(*[ctypes.c_void_p(1)] * 5)
    status = t4a_amd._lib.t4a_gpu_mpo_compress_many(arr, ctypes.c_size_t(5), ctypes.c_double(1e-8), ctypes.c_size_t(0), ctypes.c_int32(1), out)
    assert status == t4a_amd.INVALID_ARGUMENT and not any(out[k] for k in range(5))
    # the clean items of the same list still compress
    assert len(compress_many(ops[:2] + ops[3:4], ContractionOptions(1e-8, None), "batched")) == 3


def test_mixed_lengths_are_refused():
    a = MPO(H.batch(2, 1)[1][0])
    b = MPO(H.batch(3, 1)[1][0])
    with pytest.raises(T4aError) as e:
        compress_many([a, a, b], route="batched")
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and e.value.message == "compress_many: item 2 has 3 sites, item 0 has 2"


# ------------------------------------------------------------------------------------------------ the partitioned contraction
def device(ts_list, projectors):
    return PartitionedMPO([MPO(t) for t in ts_list], projectors)


@pytest.mark.parametrize("tol, cap", H.PMPO_OPTIONS)
@pytest.mark.parametrize("n, ys, xs, zs", H.PMPO_CASES)
def test_partitioned_contract_on_the_batched_route(n, ys, xs, zs, tol, cap):
    sda, sdb, pa, ta, pb, tb = H.pmpo_operands(n, ys, xs, zs, cap)
    a, b = device(ta, pa), device(tb, pb)
    opt = ContractionOptions(tolerance=tol, max_bond_dim=cap)
    serial = a.contract(b, ContractionAlgorithm.Naive, True, opt, compress_route="serial")
    batched = a.contract(b, ContractionAlgorithm.Naive, True, opt, compress_route="batched")
    assert [p.as_dict() for p in batched.projectors()] == [p.as_dict() for p in serial.projectors()]
    assert batched.link_dims() == serial.link_dims()
    exact = P.dense_product(P.full_sum([P.mask(t, p) for t, p in zip(ta, pa)]), P.full_sum([P.mask(t, p) for t, p in zip(tb, pb)]))
    scale = max(1.0, float(np.abs(exact).max()))
    worst = 0.0
    for k in range(len(serial)):
        diff = float(np.abs(batched.patch(k).full_tensor() - serial.patch(k).full_tensor()).max())
        worst = max(worst, diff)
        assert diff <= MARGIN * scale, (n, ys, tol, cap, k, diff)
    print(f"n={n} ys={ys} tol={tol} cap={cap}: batched against serial, worst patch difference {worst:.3e} (bound {MARGIN * scale:.3e})")
    # the default call is the serial route, bit for bit; the module-level functions pass the route on
    default = a.contract(b, ContractionAlgorithm.Naive, True, opt)
    for k in range(len(serial)):
        assert same_bits(sites_of(default.patch(k)), sites_of(serial.patch(k)))
    again = pt.contract(a, b, tolerance=tol, max_bond_dim=cap, compress_route="batched")
    for k in range(len(serial)):
        assert same_bits(sites_of(again.patch(k)), sites_of(batched.patch(k)))
    with pytest.raises(T4aError) as e:
        a.contract(b, ContractionAlgorithm.ZipUp, True, opt, compress_route="batched")
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    assert e.value.message == ("contract: the batched compress route needs the naive algorithm (the SVDs of zip-up interleave with its "
                               "products)")


def test_proj_contract_takes_the_route_and_the_timing_hooks_run():
    n, ys, xs, zs = 3, 0, 1, 2
    sda, sdb, pa, ta, pb, tb = H.pmpo_operands(n, ys, xs, zs, None)
    a, b = device(ta, pa), device(tb, pb)
    rp, shared = {(xs, 0): 1, (zs, 1): 0}, {ys: 1}
    s = pt.proj_contract(a, b, rp, shared=shared, tolerance=1e-12)
    g = pt.proj_contract(a, b, rp, shared=shared, tolerance=1e-12, compress_route="batched")
    assert len(s) == len(g) == 1 and g.link_dims() == s.link_dims()
    assert float(np.abs(g.full_tensor() - s.full_tensor()).max()) <= MARGIN * max(1.0, float(np.abs(s.full_tensor()).max()))
    ms = pt._time_compress(a, b, reps=1)
    assert len(ms) == 2 and all(v > 0 for v in ms)
    ms = M._time_compress_many([MPO(t) for t in H.batch(3, 11)[1]], ContractionOptions(1e-8, None), reps=1)
    assert len(ms) == 2 and all(v > 0 for v in ms)
