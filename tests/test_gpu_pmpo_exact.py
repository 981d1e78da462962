"""The launches of the partitioned MPO (kernels_pmpo.hip) and the exact routes of t4a_amd.partitioned on integer-valued operands:
every comparison is `==` against int64 arithmetic or against the bits of the existing MPO kernels.

Site tensors hold integers from [-2, 2]; with bonds <= 17, site dims <= 4 and n <= 4 every product and partial sum stays far below
2^53, so f64 holds them exactly whatever the order of summation.  Shapes: n = 3 and n = 4, site dims mixed per site (pmpo_np.SD3 /
SD4), patch bonds mixed in 1 .. 5, one patch per operand with bonds of 17.  The pair of bond-17 patches gives a site product of
17*17 x (3*4) x 17*17 = 1 002 252 elements: more than the 2048 * 256 threads of one grid pass of the launch."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, T4aError, contract_naive
from t4a_amd import partitioned as pt
from t4a_amd.partitioned import PartitionedMPO, Projector

import pmpo_np as P

pytestmark = pytest.mark.gpu

GRID_PASS = 2048 * 256  # kernels_pmpo.hip: pmpo_launch_blocks


def ints(rng, bonds, sd, lo=-2, hi=3):
    return [rng.integers(lo, hi, size=(bonds[i], sd[i][0], sd[i][1], bonds[i + 1])).astype(np.float64) for i in range(len(sd))]


def exact(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and want.dtype == np.int64, (got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, np.rint(got)), f"{what}: the device returned values that are no integers"
    bad = np.argwhere(got.astype(np.int64) != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} entries differ, first at {tuple(bad[0])}"


def i64(ts):
    return [np.rint(t).astype(np.int64) for t in ts]


def dense_i64(ts_list):
    return P.full_sum([i64(t) for t in ts_list])


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


def operands(n, ys, xs, zs, seed, big=False, integer=True):
    sda, sdb = P.SD3 if n == 3 else P.SD4
    pa, pb = P.split_projectors(sda, sdb, ys, xs, zs)
    rng = np.random.default_rng(seed)

    def make(bonds, sd):
        if integer:
            return ints(rng, bonds, sd)
        return [rng.uniform(-1, 1, size=(bonds[i], sd[i][0], sd[i][1], bonds[i + 1])) for i in range(n)]
    ta = [make(P.random_bonds(rng, n), sda) for _ in pa]
    tb = [make(P.random_bonds(rng, n), sdb) for _ in pb]
    if big:  # the first patch of A and the last of B are compatible with every patch of the other side
        ta[0] = make([1] + [17] * (n - 1) + [1], sda)
        tb[-1] = make([1] + [17] * (n - 1) + [1], sdb)
    return sda, sdb, pa, ta, pb, tb


def device(ts_list, projectors):
    return PartitionedMPO([MPO(t) for t in ts_list], projectors)


CASES = [(3, 0, 1, 2, False), (3, 1, 0, 0, True), (4, 3, 1, 1, False), (4, 2, 0, 3, False)]


# ------------------------------------------------------------------------------------------------ the fused launch through its hook
def ref_job(a, b, k0, k1, sm, tm):
    a, b = np.rint(a).astype(np.int64), np.rint(b).astype(np.int64)
    a[:, :, :k0, :] = 0
    a[:, :, k1:, :] = 0
    if sm >= 0:
        a[:, [s for s in range(a.shape[1]) if s != sm], :, :] = 0
    if tm >= 0:
        b[:, :, [t for t in range(b.shape[2]) if t != tm], :] = 0
    return P.site_product(a, b)


def test_pair_products_every_selector_at_every_position():
    """4 tasks x 3 sites in one launch: the contracted leg as one value (first, inner, last k) or the full range, an s mask alone, a t
    mask alone, both and none, each at the first, an inner and the last site; site outputs from 8 to 1 002 252 elements, so the offset
    search has an interior and the grid-stride loop makes a second trip."""
    rng = np.random.default_rng(1)
    sda, sdb = P.SD3
    bonds_a = [[1, 2, 3, 1], [1, 17, 17, 1], [1, 5, 1, 1], [1, 4, 2, 1]]
    bonds_b = [[1, 3, 2, 1], [1, 17, 17, 1], [1, 1, 4, 1], [1, 2, 5, 1]]
    # (k selector, s mask, t mask) per task and site; k selector: None = full range, else the value
    sel = [[(None, -1, -1), (0, 2, -1), (1, -1, 2)],
           [(2, 1, -1), (None, -1, 3), (0, 0, 1)],
           [(1, -1, 1), (1, 1, 2), (None, 1, -1)],
           [(0, 0, 0), (None, -1, -1), (None, -1, -1)]]
    A, B, dims, sels, want = [], [], [], [], []
    for t in range(4):
        ta, tb = ints(rng, bonds_a[t], sda), ints(rng, bonds_b[t], sdb)
        for i in range(3):
            kv, sm, tm = sel[t][i]
            K = sda[i][1]
            k0, k1 = (0, K) if kv is None else (kv, kv + 1)
            A.append(ta[i])
            B.append(tb[i])
            dims.append([bonds_a[t][i], sda[i][0], K, bonds_a[t][i + 1], bonds_b[t][i], sdb[i][1], bonds_b[t][i + 1]])
            sels.append([k0, k1, sm, tm])
            want.append(ref_job(ta[i], tb[i], k0, k1, sm, tm))
    assert sum(w.size for w in want) > GRID_PASS and pt._launch_blocks(sum(w.size for w in want)) * 256 == GRID_PASS
    got = pt._pair_products(dims, sels, A, B)
    for q, (g, w) in enumerate(zip(got, want)):
        exact(g, w, f"job {q}")
        if sels[q][2] >= 0 or sels[q][3] >= 0:  # masked outputs are +0.0, not -0.0
            assert not np.signbit(g[g == 0]).any()


def test_pair_products_hook_refuses_bad_selectors():
    a, b = np.ones((1, 2, 2, 1)), np.ones((1, 2, 2, 1))
    for sel in ([0, 3, -1, -1], [2, 1, -1, -1], [0, 2, 2, -1], [0, 2, -1, 2]):
        with pytest.raises(T4aError) as e:
            pt._pair_products([[1, 2, 2, 1, 1, 2, 1]], [sel], [a], [b])
        assert e.value.code == t4a_amd.INVALID_ARGUMENT


@pytest.mark.parametrize("n, ys, xs, zs, big", CASES)
def test_fused_products_have_the_bits_of_the_site_kernel_on_masked_operands(n, ys, xs, zs, big):
    """contract(Naive, compress=False) on random f64 operands against mpo.contract_naive(masked a, masked b): the same bits in every
    site of every task (results of one slot are direct sums, which copy)."""
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=20 + n + ys, big=big, integer=False)
    r = device(ta, pa).contract(device(tb, pb), compress=False)
    tasks, results = P.contraction_tasks(pa, pb)
    assert [p.as_dict() for p in r.projectors()] == results
    want = [None] * len(results)
    for i, j, slot in tasks:
        c = contract_naive(MPO(P.mask(ta[i], pa[i])), MPO(P.mask(tb[j], pb[j]))).site_tensors()
        want[slot] = c if want[slot] is None else P.direct_sum(want[slot], c)
    for slot, w in enumerate(want):
        got = r.patch(slot).site_tensors()
        for s in range(n):
            same_bits(got[s], w[s], f"slot {slot} site {s}")


# ------------------------------------------------------------------------------------------------ the mask launch
def test_mask_launch_writes_zeros_outside_and_touches_nothing_inside():
    rng = np.random.default_rng(2)
    shapes = [(1, 2, 3, 4), (4, 3, 2, 17), (17, 2, 2, 5), (5, 4, 1, 3), (3, 2, 4, 1), (1, 3, 3, 1)] + [(5, 3, 4, 5)] * 30
    sel = [(1, -1), (-1, 0), (0, 1), (3, 0), (-1, 3), (-1, -1)] + [(k % 3, (k // 3) % 4) for k in range(30)]
    sites = [rng.uniform(-1, 1, size=s) for s in shapes]
    for x, (m1, m2) in zip(sites, sel):  # non-finite values outside the subdomain
        if m1 >= 0:
            x[:, (m1 + 1) % x.shape[1], 0, :] = np.nan
        if m2 >= 0 and x.shape[2] > 1:
            x[0, :, (m2 + 1) % x.shape[2], -1] = np.inf
    got = pt._mask_sites(sites, sel)
    assert sum(x.size for x in sites) > 4 * 256
    for q, (x, g, (m1, m2)) in enumerate(zip(sites, got, sel)):
        inside = np.ones(x.shape, dtype=bool)
        if m1 >= 0:
            inside[:, [s for s in range(x.shape[1]) if s != m1], :, :] = False
        if m2 >= 0:
            inside[:, :, [s for s in range(x.shape[2]) if s != m2], :] = False
        same_bits(g[inside], x[inside], f"site {q}: inside")
        assert np.array_equal(g[~inside].view(np.uint64), np.zeros(int((~inside).sum()), dtype=np.uint64)), f"site {q}: outside"


@pytest.mark.parametrize("n, ys, xs, zs, big", CASES[:2])
def test_project_drops_masks_and_intersects(n, ys, xs, zs, big):
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=3, big=big)
    ta[0][xs][0, 1, 0, 0] = np.nan  # pa[0] projects (xs, 0) = 0: s1 = 1 is outside its subdomain
    a = device(ta, pa)
    own = a.project({})  # every patch onto its own projector
    assert [p.as_dict() for p in own.projectors()] == pa
    for k in range(len(pa)):
        for s, (g, w) in enumerate(zip(own.patch(k).site_tensors(), P.mask(ta[k], pa[k]))):
            same_bits(g, w, f"patch {k} site {s}")
    proj = {(ys, 1): 0, (n - 1, 0): 1}
    want_p, want_t = P.project(pa, ta, proj)
    got = a.project(proj)
    assert len(got) == len(want_p) < len(pa) and [p.as_dict() for p in got.projectors()] == want_p
    for k in range(len(want_p)):
        for s, (g, w) in enumerate(zip(got.patch(k).site_tensors(), want_t[k])):
            same_bits(g, w, f"patch {k} site {s}")
    assert len(a.project({(xs, 0): 0, (ys, 1): 0})) == 1
    with pytest.raises(T4aError) as e:
        a.project({(n, 0): 0})
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "is absent from the chain" in e.value.message


# ------------------------------------------------------------------------------------------------ contract, exact
@pytest.mark.parametrize("n, ys, xs, zs, big", CASES)
def test_naive_contract_without_compression_is_the_dense_product(n, ys, xs, zs, big):
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=40 + n + ys, big=big)
    a, b = device(ta, pa), device(tb, pb)
    r = a.contract(b, compress=False)
    want_p, want_t = P.contract(pa, ta, pb, tb, do_compress=False)
    tasks, _ = P.contraction_tasks(pa, pb)
    assert len(tasks) < len(pa) * len(pb)  # the pairs that differ on the contracted leg give no task
    assert [p.as_dict() for p in r.projectors()] == want_p
    assert r.link_dims() == [[t.shape[0] for t in w[1:]] for w in want_t]
    assert r.site_dims() == [(sda[i][0], sdb[i][1]) for i in range(n)]
    for k, w in enumerate(want_t):
        for s, (g, ws) in enumerate(zip(r.patch(k).site_tensors(), w)):
            exact(g, np.rint(ws).astype(np.int64), f"patch {k} site {s}")
    fa = dense_i64([P.mask(t, p) for t, p in zip(ta, pa)])
    fb = dense_i64([P.mask(t, p) for t, p in zip(tb, pb)])
    exact(r.full_tensor(), P.dense_product(fa, fb), "patch-wise sum against the dense product")
    # every result patch vanishes outside its projector: projecting it onto itself changes nothing
    same_bits(r.project({}).full_tensor(), r.full_tensor())


def test_incompatible_pair_gives_no_task_and_the_canonical_case_sums_two():
    rng = np.random.default_rng(6)
    sda, sdb = P.SD3
    ta = [ints(rng, [1, 2, 3, 1], sda), ints(rng, [1, 4, 2, 1], sda)]
    tb = [ints(rng, [1, 3, 1, 1], sdb), ints(rng, [1, 2, 5, 1], sdb)]
    none = device(ta[:1], [{(0, 1): 0}]).contract(device(tb[:1], [{(0, 0): 1}]), compress=False)
    assert len(none) == 0 and none.site_dims() == [(2, 2), (3, 4), (2, 3)]
    assert np.array_equal(none.full_tensor(), np.zeros((2, 2, 3, 4, 2, 3)))
    # A split on a y leg into two patches against B split on the same leg: two tasks, one (empty) result projector, summed
    pa, pb = [{(1, 1): 0}, {(1, 1): 1}], [{(1, 0): 0}, {(1, 0): 1}]
    r = device(ta, pa).contract(device(tb, pb), compress=False)
    assert len(r) == 1 and r.projector(0) == Projector() and r.link_dims() == [[2 * 3 + 4 * 2, 3 * 1 + 2 * 5]]
    fa = dense_i64([P.mask(t, p) for t, p in zip(ta, pa)])
    fb = dense_i64([P.mask(t, p) for t, p in zip(tb, pb)])
    exact(r.full_tensor(), P.dense_product(fa, fb))
    # the same operands as plain MPOs: one patch each with the empty projector
    whole = device([P.to_mpo(pa, [P.mask(t, p) for t, p in zip(ta, pa)])], [{}]).contract(
        device([P.to_mpo(pb, [P.mask(t, p) for t, p in zip(tb, pb)])], [{}]), compress=False)
    exact(whole.full_tensor(), P.dense_product(fa, fb))


# ------------------------------------------------------------------------------------------------ to_mpo and add, exact
@pytest.mark.parametrize("n, ys, xs, zs, big", CASES[1:3])
def test_to_mpo_is_the_direct_sum_in_projector_order(n, ys, xs, zs, big):
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=7, big=big)
    order = [2, 0, 1] + list(range(3, len(pa)))  # insertion order differs from the projector order
    a = device([ta[k] for k in order], [pa[k] for k in order])
    m = a.to_mpo()
    want = P.to_mpo(pa, ta)
    assert m.link_dims() == [t.shape[0] for t in want[1:]] == [sum(t[s].shape[0] for t in ta) for s in range(1, n)]
    for s, (g, w) in enumerate(zip(m.site_tensors(), want)):
        exact(g, np.rint(w).astype(np.int64), f"site {s}")
    exact(m.full_tensor(), dense_i64(ta))
    # the chain of pairwise additions and the one launch copy the same values to the same places
    for route in (1, 2):
        for s, (g, w) in enumerate(zip(a._to_mpo_route(route).site_tensors(), m.site_tensors())):
            same_bits(g, w, f"route {route} site {s}")
    one = device(ta[:1], pa[:1]).to_mpo()
    for s, (g, w) in enumerate(zip(one.site_tensors(), ta[0])):
        same_bits(g, w, f"one patch, site {s}")
    with pytest.raises(T4aError) as e:
        a._to_mpo_route(3)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    with pytest.raises(T4aError) as e:
        PartitionedMPO([], [], site_dims=sda).to_mpo()
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and e.value.message == "Partitioned tensor train is empty"


@pytest.mark.parametrize("n, ys, xs, zs, big", CASES[1:3])
def test_add_without_truncation_is_exact(n, ys, xs, zs, big):
    sda, sdb, pa, ta, pb, tb = operands(n, ys, xs, zs, seed=8, big=big)
    rng = np.random.default_rng(9)
    # the other side: patches 1 and 0 of the same partition (in that order) with other bonds; patch 2 is missing there
    qa = [pa[1], pa[0]]
    ua = [ints(rng, P.random_bonds(rng, n), sda) for _ in qa]
    x, y = device(ta, pa), device(ua, qa)
    for lhs, rhs, lp, lt, rp, rt in ((x, y, pa, ta, qa, ua), (y, x, qa, ua, pa, ta)):
        s = lhs.add(rhs, tolerance=0.0)
        want_p, want_t = P.add(lp, lt, rp, rt, tol=0.0)
        assert [p.as_dict() for p in s.projectors()] == want_p
        for k, w in enumerate(want_t):
            for site, (g, ws) in enumerate(zip(s.patch(k).site_tensors(), w)):
                exact(g, np.rint(ws).astype(np.int64), f"patch {k} site {site}")
        exact(s.full_tensor(), dense_i64(lt) + dense_i64(rt))


# ------------------------------------------------------------------------------------------------ from the patching driver
def test_from_partitioned_tt_evaluates_bit_for_bit():
    f = lambda i: 2.0 if all(v == i[0] for v in i) else 0.5  # noqa: E731
    opt = t4a_amd.TCI2Options(tolerance=1e-14, max_bond_dim=1, max_iter=4, ncheck_history=1, nsearch=0, max_nglobal_pivot=0)
    g = t4a_amd.adaptiveinterpolate(f, [4, 4, 4], [[0, 0, 0], [3, 3, 3]], opt, patch_order=[0, 1, 2], recycle_pivots=True)
    assert len(g) >= 2
    m = g.as_mpo([(2, 2)] * 3)
    assert len(m) == len(g) and m.site_dims() == [(2, 2)] * 3
    for k in range(len(g)):
        want = {}
        for site, v in g.projector(k).items():
            want[(site, 0)], want[(site, 1)] = v % 2, v // 2
        assert m.projector(k).as_dict() == want
        assert m.patch(k).link_dims() == g.patch(k).link_dims()
    grid = np.indices([4, 4, 4]).reshape(3, -1).T
    pairs = np.stack([grid % 2, grid // 2], axis=2).reshape(len(grid), 6)
    same_bits(m.evaluate(pairs), g.evaluate(grid))
    flat = g.as_mpo()
    assert flat.site_dims() == [(4, 1)] * 3
    for k in range(len(g)):
        want = {}
        for site, v in g.projector(k).items():
            want[(site, 0)], want[(site, 1)] = v, 0
        assert flat.projector(k).as_dict() == want
    same_bits(flat.evaluate(np.stack([grid, np.zeros_like(grid)], axis=2).reshape(len(grid), 6)), g.evaluate(grid))
    with pytest.raises(T4aError) as e:
        g.as_mpo([(2, 2), (3, 1), (2, 2)])
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and e.value.message == "relabel_site_dims: site 1 has 4 fused indices, not 3 * 1"


def test_to_mpo_of_one_site_adds_the_values():
    rng = np.random.default_rng(12)
    sd = [(3, 2)]
    ps = [{(0, 0): v} for v in range(3)]
    ts = [P.mask(ints(rng, [1, 1], sd), p) for p in ps]
    for route in (0, 1, 2):
        m = device(ts, ps)._to_mpo_route(route)
        assert m.link_dims() == []
        exact(m.site_tensor(0), np.rint(ts[0][0] + ts[1][0] + ts[2][0]).astype(np.int64), f"route {route}")
