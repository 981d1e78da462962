"""The fixtures of fill_exact_np.py, pinned on the CPU: for every profile the bit budget holds, the function table is consistent, partial
pivoting on every A_b reproduces the constructed row swaps, the route family the launchers derive from (max_n, max_nrhs) is the one the
table names, and — on the profiles marked for it, with both zero sites and on the linear chain — the oracle's fill_site_tensors returns
the constructed cores bit for bit (small=True: inside the pivot-sensitive bounds).  test_gpu_fill_exact.py takes its expected values from
the construction alone, never from the oracle.
"""
import numpy as np
import pytest

import fill_exact_np as fx
import oracle_binding as ob

IDS = [fx.profile_id(p) for p in fx.PROFILES]
ORACLE = [p for p in fx.PROFILES if p[3]]


def test_the_table_holds_every_required_profile():
    have = [(p[0], p[1]) for p in fx.PROFILES]
    assert have == [([3, 2, 2, 12], [3, 5, 2]), ([8, 6, 4, 3, 80], [3, 17, 9, 5]), ([8, 6, 4, 3, 80], [3, 17, 40, 5]),
                    ([40, 12, 4, 4, 160], [33, 300, 64, 7]), ([64, 64, 8, 6, 64], [9, 530, 40, 2]), ([64, 20, 40, 120], [60, 1030, 20])]
    assert [p[3] for p in fx.PROFILES] == [True, True, True, True, False, False]
    assert fx.LINEAR_DIMS == [[3, 5, 7, 4, 2, 6], [3, 5, 300, 4, 2, 6]]


@pytest.mark.parametrize("p", fx.PROFILES, ids=IDS)
def test_route_named_in_the_table_is_the_launchers(p):
    c = fx.chain(p)
    assert c.max_n() == max(p[1])
    assert fx.fill_route(c.max_n(), c.max_nrhs()) == p[2]
    # a flagged problem does not change the plan, and neither do the values
    assert fx.fill_route(fx.chain(p, small=True).max_n(), fx.chain(p, small=True).max_nrhs()) == p[2]


def test_route_switches():
    """Both sides of every switch of the launchers."""
    r = fx.fill_route
    assert r(31, 16) == "blocked LU nb 32, upper scalar trsm" and r(32, 15) == "blocked LU nb 32, upper scalar trsm"
    assert r(32, 16) == "fused lu_solve_kernel, nb 32" and r(256, 16) == "fused lu_solve_kernel, nb 32"
    assert r(257, 16) == "fused lu_solve_kernel, nb 16" and r(512, 16) == "fused lu_solve_kernel, nb 16"
    assert r(513, 16) == "blocked LU nb 8, upper matrix-core trsm" and r(513, 15) == "blocked LU nb 8, upper scalar trsm"
    assert r(257, 15) == "blocked LU nb 16, upper scalar trsm" and r(64, 15) == "blocked LU nb 32, upper scalar trsm"
    assert r(1024, 16) == "blocked LU nb 8, upper matrix-core trsm" and r(1025, 16) == "lu_kernel, two matrix-core trsm"
    assert r(1264, 16) == "lu_kernel, two scalar trsm"
    assert fx.linear_route(fx.LINEAR_DIMS[0]) == "fill_small_kernel"
    assert fx.linear_route(fx.LINEAR_DIMS[1]) == "pi_eval_batched_kernel, blocked LU nb 32, upper scalar trsm"


@pytest.mark.parametrize("small", [False, True], ids=["exact", "small"])
@pytest.mark.parametrize("p", fx.PROFILES, ids=IDS)
def test_function_table_and_row_swaps(p, small):
    c = fx.chain(p, small=small)
    n = len(c.dims)
    # sets: nested I, distinct J with the bond's residue in the last coordinate
    for b in range(n - 1):
        kron = fx.kron_i(c.i_sets[b], c.dims[b])
        assert len({tuple(r) for r in c.i_sets[b + 1].tolist()}) == c.bonds[b]
        assert np.array_equal(c.i_sets[b + 1], kron[c.nested_cols[b]])
        assert len({tuple(r) for r in c.j_sets[b].tolist()}) == c.bonds[b]
        assert np.all(c.j_sets[b][:, -1] % (n - 1) == b)
        assert np.all(c.j_sets[b] < np.array(c.dims[b + 1:])) and np.all(c.i_sets[b + 1] < np.array(c.dims[:b + 1]))
        # f gives back A and B (the duplicates — nested rows — carry one value: asserted when the table was built)
        assert np.array_equal(c.f.batched(fx._cross(c.i_sets[b + 1], c.j_sets[b])).reshape(c.bonds[b], c.bonds[b]).T, c.A[b])
        assert np.array_equal(c.f.batched(fx._cross(kron, c.j_sets[b])).reshape(len(kron), c.bonds[b]).T, c.B[b])
        assert np.array_equal(c.X[b][:, c.nested_cols[b]], np.eye(c.bonds[b]))
        # partial pivoting must take the constructed rows
        _, _, ipiv = fx.partial_pivot_lu(c.A[b])
        assert np.array_equal(ipiv, c.ipiv[b]), (b, int((ipiv != c.ipiv[b]).sum()))
    assert any((c.ipiv[b] != np.arange(c.bonds[b])).any() for b in range(n - 1))
    assert c.f.n_duplicates == sum(b * b for b in c.bonds)
    # scalar and batched agree, on and off the table
    rng = np.random.default_rng(1)
    pts = np.concatenate([fx._cross(c.i_sets[1], c.j_sets[0])[:5], rng.integers(0, 2, size=(5, n))])
    assert np.array_equal(c.f.batched(pts), [c.f(list(q)) for q in pts])
    assert c.cores[-1].any()  # (the last core reads the pivot matrix of the last bond)


@pytest.mark.parametrize("p", fx.PROFILES, ids=IDS)
def test_bit_budget(p):
    assert fx.assert_bit_budget(fx.chain(p)) < 53
    for z in ((1, 2) if p is fx.P40 else ()):
        c = fx.chain(p, zero_site=z)
        assert fx.assert_bit_budget(c) < 53
        # a zero pivot matrix leaves its neighbours as they were
        ref = fx.chain(p)
        for b in range(len(c.dims) - 1):
            if b != z:
                assert np.array_equal(c.A[b], ref.A[b]) and np.array_equal(c.cores[b], ref.cores[b])


def test_bit_budget_sees_a_fractional_entry():
    c = fx.build([3, 2, 2, 12], [3, 5, 2], 5)
    c.X[1][0, 0] += 0.125
    with pytest.raises(AssertionError):
        fx.assert_bit_budget(c)


def _oracle_fill(c, f):
    tci = ob.OracleTCI2(c.dims)
    tci.set_function(f)
    fx.apply_sets(tci, c)
    tci.fill_site_tensors()
    return tci


@pytest.mark.parametrize("p", ORACLE, ids=[fx.profile_id(p) for p in ORACLE])
def test_oracle_returns_the_constructed_cores(p):
    c = fx.chain(p)
    fx.assert_cores_exact(_oracle_fill(c, c.f), c)


@pytest.mark.parametrize("zero_site", [1, 2])
def test_oracle_zero_pivot_matrix(zero_site):
    c = fx.chain(fx.P40, zero_site=zero_site)
    tci = _oracle_fill(c, c.f)
    assert not tci.site_tensor(zero_site).any()
    fx.assert_cores_exact(tci, c)


@pytest.mark.parametrize("p", ORACLE, ids=[fx.profile_id(p) for p in ORACLE])
def test_oracle_stays_inside_the_pivot_sensitive_bounds(p):
    c = fx.chain(p, small=True)
    tci = _oracle_fill(c, c.f)
    n = len(c.dims)
    ratios = fx.pivot_sensitive_ratios(c, [tci.site_tensor(s) for s in range(n)])
    print(fx.profile_id(p), "ratios to the (forward, backward) bounds per site:", ratios)
    assert sorted(ratios) == list(range(n - 1))
    for b, (fwd, back) in ratios.items():
        assert fwd <= 1.0 and back <= 1.0, (b, fwd, back)
    fx.assert_cores_exact(tci, c, sites=[n - 1])


def test_pivot_sensitive_bound_sees_a_wrong_pivot():
    """The check itself: an elimination that skips one row in one pivot search is outside the forward bound by orders of magnitude."""
    c = fx.chain(fx.P40, small=True)
    b = 2
    a = c.A[b].copy()
    n = len(a)
    bm = c.B[b].copy()
    k0 = int(np.flatnonzero(c.ipiv[b] != np.arange(n))[0])
    for k in range(n):  # elimination without the row swap of step k0
        p = k if k == k0 else k + int(np.argmax(np.abs(a[k:, k])))
        a[[k, p]], bm[[k, p]] = a[[p, k]], bm[[p, k]]
        m = a[k + 1:, k] / a[k, k]
        a[k + 1:, k:] -= np.outer(m, a[k, k:])
        bm[k + 1:] -= np.outer(m, bm[k])
    x = np.linalg.solve(np.triu(a), bm)
    cores = [t.copy() for t in c.cores]
    cores[b] = x.T.reshape(c.cores[b].shape)
    fwd, _ = fx.pivot_sensitive_ratios(c, cores, sites=[b])[b]
    assert fwd > 1e3, fwd


def test_sliced_residual_is_the_longdouble_residual():
    """residual_longdouble takes the sliced route above 2e7 products; on the 300-site both routes are affordable."""
    c = fx.chain(fx.PROFILES[3], small=True)
    a, x, bm = c.A[1], c.X[1], c.B[1]
    g = x * (1 + 1e-13)
    direct = bm.astype(np.longdouble) - a.astype(np.longdouble) @ g.astype(np.longdouble)
    assert a.shape[0] ** 2 * g.shape[1] > 2e7
    sliced = fx.residual_longdouble(a, g, bm)
    scale = np.abs(a).sum(axis=1).max() * np.abs(g).max()
    assert float(np.abs(direct).max() / scale) > 1e-15  # (a residual worth comparing)
    assert float(np.abs(sliced - direct).max() / scale) < 2.0 ** -58


@pytest.mark.parametrize("dims", fx.LINEAR_DIMS, ids=["small", "general"])
def test_oracle_linear_chain(dims):
    c = fx.linear_chain(dims, seed=3)
    # every pivot matrix is [[1, 0], [0, -1]]
    for b in range(len(dims) - 1):
        pts = fx._cross(c.i_sets[b + 1], c.j_sets[b])
        vals = c.spec.accumulators(pts)[:, 0].astype(np.int64).astype(np.float64).reshape(2, 2)
        assert np.array_equal(vals, [[1.0, 0.0], [0.0, -1.0]])
    assert all(np.array_equal(t, np.rint(t)) and np.abs(t).max() < 100 for t in c.cores)
    fx.assert_cores_exact(_oracle_fill(c, c.spec), c)
