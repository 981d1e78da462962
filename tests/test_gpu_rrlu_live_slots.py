"""Live row slots of the single-XCD rrLU kernel (kernels_rrlu_xcd2.hip, xcd_live_slots in kernels_rrlu_xcd_common.hpp).

A plan has 1, 2, 3, 4, 6, 8, 12 or 16 row slots per lane (64 rows each); a matrix of M rows fills ceil(M / 64) of them.  The
step loop leaves the LAST slot of the plan out when it holds no row: it is not updated, not published and not divided.  Here:
matrices whose M sits just around slot boundaries of their plan, as the kernel sees them in both tie orders (a right-orthogonal
factorisation runs on the transpose), with inputs that leave the fast paths — against the oracle, bitwise: pivot order
(permutations), pivot values (the diagonal of the factored matrix), the last pivot error and the whole factored matrix, which the
dense entry point always returns.  And one chained TCI2 run whose bonds are planned for upper bounds their matrices undercut by a
whole slot, with and without the device-table verification of the bond chain."""
import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

# rows x columns as the KERNEL sees them; planned / live row slots
SHAPES = [(260, 130),   # 6 / 5, the last live slot holds four rows
          (320, 130),   # 6 / 5, the last live slot is full
          (321, 130),   # 6 / 6, one row in the last slot
          (513, 140),   # 12 / 9
          (704, 96),    # 12 / 11
          (705, 96),    # 12 / 12, one row in the last slot
          (768, 96)]    # 12 / 12: nothing to skip
EXACT = dict(rel_tol=0.0, abs_tol=0.0)


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def _same_outcome(t4a, a, **opts):
    f, rp, cp, npiv, err = ob.rrlu(a, **opts)
    lu = t4a.rrlu(a, **opts)
    assert lu.npivots() == npiv
    assert np.array_equal(lu.row_permutation, rp) and np.array_equal(lu.col_permutation, cp)
    assert np.array_equal(lu.factored.view(np.uint64), f.view(np.uint64))   # (pivot values: its diagonal; signs of zeros included)
    assert lu.error == err or (np.isnan(lu.error) and np.isnan(err))
    return lu


def _oriented(a, left):
    """The kernel factorises a as it stands (left-orthogonal, column-major tie order) or a.T's transpose, i.e. the caller hands a.T
    over for a right-orthogonal factorisation (row-major tie order): the kernel's rows are the rows of `a` both times."""
    return np.ascontiguousarray(a if left else a.T)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_generic_matrix(t4a, left, shape):
    m, n = shape
    rng = np.random.default_rng(7100 + 3 * m + n)
    a = rng.uniform(-1, 1, size=(m, n))
    lu = _same_outcome(t4a, _oriented(a, left), left_orthogonal=left, **EXACT)   # every step down to the last column
    assert lu.npivots() == n
    _same_outcome(t4a, _oriented(a, left), left_orthogonal=left)                  # default tolerances
    wide = a * 10.0 ** rng.integers(-12, 3, size=(m, 1))
    _same_outcome(t4a, _oriented(wide, left), max_bond_dim=40, rel_tol=1e-9, abs_tol=0.0, left_orthogonal=left)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_low_rank_with_ties(t4a, left, shape):
    """Small integers: most steps find many entries on the largest magnitude (exact sweep in the agents, exact pick in the polling
    wave); behind the rank of the low-rank product the trailing block is zeros and rounding residue."""
    m, n = shape
    rng = np.random.default_rng(7200 + 3 * m + n)
    r = 7
    low = (rng.integers(-2, 3, size=(m, r)) @ rng.integers(-2, 3, size=(r, n))).astype(float)
    _same_outcome(t4a, _oriented(low, left), left_orthogonal=left, **EXACT)
    _same_outcome(t4a, _oriented(low, left), max_bond_dim=r + 5, left_orthogonal=left, **EXACT)
    dense = rng.integers(-2, 3, size=(m, n)).astype(float)
    _same_outcome(t4a, _oriented(dense, left), max_bond_dim=24, left_orthogonal=left, **EXACT)
    last_rows = np.zeros((m, n))            # everything that is not zero sits in the last rows: the last LIVE slot carries the pivots
    last_rows[m - 3:, :] = rng.integers(-3, 4, size=(3, n))
    _same_outcome(t4a, _oriented(last_rows, left), left_orthogonal=left, **EXACT)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_negative_pivots(t4a, left, shape):
    """A negative dominant entry: the first pivot is negative, so 0 / pivot is -0.0 in every padding row, where a slot that is left
    out keeps +0.0 — no result may see the difference.  Then a matrix whose pivots are all negative, and one with zeros of both signs."""
    m, n = shape
    rng = np.random.default_rng(7300 + 3 * m + n)
    a = rng.uniform(-1, 1, size=(m, n))
    a[m - 1, n // 2] = -7.5
    lu = _same_outcome(t4a, _oriented(a, left), left_orthogonal=left, **EXACT)
    d = lu.factored[0, 0]
    assert d == -7.5
    neg = -np.abs(rng.uniform(0.1, 1, size=(m, n))) - 3.0 * np.eye(m, n)[rng.permutation(m)]
    _same_outcome(t4a, _oriented(neg, left), max_bond_dim=32, left_orthogonal=left, **EXACT)
    z = rng.uniform(-1, 1, size=(m, n))
    z[rng.random((m, n)) < 0.3] = 0.0
    z[rng.random((m, n)) < 0.3] = -0.0
    z[0, 0] = -2.0
    _same_outcome(t4a, _oriented(z, left), max_bond_dim=32, left_orthogonal=left, **EXACT)


@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_rank_cap_below_the_rank(t4a, left, shape):
    m, n = shape
    rng = np.random.default_rng(7400 + 3 * m + n)
    a = rng.standard_normal((m, n))
    for cap in (1, 17):
        lu = _same_outcome(t4a, _oriented(a, left), max_bond_dim=cap, left_orthogonal=left, **EXACT)
        assert lu.npivots() == cap   # (the trailing block of the factored matrix is the un-pivoted remainder: compared above)


# ------------------------------------------------------------------------------------------------
# chained TCI2 run: bonds planned for upper bounds their matrices undercut by a whole row slot
# ------------------------------------------------------------------------------------------------
N_SITES, CHI, N_ITER = 14, 48, 7
PARITY = dict(nsearch=0, max_nglobal_pivot=0)


def _spec():
    from t4a_amd.functions import quantics_osc2d
    return quantics_osc2d(N_SITES, k1=37, k2=53, k3=2111, eps=0.5, k4=16411, delta=0.5)


def _options(t4a, k):
    return t4a.TCI2Options(tolerance=1e-12, max_bond_dim=CHI, max_iter=k, ncheck_history=20, **PARITY)


def _start(t):
    t.add_global_pivots([[0] * N_SITES])
    t.set_max_sample_value(1.0)


@pytest.fixture(scope="module")
def oracle_runs(t4a):
    """The oracle's state after k = 1 .. N_ITER iterations from the single initial pivot (a run of k iterations ends in the state a
    longer run passes through after its k-th iteration), computed once."""
    runs = {}
    for k in range(1, N_ITER + 1):
        o = ob.OracleTCI2([2] * N_SITES)
        o.set_function(_spec())
        _start(o)
        o.optimize(_options(t4a, k), final_sweep1site=False)
        runs[k] = dict(i=[np.array(o.i_set(p)) for p in range(N_SITES)], j=[np.array(o.j_set(p)) for p in range(N_SITES)],
                       link_dims=list(o.link_dims()), bond_errors=np.array(o.bond_errors()), pivot_errors=np.array(o.pivot_errors()),
                       history=(list(o.history()[0]), np.array(o.history()[1])), shapes=np.array(o.last_sweep_shapes()),
                       max_sample=o.max_sample_value())
    return runs


def _device_run(t4a, k, verify=False, profile=False):
    g = t4a.TensorCI2([2] * N_SITES)
    g.set_function(_spec())
    g.set_chain(enable=True, verify=verify, small_engine=False)   # the LAUNCHED bond chain, not the one-launch engine for small problems
    if profile:
        g.profile_enable(True)
        g.profile_reset()
    _start(g)
    g.optimize(_options(t4a, k), final_sweep1site=False)
    return g


def _assert_matches(g, ref, k):
    for p in range(N_SITES):
        assert np.array_equal(g.i_set(p), ref["i"][p]), (k, p)
        assert np.array_equal(g.j_set(p), ref["j"][p]), (k, p)
    assert list(g.link_dims()) == ref["link_dims"], k
    assert np.array_equal(g.bond_errors(), ref["bond_errors"]), k
    assert np.array_equal(g.pivot_errors(), ref["pivot_errors"]), k
    assert list(g.history()[0]) == ref["history"][0] and np.array_equal(g.history()[1], ref["history"][1]), k
    assert np.array_equal(g.last_sweep_shapes(), ref["shapes"]), k
    assert g.max_sample_value() == ref["max_sample"], k
    st = g.chain_stats()
    assert st["half_sweeps"] >= 1 and st["fell_back"] == 0 and st["not_eligible"] == 0, (k, st)


def _planned_row_slots(g):
    """Row slots of the widest single-XCD instantiation the profiled run launched (profile code 100000 + 100 RPT + 10 CPT + tie
    order, + 10000000 for the saturated sub-aggregate)."""
    rpts = [(v["code"] % 10000000 - 100000) // 100 for v in g.profile_variants() if 100000 <= v["code"] % 10000000 < 200000 and v["launches"] > 0]
    assert rpts, g.profile_variants()
    return max(rpts)


def test_chained_run_with_dead_slots_matches_oracle(t4a, oracle_runs):
    """Binary sites, chi = 48: a saturated bond is planned for 2 chi + chi = 144 rows (the history extras could add chi), i.e. three
    row slots, and its matrix has at most 128.  Every iteration is compared with the oracle exactly.  The run must have HAD a launch
    with a dead slot: the widest single-XCD plan it launched has more row slots than the largest side of any candidate matrix of
    any of its sweeps fills (the runs of k < N_ITER iterations are the earlier sweeps of the last run)."""
    largest = 0
    for k in range(1, N_ITER + 1):
        g = _device_run(t4a, k, profile=(k == N_ITER))
        _assert_matches(g, oracle_runs[k], k)
        largest = max(largest, int(g.last_sweep_shapes()[:, :2].max()))
    planned = _planned_row_slots(g)
    live = (largest + 63) // 64
    print(f"largest side of any candidate matrix {largest} -> {live} live row slots; widest single-XCD plan launched: {planned} row slots")
    assert planned > live, (planned, live, largest)


def test_chained_run_with_table_verification(t4a, oracle_runs):
    """The same run with set_chain(verify): after every chain the host's mirror must decode to the index sets and equal the device
    tables."""
    g = _device_run(t4a, N_ITER, verify=True)
    _assert_matches(g, oracle_runs[N_ITER], N_ITER)
    g.fill_site_tensors()
    o = ob.OracleTCI2([2] * N_SITES)
    o.set_function(_spec())
    for p in range(N_SITES):
        o.set_index_set(0, p, g.i_set(p))
        o.set_index_set(1, p, g.j_set(p))
    o.fill_site_tensors()
    pts = np.random.default_rng(8).integers(0, 2, size=(200, N_SITES))
    gv, ov = g.evaluate(pts), o.evaluate(pts)
    assert np.abs(gv - ov).max() <= 1e-10 * max(1.0, np.abs(ov).max())
