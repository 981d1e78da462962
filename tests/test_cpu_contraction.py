"""The MPO Contraction handle and contract_tci without a GPU: exported symbols, NULL arguments refused before the device is touched,
the Python argument checks, and what the reference algorithm alone achieves on the inputs of tests/test_gpu_contraction.py — the
oracle's crossinterpolate2 over the fused site index, fed by the numpy restatement of contraction.rs (tests/contraction_np.py)."""
import ctypes
import os

import numpy as np
import pytest

import contraction_np as cnp

SYMBOLS = ["t4a_gpu_contraction_new", "t4a_gpu_contraction_release", "t4a_gpu_contraction_len", "t4a_gpu_contraction_result_site_dims",
           "t4a_gpu_contraction_evaluate", "t4a_gpu_contraction_evaluate_left", "t4a_gpu_contraction_evaluate_right",
           "t4a_gpu_contraction_evaluate_many", "t4a_gpu_contraction_clear_cache", "t4a_gpu_contraction_n_evaluated", "t4a_gpu_contraction_batch_eval",
           "t4a_gpu_mpo_contract_tci"]

# (n, bond_a, bond_b, tolerance) -> link dims min(4^k, la*lb, 4^(n-k)) of the exact product
TCI_CASES = [((5, 2, 2, 1e-10), [4, 4, 4, 4]), ((6, 2, 3, 1e-10), [4, 6, 6, 6, 4]), ((5, 3, 3, 1e-10), [4, 9, 9, 4]),
             ((6, 2, 2, 1e-12), [4, 4, 4, 4, 4])]
TCI_SEEDS = [cnp.SEED, 12345]


def operands(n, bond_a, bond_b, seed):
    a = cnp.random_tensors([1] + [bond_a] * (n - 1) + [1], 2, 2, seed)
    b = cnp.random_tensors([1] + [bond_b] * (n - 1) + [1], 2, 2, seed ^ 0x5555)
    return a, b


def test_every_contraction_symbol_is_exported():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t4a_gpu.h")).read()
    assert all(s + "(" in header for s in SYMBOLS)


def test_null_arguments_are_refused_before_the_device():
    import t4a_amd
    lib = t4a_amd._lib
    h = ctypes.c_void_p()
    buf = np.zeros(8)
    idx = np.zeros(8, dtype=np.uintp)
    dims = np.zeros(2, dtype=np.uintp)
    used = ctypes.c_size_t(0)
    o = t4a_amd.TCI2Options().to_c()
    one = ctypes.c_size_t(1)
    p = t4a_amd._p
    calls = {
        "new": lambda: lib.t4a_gpu_contraction_new(None, None, ctypes.byref(h)),
        "new out": lambda: lib.t4a_gpu_contraction_new(None, None, None),
        "len": lambda: lib.t4a_gpu_contraction_len(None, ctypes.byref(used)),
        "result_site_dims": lambda: lib.t4a_gpu_contraction_result_site_dims(None, p(dims)),
        "evaluate": lambda: lib.t4a_gpu_contraction_evaluate(None, p(idx), one, p(buf)),
        "evaluate_left": lambda: lib.t4a_gpu_contraction_evaluate_left(None, one, p(idx), one, p(buf), p(dims)),
        "evaluate_right": lambda: lib.t4a_gpu_contraction_evaluate_right(None, one, p(idx), one, p(buf), p(dims)),
        "evaluate_many": lambda: lib.t4a_gpu_contraction_evaluate_many(None, p(idx), one, one, p(buf), ctypes.byref(used)),
        "clear_cache": lambda: lib.t4a_gpu_contraction_clear_cache(None),
        "n_evaluated": lambda: lib.t4a_gpu_contraction_n_evaluated(None, ctypes.byref(used)),
        "contract_tci": lambda: lib.t4a_gpu_mpo_contract_tci(None, None, ctypes.byref(o), None, ctypes.c_size_t(0), ctypes.byref(h), p(buf)),
    }
    for name, call in calls.items():
        assert call() == t4a_amd.NULL_POINTER, name
        assert "null" in t4a_amd.last_error_message(), name
        assert not h, name
    lib.t4a_gpu_contraction_batch_eval.restype = ctypes.c_int64
    idx32 = np.zeros(4, dtype=np.uint32)
    assert lib.t4a_gpu_contraction_batch_eval(None, p(idx32), ctypes.c_size_t(2), one, p(buf)) == t4a_amd.NULL_POINTER
    assert "ctx is null" in t4a_amd.last_error_message()
    lib.t4a_gpu_contraction_release(None)  # releasing nothing is allowed, as for every other handle


def test_python_index_checks():
    import t4a_amd
    from t4a_amd.mpo import _index_pairs, _fused_pivots
    full, single = _index_pairs([(0, 1), (1, 0), (1, 1)], 3, 3, True)
    assert single and full.shape == (1, 3, 2) and full.dtype == np.uintp and full[0].tolist() == [[0, 1], [1, 0], [1, 1]]
    full, single = _index_pairs(np.zeros((5, 2, 2), dtype=int), 4, 2, False)  # a left environment of two sites of four
    assert not single and full.shape == (5, 4, 2)
    full, single = _index_pairs([], 3, 0, False)  # evaluate_left(0, [])
    assert single and full.shape == (1, 3, 2)
    for args, needle in ((([(0, 1), (1, 0)], 3, 3, True), "Expected 3 index pairs, got 2"),
                         (([(0, 1)] * 4, 3, 3, True), "Expected 3 index pairs, got 4"),
                         (([(0, 1)], 3, 2, False), "Expected at least 2 index pairs, got 1"),
                         (([(0, 1, 2)] * 3, 3, 3, True), "indices must be"),  # three legs where a pair is needed
                         (([0, 1, 0, 1, 0, 1], 3, 3, True), "indices must be"),
                         (([(0, 1), (-1, 0), (0, 0)], 3, 3, True), "negative index")):
        with pytest.raises(t4a_amd.T4aError) as e:
            _index_pairs(*args)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and needle in e.value.message
    assert _fused_pivots(None, 4)[1] == 0 and _fused_pivots([], 4)[1] == 0
    piv, k = _fused_pivots([[0, 1, 2, 3], [3, 2, 1, 0]], 4)
    assert k == 2 and piv.dtype == np.uintp and piv.tolist() == [[0, 1, 2, 3], [3, 2, 1, 0]]
    for bad, needle in (([[0, 1, 2]], "Pivot length must match number of sites"), ([[0, -1, 2, 3]], "negative index")):
        with pytest.raises(t4a_amd.T4aError) as e:
            _fused_pivots(bad, 4)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and needle in e.value.message


def test_contract_tci_defaults_and_the_fit_algorithm_constant_stay():
    import inspect
    import t4a_amd
    assert t4a_amd.Contraction is t4a_amd.mpo.Contraction and t4a_amd.contract_tci is t4a_amd.mpo.contract_tci
    assert (t4a_amd.ContractionAlgorithm.Naive, t4a_amd.ContractionAlgorithm.ZipUp, t4a_amd.ContractionAlgorithm.Fit) == (0, 1, 2)
    src = inspect.getsource(t4a_amd.mpo.contract_tci)
    assert "tolerance=1e-12, max_nglobal_pivot=0, nsearch=0" in src


def test_restatement_agrees_with_the_dense_product():
    """the checker checked: evaluate, and left · right environments at every cut, against the dense product of the site contractions"""
    for n, la, lb in ((1, 1, 1), (3, 2, 3), (4, 5, 4)):
        a, b = operands(n, la, lb, cnp.SEED)
        c = cnp.ContractionNP(a, b)
        dense = cnp.dense_product(a, b)
        pairs = cnp.lcg_points(40, [[2, 2]] * n, 7)
        want = np.array([dense[tuple(p.reshape(-1))] for p in pairs])
        assert np.abs(c.evaluate(pairs) - want).max() <= 1e-14 * max(1.0, np.abs(dense).max())
        for cut in range(n + 1):
            left, right = c.evaluate_left(cut, pairs), c.evaluate_right(cut, pairs)
            assert np.abs(np.einsum("pab,pab->p", left, right) - want).max() <= 1e-14 * max(1.0, np.abs(dense).max())
            if 1 <= cut:
                assert np.abs(c.evaluate_many(pairs, cut) - want).max() <= 1e-14 * max(1.0, np.abs(dense).max())
        grid = np.indices([2, 2] * n).reshape(2 * n, -1).T.reshape(-1, n, 2)  # every entry: an outer product at any cut
        assert np.abs(c.evaluate_many(grid, max(n // 2, 1)) - dense.reshape(-1)).max() <= 1e-14 * max(1.0, np.abs(dense).max())
    assert cnp.find_split(np.zeros((3, 1, 2), dtype=int)) == 1
    # 8 sites, the outer product of 2 prefixes that differ at site 5 with 8 suffixes over sites 6 and 7: the cut at 6 sees 2 + 8 unique
    # halves, the cuts at 2 and 4 see 1 + 16
    pts = np.zeros((16, 8, 2), dtype=int)
    for q in range(16):
        p, k = q // 8, q % 8
        pts[q, 5] = (p, 0)
        pts[q, 6] = (k & 1, (k >> 1) & 1)
        pts[q, 7] = ((k >> 2) & 1, 0)
    assert cnp.find_split(pts) == 6
    assert cnp.find_split(pts[:, ::-1]) == 2


@pytest.mark.parametrize("seed", TCI_SEEDS)
@pytest.mark.parametrize("case, links", TCI_CASES)
def test_reference_tci_recovers_the_exact_product(case, links, seed):
    """crossinterpolate2 of the reference over the fused index, fed by the restated Contraction::evaluate, started at the arg-max of the
    dense product without global pivot search: the exact ranks min(4^k, la*lb, 4^(n-k)) and the product to rounding.  Measured when this
    test was written: largest deviation relative to the largest entry between 4.0e-16 and 8.7e-16 over the four cases; the bound asserted
    is 1e-12."""
    import oracle_binding as ob
    import t4a_amd
    n, la, lb, tol = case
    a, b = operands(n, la, lb, seed)
    c = cnp.ContractionNP(a, b)
    dense = cnp.fused_dense(cnp.dense_product(a, b), c.site_dims)
    first = [int(v) for v in np.unravel_index(int(np.abs(dense).argmax()), dense.shape)]
    opts = t4a_amd.TCI2Options(tolerance=tol, max_nglobal_pivot=0, nsearch=0)
    o = ob.OracleTCI2(c.fused_dims())
    o.set_function(c.fused_function())
    o.crossinterpolate2([first], opts)
    assert [int(x) for x in o.link_dims()] == links
    grid = np.indices(dense.shape).reshape(n, -1).T
    got = np.asarray(o.evaluate(grid)).reshape(dense.shape)
    dev = float(np.abs(got - dense).max() / np.abs(dense).max())
    print(f"reference TCI of A.B: case {case} seed {seed:#x} link dims {links} deviation {dev:.3e}")
    assert dev <= 1e-12


# ------------------------------------------------------------------------------------------------ the exact reference
def test_exact_bound_is_the_all_ones_product_and_below_2_53_on_every_profile():
    """exact_bound is the element of the product of all-ones operands (every element is the same), and every profile of the exact
    device tests keeps it below 2^53: the largest is the mixed profile with a shared dimension of 3."""
    for name, (bonds_a, bonds_b, (s1, k, s2)) in cnp.EXACT_PROFILES.items():
        a = [np.ones((l, s1, k, r)) for l, r in zip(bonds_a[:-1], bonds_a[1:])]
        b = [np.ones((l, k, s2, r)) for l, r in zip(bonds_b[:-1], bonds_b[1:])]
        bound = cnp.exact_bound(a, b)
        assert isinstance(bound, int) and 0 < bound < 2 ** 53, (name, bound)
        assert bound == cnp.exact_bound(*cnp.exact_operands(name)), name
        n = len(a)
        ones = cnp.ContractionNP(a, b, exact=True).evaluate(np.zeros((1, n, 2), dtype=np.int64))
        assert ones.dtype == np.int64 and int(ones[0]) == bound, (name, int(ones[0]), bound)
    assert cnp.exact_bound(*cnp.exact_operands("P1")) == cnp.exact_bound(*cnp.exact_operands("P2")) == 3077288755200  # 3.08e12
    assert cnp.exact_bound(*cnp.exact_operands("P1_k3")) == 3077288755200 // 2 ** 6 * 3 ** 6 == 35052242227200  # 3.5e13
    assert cnp.exact_bound(*cnp.exact_operands("scratch")) == 8 * (64 * 33) ** 2
    small_a, small_b = [np.ones((1, 2, 3, 4)), np.ones((4, 2, 3, 1))], [np.ones((1, 3, 2, 5)), np.ones((5, 3, 2, 1))]
    assert cnp.exact_bound(small_a, small_b) == 3 * 3 * 4 * 5
    assert np.array_equal(cnp.dense_product(small_a, small_b), np.full((2, 2, 2, 2), 180.0))


def test_integer_tensors_hold_minus_one_zero_and_one():
    ts = cnp.integer_tensors([1, 5, 7, 1], 2, 3, cnp.SEED)
    assert [t.shape for t in ts] == [(1, 2, 3, 5), (5, 2, 3, 7), (7, 2, 3, 1)] and all(t.dtype == np.float64 for t in ts)
    flat = np.concatenate([t.reshape(-1, order="F") for t in ts])
    assert set(np.unique(flat)) == {-1.0, 0.0, 1.0}
    state, want = cnp.SEED, []
    for _ in range(flat.size):  # one LCG stream through the sites, column-major, as random_tensors draws it
        state = (state * 6364136223846793005 + 1442695040888963407) & cnp.MASK
        want.append((state >> 33) % 3 - 1)
    assert np.array_equal(flat, np.array(want, dtype=np.float64))
    with pytest.raises(AssertionError):
        cnp.ContractionNP(cnp.random_tensors([1, 2, 1], 2, 2, 1), cnp.random_tensors([1, 2, 1], 2, 2, 2), exact=True)


@pytest.mark.parametrize("name", ["P1", "P2"])
def test_int64_reference_equals_the_float_restatement_and_the_dense_product(name):
    """With entries from {-1, 0, 1} and exact_bound < 2^53 the float restatement is exact whatever its order of summation, so the
    int64 reference, the float restatement and the dense product of the site contractions agree in every digit."""
    a, b = cnp.exact_operands(name)
    n = len(a)
    assert cnp.exact_bound(a, b) < 2 ** 53
    ref_i, ref_f = cnp.ContractionNP(a, b, exact=True), cnp.ContractionNP(a, b)
    dense = cnp.dense_product(a, b)
    assert np.array_equal(dense, np.rint(dense)) and np.abs(dense).max() > 1
    dims = [[2, 2]] * n
    pairs = cnp.lcg_points(40, dims, 7)
    want = dense[tuple(pairs.reshape(len(pairs), -1).T)].astype(np.int64)
    got = ref_i.evaluate(pairs)
    assert got.dtype == np.int64 and np.array_equal(got, want) and np.array_equal(ref_f.evaluate(pairs), want)
    for cut in range(n + 1):
        left, right = ref_i.evaluate_left(cut, pairs), ref_i.evaluate_right(cut, pairs)
        assert left.dtype == right.dtype == np.int64
        assert np.array_equal(left, ref_f.evaluate_left(cut, pairs)) and np.array_equal(right, ref_f.evaluate_right(cut, pairs))
        assert np.array_equal(np.einsum("pab,pab->p", left, right), want)
        if cut >= 1:
            many = ref_i.evaluate_many(pairs, cut)
            assert many.dtype == np.int64 and np.array_equal(many, want) and np.array_equal(ref_f.evaluate_many(pairs, cut), want)
        rows, cols = pairs[:5, :cut], pairs[5:12, cut:]
        block = ref_i.evaluate_matrix(cut, rows, cols)
        full = np.concatenate([np.repeat(rows, len(cols), axis=0), np.tile(cols, (len(rows), 1, 1))], axis=1)
        assert block.dtype == np.int64 and block.shape == (5, 7)
        assert np.array_equal(block, dense[tuple(full.reshape(len(full), -1).T)].reshape(5, 7))
        assert np.array_equal(block, ref_f.evaluate_matrix(cut, rows, cols))
    sites_i = [cnp.np_site(x.astype(np.int64), y.astype(np.int64)) for x, y in zip(a, b)]
    assert all(s.dtype == np.int64 and np.array_equal(s, cnp.np_site(x, y)) for s, x, y in zip(sites_i, a, b))


CONTRACTION_LDS_DOUBLES = 8192  # kernels.hpp: what of a working set fits the LDS


def core_use(m, n):
    return m >= 16 and n >= 16


def walk_branches(bonds_a, bonds_b):
    """(left, right): per site the pair (product 1 on the cores, product 2 on the cores) that wg_product decides from the shapes"""
    left, right = [], []
    for s in range(len(bonds_a) - 1):
        la, ra, lb, rb = bonds_a[s], bonds_a[s + 1], bonds_b[s], bonds_b[s + 1]
        left.append((core_use(ra, lb), core_use(ra, rb)))
        right.append((core_use(la, rb), core_use(la, lb)))
    return left, right


def test_the_mixed_profiles_reach_every_branch_combination():
    """The branch table in the docstring of tests/test_gpu_mpo_exact.py restated from the bonds, so that an edit of a profile that
    loses a combination fails here."""
    seen_l, seen_r, both_scalar_beside_wide, summed, tiles, edges = set(), set(), 0, set(), set(), set()
    for name in ("P1", "P2"):
        ba, bb, _ = cnp.EXACT_PROFILES[name]
        left, right = walk_branches(ba, bb)
        seen_l |= set(left)
        seen_r |= set(right)
        for s in range(len(ba) - 1):
            la, ra, lb, rb = ba[s], ba[s + 1], bb[s], bb[s + 1]
            both_scalar_beside_wide += (ra < 16 and lb >= 16 and rb >= 16) + (la < 16 and lb >= 16 and rb >= 16)
            for on_cores, m, n, k2 in ((left[s][0], ra, lb, la), (left[s][1], ra, rb, lb), (right[s][0], la, rb, ra), (right[s][1], la, lb, rb)):
                if on_cores:
                    summed.add(k2)
                    tiles.add(((m + 15) // 16) * ((n + 15) // 16))
                    edges |= {m, n}
    every = {(False, False), (False, True), (True, False), (True, True)}
    assert seen_l == every and seen_r == every
    assert both_scalar_beside_wide >= 2
    assert {3, 5, 16, 17, 18, 31, 33} <= summed
    assert 6 in tiles and max(tiles) > 4
    assert {16, 17, 18, 20, 31, 33} <= edges
    for name in ("P1", "P2", "P1_k3", "P1_k1"):  # all of them walk in the LDS, "scratch" does not
        ba, bb, (_, k, _) = cnp.EXACT_PROFILES[name]
        env = max(x * y for x, y in zip(ba, bb))
        t = max(k * max(ba[s + 1] * bb[s], ba[s] * bb[s + 1]) for s in range(len(ba) - 1))
        assert 2 * env + t <= CONTRACTION_LDS_DOUBLES
    ba, bb, (_, k, _) = cnp.EXACT_PROFILES["scratch"]
    assert 2 * ba[1] * bb[1] + k * ba[2] * bb[1] == 8448 > CONTRACTION_LDS_DOUBLES
