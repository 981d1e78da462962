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
