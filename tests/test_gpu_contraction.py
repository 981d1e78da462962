"""The device-resident Contraction of two MPOs (tensor4all-simplett/src/mpo/contraction.rs:60-383) and MPO products by TCI2 against the
numpy restatement tests/contraction_np.py and the dense product of the site contractions.  Values are compared at 1e-10 relative to
max(1, max|dense|) — the tolerance tests/test_gpu_mpo.py states for this layer; ranks, shapes and splits exactly."""
import gc

import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, Contraction, contract_tci, contract_naive, contract_zipup, TCI2Options, TensorCI2

import contraction_np as cnp

pytestmark = pytest.mark.gpu

SEED = cnp.SEED


def close(got, want, scale_from=None, rel=1e-10):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    ref = want if scale_from is None else np.asarray(scale_from)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    print(f"max deviation {err:.3e} at scale {scale:.3e}")
    assert err <= rel * scale, f"max deviation {err:.3e} at scale {scale:.3e}"


def bonds_of(n, bond):
    return [1] + [bond] * (n - 1) + [1]


def operands(n, bond_a, bond_b, seed=SEED, s1=2, k=2, s2=2):
    a = cnp.random_tensors(bonds_of(n, bond_a), s1, k, seed)
    b = cnp.random_tensors(bonds_of(n, bond_b), k, s2, seed ^ 0x5555)
    return a, b


def all_pairs(site_dims):
    """every index tuple of the product, (total, n, 2)"""
    shape = [d for pair in site_dims for d in pair]
    grid = np.indices(shape).reshape(len(shape), -1).T
    return grid.reshape(-1, len(site_dims), 2)


def dense_at(dense, pairs):
    return dense[tuple(pairs.reshape(len(pairs), -1).T)]


# ------------------------------------------------------------------------------------------------ 1. evaluate
@pytest.mark.parametrize("n", [1, 2, 3, 6])
@pytest.mark.parametrize("bond_a, bond_b", [(1, 1), (2, 3), (5, 4)])
def test_evaluate_matches_the_dense_product_on_every_entry(n, bond_a, bond_b):
    a, b = operands(n, bond_a, bond_b)
    c = Contraction(MPO(a), MPO(b))
    assert len(c) == n and c.len() == n and c.result_site_dims() == [(2, 2)] * n
    dense = cnp.dense_product(a, b)
    pairs = all_pairs(c.result_site_dims())
    close(c.evaluate(pairs), dense_at(dense, pairs), dense)
    one = c.evaluate([tuple(p) for p in pairs[-1]])
    assert isinstance(one, float) and abs(one - dense_at(dense, pairs[-1:])[0]) <= 1e-10 * max(1.0, np.abs(dense).max())


def test_evaluate_with_non_square_site_dims():
    a, b = operands(4, 3, 2, s1=2, k=3, s2=2)
    c = Contraction(MPO(a), MPO(b))
    assert c.result_site_dims() == [(2, 2)] * 4
    dense = cnp.dense_product(a, b)
    pairs = all_pairs(c.result_site_dims())
    close(c.evaluate(pairs), dense_at(dense, pairs), dense)
    a, b = operands(3, 2, 3, s1=3, k=2, s2=1)  # an operator applied to a state
    c = Contraction(MPO(a), MPO(b))
    assert c.result_site_dims() == [(3, 1)] * 3
    dense = cnp.dense_product(a, b)
    pairs = all_pairs(c.result_site_dims())
    close(c.evaluate(pairs), dense_at(dense, pairs), dense)
    close(c.evaluate_many(pairs)[0], dense_at(dense, pairs), dense)


def test_identity_times_b_is_b():
    b = cnp.random_tensors(bonds_of(5, 3), 2, 2, SEED)
    mb = MPO(b)
    c = Contraction(MPO.identity([2] * 5), mb)
    pairs = all_pairs([(2, 2)] * 5)
    close(c.evaluate(pairs), mb.evaluate(pairs.reshape(len(pairs), -1)), cnp.np_full(b))
    close(c.evaluate(pairs), dense_at(cnp.np_full(b), pairs), cnp.np_full(b))


# ------------------------------------------------------------------------------------------------ 2. environments
@pytest.mark.parametrize("n, bond_a, bond_b, dims", [(1, 1, 1, (2, 2, 2)), (4, 2, 3, (2, 2, 2)), (5, 5, 4, (2, 3, 2)), (3, 20, 17, (2, 2, 2)),
                                                     (3, 20, 17, (2, 3, 2)), (4, 18, 16, (2, 2, 1))])  # the last three: matrix cores
def test_environments_match_the_restatement(n, bond_a, bond_b, dims):
    s1, k, s2 = dims
    a, b = operands(n, bond_a, bond_b, s1=s1, k=k, s2=s2)
    c = Contraction(MPO(a), MPO(b))
    ref = cnp.ContractionNP(a, b)
    pairs = cnp.lcg_points(23, [[s1, s2]] * n, 99)
    scale = cnp.dense_product(a, b)
    for cut in range(n + 1):
        left = c.evaluate_left(cut, pairs)
        right = c.evaluate_right(cut, pairs)
        want_l, want_r = ref.evaluate_left(cut, pairs), ref.evaluate_right(cut, pairs)
        assert left.shape == want_l.shape == (23,) + ((1, 1) if cut == 0 else (a[cut - 1].shape[3], b[cut - 1].shape[3]))
        assert right.shape == want_r.shape == (23,) + ((1, 1) if cut == n else (a[cut].shape[0], b[cut].shape[0]))
        close(left, want_l, scale)
        close(right, want_r, scale)
        # a left environment needs only the first `cut` pairs, a single tuple gives a single matrix
        single = c.evaluate_left(cut, [tuple(p) for p in pairs[0, :cut]])
        assert single.shape == want_l.shape[1:] and np.array_equal(single, left[0])
    assert np.array_equal(c.evaluate_left(0, []), np.ones((1, 1))) and np.array_equal(c.evaluate_right(n, []), np.ones((1, 1)))


# ------------------------------------------------------------------------------------------------ 3. evaluate_many
@pytest.mark.parametrize("n, bond_a, bond_b", [(1, 1, 1), (2, 2, 3), (6, 2, 3), (8, 5, 4)])
def test_evaluate_many_agrees_for_every_split(n, bond_a, bond_b):
    a, b = operands(n, bond_a, bond_b)
    c = Contraction(MPO(a), MPO(b))
    dense = cnp.dense_product(a, b)
    pairs = cnp.lcg_points(300, [[2, 2]] * n, 5)
    pairs[17] = pairs[3]  # duplicate points
    pairs[250] = pairs[3]
    want = dense_at(dense, pairs)
    close(c.evaluate(pairs), want, dense)
    for split in range(1, n + 1):
        vals, used = c.evaluate_many(pairs, split=split)
        assert used == split
        close(vals, want, dense)
    vals, used = c.evaluate_many(pairs)
    assert used == cnp.find_split(pairs)
    close(vals, want, dense)
    vals, used = c.evaluate_many(pairs[:1])  # a single point
    assert vals.shape == (1,) and used == cnp.find_split(pairs[:1])
    close(vals, want[:1], dense)
    vals, used = c.evaluate_many(np.zeros((0, n, 2), dtype=int), split=None)
    assert vals.shape == (0,)


def test_evaluate_many_reports_the_split_of_the_heuristic():
    n = 8
    a, b = operands(n, 3, 2)
    c = Contraction(MPO(a), MPO(b))
    dense = cnp.dense_product(a, b)
    pts = np.zeros((16, n, 2), dtype=int)
    for q in range(16):
        p, k = q // 8, q % 8
        pts[q, 5] = (p, 0)
        pts[q, 6] = (k & 1, (k >> 1) & 1)
        pts[q, 7] = ((k >> 2) & 1, 0)
    for batch, want_split in ((pts, 6), (pts[:, ::-1].copy(), 2), (cnp.lcg_points(500, [[2, 2]] * n, 11), None)):
        vals, used = c.evaluate_many(batch)
        assert used == cnp.find_split(batch) and (want_split is None or used == want_split)
        close(vals, dense_at(dense, batch), dense)


# ------------------------------------------------------------------------------------------------ 4. errors
def raises(code, needle, call):
    with pytest.raises(t4a_amd.T4aError) as e:
        call()
    assert e.value.code == code and needle in e.value.message, e.value


def test_errors_carry_the_reference_messages():
    inv = t4a_amd.INVALID_ARGUMENT
    a3 = MPO(cnp.random_tensors(bonds_of(3, 2), 2, 2, SEED))
    b2 = MPO(cnp.random_tensors(bonds_of(2, 2), 2, 2, SEED))
    raises(inv, "MPO length mismatch: expected 3, got 2", lambda: Contraction(a3, b2))
    a_k3 = MPO(cnp.random_tensors(bonds_of(3, 2), 2, 3, SEED))
    raises(inv, "Shared shape mismatch at site 0: MPO A has site_dim_2=3, MPO B has site_dim_1=2", lambda: Contraction(a_k3, a3))
    mixed = cnp.random_tensors(bonds_of(3, 2), 2, 2, SEED)
    mixed[1] = cnp.random_tensors([2, 2], 2, 3, SEED)[0]
    raises(inv, "Shared shape mismatch at site 1: MPO A has site_dim_2=3, MPO B has site_dim_1=2", lambda: Contraction(MPO(mixed), a3))
    raises(inv, "MPO length mismatch", lambda: contract_tci(a3, b2))
    raises(inv, "Shared shape mismatch at site 0", lambda: contract_tci(a_k3, a3))
    c = Contraction(a3, MPO(cnp.random_tensors(bonds_of(3, 3), 2, 3, SEED)))  # result site dims (2, 3)
    ok = [(0, 0), (1, 2), (1, 1)]
    assert isinstance(c.evaluate(ok), float)
    raises(inv, "Expected 3 index pairs, got 2", lambda: c.evaluate(ok[:2]))
    raises(inv, "Expected 3 index pairs, got 4", lambda: c.evaluate(ok + [(0, 0)]))
    raises(inv, "Expected 3 index pairs, got 2", lambda: c.evaluate_many(np.zeros((4, 2, 2), dtype=int)))
    raises(inv, "Index out of bounds: index 2 at site 0 (max: 3)", lambda: c.evaluate([(2, 0), (0, 0), (0, 0)]))
    raises(inv, "Index out of bounds: index 3 at site 1 (max: 3)", lambda: c.evaluate([(0, 0), (1, 3), (0, 0)]))
    raises(inv, "Index out of bounds: index 3 at site 2 (max: 3)", lambda: c.evaluate_many([[(0, 0), (0, 0), (0, 3)]]))
    raises(inv, "negative index", lambda: c.evaluate([(0, 0), (-1, 0), (0, 0)]))
    raises(inv, "Site 4 is out of range [0, 3]", lambda: c.evaluate_left(4, ok))
    raises(inv, "Site 4 is out of range [0, 3]", lambda: c.evaluate_right(4, ok))
    raises(inv, "Expected at least 2 index pairs, got 1", lambda: c.evaluate_left(2, ok[:1]))
    raises(inv, "Expected at least 3 index pairs, got 2", lambda: c.evaluate_right(2, ok[:2]))
    raises(inv, "Index out of bounds: index 2 at site 0 (max: 3)", lambda: c.evaluate_left(1, [(2, 0)]))
    raises(inv, "Index out of bounds: index 5 at site 2 (max: 3)", lambda: c.evaluate_right(2, [(9, 9), (9, 9), (0, 5)]))
    # only the sites an environment covers are checked (contraction.rs:280, :349)
    assert c.evaluate_left(1, [(1, 2), (9, 9), (9, 9)]).shape == (2, 3)
    assert c.evaluate_right(2, [(9, 9), (9, 9), (1, 2)]).shape == (2, 3)
    raises(inv, "Invalid split position: 4 (n_sites=3)", lambda: c.evaluate_many([ok], split=4))
    raises(inv, "Invalid split position: 0 (n_sites=3)", lambda: c.evaluate_many([ok], split=0))
    # the native callback refuses what the handle refuses: a fused index beyond s1 * s2, a wrong number of sites
    import ctypes
    fn, ctx, _ = c.as_callback()
    cb = ctypes.cast(fn, ctypes.CFUNCTYPE(ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p))
    out = np.zeros(1)
    assert cb(ctx, t4a_amd._p(np.array([0, 6, 0], dtype=np.uint32)), 3, 1, t4a_amd._p(out)) == inv
    assert "Index out of bounds" in t4a_amd.last_error_message()
    assert cb(ctx, t4a_amd._p(np.array([0, 0], dtype=np.uint32)), 2, 1, t4a_amd._p(out)) == inv
    assert cb(ctx, t4a_amd._p(np.array([1, 5, 3], dtype=np.uint32)), 3, 1, t4a_amd._p(out)) == 1
    assert abs(out[0] - c.evaluate([(1, 0), (1, 2), (1, 1)])) <= 1e-10
    before = c.evaluate_many([ok])[0]
    c.clear_cache()  # nothing is kept between calls: the same bits afterwards
    assert np.array_equal(before, c.evaluate_many([ok])[0])


def test_the_empty_contraction():
    c = Contraction(MPO([]), MPO([]))
    assert len(c) == 0 and c.result_site_dims() == []
    raises(t4a_amd.INVALID_ARGUMENT, "MPO is empty", lambda: c.evaluate([]))
    raises(t4a_amd.INVALID_ARGUMENT, "MPO is empty", lambda: c.evaluate_many(np.zeros((2, 0, 2), dtype=int)))
    assert np.array_equal(c.evaluate_left(0, []), np.ones((1, 1))) and np.array_equal(c.evaluate_right(0, []), np.ones((1, 1)))
    raises(t4a_amd.INVALID_ARGUMENT, "Site 1 is out of range [0, 0]", lambda: c.evaluate_left(1, []))


def test_operands_may_be_released_before_the_first_evaluate():
    a, b = operands(5, 3, 4)
    ma, mb = MPO(a), MPO(b)
    c = Contraction(ma, mb)
    del ma, mb
    gc.collect()
    junk = [MPO(cnp.random_tensors(bonds_of(5, 4), 2, 2, 77 + i)) for i in range(4)]  # reuse what the operands gave back to the pool
    dense = cnp.dense_product(a, b)
    pairs = all_pairs([(2, 2)] * 5)
    close(c.evaluate(pairs), dense_at(dense, pairs), dense)
    close(c.evaluate_many(pairs)[0], dense_at(dense, pairs), dense)
    del junk


# ------------------------------------------------------------------------------------------------ 5. transform
def test_with_transform_squares_the_values():
    a, b = operands(4, 2, 3)
    plain = Contraction(MPO(a), MPO(b))
    pairs = all_pairs([(2, 2)] * 4)
    vals = plain.evaluate(pairs)

    def scalar_only(v):
        if not isinstance(v, float):
            raise TypeError("scalars only")
        return v * v

    for f in (lambda v: v * v, scalar_only):
        sq = Contraction.with_transform(MPO(a), MPO(b), f)
        assert np.array_equal(sq.evaluate(pairs), vals * vals)
        assert np.array_equal(sq.evaluate_many(pairs)[0], plain.evaluate_many(pairs)[0] ** 2)
        assert sq.evaluate([tuple(p) for p in pairs[5]]) == vals[5] * vals[5]
        raises(t4a_amd.INVALID_ARGUMENT, "transform", sq.as_callback)


# ------------------------------------------------------------------------------------------------ 6. plumbing, exact
def run_tci(dims, first, opts, attach, threads=None):
    g = TensorCI2(dims)
    attach(g)
    if threads:
        g.set_callback_threads(threads)
    g.crossinterpolate2([first], opts)
    return g


def same_bits(g, h):
    n = len(g.local_dims)
    for p in range(n):
        assert np.array_equal(g.i_set(p), h.i_set(p)) and np.array_equal(g.j_set(p), h.j_set(p)), f"index sets differ at {p}"
        assert np.array_equal(g.site_tensor(p).view(np.uint64), h.site_tensor(p).view(np.uint64)), f"site tensor {p} differs"
    assert np.array_equal(g.pivot_errors().view(np.uint64), h.pivot_errors().view(np.uint64))
    assert g.history()[0] == h.history()[0] and np.array_equal(g.history()[1].view(np.uint64), h.history()[1].view(np.uint64))
    assert g.link_dims() == h.link_dims() and g.termination() == h.termination()


def test_native_callback_and_python_callable_give_the_same_bits():
    """A TensorCI2 fed by t4a_gpu_contraction_batch_eval directly and one fed by a Python callable that calls evaluate_many on the same
    fused indices see the same values, so they choose the same pivots and end with the same bits; so does a run whose large candidate
    matrices are evaluated by four host threads."""
    n = 8
    a, b = operands(n, 6, 6)
    ref = cnp.ContractionNP(a, b)
    dense = cnp.fused_dense(cnp.dense_product(a, b), ref.site_dims)
    first = [int(v) for v in np.unravel_index(int(np.abs(dense).argmax()), dense.shape)]
    opts = TCI2Options(tolerance=1e-10, max_nglobal_pivot=0, nsearch=0)
    dims = ref.fused_dims()

    c_native = Contraction(MPO(a), MPO(b))
    run_a = run_tci(dims, first, opts, lambda g: g.set_callback_raw(*c_native.as_callback()))

    c_python = Contraction(MPO(a), MPO(b))
    batches = []

    def scalar(idx):
        return float(c_python.evaluate_many(ref.decode([idx]))[0][0])

    def batched(arr):
        batches.append(len(arr))
        return c_python.evaluate_many(ref.decode(arr))[0]

    scalar.batched = batched
    run_b = run_tci(dims, first, opts, lambda g: g.set_function(scalar))
    same_bits(run_a, run_b)
    assert c_native.n_evaluated() == c_python.n_evaluated() == sum(batches)
    assert max(batches) >= 1 << 14  # large enough for the threaded route below to split a candidate matrix

    c_threads = Contraction(MPO(a), MPO(b))
    run_c = run_tci(dims, first, opts, lambda g: g.set_callback_raw(*c_threads.as_callback()), threads=4)
    same_bits(run_a, run_c)
    assert c_threads.n_evaluated() == c_native.n_evaluated()

    assert run_a.link_dims() == [min(4 ** (k + 1), 36, 4 ** (n - k - 1)) for k in range(n - 1)]
    grid = cnp.lcg_points(2000, dims, 3)
    close(run_a.evaluate(grid), dense[tuple(grid.T)], dense)


# ------------------------------------------------------------------------------------------------ 7. contract_tci
TCI_CASES = [((5, 2, 2, 1e-10), [4, 4, 4, 4]), ((6, 2, 3, 1e-10), [4, 6, 6, 6, 4]), ((5, 3, 3, 1e-10), [4, 9, 9, 4]),
             ((6, 2, 2, 1e-12), [4, 4, 4, 4, 4])]


@pytest.mark.parametrize("seed", [SEED, 12345])
@pytest.mark.parametrize("case, links", TCI_CASES)
def test_contract_tci_recovers_the_exact_product(case, links, seed):
    """The reference's own crossinterpolate2 reaches <= 8.7e-16 on these inputs (tests/test_cpu_contraction.py): the 1e-10 asked here
    is room for the device's summation order, not for the algorithm."""
    n, la, lb, tol = case
    a, b = operands(n, la, lb, seed)
    dense = cnp.dense_product(a, b)
    opts = TCI2Options(tolerance=tol, max_nglobal_pivot=0, nsearch=0)
    fused = cnp.fused_dense(dense, [(2, 2)] * n)
    first = [int(v) for v in np.unravel_index(int(np.abs(fused).argmax()), fused.shape)]
    for pivots in (None, [first]):  # opt_first_pivot from the all-zero index, the arg-max of the dense product
        m = contract_tci(MPO(a), MPO(b), opts, pivots)
        assert m.link_dims() == links and m.site_dims() == [(2, 2)] * n
        info = m.tci_info
        assert info["termination"] == t4a_amd.CONVERGED and info["rank"] == max(links) and info["n_evaluations"] > 0 and info["error"] <= tol
        close(m.full_tensor(), dense, rel=1e-10)


def test_contract_tci_default_options_and_fit_stays_unimplemented():
    a, b = operands(5, 2, 2)
    ma, mb = MPO(a), MPO(b)
    m = contract_tci(ma, mb)
    assert m.link_dims() == [4, 4, 4, 4]
    close(m.full_tensor(), cnp.dense_product(a, b))
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.mpo.contract(ma, mb, t4a_amd.ContractionAlgorithm.Fit)
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED


def test_contract_tci_applies_a_shift_operator_to_a_state():
    from t4a_amd import shift_operator, BoundaryCondition
    op = shift_operator(6, 5, BoundaryCondition.Periodic).mpo()
    state = MPO(cnp.random_tensors(bonds_of(6, 4), 2, 1, SEED))
    want = contract_zipup(op, state)
    got = contract_tci(op, state)
    assert got.site_dims() == [(2, 1)] * 6 == want.site_dims()
    close(got.full_tensor(), want.full_tensor(), rel=1e-10)


# ------------------------------------------------------------------------------------------------ 8. size
def test_twelve_sites_against_the_naive_product_on_the_device():
    n = 12
    a, b = operands(n, 24, 20)
    ma, mb = MPO(a), MPO(b)
    c = Contraction(ma, mb)
    naive = contract_naive(ma, mb, None)
    assert naive.link_dims() == [480] * (n - 1)
    pts = cnp.lcg_points(4096, [[2, 2]] * n, 21)
    want = naive.evaluate(pts.reshape(len(pts), -1))
    scale = np.abs(want)
    close(c.evaluate_many(pts)[0], want, scale)
    close(c.evaluate(pts[:512]), want[:512], scale)
    rows = cnp.lcg_points(256, [[2, 2]] * (n // 2), 22)
    cols = cnp.lcg_points(256, [[2, 2]] * (n - n // 2), 23)
    outer = np.concatenate([np.repeat(rows, 256, axis=0), np.tile(cols, (256, 1, 1))], axis=1)
    assert outer.shape == (65536, n, 2)
    want = naive.evaluate(outer.reshape(len(outer), -1))
    vals, used = c.evaluate_many(outer)
    assert used == cnp.find_split(outer) == n // 2
    close(vals, want, want)
    vals, used = c.evaluate_many(outer, split=3)
    close(vals, want, want)


@pytest.mark.parametrize("bond_a, bond_b, where", [(64, 32, "inside"), (64, 33, "outside")])
def test_either_side_of_the_lds_limit(bond_a, bond_b, where):
    """The working set of a site step is 2 * la*lb + K * lb * ra doubles; 8192 of them (64 KiB) fit the LDS.  With K = 2 and equal bonds on
    both sides of a site that is 4 * la * lb: 64 x 32 is the largest pair inside, 64 x 33 the first outside, which walks through global
    scratch and gives the same values."""
    assert (4 * bond_a * bond_b <= 8192) == (where == "inside")
    n = 4
    a, b = operands(n, bond_a, bond_b)
    c = Contraction(MPO(a), MPO(b))
    ref = cnp.ContractionNP(a, b)
    pts = cnp.lcg_points(200, [[2, 2]] * n, 31)
    want = ref.evaluate(pts)
    scale = np.abs(want)
    close(c.evaluate(pts), want, scale)
    for split in (None, 1, 2, 3, 4):
        close(c.evaluate_many(pts, split=split)[0], want, scale)
    close(c.evaluate_left(2, pts[:5]), ref.evaluate_left(2, pts[:5]), scale)
    close(c.evaluate_right(2, pts[:5]), ref.evaluate_right(2, pts[:5]), scale)
