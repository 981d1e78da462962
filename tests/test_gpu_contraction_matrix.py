"""Candidate matrices of the lazy MPO product filled on the device: Contraction.evaluate_matrix (two environment launches and the pairing
kernel of kernels_contraction.hip), the contraction as the device matrix source of a TensorCI2, and contract_tci(..., route="device").
Values are compared with the dense product / the numpy restatement tests/contraction_np.py at 1e-10 relative to max(1, max|dense|), the
tolerance tests/test_gpu_contraction.py states for this layer; shapes, ranks, counters and bit identities exactly."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, Contraction, contract_tci, contract_zipup, TCI2Options, TensorCI2

import contraction_np as cnp

pytestmark = pytest.mark.gpu

SEED = cnp.SEED
INV = t4a_amd.INVALID_ARGUMENT


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


def all_halves(site_dims):
    """every index half over the given sites, (total, len(site_dims), 2); one empty half for no sites"""
    shape = [d for pair in site_dims for d in pair]
    if not shape:
        return np.zeros((1, 0, 2), dtype=np.int64)
    grid = np.indices(shape).reshape(len(shape), -1).T
    return grid.reshape(-1, len(site_dims), 2)


def dense_block(dense, rows, cols):
    """dense[rows[r] + cols[c]] as an (n_rows, n_cols) array"""
    full = np.concatenate([np.repeat(rows, len(cols), axis=0), np.tile(cols, (len(rows), 1, 1))], axis=1)
    return dense[tuple(full.reshape(len(full), -1).T)].reshape(len(rows), len(cols))


def restated_block(ref, cut, rows, cols):
    """the numpy restatement: left environments of the rows times right environments of the columns"""
    full_l = np.zeros((len(rows), ref.n, 2), dtype=np.int64)
    full_l[:, :cut] = rows
    full_r = np.zeros((len(cols), ref.n, 2), dtype=np.int64)
    full_r[:, cut:] = cols
    left = ref.evaluate_left(cut, full_l).reshape(len(rows), -1)
    right = ref.evaluate_right(cut, full_r).reshape(len(cols), -1)
    return left @ right.T


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. the dense product, every cut
def check_every_cut(a, b):
    c = Contraction(MPO(a), MPO(b))
    dims = c.result_site_dims()
    n = len(dims)
    dense = cnp.dense_product(a, b)
    before = c.n_evaluated()
    for cut in range(n + 1):
        rows, cols = all_halves(dims[:cut]), all_halves(dims[cut:])
        got = c.evaluate_matrix(cut, rows, cols)
        assert got.shape == (len(rows), len(cols)) and got.flags["C_CONTIGUOUS"]
        close(got, dense_block(dense, rows, cols), dense)
    assert c.n_evaluated() - before == (n + 1) * dense.size


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("bond_a, bond_b", [(1, 1), (2, 3), (5, 3), (20, 17)])  # K = la * lb: 1, 6, 15 (no multiple of 4), 340
def test_evaluate_matrix_gives_the_dense_product_at_every_cut(n, bond_a, bond_b):
    check_every_cut(*operands(n, bond_a, bond_b))


@pytest.mark.parametrize("dims", [(2, 3, 2), (3, 2, 1)])
def test_evaluate_matrix_with_non_square_site_dims(dims):
    s1, k, s2 = dims
    check_every_cut(*operands(4, 5, 3, s1=s1, k=k, s2=s2))


# ------------------------------------------------------------------------------------------------ 2. tile edges, 3. shape independence
@pytest.fixture(scope="module")
def edge_case():
    n, cut = 8, 4
    a, b = operands(n, 5, 4)
    ref = cnp.ContractionNP(a, b)
    rows = cnp.lcg_points(33, [[2, 2]] * cut, 41)       # a shorter list is a prefix of a longer one: the same generator
    cols = cnp.lcg_points(65, [[2, 2]] * (n - cut), 42)
    want = restated_block(ref, cut, rows, cols)
    want.setflags(write=False)
    scale = float(np.abs(cnp.dense_product(a, b)).max())
    return Contraction(MPO(a), MPO(b)), cut, rows, cols, want, scale


@pytest.mark.parametrize("n_cols", [1, 16, 17, 65])
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 33])
def test_tile_edges(edge_case, n_rows, n_cols):
    c, cut, rows, cols, want, scale = edge_case
    got = c.evaluate_matrix(cut, rows[:n_rows], cols[:n_cols])
    close(got, want[:n_rows, :n_cols], [scale])


def test_the_bits_of_an_entry_do_not_depend_on_the_request(edge_case):
    c, cut, rows, cols, want, scale = edge_case
    full = c.evaluate_matrix(cut, rows, cols)
    assert full.shape == (33, 65)
    assert np.array_equal(bits(full), bits(c.evaluate_matrix(cut, rows, cols))), "two identical calls differ"
    single = np.array([[c.evaluate_matrix(cut, rows[r:r + 1], cols[q:q + 1])[0, 0] for q in range(65)] for r in range(33)])
    assert np.array_equal(bits(full), bits(single)), "an entry computed alone differs from the entry in the 33 x 65 matrix"
    sub = c.evaluate_matrix(cut, rows[16:33], cols[:16])
    assert sub.shape == (17, 16) and np.array_equal(bits(sub), bits(full[16:33, :16])), "the 17 x 16 sub-request differs"
    rev = c.evaluate_matrix(cut, rows[::-1], cols)
    assert np.array_equal(bits(rev), bits(full[::-1])), "the request with reversed rows differs"


# ------------------------------------------------------------------------------------------------ 4. the LDS limit of the environments
@pytest.mark.parametrize("bond_a, bond_b, where", [(64, 32, "inside"), (64, 33, "outside")])
def test_either_side_of_the_lds_limit(bond_a, bond_b, where):
    """the shapes of test_gpu_contraction.py::test_either_side_of_the_lds_limit: 64 x 33 walks the environments through global scratch"""
    assert (4 * bond_a * bond_b <= 8192) == (where == "inside")
    n = 4
    a, b = operands(n, bond_a, bond_b)
    c = Contraction(MPO(a), MPO(b))
    ref = cnp.ContractionNP(a, b)
    for cut in (1, 2, 3):
        rows = cnp.lcg_points(20, [[2, 2]] * cut, 31)
        cols = cnp.lcg_points(20, [[2, 2]] * (n - cut), 32)
        want = restated_block(ref, cut, rows, cols)
        close(c.evaluate_matrix(cut, rows, cols), want, np.abs(want))


# ------------------------------------------------------------------------------------------------ 5. errors
def raises(code, needle, call):
    with pytest.raises(t4a_amd.T4aError) as e:
        call()
    assert e.value.code == code and needle in e.value.message, e.value


def test_errors_carry_the_messages_of_evaluate_many():
    a3 = MPO(cnp.random_tensors(bonds_of(3, 2), 2, 2, SEED))
    c = Contraction(a3, MPO(cnp.random_tensors(bonds_of(3, 3), 2, 3, SEED)))  # result site dims (2, 3)
    r1, c2 = [[(0, 0)]], [[(1, 2), (1, 1)]]
    assert c.evaluate_matrix(1, r1, c2).shape == (1, 1)
    before = c.n_evaluated()
    raises(INV, "Index out of bounds: index 2 at site 0 (max: 3)", lambda: c.evaluate_matrix(1, [[(2, 0)]], c2))
    raises(INV, "Index out of bounds: index 3 at site 1 (max: 3)", lambda: c.evaluate_matrix(1, r1, [[(0, 3), (0, 0)]]))
    raises(INV, "Index out of bounds: index 3 at site 2 (max: 3)", lambda: c.evaluate_matrix(2, [[(0, 0), (0, 0)]], [[(0, 3)]]))
    raises(INV, "Invalid split position: 4 (n_sites=3)", lambda: c.evaluate_matrix(4, r1, c2))
    raises(INV, "Expected 1 index pairs, got 2", lambda: c.evaluate_matrix(1, c2, c2))
    raises(INV, "Expected 2 index pairs, got 1", lambda: c.evaluate_matrix(1, r1, r1))
    raises(INV, "Expected 0 index pairs, got 1", lambda: c.evaluate_matrix(0, r1, [[(0, 0), (1, 2), (1, 1)]]))
    raises(INV, "negative index", lambda: c.evaluate_matrix(1, [[(-1, 0)]], c2))
    raises(INV, "MPO is empty", lambda: Contraction(MPO([]), MPO([])).evaluate_matrix(0, np.zeros((1, 0, 2)), np.zeros((1, 0, 2))))
    assert c.n_evaluated() == before
    empty = c.evaluate_matrix(1, np.zeros((0, 1, 2), dtype=int), c2)
    assert empty.shape == (0, 1)
    empty = c.evaluate_matrix(1, r1, np.zeros((0, 2, 2), dtype=int))
    assert empty.shape == (1, 0) and c.n_evaluated() == before


def test_the_transform_is_applied_to_the_matrix():
    a, b = operands(4, 2, 3)
    plain = Contraction(MPO(a), MPO(b))
    sq = Contraction.with_transform(MPO(a), MPO(b), lambda v: v * v)
    rows, cols = all_halves([(2, 2)] * 2), all_halves([(2, 2)] * 2)
    assert np.array_equal(sq.evaluate_matrix(2, rows, cols), plain.evaluate_matrix(2, rows, cols) ** 2)


# ------------------------------------------------------------------------------------------------ 6. a TensorCI2 fed by the source
def same_bits(g, h):
    n = len(g.local_dims)
    for p in range(n):
        assert np.array_equal(g.i_set(p), h.i_set(p)) and np.array_equal(g.j_set(p), h.j_set(p)), f"index sets differ at {p}"
        assert np.array_equal(g.site_tensor(p).view(np.uint64), h.site_tensor(p).view(np.uint64)), f"site tensor {p} differs"
    assert np.array_equal(g.pivot_errors().view(np.uint64), h.pivot_errors().view(np.uint64))
    assert g.history()[0] == h.history()[0] and np.array_equal(g.history()[1].view(np.uint64), h.history()[1].view(np.uint64))
    assert g.link_dims() == h.link_dims() and g.termination() == h.termination()


@pytest.fixture(scope="module")
def eight_sites():
    """the setup of test_gpu_contraction.py::test_native_callback_and_python_callable_give_the_same_bits"""
    n = 8
    a, b = operands(n, 6, 6)
    ref = cnp.ContractionNP(a, b)
    dense = cnp.fused_dense(cnp.dense_product(a, b), ref.site_dims)
    dense.setflags(write=False)
    first = [int(v) for v in np.unravel_index(int(np.abs(dense).argmax()), dense.shape)]
    links = [min(4 ** (k + 1), 36, 4 ** (n - k - 1)) for k in range(n - 1)]
    return a, b, ref.fused_dims(), dense, first, links


def run_source(a, b, dims, first, opts):
    c = Contraction(MPO(a), MPO(b))
    g = TensorCI2(dims)
    g.set_contraction_source(c)
    g.crossinterpolate2([first], opts)
    return g, c


def check_source_run(g, c, dense, links):
    assert g.link_dims() == links and g.termination() == t4a_amd.CONVERGED
    grid = cnp.lcg_points(2000, list(dense.shape), 3)
    close(g.evaluate(grid), dense[tuple(grid.T)], dense)
    stats = g.source_stats()
    print("source stats", stats, "evaluated", c.n_evaluated())
    assert stats["matrices"] > 0 and stats["entries"] > 0
    assert stats["entries"] + stats["host_entries"] == c.n_evaluated()
    return stats


def test_tensorci2_with_a_contraction_source(eight_sites):
    a, b, dims, dense, first, links = eight_sites
    opts = TCI2Options(tolerance=1e-10, max_nglobal_pivot=0, nsearch=0)
    g, c = run_source(a, b, dims, first, opts)
    check_source_run(g, c, dense, links)
    h, c2 = run_source(a, b, dims, first, opts)
    same_bits(g, h)
    assert c2.n_evaluated() == c.n_evaluated() and h.source_stats() == g.source_stats()


def test_source_beside_the_global_pivot_search(eight_sites):
    a, b, dims, dense, first, links = eight_sites
    g, c = run_source(a, b, dims, first, TCI2Options(tolerance=1e-10, max_nglobal_pivot=5, nsearch=5, seed=7))
    stats = check_source_run(g, c, dense, links)
    plain, _ = run_source(a, b, dims, first, TCI2Options(tolerance=1e-10, max_nglobal_pivot=0, nsearch=0))
    assert stats["host_entries"] > plain.source_stats()["host_entries"] > 0  # the searches went through the host point evaluator


def test_source_with_the_rook_search(eight_sites):
    """pivot_search == 1 asks for single rows and columns of a candidate matrix: they stay on the host evaluator (t4a_gpu.h), the
    matrices of fill_site_tensors come from the source"""
    a, b, dims, dense, first, links = eight_sites
    g, c = run_source(a, b, dims, first, TCI2Options(tolerance=1e-10, max_nglobal_pivot=0, nsearch=0, pivot_search=1))
    check_source_run(g, c, dense, links)


# ------------------------------------------------------------------------------------------------ 7. contract_tci(route="device")
TCI_CASES = [((5, 2, 2, 1e-10), [4, 4, 4, 4]), ((6, 2, 3, 1e-10), [4, 6, 6, 6, 4]), ((5, 3, 3, 1e-10), [4, 9, 9, 4]),
             ((6, 2, 2, 1e-12), [4, 4, 4, 4, 4])]


@pytest.mark.parametrize("seed", [SEED, 12345])
@pytest.mark.parametrize("case, links", TCI_CASES)
def test_contract_tci_on_the_device_route(case, links, seed):
    n, la, lb, tol = case
    a, b = operands(n, la, lb, seed)
    dense = cnp.dense_product(a, b)
    opts = TCI2Options(tolerance=tol, max_nglobal_pivot=0, nsearch=0)
    fused = cnp.fused_dense(dense, [(2, 2)] * n)
    first = [int(v) for v in np.unravel_index(int(np.abs(fused).argmax()), fused.shape)]
    for pivots in (None, [first]):
        m = contract_tci(MPO(a), MPO(b), opts, pivots, route="device")
        assert m.link_dims() == links and m.site_dims() == [(2, 2)] * n
        info = m.tci_info
        assert info["termination"] == t4a_amd.CONVERGED and info["rank"] == max(links) and info["n_evaluations"] > 0 and info["error"] <= tol
        close(m.full_tensor(), dense, rel=1e-10)
        # the host route is what it was: the default, and the same bits when named
        host = contract_tci(MPO(a), MPO(b), opts, pivots)
        named = contract_tci(MPO(a), MPO(b), opts, pivots, route="host")
        assert host.link_dims() == links and host.tci_info == named.tci_info
        assert np.array_equal(bits(host.full_tensor()), bits(named.full_tensor()))
        close(host.full_tensor(), dense, rel=1e-10)


def test_contract_tci_device_applies_a_shift_operator_to_a_state():
    from t4a_amd import shift_operator, BoundaryCondition
    op = shift_operator(6, 5, BoundaryCondition.Periodic).mpo()
    state = MPO(cnp.random_tensors(bonds_of(6, 4), 2, 1, SEED))
    want = contract_zipup(op, state)
    got = contract_tci(op, state, route="device")
    assert got.site_dims() == [(2, 1)] * 6 == want.site_dims()
    close(got.full_tensor(), want.full_tensor(), rel=1e-10)


# ------------------------------------------------------------------------------------------------ 10. argument checks
def test_argument_checks():
    a, b = operands(5, 2, 3)
    c = Contraction(MPO(a), MPO(b))
    raises(INV, "length mismatch", lambda: TensorCI2([4] * 4).set_contraction_source(c))
    raises(INV, "local dimension mismatch at site 2", lambda: TensorCI2([4, 4, 2, 4, 4]).set_contraction_source(c))
    sq = Contraction.with_transform(MPO(a), MPO(b), lambda v: v * v)
    raises(INV, "transform", lambda: TensorCI2([4] * 5).set_contraction_source(sq))
    raises(INV, "unknown route", lambda: contract_tci(MPO(a), MPO(b), route="gpu"))
    raises(INV, "unknown route", lambda: contract_tci(MPO(a), MPO(b), route=None))
    g = TensorCI2([4] * 5)
    assert g.source_stats() == {"matrices": 0, "entries": 0, "host_entries": 0}
    g.set_contraction_source(c)  # a fitting source is accepted, and replaced by a callback again
    g.set_callback_raw(*c.as_callback())
    g.crossinterpolate2([[0] * 5], TCI2Options(tolerance=1e-10, max_nglobal_pivot=0, nsearch=0))
    assert g.source_stats()["matrices"] == 0 and g.source_stats()["host_entries"] == c.n_evaluated() > 0
