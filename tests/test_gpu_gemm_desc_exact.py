"""The GEMM under every layer (csrc/kernels_dense.hip gemm_launch, gemm_kernel, gemm_splitk_reduce_kernel) on whole descriptors, against
answers that are exact by construction.

mat_mul and batched_mat_mul_same_shape reach the kernel with one descriptor: plain A B, dense leading dimensions and strides, alpha = 1,
beta = 0.  The layers above use all of it -- one transpose, alpha = -1 with beta = 1, leading dimensions above the operand, zero strides
for a shared operand, and split-K behind their back.  Here every option runs on every launch route through the test hook gemm_desc:

- operands are integers in [-3, 3], alpha in {1, -1, 2, 1/2}, beta in {0, 1, -1, 1/4}, C integers in [-8, 8]: every partial sum is a
  multiple of 1/8 below 2^53 in magnitude (k <= 1000: |sum| <= 9000 |alpha| + 8 |beta|), so every summation order, slice split and MFMA
  association returns the same bits and the assertion is equality;
- padding rows, gaps between problems, the regions before the first and behind the last result hold a NaN with a fixed payload and must
  come back bit for bit; with beta == 0 the result region itself holds it, and must come back finite: C is not read then; the padding
  of A and B holds it too, so an operand read from outside its matrix poisons the result;
- each case asserts its route first (tests/gemm_desc_np.py GPU_ROWS, the table of tests/test_cpu_gemm_desc.py).
"""
import numpy as np
import pytest

import gemm_desc_np as gd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def _assert_route(t4a, shape, route):
    got = t4a.gemm_route(*shape)
    assert tuple(got[key] for key in gd.ROUTE_KEYS) == route, (shape, got)


def _seed(shape, i):
    return [*shape, i]


SPLIT_CHAIN = [(64, 32, 256, 1), (70, 70, 321, 5), (64, 64, 512, 1), (64, 32, 256, 1)]


def test_back_to_back_split_products_share_and_grow_the_workspace(t4a):
    """Four split-K products queued in one call with no synchronisation between them: workspaces of 4 x 2048, 25 x 4900, 8 x 4096 and
    again 4 x 2048 doubles.  The per-stream workspace is reused by a product while its predecessor may still be running, and replaced by
    a larger block behind work in flight.  (The workspace only ever grows and lives as long as the process: this call grows
    it at its second product when no larger split product ran on the stream before -- this file alone, the soak.  In the whole suite
    earlier files have grown it already, and the call pins the reuse alone.)  All four results are exact."""
    rows = {shape: route for shape, route, _ in gd.GPU_ROWS}
    descs, bufs = [], []
    off = [0, 0, 0]
    for i, shape in enumerate(SPLIT_CHAIN):
        _assert_route(t4a, shape, rows[shape])
        assert rows[shape][1] > 1
        (ta, tb), (alpha, beta) = gd.TRANS[i], gd.ALPHA_BETA[(i + 1) % 4]
        d, sizes = gd.make_desc(*shape, ta, tb, alpha, beta, True, "cpad" if shape[3] > 1 else "dense")
        a, b, c = gd.fill_case(np.random.default_rng(_seed(shape, 100 + i)), d, sizes)
        bufs.append((a, b, c))
        d = dict(d, off_a=d["off_a"] + off[0], off_b=d["off_b"] + off[1], off_c=d["off_c"] + off[2])
        descs.append((d, tuple(off)))
        off = [off[0] + sizes[0], off[1] + sizes[1], off[2] + sizes[2]]
    a, b, c = (np.concatenate([t[q] for t in bufs]) for q in range(3))
    got = t4a.gemm_desc([d for d, _ in descs], a, b, c)
    want = c.copy()
    for d, _ in descs:  # (the results are disjoint: each product of the reference starts from the buffer its predecessors left)
        want = gd.gemm_desc_ref(d, a, b, want)
    union = np.zeros(c.size, dtype=bool)
    for i, (d, _) in enumerate(descs):
        mask = gd.c_mask(d, c.size)
        assert not (mask & union).any()
        assert np.all(np.isfinite(got[mask])) and np.array_equal(got[mask], want[mask]), (i, SPLIT_CHAIN[i], int((got[mask] != want[mask]).sum()))
        union |= mask
    assert np.array_equal(got.view(np.uint64)[~union], c.view(np.uint64)[~union])


ROW_IDS = ["x".join(str(v) for v in shape) for shape, _, _ in gd.GPU_ROWS]


@pytest.mark.parametrize("shape,route,what", gd.GPU_ROWS, ids=ROW_IDS)
def test_every_option_on_every_route_is_exact(t4a, shape, route, what):
    """all four transposes x four (alpha, beta) x dense / odd-padded leading dimensions on an unbatched row; on a batched row the fixed
    selection of gemm_desc_np.row_cases over those and the stride modes (zero stride_a, zero stride_b, both, padded strides): every
    value of every option occurs there, not every pairing of two options"""
    _assert_route(t4a, shape, route)
    for i, ((ta, tb), (alpha, beta), pad, mode) in enumerate(gd.row_cases(shape)):
        d, sizes = gd.make_desc(*shape, ta, tb, alpha, beta, pad, mode)
        a, b, c = gd.fill_case(np.random.default_rng(_seed(shape, i)), d, sizes)
        got = t4a.gemm_desc([d], a, b, c)
        problem = gd.check_exact(d, c, got, gd.gemm_desc_ref(d, a, b, c))
        assert problem is None, (shape, what, (ta, tb), (alpha, beta), pad, mode, problem)


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.25])
def test_an_empty_sum_scales_c(t4a, beta):
    """k == 0 goes to the kernel as it stands: C = beta C exactly (zeros for beta == 0, without reading C), the padding untouched"""
    for shape in ((5, 3, 0, 1), (70, 40, 0, 3)):
        for ta, tb in gd.TRANS:
            d, sizes = gd.make_desc(*shape, ta, tb, -1.0, beta, True, "cpad" if shape[3] > 1 else "dense")
            a, b, c = gd.fill_case(np.random.default_rng(_seed(shape, ta + 2 * tb)), d, sizes)
            assert (beta == 0.0) == bool(np.isnan(c[d["off_c"]]))
            got = t4a.gemm_desc([d], a, b, c)
            want = c.copy()
            mask = gd.c_mask(d, c.size)
            want[mask] = beta * c[mask] if beta != 0.0 else 0.0
            problem = gd.check_exact(d, c, got, want)
            assert problem is None, (shape, ta, tb, problem)


# rows 2, 9 and 10 of the routes (counted without the batch-3 copy of row 2), and the split, remapped row 11 beside them
REAL_ROWS = [gd.GPU_ROWS[i] for i in (1, 9, 10, 11)]
assert [r[0] for r in REAL_ROWS] == [(70, 40, 33, 1), (64, 64, 512, 1), (70, 70, 321, 5), (100, 100, 289, 1)]


@pytest.mark.parametrize("trans", gd.TRANS, ids=["nn", "tn", "nt", "tt"])
@pytest.mark.parametrize("shape,route,what", REAL_ROWS, ids=["x".join(str(v) for v in r[0]) for r in REAL_ROWS])
def test_real_operands_within_the_derived_bound(t4a, shape, route, what, trans):
    """Uniform operands in [-1, 1], alpha = -1, beta = 1, every transpose, against the tight restatement, componentwise:
        |got - value| <= (k + 19) 2^-53 (|op A| |op B| + |C|).
    Derivation (first order in u = 2^-53, the standard model of a rounded operation; nothing here is measured): an element is a chain of
    k fused multiply-adds, each rounding once -- the products themselves are not rounded -- which perturbs the sum by at most k u times
    sum |a| |b|, split over slices or not (a slice's chain is shorter by what the other slices take); the reduce pass adds at most 16
    slices in order, 16 u more; alpha s, beta c and their sum are one rounding each, 3 u -- together (k + 19) u of the magnitude
    |alpha| sum |a| |b| + |beta| |c|.  The restatement itself is good to k 2^-64 of it, a thousandth of one u."""
    _assert_route(t4a, shape, route)
    m, n, k, batch = shape
    (ta, tb), i = trans, gd.TRANS.index(trans)
    d, sizes = gd.make_desc(m, n, k, batch, ta, tb, -1.0, 1.0, True, "cpad" if batch > 1 else "dense")
    a, b, c = gd.fill_case(np.random.default_rng(_seed(shape, 200 + i)), d, sizes, real=True)
    got = t4a.gemm_desc([d], a, b, c)
    value, mag = gd.gemm_desc_ref(d, a, b, c, mode="tight")
    mask = gd.c_mask(d, c.size)
    assert np.array_equal(got.view(np.uint64)[~mask], c.view(np.uint64)[~mask])
    err = np.abs(got[mask].astype(np.longdouble) - value[mask])
    bound = np.longdouble((k + 19) * 2.0 ** -53) * mag[mask]
    print(f"{shape} trans {ta}{tb}: largest error / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), (shape, ta, tb, float((err / bound).max()))


@pytest.mark.parametrize("shape", [(256, 128, 70, 1), (70, 70, 321, 5)], ids=["unsplit", "split"])
def test_the_same_descriptor_twice_gives_the_same_bits(t4a, shape):
    """real operands (on integers every order agrees): the slices of a split product are summed in a fixed order"""
    assert (t4a.gemm_route(*shape)["ksplit"] > 1) == (shape == (70, 70, 321, 5))
    d, sizes = gd.make_desc(*shape, 1, 0, -1.0, 1.0, True, "dense" if shape[3] == 1 else "cpad")
    a, b, c = gd.fill_case(np.random.default_rng(_seed(shape, 300)), d, sizes, real=True)
    first = t4a.gemm_desc([d], a, b, c)
    second = t4a.gemm_desc([d], a, b, c)
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    # ... and inside one call: the second product of the pair starts from the same C (a copy behind the first)
    d2 = dict(d, off_c=d["off_c"] + c.size)
    both = t4a.gemm_desc([d, d2], a, b, np.concatenate([c, c]))
    assert np.array_equal(both[:c.size].view(np.uint64), first.view(np.uint64))
    assert np.array_equal(both[c.size:].view(np.uint64), first.view(np.uint64))
