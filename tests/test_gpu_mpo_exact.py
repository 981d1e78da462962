"""The MPO and Contraction kernels (kernels_contraction.hip, kernels_mpo.hip) on integer-valued operands, every comparison exact.

With site tensors from {-1, 0, 1} and cnp.exact_bound < 2^53 every product and every partial sum is an integer that f64 holds exactly,
so the scalar branch, the matrix-core branch and the pairing kernel must all give the bits of integer arithmetic, whatever their order
of summation: the device's values are compared with np.array_equal against the int64 reference cnp.ContractionNP(..., exact=True).

What the profiles of cnp.EXACT_PROFILES reach, derived from the shapes (wg_product takes the matrix cores where its output has at
least 16 rows and 16 columns; left walk: product 1 is ra x lb summed over la, product 2 is ra x rb summed over K x lb; right walk:
product 1 is la x rb summed over ra, product 2 is la x lb summed over K x rb):

P1 (A bonds 1 17 33 16 5 20 1, B bonds 1 3 16 31 18 2 1), left walk by site:
  0: 17 x 1, 17 x 3             scalar, scalar
  1: 33 x 3 over 17 scalar,     33 x 16 over 3 cores (three tiles, edge at 33)             -> scalar then cores
  2: 16 x 16 over 33 cores,     16 x 31 over 16 cores
  3: 5 x 31, 5 x 18             both scalar because ra = 5 < 16, with lb = 31 and rb = 18
  4: 20 x 18 over 5 cores,      20 x 2 over 18 scalar                                      -> cores then scalar
  5: 1 x 2, 1 x 1               scalar, scalar
P1, right walk by site:
  5, 4: la x ... with rb = 1 / la = 5: scalar (site 4: both scalar because la = 5 < 16, with rb = 2, lb = 18)
  3: 16 x 18 over 5 cores,      16 x 31 over 18 cores
  2: 33 x 31 over 16 cores (six tiles for four wavefronts), 33 x 16 over 31 cores
  1: 17 x 16 over 33 cores,     17 x 3 over 16 scalar                                      -> cores then scalar
  0: scalar
P2 (A and B swapped), left walk: site 1: 16 x 17 over 3 and 16 x 33 over 17 on the cores; site 2: 31 x 33 over 16 (six tiles) and
  31 x 16 over 33 on the cores; site 3: 18 x 16 over 31 cores then 18 x 5 scalar; site 4: both scalar because ra = 2; right walk:
  site 4: 18 x 20 over 2 cores then 18 x 5 over 20 scalar; site 3: 31 x 5 over 18 scalar then 31 x 16 over 5 cores; site 2: 16 x 16
  over 31 and 16 x 33 over 16 on the cores; site 1: both scalar because la = 3 < 16, with rb = 33 and lb = 17.
P1_k3 / P1_k1: the same shapes with K1 = 3 and K1 = 1 in every second product and non-square sites (2, 3, 2) / (3, 1, 2).
scratch (bonds 64 x 33, three sites): the middle site needs 2 * 2112 + 2 * 33 * 64 = 8448 doubles, above the 8192 of the LDS: every
  walk through site 1 runs in global scratch, on the cores (64 x 33 over 64 and over 2 x 33: twelve tiles for four wavefronts).
stride: 16384 items on the LDS route (two per workgroup at 8192 workgroups); the scratch operands with 2100 items (1024 workgroups).
seam31 ... seam65: the pairing kernel with K ending inside the first chunk of panel 1 (33, 37), of panel 2 (65), on a panel edge (32,
  64) and one short of it (31).
naive: mpo_site_contract_kernel with site outputs from 160 to 1 047 552 elements in one launch (the binary search over job offsets),
  and with 2 125 764 + 2 * 2916 output elements, more than the 8192 * 256 threads of a launch (the grid-stride loop's second trip).
tests/test_cpu_contraction.py restates the branch table from the bonds, so an edit of a profile that loses a combination fails there."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, Contraction, contract_naive

import contraction_np as cnp

pytestmark = pytest.mark.gpu

ENV_MAX_BLOCKS = 8192          # contraction.hip: workgroups of an environment launch on the LDS route
ENV_MAX_BLOCKS_SCRATCH = 1024  # ... on the scratch route
CONTRACTION_LDS_DOUBLES = 8192  # kernels.hpp: what of a working set fits the LDS
SITE_CONTRACT_THREADS = 8192 * 256  # kernels_mpo.hip: the largest launch of mpo_site_contract_kernel


def exact(got, want, what=""):
    """the device's f64 values are integers and equal the int64 reference in every element"""
    got, want = np.asarray(got), np.asarray(want)
    assert want.dtype == np.int64 and got.dtype == np.float64, (got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, np.rint(got)), f"{what}: the device returned values that are no integers"
    as_int = got.astype(np.int64)
    if not np.array_equal(as_int, want):
        bad = np.argwhere(as_int != want)
        first = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} entries differ, first at {first}: device {got[first]!r}, "
                             f"reference {int(want[first])}; last at {tuple(int(v) for v in bad[-1])}")


def halves(n_pts, site_dims, seed):
    """n_pts LCG index halves over the given sites, (n_pts, len(site_dims), 2); halves of width 0 for no sites"""
    if not len(site_dims):
        return np.zeros((n_pts, 0, 2), dtype=np.int64)
    return cnp.lcg_points(n_pts, [list(d) for d in site_dims], seed)


def all_pairs(site_dims):
    """every index tuple over the given sites, (total, len(site_dims), 2), the first index slowest"""
    shape = [d for pair in site_dims for d in pair]
    return np.indices(shape).reshape(len(shape), -1).T.reshape(-1, len(site_dims), 2)


class Case:
    def __init__(self, name):
        self.name = name
        self.a, self.b = cnp.exact_operands(name)
        # a later edit of a profile must not make the comparison inexact without anybody noticing
        assert cnp.exact_bound(self.a, self.b) < 2 ** 53, (name, cnp.exact_bound(self.a, self.b))
        self.n = len(self.a)
        self.c = Contraction(MPO(self.a), MPO(self.b))
        self.ref = cnp.ContractionNP(self.a, self.b, exact=True)
        self.dims = self.c.result_site_dims()
        assert self.dims == self.ref.site_dims
        self.pts = cnp.lcg_points(40, [list(d) for d in self.dims], 99)
        self.pts.setflags(write=False)
        self._want = None

    def want(self):
        """the reference values of the 40 points, computed once"""
        if self._want is None:
            self._want = self.ref.evaluate(self.pts)
            self._want.setflags(write=False)
            assert np.abs(self._want).max() > 1, "a degenerate profile: nothing but 0 and +-1"
        return self._want


@pytest.fixture(scope="module", params=["P1", "P2", "P1_k3", "P1_k1", "scratch"])
def case(request):
    return Case(request.param)


# ------------------------------------------------------------------------------------------------ 1. environments, evaluate, evaluate_many, matrices
def test_environments_at_every_cut(case):
    for cut in range(case.n + 1):
        want_l, want_r = case.ref.evaluate_left(cut, case.pts), case.ref.evaluate_right(cut, case.pts)
        assert want_l.shape == (40,) + ((1, 1) if cut == 0 else (case.a[cut - 1].shape[3], case.b[cut - 1].shape[3]))
        assert want_r.shape == (40,) + ((1, 1) if cut == case.n else (case.a[cut].shape[0], case.b[cut].shape[0]))
        exact(case.c.evaluate_left(cut, case.pts), want_l, f"{case.name} evaluate_left({cut})")
        exact(case.c.evaluate_right(cut, case.pts), want_r, f"{case.name} evaluate_right({cut})")


def test_evaluate(case):
    exact(case.c.evaluate(case.pts), case.want(), f"{case.name} evaluate")
    one = case.c.evaluate([tuple(int(v) for v in p) for p in case.pts[7]])
    assert isinstance(one, float) and one == float(case.want()[7])


def test_evaluate_many_for_every_split(case):
    pts = np.array(case.pts)
    pts[17] = pts[3]  # duplicate points
    want = np.array(case.want())
    want[17] = want[3]
    for split in range(1, case.n + 1):
        vals, used = case.c.evaluate_many(pts, split=split)
        assert used == split
        exact(vals, want, f"{case.name} evaluate_many(split={split})")
    vals, used = case.c.evaluate_many(pts)
    assert used == cnp.find_split(pts)
    exact(vals, want, f"{case.name} evaluate_many(split=None)")


def test_evaluate_matrix_at_every_cut(case):
    for cut in range(case.n + 1):
        rows, cols = halves(33, case.dims[:cut], 41 + cut), halves(65, case.dims[cut:], 42 + cut)
        got = case.c.evaluate_matrix(cut, rows, cols)
        assert got.shape == (33, 65)
        exact(got, case.ref.evaluate_matrix(cut, rows, cols), f"{case.name} evaluate_matrix(cut={cut})")


# ------------------------------------------------------------------------------------------------ 2. grid-stride walks
def test_grid_stride_walk_on_the_lds_route():
    """16384 items for at most 8192 workgroups: every workgroup walks two items, and the seven sites of a walk leave the cur / nxt
    buffers swapped for the second one."""
    a, b = cnp.exact_operands("stride")
    assert cnp.exact_bound(a, b) < 2 ** 53
    n = len(a)
    ba, bb, (_, k, _) = cnp.EXACT_PROFILES["stride"]
    assert 2 * max(x * y for x, y in zip(ba, bb)) + k * max(ba) * max(bb) <= CONTRACTION_LDS_DOUBLES and n % 2 == 1
    c, ref = Contraction(MPO(a), MPO(b)), cnp.ContractionNP(a, b, exact=True)
    pts = all_pairs([(2, 2)] * n)
    assert len(pts) == 4 ** 7 == 2 * ENV_MAX_BLOCKS
    want = ref.evaluate(pts)
    assert not np.array_equal(want[:ENV_MAX_BLOCKS], want[ENV_MAX_BLOCKS:]) and np.abs(want).max() > 1
    for what, got in (("evaluate", c.evaluate(pts)), ("evaluate_left(7)", c.evaluate_left(n, pts)[:, 0, 0]),
                      ("evaluate_right(0)", c.evaluate_right(0, pts)[:, 0, 0])):
        exact(got[ENV_MAX_BLOCKS:], want[ENV_MAX_BLOCKS:], f"stride {what}, the second trip")
        exact(got, want, f"stride {what}")
    # the right walk of the last three sites alone: an odd number of swaps again, a 2 x 3 environment per item
    exact(c.evaluate_right(n - 3, pts), ref.evaluate_right(n - 3, pts), "stride evaluate_right(4)")


def test_grid_stride_walk_on_the_scratch_route():
    """2100 items for 1024 workgroups whose working sets are slices of global scratch: two or three items per workgroup, the last
    trip taken by 52 workgroups only; neighbouring trips of a workgroup walk different tuples."""
    a, b = cnp.exact_operands("scratch")
    assert cnp.exact_bound(a, b) < 2 ** 53
    c, ref = Contraction(MPO(a), MPO(b)), cnp.ContractionNP(a, b, exact=True)
    tuples = all_pairs([(2, 2)] * 3)
    assert len(tuples) == 64
    n_pts = 2100
    assert n_pts % ENV_MAX_BLOCKS_SCRATCH != 0 and n_pts > 2 * ENV_MAX_BLOCKS_SCRATCH
    order = (np.arange(n_pts) * 5 + np.arange(n_pts) // ENV_MAX_BLOCKS_SCRATCH) % 64
    assert (order[:n_pts - ENV_MAX_BLOCKS_SCRATCH] != order[ENV_MAX_BLOCKS_SCRATCH:]).all() and len(set(order.tolist())) == 64
    want = ref.evaluate(tuples)[order]
    got = c.evaluate(tuples[order])
    exact(got[ENV_MAX_BLOCKS_SCRATCH:], want[ENV_MAX_BLOCKS_SCRATCH:], "scratch evaluate, the later trips")
    exact(got, want, "scratch evaluate")


# ------------------------------------------------------------------------------------------------ 3. the pairing kernel around its K panels
@pytest.mark.parametrize("bond_a, bond_b", cnp.PAIR_SEAMS)
def test_pairing_kernel_k_seams(bond_a, bond_b):
    name = f"seam{bond_a * bond_b}"
    a, b = cnp.exact_operands(name)
    assert cnp.exact_bound(a, b) < 2 ** 53 and a[1].shape[0] * b[1].shape[0] == bond_a * bond_b
    c, ref = Contraction(MPO(a), MPO(b)), cnp.ContractionNP(a, b, exact=True)
    dims = c.result_site_dims()
    rows, cols = all_pairs(dims[:1]), all_pairs(dims[1:])
    assert len(rows) == len(cols) == 9
    want = ref.evaluate_matrix(1, rows, cols)
    assert np.abs(want).max() > 1
    exact(c.evaluate_matrix(1, rows, cols), want, f"{name} every half")
    exact(c.evaluate_matrix(1, rows[4:5], cols[7:8]), want[4:5, 7:8], f"{name} 1 x 1")
    r17, c3 = halves(17, dims[:1], 51), halves(3, dims[1:], 52)
    exact(c.evaluate_matrix(1, r17, c3), ref.evaluate_matrix(1, r17, c3), f"{name} 17 x 3")
    full = np.concatenate([np.repeat(rows, 9, axis=0), np.tile(cols, (9, 1, 1))], axis=1)
    exact(c.evaluate_many(full, split=1)[0].reshape(9, 9), want, f"{name} evaluate_many")  # tt_env_dot over the same K


# ------------------------------------------------------------------------------------------------ 4. the naive product
@pytest.mark.parametrize("name", ["P1", "P2", "naive27"])
def test_naive_product_site_tensors(name):
    a, b = cnp.exact_operands(name)
    assert cnp.exact_bound(a, b) < 2 ** 53
    want = [cnp.np_site(x.astype(np.int64), y.astype(np.int64)) for x, y in zip(a, b)]
    sizes = [w.size for w in want]
    if name == "naive27":
        assert max(sizes) == 2125764 > SITE_CONTRACT_THREADS and sum(sizes) > SITE_CONTRACT_THREADS
    else:
        assert min(sizes) == 160 and sizes[0] == 204 and max(sizes) == 1047552 and sum(sizes) <= SITE_CONTRACT_THREADS
    r = contract_naive(MPO(a), MPO(b))
    assert r.link_dims() == [w.shape[0] for w in want[1:]]
    for s, w in enumerate(want):
        exact(r.site_tensor(s), w, f"{name} site {s}")
