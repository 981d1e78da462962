"""fill_site_tensors VALUES on ragged batches of pivot matrices, against answers that are exact by construction.

Tci2::fill_run (csrc/tci2_fill.hip) puts the pivot matrices of all sites into ONE LuProblem table and hands max_n and max_nrhs over the
sites to lu_solve_blocked_launch / lu_forward_blocked_launch / lu_batched_launch / trsm_left_batched_launch: the route family, the panel
width, the tile count of lu_update_kernel, the chunk width of lu_solve_kernel and the trsm kernel all come from the LARGEST site, and every
smaller problem relies on the guards inside the kernels (kb >= n, c0 >= nrhs, item / tiles, partial tiles, info == -1).
test_gpu_dense_exact.py runs the same kernels with one problem per launch; test_gpu_fill.py compares fills with fills.  Here the chains
of fill_exact_np.py go through set_index_set and ONE fill_site_tensors, and every site_tensor must equal the construction:

  dims                 bonds               max_n / max_nrhs   route family of the whole batch (fill_exact_np.fill_route)
  [3, 2, 2, 12]        [3, 5, 2]           5 / 10             blocked LU nb 32, scalar trsm (max_nrhs < 16)
  [8, 6, 4, 3, 80]     [3, 17, 9, 5]       17 / 68            blocked LU nb 32, scalar trsm (max_n < 32)
  [8, 6, 4, 3, 80]     [3, 17, 40, 5]      40 / 68            fused lu_solve_kernel, nb 32: one full and one partial panel beside 3, 5, 17
  [40, 12, 4, 4, 160]  [33, 300, 64, 7]    300 / 1200         fused lu_solve_kernel, nb 16
  [64, 64, 8, 6, 64]   [9, 530, 40, 2]     530 / 4240         blocked LU nb 8, matrix-core trsm
  [64, 20, 40, 120]    [60, 1030, 20]      1030 / 41200       lu_kernel and two matrix-core trsm (1025 is the first size of this route)

- small=False: np.array_equal on every core (every partial sum a multiple of 1/4 below 2^53: fill_exact_np.assert_bit_budget);
- a zero pivot matrix in the middle of the batch, at a small and at the largest site: that core all zeros, every other core exact;
- small=True (multipliers ~1e-9: any pivot other than the column maximum inflates the error by ~1e9): per solved site forward error
  <= 4 n eps kappa_inf(A_b) with kappa < 1e3 and longdouble backward error <= 2 n eps, n = bonds[b]; the last core exact;
- a repeated, a sharded and a grouped fill, each against the construction;
- the built-in functor on a linear chain: [3, 5, 7, 4, 2, 6] runs fill_small_kernel, [3, 5, 300, 4, 2, 6] the general route with
  pi_eval_batched_kernel on a job of N = 600 beside jobs of N = 2 .. 12 (beyond the launcher's cap of 512 on gridDim.y: a second trip
  of the column loop, and `j < jb.N` as the only guard of the narrow jobs; every job has at most 12 rows, so the whole-block return
  `blockIdx.x * blockDim.x >= jb.M` is not reached), and four fills on one handle — direct, captured, replayed twice — each equal to
  the construction.

test_cpu_fill_exact.py shows without a device that the oracle returns the constructed cores and that the routes above are the launchers'.
Not reached: the ticket / avoid_xcc dispatch of lu_update_kernel and lu_solve_kernel, which runs only for a built-in functor beside a bond
chain (tests/test_gpu_chain.py holds it bitwise to the host path).
"""
import numpy as np
import pytest

import fill_exact_np as fx

pytestmark = pytest.mark.gpu

IDS = [fx.profile_id(p) for p in fx.PROFILES]


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def handle(t4a, c, f=None):
    g = t4a.TensorCI2(c.dims)
    g.set_function(c.f if f is None else f)
    fx.apply_sets(g, c)
    return g


@pytest.mark.parametrize("p", fx.PROFILES, ids=IDS)
def test_fill_exact_on_every_route(t4a, p):
    c = fx.chain(p)
    assert fx.fill_route(c.max_n(), c.max_nrhs()) == p[2]
    g = handle(t4a, c)
    g.fill_site_tensors()
    fx.assert_cores_exact(g, c)


@pytest.mark.parametrize("zero_site", [1, 2])
def test_zero_pivot_matrix_inside_the_batch(t4a, zero_site):
    c = fx.chain(fx.P40, zero_site=zero_site)
    g = handle(t4a, c)
    g.fill_site_tensors()
    z = g.site_tensor(zero_site)
    assert z.shape == c.cores[zero_site].shape and not z.any()
    fx.assert_cores_exact(g, c)


@pytest.mark.parametrize("p", fx.PROFILES, ids=IDS)
def test_fill_pivot_sensitive_on_every_route(t4a, p):
    c = fx.chain(p, small=True)
    n = len(c.dims)
    g = handle(t4a, c)
    g.fill_site_tensors()
    cores = [g.site_tensor(s) for s in range(n)]
    for s in range(n):
        assert cores[s].shape == c.cores[s].shape, s
    ratios = fx.pivot_sensitive_ratios(c, cores)
    print(fx.profile_id(p), "ratios to the (forward, backward) bounds per site:", ratios)
    assert sorted(ratios) == list(range(n - 1))
    for b, (fwd, back) in ratios.items():
        assert fwd <= 1.0, (p[2], b, fwd)
        assert back <= 1.0, (p[2], b, back)
    fx.assert_cores_exact(g, c, sites=[n - 1])


def test_second_fill_on_one_handle_exact(t4a):
    c = fx.chain(fx.P40)
    g = handle(t4a, c)
    for _ in range(2):
        g.fill_site_tensors()
        fx.assert_cores_exact(g, c)


def test_sharded_fill_exact(t4a):
    c = fx.chain(fx.P40)
    g = handle(t4a, c)
    g.set_site_shard(1, 2)
    g.fill_site_tensors()
    fx.assert_cores_exact(g, c, sites=range(1, len(c.dims), 2))


def test_group_fill_exact(t4a):
    chains = [fx.chain(fx.P40), fx.chain(fx.P5), fx.linear_chain(fx.LINEAR_DIMS[0], seed=3)]
    hs = [handle(t4a, chains[0]), handle(t4a, chains[1]), handle(t4a, chains[2], chains[2].spec)]
    t4a.fill_site_tensors_group(hs)
    for h, c in zip(hs, chains):
        fx.assert_cores_exact(h, c)


@pytest.mark.parametrize("dims", fx.LINEAR_DIMS, ids=["small", "general"])
def test_linear_chain_exact(t4a, dims):
    c = fx.linear_chain(dims, seed=3)
    g = handle(t4a, c, c.spec)
    g.fill_site_tensors()
    fx.assert_cores_exact(g, c)


@pytest.mark.parametrize("dims", fx.LINEAR_DIMS, ids=["small", "general"])
def test_linear_chain_replayed_fills_exact(t4a, dims):
    """Four fills on one handle: the first is issued directly, the second repeats it and is captured, the third and fourth are replays
    (test_gpu_fill.py test_replayed_fill_equals_direct_issue) — each against the construction."""
    c = fx.linear_chain(dims, seed=4)
    g = handle(t4a, c, c.spec)
    before = g.fill_stats()
    for _ in range(4):
        g.fill_site_tensors()
        fx.assert_cores_exact(g, c)
    st = g.fill_stats()
    assert st["fills"] == before["fills"] + 4, (before, st)
    assert st["graph_captures"] == before["graph_captures"] + 1 and st["graph_replays"] == before["graph_replays"] + 2, (before, st)
