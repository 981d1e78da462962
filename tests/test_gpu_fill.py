"""fill_site_tensors (csrc/tci2_fill.hip): a fill replayed from its captured graph, a sharded fill, the fill of empty sets and a
group of fills must produce the cores of a directly issued fill, bit for bit, on both routes (one-launch small route; general
LU / triangular solve / pack route) — and the graph key must cover everything the replayed operations read.

The reference in every case: a fresh handle with the same function and the same I/J sets (set_index_set), filled ONCE — the first
fill of a handle is always issued directly.

This file compares fills with fills: it holds the replayed, sharded and grouped fills to the direct one and says nothing about the
values.  Those are pinned in tests/test_gpu_fill_exact.py, where every core of a ragged batch — on each route family of fill_issue, with
a zero pivot matrix inside the batch, replayed, sharded and grouped — must equal an answer that is exact by construction.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARITY = dict(nsearch=0, max_nglobal_pivot=0)
MIXED = [3, 2, 4, 5, 2, 3, 4]
N_B = 16


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def osc(t4a, k1=37):
    return t4a.quantics_osc2d(N_B, k1=k1, k2=53, k3=211, eps=0.3)


def optimised(t4a, case, chi=None):
    """(a): mixed local dimensions, bonds <= 16: every site fits the one-launch small route (nj <= 32, ni <= 64).
    (b): 16 binary sites, bonds beyond 32: ni = 2 chi > 64 forces the general route."""
    from t4a_amd.functions import lorentz
    if case == "a":
        dims, spec, chi, pivot = MIXED, lorentz(MIXED), chi or 16, [1, 1, 2, 3, 0, 2, 1]
    else:
        dims, spec, chi, pivot = [2] * N_B, osc(t4a), chi or 40, [0] * N_B
    g = t4a.TensorCI2(dims)
    g.set_function(spec)
    g.add_global_pivots([pivot])
    g.optimize(t4a.TCI2Options(tolerance=1e-12, max_bond_dim=chi, max_iter=12, ncheck_history=10 ** 6, **PARITY))
    if case == "b":
        assert max(g.link_dims()) > 32, g.link_dims()
    else:
        assert 1 < max(g.link_dims()) <= 16, g.link_dims()
    return g, dims, spec


def with_sets_of(t4a, src, dims, spec):
    g = t4a.TensorCI2(dims)
    g.set_function(spec)
    for s in range(len(dims)):
        g.set_index_set(0, s, src.i_set(s))
        g.set_index_set(1, s, src.j_set(s))
    return g


def reference(t4a, src, dims, spec):
    ref = with_sets_of(t4a, src, dims, spec)
    ref.fill_site_tensors()
    st = ref.fill_stats()
    assert st["graph_replays"] == 0 and st["graph_captures"] == 0, st
    return [ref.site_tensor(s) for s in range(len(dims))]


def assert_cores_equal(g, ref, sites=None):
    for s in (range(len(ref)) if sites is None else sites):
        a = g.site_tensor(s)
        assert a.shape == ref[s].shape and np.array_equal(a, ref[s]), f"site {s}"


@pytest.mark.parametrize("case", ["a", "b"])
def test_replayed_fill_equals_direct_issue(t4a, case):
    """Four fills behind an optimize: the first is issued directly (its records differ from the optimize loop's own fills), the second
    repeats it and is captured, the third and fourth are replays."""
    g, dims, spec = optimised(t4a, case)
    ref = reference(t4a, g, dims, spec)
    before = g.fill_stats()
    for k in range(4):
        g.fill_site_tensors()
        assert_cores_equal(g, ref)
    st = g.fill_stats()
    print(case, "fill stats before", before, "after", st)
    assert st["fills"] == before["fills"] + 4, (before, st)
    assert st["graph_captures"] >= 1 and st["graph_replays"] >= 1, st
    # of the four compared fills the second was a capture and the last two were replays (so on the parent of this test's commit too)
    assert st["graph_captures"] == before["graph_captures"] + 1 and st["graph_replays"] == before["graph_replays"] + 2, (before, st)


def test_graph_key_covers_what_the_operations_read(t4a):
    g, dims, spec = optimised(t4a, "b")
    replays = g.fill_stats()["graph_replays"]
    for _ in range(4):
        g.fill_site_tensors()
    assert g.fill_stats()["graph_replays"] >= replays + 1, (replays, g.fill_stats())
    # another parameter of the same function: shapes and addresses stay, the kernels' functor argument does not
    spec2 = osc(t4a, k1=41)
    g.set_function(spec2)
    g.fill_site_tensors()
    assert_cores_equal(g, reference(t4a, g, dims, spec2))
    # the rows of one I set permuted: counts stay, so the records stay and this fill captures (the one before was issued directly) ...
    s = N_B // 2
    rows = g.i_set(s)
    assert len(rows) > 2
    rng = np.random.default_rng(5)
    st0 = g.fill_stats()
    g.set_index_set(0, s, rows[rng.permutation(len(rows))])
    assert not np.array_equal(g.i_set(s), rows)
    g.fill_site_tensors()
    assert_cores_equal(g, reference(t4a, g, dims, spec2))
    assert g.fill_stats()["graph_captures"] == st0["graph_captures"] + 1, (st0, g.fill_stats())
    # ... and permuted again behind the capture: a replay with staged accumulators other than the captured fill's — the replayed
    # copy reads the staging buffer anew
    rows2 = g.i_set(s)
    while np.array_equal(g.i_set(s), rows2):
        g.set_index_set(0, s, rows[rng.permutation(len(rows))])
    g.fill_site_tensors()
    assert g.fill_stats()["graph_replays"] == st0["graph_replays"] + 1, (st0, g.fill_stats())
    assert_cores_equal(g, reference(t4a, g, dims, spec2))
    # larger bonds: other shapes, no replay
    links, replays = g.link_dims(), g.fill_stats()["graph_replays"]
    g.optimize(t4a.TCI2Options(tolerance=1e-12, max_bond_dim=48, max_iter=1, ncheck_history=10 ** 6, **PARITY), final_sweep1site=False)
    assert g.link_dims() != links and max(g.link_dims()) > max(links), (links, g.link_dims())
    g.fill_site_tensors()
    assert g.fill_stats()["graph_replays"] == replays, (replays, g.fill_stats())
    assert_cores_equal(g, reference(t4a, g, dims, spec2))


@pytest.mark.parametrize("case", ["a", "b"])
def test_sharded_fill_on_one_process(t4a, case):
    src, dims, spec = optimised(t4a, case)
    ref = reference(t4a, src, dims, spec)
    g = with_sets_of(t4a, src, dims, spec)
    g.set_site_shard(1, 2)
    g.fill_site_tensors()
    assert_cores_equal(g, ref, sites=range(1, len(dims), 2))


def test_fill_of_empty_sets_gives_zero_cores(t4a):
    from t4a_amd.functions import lorentz
    g = t4a.TensorCI2(MIXED)
    g.set_function(lorentz(MIXED))
    g.fill_site_tensors()
    for s, d in enumerate(MIXED):
        c = g.site_tensor(s)
        assert c.shape == (1, d, 1) and not c.any(), (s, c.shape)


def test_group_fill_equals_single_fills(t4a):
    srcs = [optimised(t4a, "a"), optimised(t4a, "a", chi=9), optimised(t4a, "b")]
    refs = [reference(t4a, g, dims, spec) for g, dims, spec in srcs]
    hs = [with_sets_of(t4a, g, dims, spec) for g, dims, spec in srcs]
    t4a.fill_site_tensors_group(hs)
    for h, ref in zip(hs, refs):
        assert_cores_equal(h, ref)
