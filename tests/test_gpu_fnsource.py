"""GPU tests of the function source shared by every driver (csrc/fnsource.hpp): the argument checks of a built-in function, the null
and missing-function answers, the count check of a batch callback on every route that calls one, and the weight offsets of sites
with UNEQUAL local dimensions (a wrong offset reads another site's weights and changes every value) against the CPU oracle."""
import ctypes

import numpy as np
import pytest

import oracle_binding as ob
from oracle_binding import OracleTreeTCI2, TreeOptions
from test_gpu_patch import assert_matches_oracle
from test_gpu_tci2 import PARITY, assert_cores_close, assert_same_sets, both
from test_gpu_tree import assert_same_state, gopts

pytestmark = pytest.mark.gpu

FN_COUNT, FN_MAX_ACC = 4, 4          # include/t4a_testfunctions.h
DIMS = [2, 3, 2, 4, 3]
BRANCHED = [(0, 1), (1, 2), (1, 3), (3, 4)]  # site 1 branches: the subtree {0, 1, 2} against {3, 4}, {0, 1, 3, 4} against {2}


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def _grid(dims):
    return np.indices(dims).reshape(len(dims), -1).T


def _bad(spec, fid=None, n_acc=None):
    """`spec` with a function id or an accumulator count out of range; the weight table is large enough for any count read."""
    from t4a_amd.functions import FnSpec
    b = FnSpec(spec.fid, spec.params, np.zeros((FN_MAX_ACC + 1, sum(spec.local_dims)), dtype=np.uint64), spec.local_dims)
    b.fid = spec.fid if fid is None else fid
    b.n_acc = spec.n_acc if n_acc is None else n_acc
    return b


@pytest.mark.parametrize("kw", [dict(fid=-1), dict(fid=FN_COUNT), dict(n_acc=0), dict(n_acc=FN_MAX_ACC + 1)])
def test_bad_builtin_arguments_are_refused_everywhere(t4a, kw):
    from t4a_amd.functions import lorentz
    dims = [2, 3, 2]
    good = lorentz(dims)
    bad = _bad(good, **kw)
    pts = _grid(dims)
    exact = 1.0 / ((pts ** 2).sum(axis=1) + 1.0)
    g = t4a.TensorCI2(dims)
    tree = t4a.TreeTCI2(dims, [(0, 1), (1, 2)])
    calls = [lambda: g.set_function(bad), lambda: tree.set_function(bad),
             lambda: t4a.adaptiveinterpolate(bad, dims, [[0, 0, 0]], t4a.TCI2Options(**PARITY)),
             lambda: t4a.fn_eval(bad, dims, pts)]
    for call in calls:
        with pytest.raises(t4a.T4aError) as e:
            call()
        assert e.value.code == t4a.INVALID_ARGUMENT
    # the handles are usable afterwards
    g.set_function(good)
    g.crossinterpolate2([[1, 1, 1]], t4a.TCI2Options(tolerance=1e-12, **PARITY))
    assert np.abs(g.evaluate(pts) - exact).max() < 1e-10
    tree.set_function(good)
    tree.crossinterpolate2([[1, 1, 1]], t4a.TreeTciOptions(tolerance=1e-12, enable_global_pivots=False))
    tree.materialize(0)
    assert np.abs(tree.evaluate(pts) - exact).max() < 1e-10
    assert np.abs(t4a.fn_eval(good, dims, pts) - exact).max() < 1e-14


def test_null_callback_and_missing_function(t4a):
    g = t4a.TensorCI2([2] * 3)
    tree = t4a.TreeTCI2([2] * 3, [(0, 1), (1, 2)])
    null = ctypes.cast(None, t4a._BATCH_CB)
    assert t4a._lib.t4a_gpu_tci2_set_callback(g._h, null, None) == t4a.NULL_POINTER
    assert t4a._lib.t4a_gpu_treetci_set_callback(tree._h, null, None) == t4a.NULL_POINTER
    with pytest.raises(t4a.T4aError) as e:
        g.optimize(t4a.TCI2Options(**PARITY))
    assert e.value.code == t4a.INVALID_ARGUMENT and "t4a_gpu_tci2_set_builtin_function" in e.value.message
    with pytest.raises(t4a.T4aError) as e:
        tree.optimize(t4a.TreeTciOptions())
    assert e.value.code == t4a.INVALID_ARGUMENT and "t4a_gpu_treetci_set_builtin_function" in e.value.message


class _Short:
    """f(idx) = 1 / (1 + sum idx) whose batch form drops its last value once `short` is set"""

    def __init__(self, short):
        self.short = short

    def __call__(self, idx):
        return 1.0 / (1.0 + sum(int(v) for v in idx))

    def batched(self, pts):
        vals = [self(p) for p in pts]
        return vals[:-1] if self.short else vals


def _tci2_sweep(t4a, pivot_search):
    f = _Short(False)
    g = t4a.TensorCI2([2] * 4)
    g.set_function(f)
    g.add_global_pivots([[0] * 4])
    f.short = True
    g.sweep2site(True, t4a.TCI2Options(pivot_search=pivot_search, **PARITY))


def _tci2_initial_pivots(t4a):
    t4a.crossinterpolate2(_Short(True), [2] * 4, [[0] * 4], t4a.TCI2Options(**PARITY))


def _tree(t4a, route):
    f = _Short(route == "points")
    t = t4a.TreeTCI2([2] * 4, [(0, 1), (1, 2), (1, 3)])
    t.set_function(f)
    if route == "points":
        t.crossinterpolate2([[0] * 4], t4a.TreeTciOptions())  # the values of the initial pivots
    else:
        t.add_global_pivots([[0] * 4])
        f.short = True
        t.update_edge(1, 2)


def _patch(t4a):
    t4a.adaptiveinterpolate(_Short(True), [2] * 4, [[0] * 4], t4a.TCI2Options(**PARITY))


@pytest.mark.parametrize("route", ["tci2 full search", "tci2 rook", "tci2 initial pivots", "tree edge update", "tree points", "patching"])
def test_short_callback_count_is_an_error_on_every_route(t4a, route):
    run = {"tci2 full search": lambda: _tci2_sweep(t4a, t4a.TCI2Options.FULL), "tci2 rook": lambda: _tci2_sweep(t4a, t4a.TCI2Options.ROOK),
           "tci2 initial pivots": lambda: _tci2_initial_pivots(t4a), "tree edge update": lambda: _tree(t4a, "edge"),
           "tree points": lambda: _tree(t4a, "points"), "patching": lambda: _patch(t4a)}[route]
    with pytest.raises(t4a.T4aError) as e:
        run()  # (the handle goes out of scope with the exception: released here)
    assert e.value.code == t4a.CALLBACK_ERROR
    assert " values for " in e.value.message


# ------------------------------------------------------------------------------------------------ unequal local dimensions
@pytest.mark.parametrize("pivot_search", [0, 1])
def test_tci2_builtin_unequal_local_dims_matches_oracle(t4a, pivot_search):
    from t4a_amd.functions import lorentz
    spec = lorentz(DIMS)
    opts = t4a.TCI2Options(tolerance=1e-10, max_iter=8, pivot_search=pivot_search, **PARITY)
    g, o = both(t4a, spec, DIMS)
    o.set_pivot_search(pivot_search)
    g.crossinterpolate2([[1] * 5], opts)
    o.crossinterpolate2([[1] * 5], opts)
    assert_same_sets(g, o, 5)
    assert_cores_close(g, o, 5, 1e-10)
    pts = _grid(DIMS)
    assert np.abs(g.evaluate(pts) - 1.0 / ((pts ** 2).sum(axis=1) + 1.0)).max() < 1e-8
    assert np.array_equal(t4a.fn_eval(spec, DIMS, pts), ob.fn_eval(spec, pts))  # (t4a_testfunctions.h is deterministic across host and device)


def test_tree_builtin_unequal_local_dims_matches_oracle(t4a):
    from t4a_amd.functions import lorentz
    spec = lorentz(DIMS)
    g = t4a.TreeTCI2(DIMS, BRANCHED)
    g.set_function(spec)
    o = OracleTreeTCI2(DIMS, BRANCHED, spec)
    opt = TreeOptions(tolerance=1e-10, max_iter=8, seed=3)  # (with the global pivot search: point evaluation of the built-in)
    og = o.crossinterpolate2([[1] * 5], opt)
    gg = g.crossinterpolate2([[1] * 5], gopts(t4a, opt))
    assert gg[0] == og[0] and np.allclose(gg[1], og[1], rtol=0, atol=1e-12)
    assert_same_state(g, o, BRANCHED)
    g.materialize(1)
    o.materialize(1)
    pts = _grid(DIMS)
    got = g.evaluate(pts)
    assert np.abs(got - o.evaluate(pts)).max() <= 1e-10
    assert np.abs(got - 1.0 / ((pts ** 2).sum(axis=1) + 1.0)).max() < 1e-8


def test_patching_builtin_unequal_local_dims_matches_oracle(t4a):
    """A rank cap below the function's rank: the queue projects sites out of order, so the weight tables restricted to a patch's active
    sites take their entries from non-adjacent offsets of the full table."""
    from t4a_amd.functions import lorentz
    spec = lorentz(DIMS)
    opt = t4a.TCI2Options(tolerance=1e-9, max_bond_dim=2, max_iter=8, **PARITY)
    kw = dict(patch_order=[3, 0, 2, 1, 4], n_initial_pivots=2, recycle_pivots=True)
    piv = [[0] * 5, [1, 2, 1, 3, 2]]
    g = t4a.adaptiveinterpolate(spec, DIMS, piv, opt, **kw)
    o = ob.adaptiveinterpolate(spec, DIMS, piv, opt, **kw)
    assert len(g) > 1
    assert_matches_oracle(g, o, tol=1e-8)
    pts = _grid(DIMS)
    assert np.abs(g.evaluate(pts) - 1.0 / ((pts ** 2).sum(axis=1) + 1.0)).max() < 1e-6
