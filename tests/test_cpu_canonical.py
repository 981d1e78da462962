"""The gauge forms (SiteTensorTrain, VidalTensorTrain, InverseTensorTrain, center_canonicalize) without a GPU: exported symbols,
argument errors that are refused before the device is touched, and the numpy restatement of the reference algorithm
(tests/canonical_np.py) checked against the dense tensor, against an exact rational expectation and across two SVDs.

The tolerances here (1e-11 reconstruction, 1e-12 orthonormality, 1e-13 lambda_max between two SVDs) are a tenth of what
tests/test_gpu_canonical.py takes from the project's SVD tests; the restatement measures 3e-16 .. 5e-15 on reconstruction and at most
3e-15 on orthonormality on these fixtures."""
import ctypes
import os
import re

import numpy as np
import pytest

import canonical_np as cn
import oracle_binding as ob

SITE = ["from_tt", "release", "len", "dims", "site_tensor", "center", "move_center_left", "move_center_right", "set_center",
        "set_site_tensor", "set_two_site_tensors", "to_tt", "tensors_tt"]
VIDAL = ["from_tt", "new", "release", "len", "dims", "site_tensor", "set_site_tensor", "partition", "singular_values",
         "set_singular_values", "to_tt", "tensors_tt"]
INVERSE = ["from_vidal", "from_tt", "release", "len", "dims", "site_tensor", "partition", "inverse_singular_values",
           "set_two_site_tensors", "to_tt", "tensors_tt"]
SYMBOLS = ([f"t4a_gpu_site_tt_{s}" for s in SITE] + [f"t4a_gpu_vidal_tt_{s}" for s in VIDAL] + [f"t4a_gpu_inverse_tt_{s}" for s in INVERSE] +
           ["t4a_gpu_tt_center_canonicalize"])

FIXTURES = {"A": cn.fixture_a, "B": cn.fixture_b, "C": cn.fixture_c, "E": cn.fixture_e, "E2": cn.fixture_e2}


def same_up_to_zero_sign(a, b):
    """bit for bit, except that -0.0 and +0.0 count as equal (0 / negative pivot is -0.0 in floating point and 0 in the rationals)"""
    return a.shape == b.shape and np.array_equal((a + 0.0).view(np.uint64), (b + 0.0).view(np.uint64))


def test_every_symbol_is_exported_with_its_declared_signature():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t4a_gpu.h")).read()
    decl = {}
    for s in SYMBOLS:
        m = re.search(r"(t4a_gpu_status|void) " + s + r"\(([^;]*)\);", header)
        assert m, s
        decl[s] = (m.group(1), [a.strip() for a in " ".join(m.group(2).split()).split(",")])
    assert all(decl[s][0] == ("void" if s.endswith("_release") else "t4a_gpu_status") for s in SYMBOLS)
    n_args = {s: len(decl[s][1]) for s in SYMBOLS}
    assert n_args["t4a_gpu_site_tt_from_tt"] == 3 and n_args["t4a_gpu_vidal_tt_from_tt"] == 4 and n_args["t4a_gpu_vidal_tt_new"] == 7
    assert n_args["t4a_gpu_inverse_tt_set_two_site_tensors"] == 8 and n_args["t4a_gpu_site_tt_set_two_site_tensors"] == 6
    assert n_args["t4a_gpu_vidal_tt_singular_values"] == 5 and n_args["t4a_gpu_inverse_tt_inverse_singular_values"] == 5
    assert n_args["t4a_gpu_tt_center_canonicalize"] == 2
    for form in ("site", "vidal", "inverse"):  # every constructor and conversion hands out a handle through its last argument
        assert decl[f"t4a_gpu_{form}_tt_to_tt"][1][-1] == "t4a_gpu_tt** out" and decl[f"t4a_gpu_{form}_tt_tensors_tt"][1][-1] == "t4a_gpu_tt** out"
    import t4a_amd.canonical as c
    assert (t4a_amd.SiteTensorTrain, t4a_amd.VidalTensorTrain, t4a_amd.InverseTensorTrain, t4a_amd.center_canonicalize) == (
        c.SiteTensorTrain, c.VidalTensorTrain, c.InverseTensorTrain, c.center_canonicalize)
    for cls, names in ((c.SiteTensorTrain, ["from_tensor_train", "new", "center", "partition", "move_center_left", "move_center_right", "set_center",
                                            "set_site_tensor", "set_two_site_tensors"]),
                       (c.VidalTensorTrain, ["from_tensor_train", "from_tensor_train_with_partition", "new", "partition", "singular_values",
                                             "all_singular_values", "set_site_tensor"]),
                       (c.InverseTensorTrain, ["from_vidal", "from_tensor_train", "partition", "inverse_singular_values", "set_two_site_tensors"])):
        for name in names + ["site_tensor", "site_tensors", "to_tensor_train", "len", "link_dims", "site_dims", "rank", "evaluate", "sum", "norm2"]:
            assert callable(getattr(cls, name)), (cls, name)


def test_argument_errors_are_refused_before_the_device():
    """What can be reached without a device: NULL handles, the vector count of VidalTensorTrain::new, and every index check on the
    empty Vidal / inverse objects (which hold no device resources).  The checks that need a train on the device — centre out of range,
    partition end beyond the length, site >= len - 1 on a real train — are in tests/test_gpu_canonical.py."""
    import t4a_amd
    lib, p = t4a_amd._lib, t4a_amd._p
    h = ctypes.c_void_p()
    sz = ctypes.c_size_t
    n = sz(0)
    buf = np.zeros(8)
    d3 = np.array([1, 2, 1, 1, 2, 1], dtype=np.uintp)
    null_calls = {
        "site from_tt": lambda: lib.t4a_gpu_site_tt_from_tt(None, sz(0), ctypes.byref(h)),
        "site len": lambda: lib.t4a_gpu_site_tt_len(None, ctypes.byref(n)),
        "site set_center": lambda: lib.t4a_gpu_site_tt_set_center(None, sz(0)),
        "site set_two": lambda: lib.t4a_gpu_site_tt_set_two_site_tensors(None, sz(0), p(d3), p(buf), p(d3), p(buf)),
        "canonicalize": lambda: lib.t4a_gpu_tt_center_canonicalize(None, sz(0)),
        "vidal from_tt": lambda: lib.t4a_gpu_vidal_tt_from_tt(None, sz(0), sz(1), ctypes.byref(h)),
        "vidal new out": lambda: lib.t4a_gpu_vidal_tt_new(p(d3), sz(2), p(buf), p(d3), sz(1), p(buf), None),
        "vidal sv": lambda: lib.t4a_gpu_vidal_tt_singular_values(None, sz(0), None, sz(0), ctypes.byref(n)),
        "inverse from_vidal": lambda: lib.t4a_gpu_inverse_tt_from_vidal(None, ctypes.byref(h)),
        "inverse from_tt": lambda: lib.t4a_gpu_inverse_tt_from_tt(None, ctypes.byref(h)),
        "inverse to_tt": lambda: lib.t4a_gpu_inverse_tt_to_tt(None, ctypes.byref(h)),
    }
    for name, call in null_calls.items():
        assert call() == t4a_amd.NULL_POINTER, name
        assert "null" in t4a_amd.last_error_message(), name
        assert not h, name
    for rel in ("site", "vidal", "inverse"):
        getattr(lib, f"t4a_gpu_{rel}_tt_release")(None)
    # VidalTensorTrain::new: "Expected {n-1} singular value vectors, got {k}" (vidal.rs:413-421), before any upload
    lens = np.array([1, 1, 1], dtype=np.uintp)
    for k in (0, 2, 3):
        assert lib.t4a_gpu_vidal_tt_new(p(d3), sz(2), p(buf), p(lens), sz(k), p(buf), ctypes.byref(h)) == t4a_amd.INVALID_ARGUMENT
        assert f"Expected 1 singular value vectors, got {k}" in t4a_amd.last_error_message() and not h
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.VidalTensorTrain([np.ones((1, 2, 1))] * 3, [np.ones(1)])
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "Expected 2 singular value vectors, got 1" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.VidalTensorTrain([np.ones((2, 1))], [])
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "three legs" in e.value.message
    # the empty objects (vidal.rs:405-411, :552-559) need no device; every index is out of range on them
    v = t4a_amd.VidalTensorTrain([], [np.ones(3)])  # (the vectors of an empty train are not looked at, as in the reference)
    assert v.len() == 0 and v.partition() == range(0, 0) and v.all_singular_values() == [] and v.link_dims() == [] and v.rank() == 1
    inv = t4a_amd.InverseTensorTrain.from_vidal(v)
    assert inv.len() == 0 and inv.partition() == range(0, 0) and inv.all_inverse_singular_values() == []
    one = np.ones((1, 2, 1))
    for call, needle in ((lambda: v.singular_values(0), "bond 0 is out of range"), (lambda: v.set_singular_values(0, [1.0]), "bond 0 is out of range"),
                         (lambda: v.set_site_tensor(0, one), "site 0 is out of range"), (lambda: v.site_tensor(0), "site 0 is out of range"),
                         (lambda: inv.inverse_singular_values(1), "bond 1 is out of range"),
                         (lambda: inv.set_two_site_tensors(0, one, [1.0], one), "Cannot set two-site tensors at site 0"),
                         (lambda: v.singular_values(-1), "negative bond")):
        with pytest.raises(t4a_amd.T4aError) as e:
            call()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and needle in e.value.message, needle


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_reproduces_the_tensor_and_gauges_it(name):
    cores = FIXTURES[name]()
    n = len(cores)
    full = cn.dense(cores)
    scale = np.abs(full).max()
    for center in (0, n // 2, n - 1):
        s = cn.site_form(cores, center)
        assert np.abs(cn.dense(s) - full).max() <= 1e-11 * scale, center
        for i in range(center):  # LU gauge: entries of magnitude <= 1 and a unit lower triangle among the rows
            m = cn.left_matrix(s[i])
            assert np.abs(m).max() <= 1.0 and m.shape[1] <= m.shape[0]
    v, sv = cn.vidal_form(cores)
    assert np.abs(cn.dense(cn.vidal_to_tt(v, sv)) - full).max() <= 1e-11 * scale
    assert cn.rows_orthonormal_defect(v, sv) <= 1e-12
    assert all(np.all(np.diff(x) <= 0) and np.all(x >= 0) for x in sv)
    it, inv = cn.inverse_from_vidal(v, sv)
    assert np.abs(cn.dense(cn.inverse_to_tt(it, inv)) - full).max() <= 1e-11 * scale
    if name == "A":  # a partition: only the bonds inside it carry values
        v, sv = cn.vidal_form(cores, 1, 4)
        assert [len(x) for x in sv] == [0, 5, 6, 0]
        assert np.abs(cn.dense(cn.vidal_to_tt(v, sv)) - full).max() <= 1e-11 * scale and cn.rows_orthonormal_defect(v, sv, 1, 4) <= 1e-12


def test_bonds_of_the_restatement():
    assert [c.shape for c in cn.site_form(cn.fixture_b(), 3)] == [(1, 2, 2), (2, 2, 4), (4, 2, 4), (4, 2, 1)]
    assert [c.shape for c in cn.site_form(cn.fixture_b(), 0)] == [(1, 2, 4), (4, 2, 4), (4, 2, 2), (2, 2, 1)]
    assert [len(x) for x in cn.vidal_form(cn.fixture_b())[1]] == [2, 4, 2]  # bonds wider than l * s shrink
    # C: the zeroed index of bond 2 is an exactly zero column; the rrLU stops at the exactly zero pivot and the bond drops from 5 to 4,
    # in the left step at site 1 as well as in the right step at site 2
    c = cn.fixture_c()
    assert cn.site_form(cn.fixture_a(), 4)[1].shape == (2, 3, 5) and cn.site_form(c, 4)[1].shape == (2, 3, 4)
    assert cn.site_form(cn.fixture_a(), 0)[2].shape == (5, 2, 6) and cn.site_form(c, 0)[2].shape == (4, 2, 6)
    q, r = cn.step_factors(c[1], True)
    assert q.shape == (6, 4) and np.all(r[:, 3] == 0.0)
    # the Vidal values are NOT the Schmidt values of the tensor: the left sweep leaves LU factors, not isometries, left of each SVD
    a = cn.fixture_a()
    sv = cn.vidal_form(a)[1]
    full = cn.dense(a)
    off = []
    for b, lam in enumerate(sv):
        schmidt = np.linalg.svd(full.reshape(int(np.prod(full.shape[:b + 1])), -1), compute_uv=False)[:len(lam)]
        off.append(np.abs(lam - schmidt).max() / schmidt.max())
    assert off[-1] < 1e-12 or max(off) > 0.05, off  # (measured: 0.3 .. 0.6 of sigma_max on the inner bonds)
    assert max(off) > 0.05, off


@pytest.mark.parametrize("name", ["d1", "d2"])
def test_monomial_chains_equal_the_exact_expectation(name):
    """D1 / D2: no operation rounds, so the restatement (oracle rrLU in doubles) must equal the site form worked out in rational
    arithmetic with the reference's pivot scan, at every centre."""
    cores = getattr(cn, "fixture_" + name)()
    for c in cores:  # one nonzero per column of the left matrix, in distinct rows
        m = cn.left_matrix(c) != 0
        assert np.all(m.sum(axis=0) == 1) and np.all(m.sum(axis=1) <= 1)
    for center in range(len(cores)):
        got, want = cn.site_form(cores, center), cn.exact_site_form(cores, center)
        assert all(same_up_to_zero_sign(g, w) for g, w in zip(got, want)), center
    left = cn.site_form(cores, len(cores) - 1)
    assert [c.shape for c in left] == [(1, 2, 2), (2, 3, 4), (4, 2, 3), (3, 3, 1)]
    for c in left[:-1]:  # pivot / pivot == 1: the gauged cores are row selections
        assert set(np.unique(np.abs(c))) <= {0.0, 1.0} and np.count_nonzero(c) == c.shape[2]


def test_two_svds_agree_on_the_vidal_values():
    a = cn.fixture_a()
    s1 = cn.vidal_form(a, svd=cn.np_svd)[1]
    s2 = cn.vidal_form(a, svd=ob.svd)[1]
    for x, y in zip(s1, s2):
        assert x.shape == y.shape and np.abs(x - y).max() <= 1e-13 * x.max()


def test_sequential_evaluate_is_the_oracles():
    a = cn.fixture_a()
    pts = cn.all_points([c.shape[1] for c in a])
    got = cn.evaluate_seq(a, pts)
    assert np.array_equal(got.view(np.uint64), ob.OracleTT(a).evaluate(pts).view(np.uint64))


def test_scale_fixture_holds_the_guard_cases():
    cores, vecs = cn.fixture_g()
    assert [c.shape for c in cores] == [(1, 2, 3), (3, 3, 5), (5, 1, 2), (2, 4, 1)]
    assert len(vecs[1]) < cores[1].shape[2] and len(vecs[2]) > cores[2].shape[2]
    flat = np.concatenate(vecs)
    assert all(v in flat for v in cn.G_VALUES) and cn.G_VALUES[2] > 1e-15 and cn.G_VALUES[2] - 1e-15 < 1e-30
    _, inv = cn.inverse_from_vidal(cores, vecs)
    assert inv[0].tolist() == [0.0, 0.0, 1.0 / cn.G_VALUES[2]] and inv[1].tolist() == [1.0 / -3.0, 0.0, 1.0 / 1e300]
