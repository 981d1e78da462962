"""fit_sum without a GPU: the options struct and its defaults, every refusal that is answered on the host (through
t4a_gpu_fit_sum_check_shapes and the Python wrappers), the launch counts of fit_sum_plan, the route rule, and the numpy restatement
(tests/fit_sum_np.py) against dense sums — from full bonds one sweep returns sum_k w_k T_k within 1e-12 of sum_k |w_k| |T_k|_F, with no
option set the link dims stay those of the initial, with max_bond_dim no bond exceeds the cap — and the gap condition on the truncating
cases the GPU tests use."""
import ctypes

import numpy as np
import pytest

import fit_sum_np as F


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_options_default_matches_the_reference():
    import t4a_amd
    o = t4a_amd.FitSumOptionsC()
    assert t4a_amd._lib.t4a_gpu_fit_sum_options_default(ctypes.byref(o)) == 0
    # FitOptions::new(1): one sweep, no cap, no policy, no QR tolerance, SVD, no convergence tolerance
    assert (o.nfullsweeps, o.has_max_bond_dim, o.has_svd_policy, o.has_qr_rtol, o.factorize_alg, o.has_convergence_tol) == (1, 0, 0, 0, 0, 0)
    d = t4a_amd.FitSumOptions().to_c()
    for name in ("nfullsweeps", "has_max_bond_dim", "max_bond_dim", "has_svd_policy", "has_qr_rtol", "qr_rtol", "factorize_alg", "has_convergence_tol",
                 "convergence_tol"):
        assert getattr(d, name) == getattr(o, name), name
    assert t4a_amd._lib.t4a_gpu_fit_sum_options_default(None) == t4a_amd.NULL_POINTER
    s = t4a_amd.FitSumOptions(nfullsweeps=3, max_bond_dim=7, svd_policy=t4a_amd.SvdTruncationPolicy(1e-5), convergence_tol=1e-8).to_c()
    assert (s.nfullsweeps, s.has_max_bond_dim, s.max_bond_dim, s.has_svd_policy, s.svd_policy.threshold, s.has_convergence_tol, s.convergence_tol) == \
        (3, 1, 7, 1, 1e-5, 1, 1e-8)


def test_symbols_are_exported_and_fit_options_of_contract_fit_is_untouched():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    for name in ("t4a_gpu_fit_sum_options_default", "t4a_gpu_fit_sum_check_shapes", "t4a_gpu_tt_fit_sum", "t4a_gpu_mpo_fit_sum", "t4a_gpu_fit_sum_half",
                 "t4a_gpu_fit_sum_route", "t4a_gpu_fit_sum_plan", "t4a_gpu_fit_sum_time_half"):
        assert hasattr(lib, name), name
    assert t4a_amd.fit_sum is t4a_amd.fitsum.fit_sum and t4a_amd.FitSumOptions is t4a_amd.fitsum.FitSumOptions
    assert t4a_amd.FitOptions is t4a_amd.mpo.FitOptions and t4a_amd.FitOptions is not t4a_amd.FitSumOptions


D = [(1, 2, 2), (2, 2, 2), (2, 2, 1)]

BAD_OPTIONS = [
    (dict(convergence_tol=-1e-3), "convergence tolerance must be finite and non-negative"),
    (dict(convergence_tol=float("nan")), "convergence tolerance must be finite and non-negative"),
    (dict(convergence_tol=float("inf")), "convergence tolerance must be finite and non-negative"),
    (dict(qr_rtol=-1.0), "QR relative tolerance must be finite and non-negative"),
    (dict(qr_rtol=float("nan"), factorize_alg=1), "QR relative tolerance must be finite and non-negative"),
    (dict(max_bond_dim=0), "max_bond_dim must be at least 1"),
    (dict(qr_rtol=1e-12), "SVD factorization does not accept qr_rtol"),
    (dict(factorize_alg=1, svd_policy="default"), "QR factorization does not accept svd_policy"),
    (dict(factorize_alg=2, svd_policy="default"), "LU/CI factorization does not accept svd_policy"),
    (dict(factorize_alg=3, qr_rtol=1e-12), "LU/CI factorization does not accept qr_rtol"),
    (dict(factorize_alg=4), "unknown factorize_alg"),
]


def make_options(kw):
    import t4a_amd
    kw = dict(kw)
    if kw.get("svd_policy") == "default":
        kw["svd_policy"] = t4a_amd.SvdTruncationPolicy()
    return t4a_amd.FitSumOptions(**kw)


@pytest.mark.parametrize("kw, message", BAD_OPTIONS)
def test_bad_options_are_refused_with_the_message_of_the_reference(kw, message):
    import t4a_amd
    with pytest.raises(t4a_amd.T4aError, match=message) as e:
        t4a_amd.fit_sum_check_shapes([D], D, 0, make_options(kw))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    # the same answer from the entry points, whose operands are NULL: anything else would mean they were looked at first
    o = make_options(kw).to_c()
    h, a, b, c = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    for fn in (t4a_amd._lib.t4a_gpu_tt_fit_sum, t4a_amd._lib.t4a_gpu_mpo_fit_sum):
        st = fn(None, ctypes.c_size_t(3), None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.c_int32(0), ctypes.byref(h), ctypes.byref(a),
                ctypes.byref(b), ctypes.byref(c), None)
        assert st == t4a_amd.INVALID_ARGUMENT and message in t4a_amd.last_error_message()


def test_an_invalid_svd_policy_goes_through_validate_svd_policy():
    import t4a_amd
    for pol in (t4a_amd.SvdTruncationPolicy(-1.0), t4a_amd.SvdTruncationPolicy(float("nan"))):
        with pytest.raises(t4a_amd.T4aError, match="threshold must be finite and non-negative"):
            t4a_amd.fit_sum_check_shapes([D], D, 0, t4a_amd.FitSumOptions(svd_policy=pol))
    o = t4a_amd.FitSumOptions(svd_policy=t4a_amd.SvdTruncationPolicy()).to_c()
    o.svd_policy.rule = 5
    with pytest.raises(t4a_amd.T4aError, match="unknown scale, measure or rule"):
        t4a_amd.fit_sum_check_shapes([D], D, 0, o)


@pytest.mark.parametrize("alg, name", [(1, "QR"), (2, "LU"), (3, "CI")])
def test_qr_lu_and_ci_answer_not_implemented_naming_the_algorithm(alg, name):
    import t4a_amd
    with pytest.raises(t4a_amd.T4aError, match=f"the {name} factorization is not implemented") as e:
        t4a_amd.fit_sum_check_shapes([D], D, 0, t4a_amd.FitSumOptions(factorize_alg=alg))
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED
    if alg == 1:  # QR with its own tolerance is a valid request of the reference, still not built
        with pytest.raises(t4a_amd.T4aError, match="the QR factorization is not implemented"):
            t4a_amd.fit_sum_check_shapes([D], D, 0, t4a_amd.FitSumOptions(factorize_alg=1, qr_rtol=1e-10))


def test_shape_refusals_in_the_order_of_the_reference():
    import t4a_amd
    other_site = [(1, 2, 2), (2, 3, 2), (2, 2, 1)]
    cases = [
        (([], D, 0), "fit_sum: targets must not be empty"),
        (([D], [], 0), "fit_sum: initial TreeTN must not be empty"),
        (([D, D], D, 3), "fit_sum: center node is not in initial TreeTN"),
        (([D, D[:1] + [(2, 2, 1)]], D, 0), "fit_sum: target 1 has an incompatible named topology"),
        (([D, D, other_site], D, 2), "fit_sum: target 2 site-space validation failed"),
        (([D[:1] + [(2, 2, 1)], other_site], D, 5), "fit_sum: center node is not in initial TreeTN"),  # the centre before the targets
        (([other_site, D], None, 0), "fit_sum: target 1 site-space validation failed"),                # no initial: the first target stands in
    ]
    for args, message in cases:
        with pytest.raises(t4a_amd.T4aError, match=message) as e:
            t4a_amd.fit_sum_check_shapes(*args)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT
        with pytest.raises(ValueError, match=message):
            F.check_shapes(*args)
    # the options come first
    with pytest.raises(t4a_amd.T4aError, match="convergence tolerance"):
        t4a_amd.fit_sum_check_shapes([], D, 0, t4a_amd.FitSumOptions(convergence_tol=-1.0))
    t4a_amd.fit_sum_check_shapes([D, D], D, 2)
    t4a_amd.fit_sum_check_shapes([D, D], None, 1, t4a_amd.FitSumOptions(nfullsweeps=0))
    t4a_amd.fit_sum_check_shapes([[(1, 5, 1)]] * 3, [(1, 5, 1)], 0)


def test_a_work_matrix_above_int_max_is_refused_per_bond_step():
    import t4a_amd
    big = 30000
    target = [(1, 2, 2), (2, 2, big), (big, 2, 1)]
    init = [(1, 2, 2), (2, 2, big), (big, 2, 1)]
    t4a_amd.fit_sum_check_shapes([target], init, 0)  # the right environment of the step (0, 1) is 30000 x 30000: fine
    with pytest.raises(t4a_amd.T4aError, match=r"a work matrix of the bond step \(0, 1\) holds more than INT_MAX elements"):
        t4a_amd.fit_sum_check_shapes([target] * 20, init, 0)  # with twenty targets it is 600000 x 30000
    # the bound follows the bonds of the initial: a small initial keeps every work matrix of these targets small
    t4a_amd.fit_sum_check_shapes([target] * 20, [(1, 2, 2), (2, 2, 2), (2, 2, 1)], 0)


def test_the_python_wrapper_refuses_before_the_library_is_called():
    import t4a_amd

    class Fake:
        _h = None
    with pytest.raises(t4a_amd.T4aError, match="must be SimpleTensorTrain or MPO"):
        t4a_amd.fit_sum([Fake()])
    with pytest.raises(t4a_amd.T4aError, match="route must be"):
        t4a_amd.fit_sum([], route="fastest")
    with pytest.raises(t4a_amd.T4aError, match="center must not be negative"):
        t4a_amd.fit_sum([], center=-1)
    with pytest.raises(t4a_amd.T4aError, match="targets must not be empty"):
        t4a_amd.fit_sum([])
    with pytest.raises(t4a_amd.T4aError, match="svd_policy must be an SvdTruncationPolicy"):
        t4a_amd.fit_sum([], options=t4a_amd.FitSumOptions(svd_policy=1e-8))
    for fn in (t4a_amd._lib.t4a_gpu_tt_fit_sum, t4a_amd._lib.t4a_gpu_mpo_fit_sum):  # an unknown route, before the operands
        o = t4a_amd.FitSumOptions().to_c()
        h, a, b, c = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
        st = fn(None, ctypes.c_size_t(1), None, None, ctypes.c_size_t(0), ctypes.byref(o), ctypes.c_int32(3), ctypes.byref(h), ctypes.byref(a), ctypes.byref(b),
                ctypes.byref(c), None)
        assert st == t4a_amd.INVALID_ARGUMENT and "unknown route" in t4a_amd.last_error_message()


def test_plan_counts():
    import t4a_amd
    for n, center, K, S in ((2, 0, 1, 2), (6, 2, 3, 2), (16, 15, 256, 2), (5, 0, 40, 4)):
        fused = t4a_amd.fit_sum_plan(n, center, K, S, "fused")
        assert fused == {"bond_steps_per_sweep": 2 * (n - 1), "half_launches_per_step": 2, "gemms_per_step": 2, "svds_per_step": 1,
                         "prepare_half_launches": n - 1, "prepare_gemms": n - 1}
        gemm = t4a_amd.fit_sum_plan(n, center, K, S, "gemm")
        assert gemm == {"bond_steps_per_sweep": 2 * (n - 1), "half_launches_per_step": 0, "gemms_per_step": 2 + K + K * S, "svds_per_step": 1,
                        "prepare_half_launches": 0, "prepare_gemms": (n - 1) + center * K + (n - 1 - center) * K * S}
        assert F.sweep_plan(n, center)[-1][0] == (center - 1 if center else 0) and len(F.sweep_plan(n, center)) == 2 * (n - 1)
    assert t4a_amd.fit_sum_plan(1, 0, 5, 2, "fused")["bond_steps_per_sweep"] == 0
    for args, message in (((0, 0, 1, 2, "fused"), "initial TreeTN must not be empty"), ((3, 3, 1, 2, "fused"), "center node is not in initial TreeTN"),
                          ((3, 0, 0, 2, "gemm"), "targets must not be empty"), ((3, 0, 1, 2, "auto"), "route must be fused or gemm")):
        with pytest.raises(t4a_amd.T4aError, match=message):
            t4a_amd.fit_sum_plan(*args)


def test_the_route_rule():
    """DESIGN.md §8 "Variational sum": the one launch wherever it measured faster than the GEMM composition (target bonds 8 .. 256),
    which is everywhere but a single target of bond 128 or more; unmeasured bonds above 256 go to the GEMM"""
    import t4a_amd
    for bond in (1, 8, 16, 32, 64, 127):
        assert t4a_amd.fit_sum_route(1, bond, 32, 2) == "fused"
    for bond in (128, 256, 257):
        assert t4a_amd.fit_sum_route(1, bond, 32, 2) == "gemm"
    for K in (2, 4, 16, 256):
        for bond in (1, 8, 16, 33, 64, 128, 256):
            assert t4a_amd.fit_sum_route(K, bond, 32, 2) == "fused"
        for bond in (257, 1000):
            assert t4a_amd.fit_sum_route(K, bond, 32, 2) == "gemm"
    with pytest.raises(t4a_amd.T4aError, match="targets must not be empty"):
        t4a_amd.fit_sum_route(0, 8)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n, site, K", F.EXACT)
def test_restated_one_sweep_from_full_bonds_returns_the_sum(n, site, K):
    """measured: at most 1.4e-15 over the cases"""
    for w in (None, [1.0, 0.5, -2.0][:K]):
        targets, initial, w = F.exact_case(n, site, K, w)
        for center in (0, n - 1, n // 2):
            res, info = F.np_fit_sum(targets, initial, center, F.Options(), w)
            dev = np.linalg.norm(F.np_full(res) - F.np_sum(targets, w)) / F.scale_of(targets, w)
            assert dev <= 1e-12, (center, dev)
            assert info["sweeps_completed"] == 1 and info["local_updates"] == 2 * (n - 1) and len(info["norms"]) == 1


def test_restated_pair_that_cancels_exactly():
    targets, initial, w = F.exact_case(5, 3, 2, cancel=True)
    res, info = F.np_fit_sum(targets, initial, 2, F.Options(), w)
    assert np.linalg.norm(F.np_full(res)) <= 1e-12 * F.scale_of(targets, w) and np.all(np.isfinite(F.np_full(res)))


def test_restated_short_circuits_and_extensions():
    one = lambda v: [np.array(v, dtype=np.float64).reshape(1, 2, 1)]  # noqa: E731
    res, info = F.np_fit_sum([one([1.0, 2.0]), one([3.0, 4.0])], one([0.0, 0.0]), 0, F.Options(nfullsweeps=1))
    assert np.array_equal(res[0].reshape(-1), [4.0, 6.0]) and info["link_dims"] == []  # the doc test of the reference
    targets, initial, _ = F.exact_case(4, 2, 3)
    res, info = F.np_fit_sum(targets, initial, 1, F.Options(nfullsweeps=0))
    assert info["sweeps_completed"] == 0 and all(np.array_equal(a, b) for a, b in zip(res, initial))
    res, info = F.np_fit_sum(targets, None, 1, F.Options(nfullsweeps=0))
    assert all(np.array_equal(a, b) for a, b in zip(res, targets[0]))
    # coefficients are the sum of scaled targets
    w = [0.5, -1.5, 2.0]
    scaled = [[t[0] * wk] + t[1:] for t, wk in zip(targets, w)]
    a, _ = F.np_fit_sum(targets, initial, 2, F.Options(), w)
    b, _ = F.np_fit_sum(scaled, initial, 2, F.Options())
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="SVD factorization does not accept qr_rtol"):
        F.np_fit_sum(targets, initial, 0, F.Options(qr_rtol=1e-10))


def test_restated_with_no_option_set_the_link_dims_stay_those_of_the_initial():
    targets, initial = F.CASES["cap"][0], F.CASES["cap"][1]
    for center in (0, 3, 5):
        res, info = F.np_fit_sum(targets, initial, center, F.Options(nfullsweeps=3))
        assert info["link_dims"] == F.links(initial) == [2, 2, 2, 2, 2]
    grown, info = F.np_fit_sum(targets, initial, 0, F.Options(nfullsweeps=3, svd_policy=(1e-12, 0, 0, 0)))
    assert max(info["link_dims"]) > 2  # a policy lifts the cap


def test_restated_with_max_bond_dim_no_bond_ever_exceeds_the_cap():
    for name in ("cap", "stop", "k40"):
        t, i, c, o, w = F.CASES[name]
        log = []
        res, info = F.np_fit_sum(t, i, c, o, w, log=log)
        assert all(keep <= o.max_bond_dim for _, _, keep, _, _ in log) and max(info["link_dims"]) <= o.max_bond_dim
        assert any(keep < len(s) for _, s, keep, _, _ in log), name  # the case truncates


def test_restated_early_stop():
    t, i, c, o, w = F.CASES["stop"]
    res, info = F.np_fit_sum(t, i, c, o, w)
    assert info["converged"] and 1 < info["sweeps_completed"] < o.nfullsweeps and len(info["norms"]) == info["sweeps_completed"]
    # the decision of every sweep is clear of the tolerance, so a device whose norms differ in the last digits stops at the same sweep
    assert all(abs(ch / o.convergence_tol - 1.0) >= 1e-3 for ch in info["changes"])
    never, info = F.np_fit_sum(t, i, c, F.Options(nfullsweeps=3, max_bond_dim=2))
    assert not info["converged"] and info["sweeps_completed"] == 3


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_gap_condition_of_the_truncating_gpu_cases(name):
    """at every cut the singular values of the restatement have a relative gap of at least 1e-6, and a policy's decision the same margin"""
    t, i, c, o, w = F.CASES[name]
    log = []
    F.np_fit_sum(t, i, c, o, w, log=log)
    g = F.gaps(log)
    assert g, "the case does not truncate"
    assert min(x[0] for x in g) >= F.GAP and min(x[1] for x in g) >= F.GAP
    for extra, center, opts in (("fixed", 4, F.Options(nfullsweeps=2)), ("none", 1, F.Options(nfullsweeps=3, svd_policy=(1e-10, 0, 0, 0)))):
        if name != "cap":
            continue
        log = []  # the two further truncating runs of tests/test_gpu_fit_sum.py on the targets of "cap"
        F.np_fit_sum(t, i if extra == "fixed" else None, center, opts, log=log)
        g = F.gaps(log)
        assert not g or (min(x[0] for x in g) >= F.GAP and min(x[1] for x in g) >= F.GAP), extra
