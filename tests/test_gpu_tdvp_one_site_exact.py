"""The kernels of one-site TDVP on operands with small integer entries, where every product and sum is exact in f64 and the result must
equal int64 arithmetic bit for bit: the bond-centre apply on both routes (the fused launch inside its envelope, the two GEMMs
everywhere), the environment that prepare_bond_center builds with an integer-valued "Q" in both directions, and one driver sweep with
tau = 0, which must hand the state back at full-rank QR accuracy with the bond dimensions unchanged."""
import numpy as np
import pytest

import restructure_np as rn
import tdvp_one_site_np as t1
from tdvp_np import _left, _right
import t4a_amd
from t4a_amd import MPO, SimpleTensorTrain, ProjectedOperator, TdvpOptions, tdvp_one_site
from t4a_amd.tdvp import _apply_bond_center, _bond_apply_route, _bond_apply_fused_admits, _bond_center_env, BOND_FUSED, BOND_GEMM, BOND_AUTO

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (16, 16), (17, 16), (32, 33)]
WS = [1, 3, 5]


def integers(rng, shape):
    return rng.integers(-2, 3, size=shape).astype(np.float64)


def operands(ka, kb, w, seed):
    rng = np.random.default_rng(seed)
    return integers(rng, (ka, w, ka)), integers(rng, (kb, w, kb)), integers(rng, (ka, kb))


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("ka, kb", SHAPES)
def test_bond_apply_equals_integer_arithmetic_on_every_route(ka, kb, w):
    la, rb, c = operands(ka, kb, w, 1000 * ka + 10 * kb + w)
    want = t1.np_bond_apply_int(la, rb, c)
    assert np.abs(want).max() < 2 ** 50
    routes = [BOND_GEMM] + ([BOND_FUSED] if _bond_apply_fused_admits(ka, kb, w) else [])
    assert BOND_FUSED in routes  # every shape of this list lies inside the envelope
    for route in routes:
        y, taken = _apply_bond_center(la, rb, c, route)
        assert taken == route
        assert np.array_equal(y.astype(np.int64), want) and np.array_equal(y, np.round(y)), (route, int(np.abs(y - want).max()))
        again, _ = _apply_bond_center(la, rb, c, route)
        assert np.array_equal(y.view(np.uint64), again.view(np.uint64))
    y, taken = _apply_bond_center(la, rb, c, BOND_AUTO)
    assert taken == _bond_apply_route(ka, kb, w) and np.array_equal(y.astype(np.int64), want)


@pytest.mark.parametrize("ka, kb, w", [(16, 129, 4), (5, 171, 3), (32, 103, 5)])
def test_shapes_just_outside_the_fused_envelope_take_the_gemm(ka, kb, w):
    assert not _bond_apply_fused_admits(ka, kb, w) and _bond_apply_fused_admits(ka, kb - 1, w)
    la, rb, c = operands(ka, kb, w, 77 + kb)
    want = t1.np_bond_apply_int(la, rb, c)
    y, taken = _apply_bond_center(la, rb, c, BOND_AUTO)
    assert taken == BOND_GEMM == _bond_apply_route(ka, kb, w) and np.array_equal(y.astype(np.int64), want)
    with pytest.raises(t4a_amd.T4aError) as e:
        _apply_bond_center(la, rb, c, BOND_FUSED)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "W k_b must be at most 512" in e.value.message


def test_the_routes_agree_to_rounding_on_real_operands_and_repeat_their_bits():
    rng = np.random.default_rng(5)
    for ka, kb, w in ((17, 16, 3), (48, 40, 4), (7, 9, 2)):
        la, rb, c = rng.uniform(-1, 1, (ka, w, ka)), rng.uniform(-1, 1, (kb, w, kb)), rng.uniform(-1, 1, (ka, kb))
        want = t1.np_bond_apply(la, rb, c)
        scale = np.einsum("bwa,ac,dwc->bd", np.abs(la), np.abs(c), np.abs(rb)).max()
        for route in (BOND_FUSED, BOND_GEMM):
            y, _ = _apply_bond_center(la, rb, c, route)
            again, _ = _apply_bond_center(la, rb, c, route)
            assert np.array_equal(y.view(np.uint64), again.view(np.uint64))
            # two chained sums of ka and W kb terms, every partial sum bounded by `scale`: (ka + W kb + 2) eps scale
            assert np.abs(y - want).max() <= (ka + w * kb + 2) * 2.0 ** -52 * scale


def integer_chain(seed):
    """n = 4, d = 2, bonds (1, 3, 5, 3, 1), operator bond 3: integer entries; site c is overwritten with a signed permutation-like
    "isometry" padded with integer entries (only the contraction is tested, orthogonality is not needed)"""
    rng = np.random.default_rng(seed)
    bonds, wb = (1, 3, 5, 3, 1), (1, 3, 3, 3, 1)
    x = [integers(rng, (bonds[k], 2, bonds[k + 1])) for k in range(4)]
    ops = []
    for k in range(4):
        a = integers(rng, (wb[k], 2, 2, wb[k + 1]))
        ops.append(a + a.transpose(0, 2, 1, 3))
    return ops, x


def signed_permutation_like(rng, shape, toward_right):
    l, s, r = shape
    rows, cols = (l * s, r) if toward_right else (s * r, l)
    q = integers(rng, (rows, cols))
    k = min(rows, cols)
    q[:k, :k] = np.diag(rng.choice([-1.0, 1.0], size=k))[rng.permutation(k)]
    return q.reshape(shape, order="F") if toward_right else q.T.reshape(shape, order="F")


@pytest.mark.parametrize("c, toward_right", [(0, True), (1, True), (2, True), (1, False), (2, False), (3, False)])
def test_prepare_bond_center_builds_the_integer_contraction(c, toward_right):
    ops, x = integer_chain(40 + c)
    x[c] = signed_permutation_like(np.random.default_rng(c), x[c].shape, toward_right)
    po = ProjectedOperator(MPO(ops), SimpleTensorTrain(x))
    env = _bond_center_env(po, c, toward_right)
    left, right = _left(ops, x, c), _right(ops, x, c + 1)
    want = t1.np_left_env(left, ops[c], x[c]) if toward_right else t1.np_right_env(right, ops[c], x[c])
    assert env.shape == want.shape and np.abs(want).max() < 2 ** 50
    assert np.array_equal(env, want)
    # the environment is also the cache entry the next step reads
    got = po.environment(0, c + 1) if toward_right else po.environment(1, c)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("center", (0, 2, 4))
@pytest.mark.parametrize("order", (1, 2))
def test_a_sweep_with_tau_zero_returns_the_state(center, order):
    ops, init = t1.thin_case()
    n = len(ops)
    r = tdvp_one_site(MPO(ops), SimpleTensorTrain(init), center, TdvpOptions(nsite=1, order=order, exponent_step=0.0))
    dense = t1.np_state_full(init)
    w = len(t1.applyexp_sub_steps(order))
    n_qr = (n - 1) + r.stats["qr_steps"]  # the canonicalisation and the sweep
    err = np.linalg.norm(t1.np_state_full(r.state.site_tensors()) - dense)
    unit = n_qr * rn.EPS * np.linalg.norm(dense)
    print(center, order, "qr steps", n_qr, "error", err / unit, "n_qr eps |T| (allowed %.2f)" % rn.C_SPLIT)
    assert err <= rn.C_SPLIT * unit
    assert r.state.link_dims() == [t.shape[2] for t in t1.np_canonicalize(init, center)[:-1]]
    assert (r.stats["one_site_steps"], r.stats["bond_corrections"], r.local_updates) == (w * n, w * (n - 1), w * (2 * n - 1))
    assert r.stats["krylov_steps"] == r.stats["apply_calls"] == 0 and r.max_krylov_iterations == 0 and r.max_error_estimate == 0.0
