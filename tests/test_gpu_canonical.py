"""The gauge forms on the device — SiteTensorTrain / center_canonicalize, VidalTensorTrain, InverseTensorTrain (t4a_amd.canonical) — against
the numpy restatement of the reference algorithm (tests/canonical_np.py, rrLU through the CPU oracle).

What is compared how:
  * a re-gauged core is left(true) (or its transpose) of an rrLU whose factored matrix is bit-identical to the oracle's: bit for bit;
  * a core that absorbed the other factor went through a GEMM: the componentwise bound gamma_k (|F| |core|), k the contracted bond,
    u = 2^-53, which holds for any summation order, fused or not;
  * values that passed through GEMMs: 1e-10 max|value| (the figure of tests/test_gpu_tt.py); singular values 1e-12 lambda_max and
    orthonormality 1e-11 (the figures of the svd_backend tests at these sizes);
  * the Vidal / inverse arithmetic (one or two correctly rounded operations per element): bit for bit against numpy;
  * on the monomial chains D1 / D2 no operation rounds: whole objects are equal double for double; only the sign of a zero is left
    open (a product sum of zeros is +0.0 or -0.0 depending on what it is accumulated from, and 0 / pivot inherits it).
"""
import numpy as np
import pytest

import canonical_np as cn
from luci_exact_np import gamma, _ratio_to_product_bound

pytestmark = pytest.mark.gpu

FIXTURES = {"A": cn.fixture_a, "B": cn.fixture_b, "C": cn.fixture_c, "E": cn.fixture_e, "E2": cn.fixture_e2}
SCALE_MAX_BLOCKS = 1024  # TT_SCALE_MAX_BLOCKS (kernels.hpp): a launch of more items walks the item loop a second time


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def equal_values(a, b):  # equal doubles, the sign of a zero left open
    return bits(np.asarray(a) + 0.0, np.asarray(b) + 0.0)


def within_product_bound(dev, a, b):
    """|dev - a b| <= gamma_k |a| |b| entry by entry, the product formed exactly"""
    k = a.shape[1]
    ratio = _ratio_to_product_bound(np.ascontiguousarray(dev), np.ascontiguousarray(a), np.ascontiguousarray(b))  # against 2 gamma_{k+2}
    return ratio * 2 * gamma(k + 2) / gamma(k) <= 1.0


def reference_values(cores, pts):
    full = cn.dense(cores)
    return full[tuple(pts.T)], float(np.abs(full).max())


def points_of(name, cores):
    dims = [c.shape[1] for c in cores]
    return cn.lcg_points(256, dims, 11) if name in ("E", "E2") else cn.all_points(dims)


def has_unit_lower_rows(m):
    """m (rows x r): entries of magnitude <= 1 and, for every column k, a row that is (*, .., *, 1.0, 0.0, .., 0.0) with the 1.0 at k"""
    if np.abs(m).max() > 1.0:
        return False
    r = m.shape[1]
    return all(any(row[k] == 1.0 and not np.any(row[k + 1:]) for row in m) for k in range(r))


# ------------------------------------------------------------------------------------------------ 1. step parity
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_every_gauge_step_from_the_devices_own_state(t4a, name):
    cores = FIXTURES[name]()
    n = len(cores)
    s = t4a.SiteTensorTrain.from_tensor_train(t4a.SimpleTensorTrain(cores), 0)
    assert s.center() == 0 and s.len() == n and s.partition() == range(0, n)
    assert s.link_dims() == [c.shape[0] for c in cn.site_form(cores, 0)[1:]]
    if name == "C":  # the zeroed index of bond 2: the right step at site 2 met an exactly zero pivot
        assert s.link_dims()[1] == 4 and cores[2].shape[0] == 5
    for i in range(n - 1):  # centre i -> i + 1
        a, b = s.site_tensor(i), s.site_tensor(i + 1)
        s.move_center_right()
        na, nb = s.site_tensor(i), s.site_tensor(i + 1)
        wa, wb = cn.left_step(a, b)
        assert s.center() == i + 1 and na.shape == wa.shape and nb.shape == wb.shape, i
        assert bits(na, wa), i
        _, r = cn.step_factors(a, True)
        assert within_product_bound(cn.right_matrix(nb), r, cn.right_matrix(b)), i
    if name == "C":
        assert s.link_dims()[1] == 4
    for i in range(n - 1, 0, -1):  # centre i -> i - 1
        a, b = s.site_tensor(i - 1), s.site_tensor(i)
        s.move_center_left()
        na, nb = s.site_tensor(i - 1), s.site_tensor(i)
        wa, wb = cn.right_step(a, b)
        assert s.center() == i - 1 and na.shape == wa.shape and nb.shape == wb.shape, i
        assert bits(nb, wb), i
        _, lt = cn.step_factors(b, False)
        assert within_product_bound(cn.left_matrix(na), cn.left_matrix(a), lt.T), i
    pts = points_of(name, cores)
    want, scale = reference_values(cores, pts)
    assert np.abs(s.to_tensor_train().evaluate(pts) - want).max() <= 1e-10 * scale


# ------------------------------------------------------------------------------------------------ 2. whole objects, exact
def _walk(t, center, target):
    t = [c.copy() for c in t]
    while center < target:
        t[center], t[center + 1] = cn.left_step(t[center], t[center + 1])
        center += 1
    while center > target:
        t[center - 1], t[center] = cn.right_step(t[center - 1], t[center])
        center -= 1
    return t


def _same_object(got, want, center):
    """every core as equal doubles: a zero of either sign that a product sum left in an absorbed core turns up as 0 / pivot in the
    cores gauged after it, so the sign of zeros is open in all of them"""
    return len(got) == len(want) and all(equal_values(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", ["d1", "d2"])
def test_monomial_chains_equal_the_restatement(t4a, name):
    cores = getattr(cn, "fixture_" + name)()
    n = len(cores)
    tt = t4a.SimpleTensorTrain(cores)
    for center in range(n):
        want = cn.site_form(cores, center)
        s = t4a.SiteTensorTrain.from_tensor_train(tt, center)
        assert _same_object(s.site_tensors(), want, center), center
        assert all(equal_values(g, w) for g, w in zip(s.site_tensors(), cn.exact_site_form(cores, center))), center
        plain = tt.clone()
        t4a.center_canonicalize(plain, center)
        assert _same_object(plain.site_tensors(), want, center), center
        other = n - 1 if center < n - 1 else 0
        s.set_center(other)
        assert s.center() == other and _same_object(s.site_tensors(), _walk(want, center, other), other), center
        s.set_center(center)
        assert s.center() == center and _same_object(s.site_tensors(), _walk(_walk(want, center, other), other, center), center), center
    assert all(bits(g, c) for g, c in zip(tt.site_tensors(), cores))  # the source train is untouched


# ------------------------------------------------------------------------------------------------ 3. whole objects, values
def _cases():
    out = [(k, f()) for k, f in sorted(FIXTURES.items())]
    f1, f2 = cn.fixture_f()
    return out + [("F1", f1), ("F2", f2)]


@pytest.mark.parametrize("name,cores", _cases(), ids=[k for k, _ in _cases()])
def test_site_form_values_bonds_and_gauge(t4a, name, cores):
    n = len(cores)
    tt = t4a.SimpleTensorTrain(cores)
    pts = points_of(name, cores)
    want, scale = reference_values(cores, pts)
    centers = sorted({0, n // 2, n - 1})
    forms = {}
    for c in centers:
        s = t4a.SiteTensorTrain.from_tensor_train(tt, c)
        forms[c] = s.site_tensors()
        assert s.center() == c and s.site_dims() == [x.shape[1] for x in cores]
        assert np.abs(s.to_tensor_train().evaluate(pts) - want).max() <= 1e-10 * scale, c
        assert np.abs(s.evaluate(pts) - want).max() <= 1e-10 * scale, c  # the trait on the stored tensors: the same train here
        ref = cn.site_form(cores, c)
        assert [x.shape for x in forms[c]] == [x.shape for x in ref], c
        assert s.link_dims() == [x.shape[0] for x in ref[1:]] and s.rank() == max([1] + s.link_dims())
        for i in range(c):
            assert has_unit_lower_rows(cn.left_matrix(forms[c][i])), (c, i)
        for i in range(c + 1, n):
            assert has_unit_lower_rows(cn.right_matrix(forms[c][i]).T), (c, i)
        plain = tt.clone()
        t4a.center_canonicalize(plain, c)
        assert all(bits(g, w) for g, w in zip(plain.site_tensors(), forms[c])), c
    for c in centers:  # the cores left of c do not depend on the centre
        for c2 in centers:
            if c2 > c:
                assert all(bits(forms[c][i], forms[c2][i]) for i in range(c)), (c, c2)
    if name == "B":
        assert t4a.SiteTensorTrain.from_tensor_train(tt, n - 1).link_dims() == [2, 4, 4] and t4a.SiteTensorTrain.from_tensor_train(tt, 0).link_dims() == [4, 4, 2]


# ------------------------------------------------------------------------------------------------ 4. Vidal
def _vidal_cases():
    out = [(k, FIXTURES[k](), None) for k in ("A", "B", "E", "E2")]
    f1, f2 = cn.fixture_f()
    return out + [("F1", f1, None), ("F2", f2, None), ("A[1..4]", cn.fixture_a(), (1, 4)), ("A[0..n]", cn.fixture_a(), (0, 5))]


@pytest.mark.parametrize("name,cores,part", _vidal_cases(), ids=[k for k, _, _ in _vidal_cases()])
def test_vidal_form(t4a, name, cores, part):
    n = len(cores)
    tt = t4a.SimpleTensorTrain(cores)
    start, end = part if part else (0, n)
    v = t4a.VidalTensorTrain.from_tensor_train_with_partition(tt, range(start, end)) if part else t4a.VidalTensorTrain.from_tensor_train(tt)
    assert v.len() == n and v.partition() == range(start, end)
    ref_t, ref_sv = cn.vidal_form(cores, start, end)
    sv = v.all_singular_values()
    assert len(sv) == n - 1 and [len(x) for x in sv] == [len(x) for x in ref_sv]
    assert [x.shape for x in v.site_tensors()] == [x.shape for x in ref_t]
    for b, (x, y) in enumerate(zip(sv, ref_sv)):
        if len(y):
            assert np.abs(x - y).max() <= 1e-12 * y.max(), b
            assert np.all(np.diff(x) <= 0) and np.all(x >= 0), b
    pts = points_of(name[0] if name[0] != "E" else name, cores)
    want, scale = reference_values(cores, pts)
    assert np.abs(v.to_tensor_train().evaluate(pts) - want).max() <= 1e-10 * scale
    assert cn.rows_orthonormal_defect(v.site_tensors(), sv, start, end) <= 1e-11


def test_vidal_on_the_rank_deficient_train_and_its_errors(t4a):
    cores = cn.fixture_c()
    tt = t4a.SimpleTensorTrain(cores)
    v = t4a.VidalTensorTrain.from_tensor_train(tt)
    ref_sv = cn.vidal_form(cores)[1]
    sv = v.all_singular_values()
    assert [len(x) for x in sv] == [len(x) for x in ref_sv]
    assert [int(np.sum(x > 1e-12 * x.max())) for x in sv] == [int(np.sum(x > 1e-12 * x.max())) for x in ref_sv]
    pts = cn.all_points([c.shape[1] for c in cores])
    want, scale = reference_values(cores, pts)
    assert np.abs(v.to_tensor_train().evaluate(pts) - want).max() <= 1e-10 * scale
    with pytest.raises(t4a.T4aError) as e:
        t4a.VidalTensorTrain.from_tensor_train_with_partition(tt, range(0, 6))
    assert e.value.code == t4a.INVALID_ARGUMENT and "Partition end 6 exceeds tensor train length 5" in e.value.message
    empty = t4a.VidalTensorTrain.from_tensor_train(t4a.SimpleTensorTrain([]))
    assert empty.len() == 0 and empty.partition() == range(0, 0) and len(empty.to_tensor_train()) == 0


# ------------------------------------------------------------------------------------------------ 5. scale kernel, exact
def _scale_cases():
    return [("G", cn.fixture_g()), ("G-large", cn.fixture_g_large(SCALE_MAX_BLOCKS))]


@pytest.mark.parametrize("name,data", _scale_cases(), ids=[k for k, _ in _scale_cases()])
def test_bond_scale_kernel_bit_for_bit(t4a, name, data):
    cores, vecs = data
    if name == "G-large":  # (256, 2, r): r / 2 items of four 256-lane columns, more than the launch has workgroups
        assert cores[1].shape[1] * cores[1].shape[2] // 4 > SCALE_MAX_BLOCKS
    with np.errstate(over="ignore", invalid="ignore"):
        v = t4a.VidalTensorTrain.new(cores, vecs)
        assert all(bits(g, c) for g, c in zip(v.site_tensors(), cores)) and all(bits(g, x) for g, x in zip(v.all_singular_values(), vecs))
        assert all(bits(g, w) for g, w in zip(v.to_tensor_train().site_tensors(), cn.vidal_to_tt(cores, vecs)))
        inv = t4a.InverseTensorTrain.from_vidal(v)
        want_t, want_inv = cn.inverse_from_vidal(cores, vecs)
        assert all(bits(g, w) for g, w in zip(inv.site_tensors(), want_t))
        assert all(bits(g, w) for g, w in zip(inv.all_inverse_singular_values(), want_inv))
        assert all(bits(g, w) for g, w in zip(inv.to_tensor_train().site_tensors(), cn.inverse_to_tt(want_t, want_inv)))
    assert inv.partition() == range(0, len(cores)) and inv.link_dims() == v.link_dims()


# ------------------------------------------------------------------------------------------------ 6. inverse form from a train
def test_inverse_from_tensor_train(t4a):
    cores = cn.fixture_a()
    tt = t4a.SimpleTensorTrain(cores)
    direct = t4a.InverseTensorTrain.from_tensor_train(tt)
    v = t4a.VidalTensorTrain.from_tensor_train(tt)
    via = t4a.InverseTensorTrain.from_vidal(v)
    assert all(bits(a, b) for a, b in zip(direct.site_tensors(), via.site_tensors()))
    assert all(bits(a, b) for a, b in zip(direct.all_inverse_singular_values(), via.all_inverse_singular_values()))
    # and both are the arithmetic of from_vidal on what the Vidal form holds
    want_t, want_inv = cn.inverse_from_vidal(v.site_tensors(), v.all_singular_values())
    assert all(bits(a, b) for a, b in zip(via.site_tensors(), want_t)) and all(bits(a, b) for a, b in zip(via.all_inverse_singular_values(), want_inv))
    pts = cn.all_points([c.shape[1] for c in cores])
    want, scale = reference_values(cores, pts)
    assert np.abs(direct.to_tensor_train().evaluate(pts) - want).max() <= 1e-10 * scale


# ------------------------------------------------------------------------------------------------ 7. setters and argument errors
def _raises(t4a, call, needle):
    with pytest.raises(t4a.T4aError) as e:
        call()
    assert e.value.code == t4a.INVALID_ARGUMENT and needle in e.value.message, (needle, e.value.message)


def test_setters_replace_without_regauging(t4a):
    cores = cn.fixture_a()
    n = len(cores)
    rng = np.random.default_rng(cn.SEED + 20)
    tt = t4a.SimpleTensorTrain(cores)
    pts = cn.all_points([c.shape[1] for c in cores])
    s = t4a.SiteTensorTrain.from_tensor_train(tt, 2)
    before = s.site_tensors()
    t0 = rng.standard_normal(before[0].shape)
    t1, t2 = rng.standard_normal((2, 3, 7)), rng.standard_normal((7, 2, 6))
    s.set_site_tensor(0, t0)
    s.set_two_site_tensors(1, t1, t2)
    now = s.site_tensors()
    assert s.center() == 2 and s.link_dims() == [2, 7, 6, 3]  # dims follow
    assert bits(now[0], t0) and bits(now[1], t1) and bits(now[2], t2) and bits(now[3], before[3]) and bits(now[4], before[4])
    assert bits(s.tensors_tt().evaluate(pts), cn.evaluate_seq(now, pts)) and bits(s.evaluate(pts), cn.evaluate_seq(now, pts))
    assert s.sum() == s.tensors_tt().sum() and s.norm2() == s.to_tensor_train().norm2()
    _raises(t4a, lambda: s.set_two_site_tensors(n - 1, t1, t2), "Cannot set two-site tensors at site 4 (max 3)")
    _raises(t4a, lambda: s.set_site_tensor(n, t0), "site 5 is out of range")
    _raises(t4a, lambda: s.set_site_tensor(0, np.zeros((2, 2))), "three legs")
    s.set_site_tensor(3, rng.standard_normal((5, 4, 3)))  # a bond that no longer chains is stored, and refused when a train is asked for
    _raises(t4a, lambda: s.tensors_tt(), "bond dimension mismatch")
    # centre and partition errors carry the reference's messages
    _raises(t4a, lambda: t4a.SiteTensorTrain.from_tensor_train(tt, n), "Center 5 is out of range for 5 tensors")
    _raises(t4a, lambda: t4a.SiteTensorTrain.from_tensor_train(t4a.SimpleTensorTrain([]), 0), "Tensor train is empty")
    s = t4a.SiteTensorTrain.new(cores, 0)
    _raises(t4a, lambda: s.set_center(n), "New center 5 is out of range for 5 tensors")
    _raises(t4a, s.move_center_left, "Cannot move center left: already at leftmost position")
    s.set_center(n - 1)
    _raises(t4a, s.move_center_right, "Cannot move center right: already at rightmost position")
    plain = tt.clone()
    t4a.center_canonicalize(plain, n)  # a silent no-op, as in the reference
    assert all(bits(g, c) for g, c in zip(plain.site_tensors(), cores))

    v = t4a.VidalTensorTrain.from_tensor_train(tt)
    held = v.site_tensors()
    lam = np.array([2.0, -0.5, 3.0, 0.25, 1.0, 7.0, 9.0])  # longer than the bond of 5: ignored beyond it
    v.set_singular_values(1, lam)
    g1 = rng.standard_normal(held[3].shape)
    v.set_site_tensor(3, g1)
    held[3] = g1
    sv = v.all_singular_values()
    assert bits(sv[1], lam) and all(bits(g, w) for g, w in zip(v.site_tensors(), held))
    assert all(bits(g, w) for g, w in zip(v.to_tensor_train().site_tensors(), cn.vidal_to_tt(held, sv)))
    assert bits(v.evaluate(pts), cn.evaluate_seq(held, pts))
    _raises(t4a, lambda: v.set_singular_values(n - 1, lam), "bond 4 is out of range")

    inv = t4a.InverseTensorTrain.from_vidal(v)
    held = inv.site_tensors()
    a1, a2, isv = rng.standard_normal((5, 2, 4)), rng.standard_normal((4, 4, 3)), np.array([0.5, 4.0])  # shorter than the bond of 4
    inv.set_two_site_tensors(2, a1, isv, a2)
    held[2], held[3] = a1, a2
    ivs = inv.all_inverse_singular_values()
    assert bits(ivs[2], isv) and inv.link_dims() == [2, 5, 4, 3] and all(bits(g, w) for g, w in zip(inv.site_tensors(), held))
    assert all(bits(g, w) for g, w in zip(inv.to_tensor_train().site_tensors(), cn.inverse_to_tt(held, ivs)))
    assert bits(inv.tensors_tt().evaluate(pts), cn.evaluate_seq(held, pts))
    _raises(t4a, lambda: inv.set_two_site_tensors(n - 1, a1, isv, a2), "Cannot set two-site tensors at site 4 (max 3)")
