"""Quantics transform operators on the device (tensor4all-quanticstransform): the upload, MPO.transpose, apply through the MPO
contraction, the difference kernel and a quantics TCI shifted end to end.  Where a tolerance is needed it is `close` of
test_gpu_mpo.py (1e-10 of max(1, max|want|)); uploads, transposes and the difference kernel's site tensors are compared exactly."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import quanticstransform as qt
from t4a_amd import MPO, SimpleTensorTrain, ContractionAlgorithm, ContractionOptions
from t4a_amd.quanticstransform import BoundaryCondition as BC, TriangleType, AffineParams
from test_cpu_quanticstransform import dense, dense_op, shift_matrix, flip_matrix, embed
from test_gpu_mpo import random_tensors, close, SEED

pytestmark = pytest.mark.gpu

P, AP, OPEN = BC.Periodic, BC.AntiPeriodic, BC.Open


def random_qtt(r, site_dim, max_bond, seed):
    """a random train with the LCG of test_gpu_mpo.py; bonds grow as far as the site dimension allows, capped at max_bond"""
    bonds = [min(max_bond, site_dim ** min(k, r - k)) for k in range(r + 1)]
    cores = [t[:, :, 0, :] for t in random_tensors(bonds, site_dim, 1, seed)]
    return SimpleTensorTrain(cores), cores


def to_vector(tt, r):
    """values of a train with one bit per variable at each site, at the flat index v0 + 2^r v1 + ..."""
    d = tt.site_dims()[0]
    nvar = d.bit_length() - 1
    flat = np.arange(1 << (r * nvar))
    idx = np.zeros((flat.size, r), dtype=np.int64)
    for k in range(r):
        for v in range(nvar):
            idx[:, k] += ((flat >> (r * v + r - 1 - k)) & 1) << v
    return tt.evaluate(idx)


# ------------------------------------------------------------------------------------------------ upload and transpose
def operators():
    return [qt.shift_operator(5, 7, AP), qt.flip_operator(4, OPEN), qt.cumsum_operator(6), qt.triangle_operator(3, TriangleType.Upper),
            qt.shift_operator_multivar(3, -2, P, 3, 1), qt.flip_operator_multivar(3, AP, 2, 0),
            qt.affine_operator(4, AffineParams.from_integers([1, 1, 0, 2, 1, 0], [11, -3], 2, 3), [P, P]),
            qt.affine_operator(4, AffineParams([(1, 2), (1, 2), (1, 2), (-1, 2)], [2, 3], 2, 2), [OPEN, OPEN])]


def test_upload_is_exact_and_cached():
    for op in operators():
        m = op.mpo()
        assert m is op.mpo()
        host, dev = op.site_tensors(), m.site_tensors()
        assert len(host) == len(dev) == len(op)
        for a, b in zip(host, dev):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert m.site_dims() == op.site_dims() and m.link_dims() == op.link_dims()


def test_transpose_on_the_device():
    for op in operators():
        m = op.mpo()
        once = m.transpose()
        assert once.site_dims() == [(b, a) for a, b in m.site_dims()]
        for a, b in zip(m.site_tensors(), once.site_tensors()):
            assert np.array_equal(b, np.swapaxes(a, 1, 2))
        for a, b in zip(m.site_tensors(), once.transpose().site_tensors()):
            assert np.array_equal(a, b)
    # a random (not 0 / 1) rectangular MPO as well
    ts = random_tensors([1, 3, 4, 1], 2, 5, SEED)
    tr = MPO(ts).transpose()
    for a, b in zip(ts, tr.site_tensors()):
        assert np.array_equal(b, np.swapaxes(a, 1, 2))
    assert MPO([]).transpose().len() == 0


def test_transposed_affine_is_the_transposed_matrix():
    for r, params, bc in ((3, AffineParams.from_integers([1, 1, 1, -1], [0, 0], 2, 2), [P, P]),
                          (3, AffineParams.from_integers([1, 0], [2], 1, 2), [OPEN]),
                          (4, AffineParams([(1, 3)], [1], 1, 1), [AP])):
        want = qt.affine_transform_matrix(r, params, bc)
        tr = qt.affine_operator(r, params, bc).mpo().transpose()
        assert np.array_equal(dense(tr.site_tensors(), r), want.T)


# ------------------------------------------------------------------------------------------------ apply
def single_variable_cases(r):
    n = 1 << r
    i, j = np.indices((n, n))
    for offset in (0, 1, -3, 300):
        for bc in (P, AP, OPEN):
            yield f"shift {offset} bc {bc}", qt.shift_operator(r, offset, bc), shift_matrix(r, offset, bc)
    for bc in (P, AP, OPEN):
        yield f"flip bc {bc}", qt.flip_operator(r, bc), flip_matrix(r, bc)
    yield "cumsum", qt.cumsum_operator(r), (i > j).astype(float)
    yield "triangle upper", qt.triangle_operator(r, TriangleType.Upper), (i < j).astype(float)


def test_apply_exact_product():
    r = 8
    g, _ = random_qtt(r, 2, 8, SEED)
    gv = to_vector(g, r)
    for name, op, mat in single_variable_cases(r):
        out = qt.apply(op, g)
        assert out.site_dims() == [2] * r, name
        assert out.link_dims() == [a * b for a, b in zip(op.link_dims(), g.link_dims())], name
        close(to_vector(out, r), mat @ gv)


@pytest.mark.parametrize("algorithm, options", [(ContractionAlgorithm.ZipUp, None), (ContractionAlgorithm.ZipUp, ContractionOptions()),
                                                (ContractionAlgorithm.Naive, ContractionOptions())])
def test_apply_truncating(algorithm, options):
    r = 8
    g, _ = random_qtt(r, 2, 8, SEED + 1)
    gv = to_vector(g, r)
    for name, op, mat in single_variable_cases(r):
        out = qt.apply(op, g, algorithm, options)
        assert out.site_dims() == [2] * r, name
        close(to_vector(out, r), mat @ gv)


def test_apply_accepts_an_mpo():
    r = 6
    g, _ = random_qtt(r, 2, 4, SEED + 2)
    op = qt.shift_operator(r, 5, P)
    close(to_vector(qt.apply(op.mpo(), g), r), shift_matrix(r, 5, P) @ to_vector(g, r))
    close(to_vector(qt.apply(qt.identity_mpo(r), g), r), to_vector(g, r))
    with pytest.raises(t4a_amd.T4aError) as e:
        qt.apply(qt.shift_operator(r - 1, 1, P), g)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    with pytest.raises(t4a_amd.T4aError) as e:
        qt.apply(qt.shift_operator_multivar(r, 1, P, 2, 0), g)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "Shared shape mismatch at site 0" in e.value.message


def test_two_variables():
    r = 5
    n = 1 << r
    g, _ = random_qtt(r, 4, 8, SEED + 3)
    gv = to_vector(g, r)
    op = qt.shift_operator_multivar(r, 3, AP, 2, 1)
    out = qt.apply(op, g)
    assert out.site_dims() == [4] * r
    close(to_vector(out, r), embed(shift_matrix(r, 3, AP), r, 2, 1) @ gv)
    # pull-back f(x, y) = g(x + y, x - y): the transpose of the forward operator of A = [[1, 1], [1, -1]] (column-major below)
    params = AffineParams.from_integers([1, 1, 1, -1], [0, 0], 2, 2)
    forward = qt.affine_operator(r, params, [P, P])
    pulled = qt.apply(forward.mpo().transpose(), g)
    assert pulled.site_dims() == [4] * r
    got = to_vector(pulled, r)
    close(got, qt.affine_transform_matrix(r, params, [P, P]).T @ gv)
    x, y = np.arange(n * n) % n, np.arange(n * n) // n
    close(got, gv[(x + y) % n + n * ((x - y) % n)])


# ------------------------------------------------------------------------------------------------ difference kernel
def np_difference_kernel(f_cores, bc):
    """difference_kernel.rs:59-101 with numpy: out[dl * fL + fl, x, x', dr * fR + fr] = sum_z delta[dl, z, x + 2 x', dr] f[fl, z, fr]"""
    r = len(f_cores)
    delta = qt.affine_operator(r, AffineParams.from_integers([1, -1], [0], 1, 2), [bc]).site_tensors()
    out = []
    for d, f in zip(delta, f_cores):
        t = np.einsum("dzpe,fzg->dfpeg", d, f)
        left, right = d.shape[0] * f.shape[0], d.shape[3] * f.shape[2]
        out.append(t.reshape(left, 2, 2, right).transpose(0, 2, 1, 3))  # p = x + 2 x' -> [x', x] -> (x, x')
    return out


@pytest.mark.parametrize("r", [2, 4, 6])
@pytest.mark.parametrize("bc", [P, AP])
def test_difference_kernel(r, bc):
    n = 1 << r
    f, cores = random_qtt(r, 2, 4, SEED + 10 + r)
    k = qt.difference_kernel_mpo(f, bc)
    assert k.site_dims() == [(2, 2)] * r
    assert k.link_dims() == [2 * b for b in f.link_dims()]
    for got, want in zip(k.site_tensors(), np_difference_kernel(cores, bc)):
        assert got.shape == want.shape and np.array_equal(got, want)
    fv = to_vector(f, r)
    x, xp = np.indices((n, n))
    want = fv[(x - xp) % n] * (np.where(x < xp, -1.0, 1.0) if bc == AP else 1.0)
    close(dense(k.site_tensors(), r), want)


def test_difference_kernel_is_a_convolution():
    r = 8
    n = 1 << r
    f, _ = random_qtt(r, 2, 4, SEED + 20)
    g, _ = random_qtt(r, 2, 8, SEED + 21)
    fv, gv = to_vector(f, r), to_vector(g, r)
    out = qt.apply(qt.difference_kernel_mpo(f, P), g)
    x, xp = np.indices((n, n))
    close(to_vector(out, r), fv[(x - xp) % n] @ gv)


def test_difference_kernel_refusals():
    f, _ = random_qtt(3, 2, 2, SEED)
    for call, needle in ((lambda: qt.difference_kernel_mpo(f, OPEN), "Open boundary is not supported for difference kernels"),
                         (lambda: qt.difference_kernel_mpo(SimpleTensorTrain([]), P), "difference kernel requires a non-empty QTT"),
                         (lambda: qt.difference_kernel_mpo(random_qtt(3, 4, 2, SEED)[0], P),
                          "difference kernel requires binary QTT cores; site 0 has site_dim=4")):
        with pytest.raises(t4a_amd.T4aError) as e:
            call()
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and needle in e.value.message


# ------------------------------------------------------------------------------------------------ end to end
def test_shift_of_a_quantics_tci():
    """quanticscrossinterpolate -> tensor_train -> apply(shift, Open): the shifted train against f(x_{i-37}), zero for i < 37.  The
    bound is what the unshifted train deviates from f, measured here, plus `close`'s 1e-10 of the scale."""
    r, offset = 10, 37
    n = 1 << r

    def f(x):
        return np.exp(-3.0 * x[0]) * np.cos(9.0 * x[0]) + 0.5 * x[0]

    f.batched = lambda pts: np.exp(-3.0 * pts[:, 0]) * np.cos(9.0 * pts[:, 0]) + 0.5 * pts[:, 0]
    q = t4a_amd.quanticscrossinterpolate([r], f, [0.0], [1.0], options=t4a_amd.QtciOptions(tolerance=1e-10, seed=11))
    tt = q.tensor_train()
    assert tt.site_dims() == [2] * r
    xs = np.arange(n) / n
    exact = f.batched(xs[:, None])
    have = to_vector(tt, r)
    deviation = float(np.abs(have - exact).max())
    print(f"unshifted train deviates from f by {deviation:.3e}")
    assert deviation < 1e-6  # the interpolation itself (tolerance 1e-10) and the bit order of to_vector, not the bound below
    shifted = to_vector(qt.apply(qt.shift_operator(r, offset, OPEN), tt), r)
    want = np.concatenate([np.zeros(offset), exact[:n - offset]])
    err = float(np.abs(shifted - want).max())
    print(f"shifted train deviates from the shifted f by {err:.3e}")
    assert err <= deviation + 1e-10 * max(1.0, float(np.abs(want).max()))
