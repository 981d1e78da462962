"""MPO<f64> and MPO-MPO contraction on the device (tensor4all-simplett/src/mpo/) against a numpy restatement of the cited
algorithms: contract_site_tensors (environment.rs:37-80), compress_mpo (contract_naive.rs:100-172) with right_canonicalize
(canonical.rs:35-89), contract_zipup (contract_zipup.rs:45-167) and the SVD rank rule of factorize (factorize.rs:126-313).
The checker's SVD is numpy's: values are compared at 1e-10 relative, ranks and link dimensions exactly."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import mpo, MPO, ContractionOptions, ContractionAlgorithm, FactorizeMethod

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ numpy restatement
def random_tensors(bonds, s1, s2, seed):
    """random_mpo (test_support.rs:8-44): an LCG fills every site tensor column-major."""
    state = seed
    out = []
    for left, right in zip(bonds[:-1], bonds[1:]):
        vals = []
        for _ in range(left * s1 * s2 * right):
            state = (state * 6364136223846793005 + 1442695040888963407) & MASK
            vals.append((state >> 33) / float(1 << 31) - 0.5)
        out.append(np.array(vals).reshape((left, s1, s2, right), order="F"))
    return out


def np_site(a, b):
    """C[(la*Lb+lb), s1, t, (ra*Rb+rb)] = sum_k A[la,s1,k,ra] B[lb,k,t,rb]"""
    la, s1, _, ra = a.shape
    lb, _, t, rb = b.shape
    return np.einsum("askr,bktq->bastqr", a, b).reshape((lb * la, s1, t, rb * ra), order="F")


def np_factorize(mat, tol, max_bond_dim):
    u, s, vt = np.linalg.svd(mat, full_matrices=False)
    s_max = s.max() if s.size else 0.0
    rank = 0
    if s_max > 0:
        for v in s:
            if max_bond_dim is not None and rank >= max_bond_dim:
                break
            if v < tol * s_max:
                break
            rank += 1
    rank = max(rank, 1)
    return u[:, :rank], s[:rank, None] * vt[:rank], rank


def np_naive(a, b, options=None):
    ts = [np_site(x, y) for x, y in zip(a, b)]
    if options is None or len(ts) <= 1:
        return ts
    for i in range(len(ts) - 1, 0, -1):  # right_canonicalize
        l, s1, s2, r = ts[i].shape
        q, rr = np.linalg.qr(ts[i].reshape((l, s1 * s2 * r), order="F").T)
        k = q.shape[1]
        ts[i] = q.T.reshape((k, s1, s2, r), order="F")
        ts[i - 1] = np.einsum("ausl,lk->ausk", ts[i - 1], rr.T)
    for i in range(len(ts) - 1):
        l, s1, s2, r = ts[i].shape
        left, right, rank = np_factorize(ts[i].reshape((l * s1 * s2, r), order="F"), options.tolerance, options.max_bond_dim)
        ts[i] = left.reshape((l, s1, s2, rank), order="F")
        ts[i + 1] = np.einsum("lk,ksqr->lsqr", right, ts[i + 1])
    return ts


def np_zipup(a, b, options):
    rem = np.ones((1, 1, 1))
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        c = np.einsum("nbskc,bktd->nstcd", np.einsum("nab,askc->nbskc", rem, x), y)
        n0, s1, t, ca, cb = c.shape
        if i == len(a) - 1:
            out.append(c.reshape((n0, s1, t, 1), order="F"))
            break
        left, right, rank = np_factorize(c.reshape((n0 * s1 * t, ca * cb), order="F"), options.tolerance, options.max_bond_dim)
        out.append(left.reshape((n0, s1, t, rank), order="F"))
        rem = right.reshape((rank, ca, cb), order="F")
    return out


def np_full(ts):
    """dense operator indexed [i1, j1, i2, j2, ...]"""
    acc = ts[0][0]
    for t in ts[1:]:
        acc = np.tensordot(acc, t, axes=([-1], [0]))
    return acc[..., 0]


def np_eval(ts, idx):
    out = []
    for p in idx:
        v = np.ones((1,))
        for k, t in enumerate(ts):
            v = v @ t[:, p[2 * k], p[2 * k + 1], :]
        out.append(v[0])
    return np.array(out)


def links(ts):
    return [t.shape[0] for t in ts[1:]]


def close(got, want, rel=1e-10):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    scale = max(1.0, float(np.abs(want).max()) if want.size else 1.0)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= rel * scale, f"max deviation {err:.3e} at scale {scale:.3e}"


def assert_left_orthogonal(m, rel=1e-10):
    for t in m.site_tensors()[:-1]:
        l, s1, s2, r = t.shape
        q = t.reshape((l * s1 * s2, r), order="F")
        assert np.abs(q.T @ q - np.eye(r)).max() <= rel * 10


def assert_matches(m, ts, rel=1e-10):
    assert m.link_dims() == links(ts)
    assert m.site_dims() == [(t.shape[1], t.shape[2]) for t in ts]
    close(m.full_tensor(), np_full(ts), rel)


# ------------------------------------------------------------------------------------------------ transcribed reference tests
@pytest.mark.parametrize("alg", [ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp])
def test_identity_times_identity(alg):
    a, b = MPO.identity([2, 2]), MPO.identity([2, 2])
    r = t4a_amd.contract_naive(a, b) if alg == ContractionAlgorithm.Naive else t4a_amd.contract_zipup(a, b)
    assert len(r) == 2
    assert abs(r.evaluate([0, 0, 0, 0]) - 1.0) < 1e-10
    assert abs(r.evaluate([0, 1, 0, 0])) < 1e-10
    assert abs(r.evaluate([1, 1, 1, 1]) - 1.0) < 1e-10


@pytest.mark.parametrize("alg", [ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp])
def test_constant_times_constant(alg):
    a, b = MPO.constant([(2, 2)], 2.0), MPO.constant([(2, 2)], 3.0)
    r = t4a_amd.contract_naive(a, b) if alg == ContractionAlgorithm.Naive else t4a_amd.contract_zipup(a, b, ContractionOptions())
    assert len(r) == 1
    assert abs(r.evaluate([0, 0]) - 12.0) < 1e-10


@pytest.mark.parametrize("alg", [ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp])
def test_compression_to_max_bond_dim(alg):
    a, b = MPO.constant([(2, 2), (2, 2)], 1.0), MPO.constant([(2, 2), (2, 2)], 1.0)
    r = mpo.contract(a, b, alg, ContractionOptions(tolerance=1e-10, max_bond_dim=2))
    assert r.rank() <= 2


def test_dispatch_naive_equals_zipup():
    a = MPO(random_tensors([1, 3, 2, 1], 2, 2, SEED))
    b = MPO(random_tensors([1, 2, 3, 1], 2, 2, SEED ^ 0xFF))
    n = mpo.contract(a, b, ContractionAlgorithm.Naive, ContractionOptions())
    z = mpo.contract(a, b, ContractionAlgorithm.ZipUp, ContractionOptions())
    close(n.full_tensor(), z.full_tensor())


@pytest.mark.parametrize("alg", [ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp, ContractionAlgorithm.Fit])
def test_length_and_shared_dimension_mismatch(alg):
    with pytest.raises(t4a_amd.T4aError) as e:
        mpo.contract(MPO.constant([(2, 2), (2, 2)], 1.0), MPO.constant([(2, 2)], 1.0), alg)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "length mismatch: expected 2, got 1" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        mpo.contract(MPO.constant([(2, 3)], 1.0), MPO.constant([(2, 2)], 1.0), alg)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT
    assert "site 0" in e.value.message and "site_dim_2=3" in e.value.message and "site_dim_1=2" in e.value.message
    if alg == ContractionAlgorithm.Naive:
        with pytest.raises(t4a_amd.T4aError) as e:
            t4a_amd.contract_naive(MPO.constant([(2, 3)], 1.0), MPO.constant([(2, 2)], 1.0))
        assert e.value.code == t4a_amd.INVALID_ARGUMENT


def test_empty_times_empty_is_empty():
    for r in (t4a_amd.contract_naive(MPO([]), MPO([])), t4a_amd.contract_zipup(MPO([]), MPO([])),
              mpo.contract(MPO([]), MPO([]))):
        assert len(r) == 0 and r.sum() == 0.0 and r.link_dims() == []


def test_fit_and_rsvd_are_not_implemented():
    a, b = MPO.identity([2, 2]), MPO.identity([2, 2])
    with pytest.raises(t4a_amd.T4aError) as e:
        mpo.contract(a, b, ContractionAlgorithm.Fit)
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED and "fitting is not implemented" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        mpo.contract(MPO([]), MPO([]), ContractionAlgorithm.Fit)
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED
    for alg in (ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp):
        with pytest.raises(t4a_amd.T4aError) as e:
            mpo.contract(a, b, alg, ContractionOptions(factorize_method=FactorizeMethod.RSVD))
        assert e.value.code == t4a_amd.NOT_IMPLEMENTED and "RSVD factorization not yet implemented" in e.value.message
    # LU and CI fall back to SVD (factorize.rs:133-137)
    for m in (FactorizeMethod.LU, FactorizeMethod.CI):
        r = mpo.contract(a, b, ContractionAlgorithm.ZipUp, ContractionOptions(factorize_method=m))
        close(r.full_tensor(), np_full([np.eye(2).reshape(1, 2, 2, 1)] * 2))


def test_zipup_untruncated_matches_naive():
    a = random_tensors([1, 3, 4, 1], 2, 3, 0x123456789ABCDEF0)
    b = random_tensors([1, 2, 5, 1], 3, 2, 0x0FEDCBA987654321)
    ma, mb = MPO(a), MPO(b)
    z = t4a_amd.contract_zipup(ma, mb, ContractionOptions(tolerance=0.0))
    x = t4a_amd.contract_naive(ma, mb)
    assert z.full_tensor().shape == (2, 2, 2, 2, 2, 2)
    close(z.full_tensor(), x.full_tensor())
    close(x.full_tensor(), np_full(np_naive(a, b)))


def test_compression_at_a_binding_rank_cap_attains_the_optimal_truncation():
    a = random_tensors([1, 3, 1], 2, 2, SEED)
    b = random_tensors([1, 3, 1], 2, 2, SEED ^ 0xFF)
    exact = t4a_amd.contract_naive(MPO(a), MPO(b))
    dense = exact.full_tensor()
    assert dense.shape == (2, 2, 2, 2)
    sigma = np.linalg.svd(dense.reshape((4, 4), order="F"), compute_uv=False)
    keep = 2
    optimal = float(np.sqrt((sigma[keep:] ** 2).sum()))
    assert optimal > 1e-3
    t = t4a_amd.contract_naive(MPO(a), MPO(b), ContractionOptions(tolerance=0.0, max_bond_dim=keep))
    assert t.rank() == keep
    achieved = float(np.linalg.norm(t.full_tensor() - dense))
    assert achieved <= optimal * (1 + 1e-9), (achieved, optimal)


def test_right_canonicalisation_shrinks_bonds():
    a = random_tensors([1, 3, 7, 1], 2, 2, SEED)
    r = t4a_amd.contract_naive(MPO(a), MPO.identity([2, 2, 2]), ContractionOptions(tolerance=0.0))
    assert r.link_dims() == [3, 4]
    close(r.full_tensor(), np_full(a))


# ------------------------------------------------------------------------------------------------ exact product and restatement
@pytest.mark.parametrize("bonds_a, bonds_b, s1, k, t", [
    ([1, 1], [1, 1], 3, 2, 4),                 # single site
    ([1, 2, 1], [1, 3, 1], 2, 1, 2),           # shared dim 1
    ([1, 3, 2, 1], [1, 2, 4, 1], 2, 3, 1),     # unequal s1 and t
    ([1, 2, 3, 2, 1], [1, 3, 2, 2, 1], 3, 5, 2),
    ([1, 4, 1], [1, 2, 1], 1, 4, 3),
])
def test_naive_without_options_is_the_exact_product(bonds_a, bonds_b, s1, k, t):
    a = random_tensors(bonds_a, s1, k, SEED + len(bonds_a))
    b = random_tensors(bonds_b, k, t, SEED ^ (k * 7919))
    r = t4a_amd.contract_naive(MPO(a), MPO(b))
    want = np_naive(a, b)
    assert r.link_dims() == [x * y for x, y in zip(bonds_a[1:-1], bonds_b[1:-1])] == links(want)
    for got, w in zip(r.site_tensors(), want):
        assert got.shape == w.shape
        close(got, w)


@pytest.mark.parametrize("tol, cap", [(1e-12, None), (1e-6, None), (1e-2, None), (0.0, 3), (1e-12, 5), (1e-3, 4)])
def test_compressed_contractions_match_the_restatement(tol, cap):
    a = random_tensors([1, 3, 4, 3, 1], 2, 2, SEED)
    b = random_tensors([1, 2, 3, 2, 1], 2, 2, SEED ^ 0xFF)
    o = ContractionOptions(tolerance=tol, max_bond_dim=cap)
    n = mpo.contract(MPO(a), MPO(b), ContractionAlgorithm.Naive, o)
    assert_matches(n, np_naive(a, b, o))
    assert_left_orthogonal(n)
    z = mpo.contract(MPO(a), MPO(b), ContractionAlgorithm.ZipUp, o)
    assert_matches(z, np_zipup(a, b, o))
    assert_left_orthogonal(z)


def test_low_rank_product_truncates_to_its_exact_rank():
    # identity-like operators with bond 1 padded to bond 3 by zero blocks: the product has exact rank 1 at every bond
    a = [np.zeros((1, 2, 2, 3)), np.zeros((3, 2, 2, 3)), np.zeros((3, 2, 2, 1))]
    a[0][0, :, :, 0] = np.eye(2)
    a[1][0, :, :, 0] = [[1, 2], [3, 4]]
    a[2][0, :, :, 0] = np.eye(2) * 2
    b = random_tensors([1, 2, 2, 1], 2, 2, SEED)
    for alg, ref in ((ContractionAlgorithm.Naive, np_naive), (ContractionAlgorithm.ZipUp, np_zipup)):
        r = mpo.contract(MPO(a), MPO(b), alg, ContractionOptions())
        assert r.link_dims() == [2, 2]
        assert_matches(r, ref(a, b, ContractionOptions()))


# ------------------------------------------------------------------------------------------------ zero and degenerate cases
def test_zero_operator_contracts_to_rank_one_bonds():
    b = MPO(random_tensors([1, 3, 2, 1], 2, 2, SEED))
    for alg in (ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp):
        r = mpo.contract(MPO.zeros([(2, 2)] * 3), b, alg, ContractionOptions())
        assert r.link_dims() == [1, 1]
        assert r.sum() == 0.0
        assert np.abs(r.full_tensor()).max() == 0.0


def test_non_finite_core_is_invalid_argument():
    a = random_tensors([1, 2, 2, 1], 2, 2, SEED)
    a[1][1, 0, 1, 0] = np.nan
    for alg in (ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp):
        with pytest.raises(t4a_amd.T4aError) as e:
            mpo.contract(MPO(a), MPO.identity([2, 2, 2]), alg, ContractionOptions())
        assert e.value.code == t4a_amd.INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ evaluate / sum / accessors
def test_evaluate_sum_and_accessors():
    ts = random_tensors([1, 3, 2, 1], 2, 3, SEED)
    m = MPO(ts)
    assert len(m) == m.len() == 3 and m.site_dims() == [(2, 3)] * 3 and m.link_dims() == [3, 2] and m.rank() == 3
    for i, t in enumerate(ts):
        assert np.array_equal(m.site_tensor(i), t)
    rng = np.random.default_rng(3)
    idx = np.zeros((50, 6), dtype=np.int64)
    idx[:, 0::2] = rng.integers(0, 2, (50, 3))
    idx[:, 1::2] = rng.integers(0, 3, (50, 3))
    close(m.evaluate(idx), np_eval(ts, idx))
    full = np_full(ts)
    close(m.full_tensor(), full)
    close([m.sum()], [full.sum()])
    assert MPO([]).sum() == 0.0
    c = m.clone()
    close(c.full_tensor(), full)
    for bad in ([2, 0, 0, 0, 0, 0], [0, 3, 0, 0, 0, 0], [0, 0, 0, 0, 0, 7]):
        with pytest.raises(t4a_amd.T4aError) as e:
            m.evaluate(bad)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and "out of bounds" in e.value.message
    with pytest.raises(t4a_amd.T4aError) as e:
        m.evaluate([0, 0])
    assert e.value.code == t4a_amd.INVALID_ARGUMENT


def test_constructors():
    close(MPO.identity([2, 3]).full_tensor(), np.einsum("ij,kl->ijkl", np.eye(2), np.eye(3)))
    c = MPO.constant([(2, 3), (1, 2), (2, 2)], 2.5)
    close(c.full_tensor(), np.full((2, 3, 1, 2, 2, 2), 2.5))
    assert c.site_tensor(0).max() == 1.0 and c.site_tensor(2).max() == 2.5
    assert MPO.zeros([(2, 2), (3, 1)]).sum() == 0.0
    assert len(MPO.identity([])) == 0


# ------------------------------------------------------------------------------------------------ apply to a state
def stencil_tensors(n):
    """sum over sites of a local difference stencil: a bond-2 MPO (n >= 2)"""
    eye, d = np.eye(2), np.array([[-1.0, 1.0], [0.0, -1.0]])
    first, last = np.zeros((1, 2, 2, 2)), np.zeros((2, 2, 2, 1))
    first[0, :, :, 0], first[0, :, :, 1] = eye, d
    last[0, :, :, 0], last[1, :, :, 0] = d, eye
    mid = np.zeros((2, 2, 2, 2))
    mid[0, :, :, 0], mid[0, :, :, 1], mid[1, :, :, 1] = eye, d, eye
    return [first] + [mid] * (n - 2) + [last]


def dense_apply(op_ts, psi_cores):
    n = len(op_ts)
    o = np_full(op_ts)  # [i1, j1, i2, j2, ...]
    o = o.transpose(list(range(0, 2 * n, 2)) + list(range(1, 2 * n, 2)))
    d_out = o.shape[:n]
    psi = psi_cores[0][0]
    for c in psi_cores[1:]:
        psi = np.tensordot(psi, c, axes=([-1], [0]))
    psi = psi[..., 0]
    return (o.reshape(int(np.prod(d_out)), -1) @ psi.reshape(-1)).reshape(d_out)


def state_values(m):
    return m.full_tensor().reshape([d for d, _ in m.site_dims()], order="F")


def tci_state(n):
    spec = t4a_amd.quantics_trig_exp(n)
    opts = t4a_amd.TCI2Options(tolerance=1e-10, max_bond_dim=16, max_iter=20, nsearch=0, max_nglobal_pivot=0)
    return t4a_amd.crossinterpolate2(spec, [2] * n, [[0] * n], opts).to_tensor_train()


@pytest.mark.parametrize("source", ["random", "tci"])
def test_apply_operators_to_a_tensor_train(source):
    n = 6
    if source == "random":
        cores = [c[:, :, 0, :] for c in random_tensors([1, 2, 4, 3, 4, 2, 1], 2, 1, SEED)]
        tt = t4a_amd.SimpleTensorTrain(cores)
    else:
        tt = tci_state(n)
        cores = tt.site_tensors()
    psi = MPO.from_tensor_train(tt)
    assert psi.site_dims() == [(2, 1)] * n
    ops = {"identity": [np.eye(2).reshape(1, 2, 2, 1)] * n, "stencil": stencil_tensors(n),
           "random": random_tensors([1, 2, 3, 3, 3, 2, 1], 2, 2, SEED ^ 0xFF)}
    for name, op_ts in ops.items():
        want = dense_apply(op_ts, cores)
        for alg in (ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp):
            r = mpo.contract(MPO(op_ts), psi, alg, ContractionOptions())
            assert r.site_dims() == [(2, 1)] * n
            out = r.to_tensor_train()
            assert out.site_dims() == [2] * n
            close(state_values(r), want)
            close(np.asarray(out.full_tensor()), want.reshape(-1, order="F"))
        close(state_values(t4a_amd.contract_naive(MPO(op_ts), psi)), want)


def test_identity_round_trip_gives_back_the_train():
    tt = tci_state(8)
    want = np.asarray(tt.full_tensor())
    for alg in (ContractionAlgorithm.Naive, ContractionAlgorithm.ZipUp):
        r = mpo.contract(MPO.identity([2] * 8), MPO.from_tensor_train(tt), alg, ContractionOptions()).to_tensor_train()
        close(np.asarray(r.full_tensor()), want, rel=1e-12)
    back = MPO.from_tensor_train(tt).to_tensor_train()
    assert np.array_equal(np.asarray(back.full_tensor()), want)


# ------------------------------------------------------------------------------------------------ one larger size
def test_zipup_at_a_size_with_multi_block_svd_and_mfma_gemms():
    n, chi_op, chi_tt, cap = 16, 8, 48, 48
    op = random_tensors([1] + [chi_op] * (n - 1) + [1], 2, 2, SEED)
    st = random_tensors([1] + [2, 4, 8, 16, 32] + [chi_tt] * (n - 11) + [32, 16, 8, 4, 2] + [1], 2, 1, SEED ^ 0xFF)
    o = ContractionOptions(tolerance=1e-12, max_bond_dim=cap)
    r = t4a_amd.contract_zipup(MPO(op), MPO(st), o)
    want = np_zipup(op, st, o)
    assert r.link_dims() == links(want)
    assert max(r.link_dims()) == cap
    rng = np.random.default_rng(7)
    idx = np.zeros((400, 2 * n), dtype=np.int64)
    idx[:, 0::2] = rng.integers(0, 2, (400, n))
    close(r.evaluate(idx), np_eval(want, idx), rel=1e-9)
    assert_left_orthogonal(r, rel=1e-9)
