"""The older element kernels past their launch caps and thread strides, exactly.

About forty launchers of csrc/ clamp their grid and leave the rest to a grid-stride loop inside the kernel; the chain kernels walk a bond
with `for (r = tid; r < R; r += 256)`.  The second trip of such a loop is where an element kernel goes wrong (a cur / nxt swap carried
over from the previous item, LDS reused without a barrier, a stride in 32 bits, a job lookup that is right for the first job only), and
the tests written beside these kernels stay below every cap.  tests/launch_caps_np.py lists the caps; the sizes here are the smallest
that go one element, or a little more, past them, and tests/test_cpu_launch_caps.py fails when a cap moves.

Operands are small integers: entries from {-1, 0, 1} for whatever sums, distinct integers for whatever only moves data, so every result
is an integer far below 2^53, exact in f64 in any order of summation, and the device must EQUAL an int64 numpy computation: no tolerance
appears in this file.  Every test asserts the part of the output that the first trip of the loop wrote and the part that later trips
wrote separately, so that a failure says which trip it was.  Outputs come from a pool and may still hold the right answer of an identical
earlier call: every test draws values that no other test of the file uses (its own seed or offset) and asserts on its first call.

Where an entry cannot be exact (SVD, QR), the comparison is between two runs of the device whose inputs differ by an exact power of
two, bit for bit."""
import numpy as np
import pytest

import apply_np as A
import launch_caps_np as lc
import linsolve_np as ln
import partial_np as pn
import t4a_amd
from t4a_amd import MPO, ApplyOptions, LabelledTensor, LegTrain, LinearOperator, SimpleTensorTrain
from t4a_amd import PartialContractionSpec as Spec
from t4a_amd.linsolve import _apply_env

pytestmark = pytest.mark.gpu


def ints(seed, shape):
    """entries from {-1, 0, 1} as int64"""
    return np.random.default_rng(seed).integers(-1, 2, size=shape)


def distinct(offset, shape):
    """distinct integers from `offset` on, column-major like the device's cores"""
    n = int(np.prod(shape))
    return np.arange(offset, offset + n, dtype=np.int64).reshape(shape, order="F")


def f64(a):
    return np.asarray(a).astype(np.float64)


def flat(a):
    return np.asarray(a).reshape(-1, order="F")


def assert_trips(got, want, later, what):
    """got == want (int64 reference), first on what the first trip wrote, then on what later trips wrote; `later` is a mask like want"""
    got, want, later = np.asarray(got), np.asarray(want), np.asarray(later, dtype=bool)
    assert want.dtype == np.int64 and got.shape == want.shape == later.shape, (what, got.shape, want.shape, later.shape)
    assert (~later).any() and later.any(), f"{what}: the case does not reach a second trip"
    assert np.abs(want[~later]).max() > 0 and np.abs(want[later]).max() > 0, f"{what}: a zero reference would test nothing"
    assert np.array_equal(got[~later], f64(want[~later])), f"{what}: FIRST trip differs from the int64 reference"
    assert np.array_equal(got[later], f64(want[later])), f"{what}: LATER trips differ from the int64 reference (the first trip is right)"


def later_of(shape, per_trip, offset=0):
    """mask of a column-major array: elements whose position offset + index in the launch is past the first trip"""
    n = int(np.prod(shape))
    return (np.arange(offset, offset + n) >= per_trip).reshape(shape, order="F")


def chain_dense(cores):
    """dense tensor of integer cores (l, s, r), one axis per site"""
    acc = cores[0][0]
    for c in cores[1:]:
        acc = np.tensordot(acc, c, axes=([-1], [0]))
    assert acc.dtype == np.int64
    return acc[..., 0]


# ================================================================================================ SimpleTensorTrain
EVAL_BONDS = (1, 20, 300, 20, 1)  # 300: the r += 256 stride of tt_eval_kernel and tt_sum_kernel takes a second step


def eval_train(seed, second_step=True):
    cores = [ints(seed + i, (l, 20, r)) for i, (l, r) in enumerate(zip(EVAL_BONDS[:-1], EVAL_BONDS[1:]))]
    if not second_step:  # nothing depends on what the second step of the stride writes
        cores[1][:, :, lc.BOND_STRIDE:] = 0
        cores[2][lc.BOND_STRIDE:, :, :] = 0
    return cores


def test_evaluate_9000_points_through_a_bond_of_300():
    """tt_eval_kernel: one workgroup per point, 4096 workgroups at most: points 4096 .. 8191 and 8192 .. 8999 are the second and third
    trip of the point loop (cur / nxt swapped three times per point), and the bond of 300 the second step of the r stride"""
    assert EVAL_BONDS[2] > lc.BOND_STRIDE
    cores = eval_train(100)
    dense = chain_dense(cores)
    assert np.abs(dense).max() < 2 ** 53
    pts = np.random.default_rng(101).integers(0, 20, size=(9000, 4))
    assert len(pts) > 2 * lc.EVAL_POINTS
    want = dense[tuple(pts.T)]
    got = SimpleTensorTrain([f64(c) for c in cores]).evaluate(pts)
    assert_trips(got, want, np.arange(len(pts)) >= lc.EVAL_POINTS, "evaluate (point loop of tt_eval_kernel)")
    assert np.array_equal(got[2 * lc.EVAL_POINTS:], f64(want[2 * lc.EVAL_POINTS:])), "evaluate: third trip"


def test_sum_through_a_bond_of_300():
    """tt_sum_kernel, one workgroup: first a train whose bond indices from 256 on carry zeros (the first step of the stride decides),
    then the full train (the second step)"""
    first = eval_train(110, second_step=False)
    assert SimpleTensorTrain([f64(c) for c in first]).sum() == float(chain_dense(first).sum()), "sum: FIRST step of the r stride"
    full = eval_train(120)
    want = int(chain_dense(full).sum())
    assert want != int(chain_dense(eval_train(120, second_step=False)).sum())
    assert SimpleTensorTrain([f64(c) for c in full]).sum() == float(want), "sum: LATER steps of the r stride (bond indices 256 .. 299)"


def halves(cores, right):
    """every half index of three integer cores -> (n_halves, bond) int64, the half index with its first site fastest"""
    if right:
        t = np.einsum("cia,ajb,bk->kjic", cores[0], cores[1], cores[2][:, :, 0])
    else:
        t = np.einsum("ia,ajb,bkc->kjic", cores[0][0], cores[1], cores[2])
    return t.reshape(-1, t.shape[-1])


def half_digits(h, d):
    return np.stack([h % d, (h // d) % d, h // (d * d)], axis=1)


def first_appearance_ids(h):
    """the number a half gets when halves are numbered in the order of their first appearance"""
    _, first, inv = np.unique(h, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.reshape(-1)]


def test_evaluate_many_past_8192_halves_and_2097152_points():
    """Six sites at split 3.  A half is three sites, so 8192 distinct halves per side need a site dim of 21 (21^3 = 9261; the 6^5 or 7^3
    of smaller dims cannot give them): tt_env_left_kernel and tt_env_right_kernel walk their item loop a second time, and
    2 097 153 + 1000 points send tt_env_dot_kernel round again.  The dense tensor of 21^6 entries is not built: a value is the dot
    product of the two dense half tensors that numpy builds from the integer cores, gathered per point."""
    d, bonds = 21, (1, 3, 4, 5, 4, 3, 1)
    cores = [ints(200 + i, (l, d, r)) for i, (l, r) in enumerate(zip(bonds[:-1], bonds[1:]))]
    left, right = halves(cores[:3], False), halves(cores[3:], True)
    n_half = d ** 3
    n_pts = lc.ENV_DOT_POINTS + 1 + 1000
    assert n_half > lc.ENV_ITEMS and left.shape == (n_half, 5) and right.shape == (n_half, 5)
    rng = np.random.default_rng(206)
    # the first 9261 points name every left and every right half once, the rest draw from them
    hl = np.concatenate([np.arange(n_half), rng.integers(0, n_half, n_pts - n_half)])
    hr = np.concatenate([(np.arange(n_half) * 5 + 3) % n_half, rng.integers(0, n_half, n_pts - n_half)])
    idx = np.concatenate([half_digits(hl, d), half_digits(hr, d)], axis=1)
    want = (left[hl] * right[hr]).sum(axis=1)
    assert want.dtype == np.int64 and len(np.unique(hr[:n_half])) == n_half
    got, split = SimpleTensorTrain([f64(c) for c in cores]).evaluate_many(idx, split=3, return_split=True)
    assert split == 3
    il, ir, p = first_appearance_ids(hl), first_appearance_ids(hr), np.arange(n_pts)
    first = (il < lc.ENV_ITEMS) & (ir < lc.ENV_ITEMS) & (p < lc.ENV_DOT_POINTS)
    assert first.any() and np.array_equal(got[first], f64(want[first])), "evaluate_many: FIRST trip of all three kernels"
    wrong = []  # every kernel is judged on the points that only its own later trips reach, and all three are reported together
    for name, later in (("tt_env_left_kernel", (il >= lc.ENV_ITEMS) & (ir < lc.ENV_ITEMS) & (p < lc.ENV_DOT_POINTS)),
                        ("tt_env_right_kernel", (il < lc.ENV_ITEMS) & (ir >= lc.ENV_ITEMS) & (p < lc.ENV_DOT_POINTS)),
                        ("tt_env_dot_kernel", (il < lc.ENV_ITEMS) & (ir < lc.ENV_ITEMS) & (p >= lc.ENV_DOT_POINTS))):
        assert later.sum() >= 100 and np.abs(want[later]).max() > 0, name
        if not np.array_equal(got[later], f64(want[later])):
            wrong.append(name)
    assert not wrong, f"evaluate_many: LATER trips of {' and '.join(wrong)} differ from the int64 reference (the first trips are right)"
    assert np.array_equal(got, f64(want))


def test_evaluate_many_with_a_bond_of_300_at_the_split():
    """the r and l strides of the two environment kernels, and the copy of 300 values per environment"""
    bonds = (1, 5, 300, 5, 1)
    for second_step, seed, what in ((False, 300, "FIRST step of the strides"), (True, 310, "LATER steps of the strides (bond indices 256 .. 299)")):
        cores = [ints(seed + i, (l, 5, r)) for i, (l, r) in enumerate(zip(bonds[:-1], bonds[1:]))]
        if not second_step:
            cores[1][:, :, lc.BOND_STRIDE:] = 0
            cores[2][lc.BOND_STRIDE:, :, :] = 0
        dense = chain_dense(cores)
        pts = np.stack(np.unravel_index(np.arange(625), (5, 5, 5, 5)), axis=1)
        got = SimpleTensorTrain([f64(c) for c in cores]).evaluate_many(pts, split=2)
        assert np.abs(dense).max() > 0 and np.array_equal(got, f64(dense[tuple(pts.T)])), f"evaluate_many: {what}"


def test_scale_of_a_last_core_past_the_cap():
    """tt_scale_kernel on a last core of 1024 x 1025 elements"""
    cores = [distinct(400, (1, 2, 1024)), distinct(500, (1024, 1025, 1))]
    assert cores[1].size > lc.ELEMENTS_4096
    t = SimpleTensorTrain([f64(c) for c in cores]).scale(3.0)
    assert np.array_equal(t.site_tensor(0), f64(cores[0]))
    assert_trips(t.site_tensor(1), 3 * cores[1], later_of(cores[1].shape, lc.ELEMENTS_4096), "scale (tt_scale_kernel)")


def test_add_and_sub_of_one_site_trains_cannot_pass_the_cap():
    """tt_add2_kernel runs on one-site trains only, whose single core is 1 x s x 1, and a train refuses a dimension above 65535: its
    4096 * 256 threads cannot be outrun through the public entry.  The refusal is asserted, so that whoever lifts the limit is sent
    here to add the second-trip case, and add and sub (tt_scale_kernel on the copy of the other operand) are exact at the limit."""
    with pytest.raises(t4a_amd.T4aError) as e:
        SimpleTensorTrain([np.zeros((1, lc.ELEMENTS_4096 + 1000, 1))])
    assert "above 65535" in str(e.value)
    n = 65535
    assert n < lc.ELEMENTS_4096
    a, b = distinct(600, (1, n, 1)), distinct(5_000_000, (1, n, 1)) * 3
    ta, tb = SimpleTensorTrain([f64(a)]), SimpleTensorTrain([f64(b)])
    assert np.array_equal(ta.add(tb).site_tensor(0), f64(a + b)), "add of one-site trains (tt_add2_kernel)"
    assert np.array_equal(ta.sub(tb).site_tensor(0), f64(a - b)), "sub of one-site trains (tt_scale_kernel, tt_add2_kernel)"
    assert np.array_equal(tb.site_tensor(0), f64(b)), "sub scaled its operand in place"


def test_add_and_sub_block_copy():
    """Three sites; the middle cores are 100 x 3 x 450: gather_kernel copies each as a matrix of s * r = 1350 columns (gridDim.y stops at
    1024) into a zero-filled core of 200 x 3 x 900 = 540 000 elements (fill_kernel stops at 2048 * 256)."""
    bonds = (1, 100, 450, 1)
    x = [distinct(700 + 1_000_000 * i, (l, 3, r)) for i, (l, r) in enumerate(zip(bonds[:-1], bonds[1:]))]
    y = [distinct(10_000_000 + 1_000_000 * i, (l, 3, r)) for i, (l, r) in enumerate(zip(bonds[:-1], bonds[1:]))]
    assert 3 * bonds[2] > lc.COLUMNS_1024 and 2 * bonds[1] * 3 * 2 * bonds[2] > lc.FILL_ELEMENTS
    tx, ty = SimpleTensorTrain([f64(c) for c in x]), SimpleTensorTrain([f64(c) for c in y])
    for name, sign, res in (("add", 1, tx.add(ty)), ("sub", -1, tx.sub(ty))):
        assert res.link_dims() == [200, 900]
        for i, (a, b) in enumerate(zip(x, y)):
            if i == len(x) - 1:
                b = sign * b  # the factor of sub sits on the last core of the other operand
            l0, r0 = (0 if i == 0 else a.shape[0]), (0 if i == len(x) - 1 else a.shape[2])
            want = np.zeros((l0 + b.shape[0], 3, r0 + b.shape[2]), dtype=np.int64)
            want[:a.shape[0], :, :a.shape[2]] = a
            want[l0:, :, r0:] = b
            got = res.site_tensor(i)
            if i != 1:
                assert np.array_equal(got, f64(want)), (name, i)
                continue
            # later trips: zeros past fill_kernel's first pass, and the columns from 1024 on of each copied block
            later = later_of(want.shape, lc.FILL_ELEMENTS)
            col = (np.arange(3)[:, None] + 3 * np.arange(a.shape[2])[None, :]) >= lc.COLUMNS_1024   # (s, r) of a block
            block_later = np.broadcast_to(col[None], a.shape)
            later[:a.shape[0], :, :a.shape[2]] = block_later
            later[l0:, :, r0:] = block_later
            assert_trips(got, want, later, f"{name}, block copy (gather_kernel's column loop, fill_kernel)")
    for c, h in zip(y, ty.site_tensors()):
        assert np.array_equal(h, f64(c)), "sub scaled its operand in place"


def test_partial_sum_over_a_site_past_the_cap():
    """Sites (1, 2, 1025), (1025, 2, 1025), (1025, 3, 1); the middle one is summed: tt_site_sum_kernel writes 1025^2 sums, and the kept
    site in front leaves a bond of 1025 for the column loop of identity_kernel.  The result's last core is
    sum_j ssum[i, j] t2[j, c]; the three columns of t2 pick the sums of the first trip (j < 1023), of later trips (j = 1024) and the
    column the boundary runs through (j = 1023: row 0 is the last element of the first trip)."""
    n = 1025
    assert n * n > lc.ELEMENTS_4096 and n > lc.COLUMNS_1024 and lc.ELEMENTS_4096 == 1023 * n + 1
    t0, t1 = ints(800, (1, 2, n)), ints(801, (n, 2, n))
    t2 = np.zeros((n, 3, 1), dtype=np.int64)
    t2[:1023, 0, 0] = ints(802, 1023) | 1   # (odd: never zero)
    t2[1024, 1, 0] = 1
    t2[1023, 2, 0] = -1
    res = SimpleTensorTrain([f64(t0), f64(t1), f64(t2)]).partial_sum([1])
    assert res.dims().tolist() == [[1, 2, n], [n, 3, 1]]
    assert np.array_equal(res.site_tensor(0), f64(t0))
    ssum = t1.sum(axis=1)
    want = (ssum @ t2[:, :, 0]).reshape(n, 3, 1)
    later = np.zeros(want.shape, dtype=bool)
    later[:, 1] = True
    later[1:, 2] = True
    assert_trips(res.site_tensor(1), want, later, "partial_sum (tt_site_sum_kernel; identity_kernel's column loop feeds both parts)")


def test_reverse_of_a_core_past_the_cap():
    """permute_kernel through tensor_permute, axes (2, 1, 0)"""
    cores = [distinct(900, (1, 3, 1025)), distinct(2_000_000, (1025, 1024, 1))]
    assert cores[1].size > lc.PERMUTE_ELEMENTS
    res = SimpleTensorTrain([f64(c) for c in cores]).reverse()
    want = [cores[1].transpose(2, 1, 0), cores[0].transpose(2, 1, 0)]
    assert np.array_equal(res.site_tensor(1), f64(want[1]))
    assert_trips(res.site_tensor(0), np.ascontiguousarray(want[0]), later_of(want[0].shape, lc.PERMUTE_ELEMENTS), "reverse (permute_kernel)")


@pytest.mark.parametrize("dims", [(2, 1025, 512), (2, 3) * 8], ids=["rank3", "rank16"])
def test_permute_at_rank_3_and_at_the_largest_rank(dims):
    """LabelledTensor.permute with a cyclic shift, which moves every axis; rank 16 is the largest the class accepts"""
    rank = len(dims)
    assert int(np.prod(dims)) > lc.PERMUTE_ELEMENTS and rank in (3, 16)
    a = distinct(3_000_000 * rank, dims)
    shift = 1 if rank == 3 else 5
    order = [(k + shift) % rank for k in range(rank)]
    assert all(o != k for k, o in enumerate(order))
    t = LabelledTensor(f64(a), list(range(rank))).permute(order)
    assert t.labels == order
    want = np.ascontiguousarray(a.transpose(order))
    assert_trips(t.to_numpy(), want, later_of(want.shape, lc.PERMUTE_ELEMENTS), f"permute at rank {rank} (permute_kernel)")


# ================================================================================================ the dense layer
DENSE_SHAPE = (600, 450)  # 270 000 elements: the scans and the power-of-two scaling stop at 1024 * 256 = 262 144


def dense_matrix(seed):
    a = f64(ints(seed, DENSE_SHAPE))
    assert a.size > lc.SCAN_ELEMENTS and np.abs(a).max() == 1.0
    return np.asfortranarray(a)


def test_svd_refuses_a_non_finite_entry_past_the_first_trip():
    """nonfinite_absmax_kernel: a NaN, then an Inf, as the very last element and at element 262 144 + 5 of the column-major matrix, refused
    with the message of a small case; the same values inside the first trip first.  (Behind a scan that missed the value, the QR of
    Engine::svd_in_range spreads it over the n x n factor and nonfinite_kernel refuses that with the same message: this test holds
    the refusal, test_svd_sees_a_magnitude_past_the_first_trip holds the later trips of the scan itself.)"""
    bad = np.ones((4, 3))
    bad[2, 1] = np.nan
    with pytest.raises(t4a_amd.T4aError) as small:
        t4a_amd.svd_backend(bad)
    assert small.value.code == t4a_amd.INVALID_ARGUMENT
    m, n = DENSE_SHAPE
    for what, pos in (("FIRST trip", 5), ("LATER trips", lc.SCAN_ELEMENTS + 5), ("LATER trips", m * n - 1)):
        for k, value in enumerate((np.nan, np.inf, -np.inf)):
            a = dense_matrix(1000 + 10 * pos % 97 + k)
            a[pos % m, pos // m] = value
            assert flat(a)[pos] != flat(a)[pos - 1] and not np.isfinite(flat(a)[pos])
            with pytest.raises(t4a_amd.T4aError) as e:
                t4a_amd.svd_backend(a)
            assert e.value.code == t4a_amd.INVALID_ARGUMENT and str(e.value) == str(small.value), f"non-finite scan, {what}: element {pos}"
    # the handle is usable afterwards
    assert np.all(np.isfinite(t4a_amd.svd_backend(np.eye(5, 4))[1]))


def test_svd_sees_a_magnitude_past_the_first_trip():
    """nonfinite_absmax_kernel's other result.  The only entry far from unit scale, 2^600, is the very last element.  The scan that sees
    it makes Engine::svd decompose 2^-600 A, whose bits are those of the matrix numpy scales by 2^-600 (every entry a power of two
    times -1, 0 or 1: exact): U and V^T of both calls are the same bits and the singular values differ by 2^600 exactly.  A scan that
    stops after its first trip sees a largest magnitude of 1, leaves the matrix as it is, and the squares of the Householder norms
    overflow."""
    a = dense_matrix(1100)
    a[-1, -1] = 2.0 ** 600
    ref = a * 2.0 ** -600
    assert np.abs(ref).max() == 1.0 and np.array_equal(ref * 2.0 ** 600, a)
    try:  # (a scan that misses the last element scales the reference by 2^600 and this matrix not at all: both overflow)
        u0, s0, vt0 = t4a_amd.svd_backend(ref)
        u, s, vt = t4a_amd.svd_backend(a)
    except t4a_amd.T4aError as e:
        pytest.fail(f"absmax scan, LATER trips: the magnitude of the last element was not seen and the matrix overflowed ({e})")
    assert np.all(np.isfinite(s0)) and s0[0] > 0.5
    assert np.array_equal(s, s0 * 2.0 ** 600) and np.array_equal(u, u0) and np.array_equal(vt, vt0), \
        "absmax scan, LATER trips: the magnitude of the last element was not seen"


@pytest.mark.parametrize("exponent", (201, -201))
def test_svd_and_qr_of_a_scaled_matrix_are_the_scaled_factors(exponent):
    """scale_pow2_kernel (svd_backend) and scale_pow2_dev_kernel (qr_backend) over 270 000 elements.  The largest entry of the finite
    matrix is 1, so 2^+-201 A is outside 2^-200 .. 2^200 and is decomposed as 2^e (2^-e A) with e = +-201: the matrix behind the scaling
    has the bits of A itself.  No hook reports the route of a call; it is a function of the shape alone (Engine::svd, Engine::qr), and
    the input behind the scaling is the same bits, so U, V^T and Q must be the same bits and the singular values and R differ by 2^e
    exactly.  A scaling kernel that stops after its first trip leaves the elements from 262 144 on unscaled or unwritten."""
    scale = 2.0 ** exponent
    a = dense_matrix(1200 + exponent)
    u0, s0, vt0 = t4a_amd.svd_backend(a)
    u, s, vt = t4a_amd.svd_backend(a * scale)
    assert np.all(np.isfinite(s0)) and s0[-1] > 0
    assert np.array_equal(s, s0 * scale), "svd: singular values of the scaled matrix"
    assert np.array_equal(u, u0) and np.array_equal(vt, vt0), "svd: factors of the scaled matrix (scale_pow2_kernel, later trips)"
    for b in (a, np.asfortranarray(a.T)):  # R is k x n: 450 x 600 has 270 000 elements as well
        q0, r0 = t4a_amd.qr_backend(b)
        q, r = t4a_amd.qr_backend(b * scale)
        later = later_of(r.shape, lc.SCAN_ELEMENTS)
        assert np.array_equal(q, q0), "qr: Q of the scaled matrix (scale_pow2_dev_kernel on the input, later trips)"
        assert np.array_equal(r[~later], (r0 * scale)[~later]), "qr: R of the scaled matrix, FIRST trip of scale_pow2_dev_kernel"
        assert np.array_equal(r, r0 * scale), "qr: R of the scaled matrix, LATER trips of scale_pow2_dev_kernel"


def test_factorize_svd_scales_540000_elements():
    """diag_scale_kernel: factorize(SVD, right-canonical) of a 9000 x 60 matrix returns U S, 540 000 products for a launch of
    2048 * 256 threads.  The same tensor's svd gives U and S (two runs of a decomposition give the same bits: test_gpu_tt.py asserts
    it), and one multiplication per element is exact to the last bit in numpy as on the device."""
    m, k = 9000, 60
    assert m * k > lc.DIAG_SCALE_ELEMENTS
    t = LabelledTensor(f64(ints(1300, (m, k))), [0, 1])
    u, s, _ = t.svd([0], 7, truncate=False)
    left, _, rank, sv = t.factorize([0], 7, alg=t4a_amd.FACTORIZE_SVD, canonical=t4a_amd.CANONICAL_RIGHT, full_rank=True)
    assert rank == k and left.dims == [m, k] and np.array_equal(sv, s.to_numpy())
    want = u.to_numpy() * s.to_numpy()[None, :]
    got, later = left.to_numpy(), later_of((m, k), lc.DIAG_SCALE_ELEMENTS)
    assert np.all(np.isfinite(want)) and np.abs(want[later]).max() > 0
    assert np.array_equal(got[~later], want[~later]), "factorize: U S, FIRST trip of diag_scale_kernel"
    assert np.array_equal(got[later], want[later]), "factorize: U S, LATER trips of diag_scale_kernel"


@pytest.mark.parametrize("left_orthogonal", (True, False))
def test_luci_factors_of_a_matrix_of_1030_columns(left_orthogonal):
    """A rank-one matrix u v^T of 3 x 1030 with the pivot 2048 in column 5: the factors are exact (a division by a power of two), and
    1030 columns send tri_extract_kernel, scatter_cols_kernel and, for the right-orthogonal form, identity_kernel and gather_kernel
    round their column loop again (1024 columns per trip).  The pivot column goes to position 0, so the columns from 1024 on keep
    their places."""
    n = 1030
    assert n > lc.COLUMNS_1024
    v = np.random.default_rng(1400 + left_orthogonal).permutation(np.arange(-600, 600)[np.arange(-600, 600) != 0])[:n]
    v[5] = 2048
    u = np.array([1, -1, 1])
    u[1 + int(left_orthogonal)] = -1 if left_orthogonal else 1
    a = np.outer(u, v)
    f = t4a_amd.matrix_luci_factors_from_matrix(f64(a), left_orthogonal=left_orthogonal)
    assert f.rank == 1 and list(f.col_indices) == [5]
    p = u[int(f.row_indices[0])]
    want_left = (u * p).reshape(3, 1) if left_orthogonal else (u * 2048).reshape(3, 1)
    assert np.array_equal(f.left, f64(want_left))
    want = p * v if left_orthogonal else v / 2048.0
    later = np.arange(n) >= lc.COLUMNS_1024
    got = np.asarray(f.right).reshape(n)
    assert np.array_equal(got[~later], f64(want[~later])), "luci factors: right factor, FIRST trip of the column loops"
    assert np.array_equal(got[later], f64(want[later])), "luci factors: right factor, LATER trips (columns 1024 .. 1029)"


# ================================================================================================ multi-job element kernels
def job_later_masks(shapes):
    """masks of the outputs of a multi-job launch, jobs back to back in the given order"""
    masks, off = [], 0
    for s in shapes:
        masks.append(later_of(s, lc.MULTI_JOB_OUTPUTS, off))
        off += int(np.prod(s))
    assert off > lc.MULTI_JOB_OUTPUTS
    return masks


def assert_jobs(got, want, masks, what, min_sites_later=2):
    assert sum(bool(m.any()) for m in masks) >= min_sites_later, f"{what}: the trip boundary must leave later-trip outputs on several sites"
    g = np.concatenate([flat(x) for x in got])
    w = np.concatenate([flat(x) for x in want]).astype(np.int64)
    assert all(x.shape == y.shape for x, y in zip(got, want)), what
    assert_trips(g, w, np.concatenate([flat(m) for m in masks]), what)
    for i, (x, y, m) in enumerate(zip(got, want, masks)):
        if m.any():
            assert np.array_equal(x[m], f64(np.asarray(y)[m])), f"{what}: LATER trips on site {i} (the job lookup behind a trip boundary)"


def test_reorder_legs_across_a_trip_boundary():
    """leg_reorder_kernel: three reordered sites of 180 x 36 x 186 elements each (legs 2, 3, 2, 3) between two small ends, 3 615 840
    outputs in one launch of 8192 * 256 threads: the second site holds the trip boundary, the third lies behind it."""
    bonds = (1, 180, 186, 180, 186, 1)
    legs = [[(0, 2)]] + [[(10 * i + k, d) for k, d in enumerate((2, 3, 2, 3))] for i in (1, 2, 3)] + [[(40, 2)]]
    cs = [distinct(1500 + 4_000_000 * i, (bonds[i], int(np.prod([d for _, d in s])), bonds[i + 1])) for i, s in enumerate(legs)]
    lt = LegTrain(SimpleTensorTrain([f64(c) for c in cs]), legs)
    orders = {1: [13, 10, 11, 12], 2: [21, 22, 23, 20], 3: [32, 33, 30, 31]}
    assert lt.reorder_legs(orders) is lt
    new = lt._tt.site_tensors()
    want = []
    for i in (1, 2, 3):
        dims, keys = [d for _, d in legs[i]], [k for k, _ in legs[i]]
        t = cs[i].reshape([cs[i].shape[0]] + dims + [cs[i].shape[2]], order="F")
        t = np.transpose(t, [0] + [1 + keys.index(k) for k in orders[i]] + [len(dims) + 1])
        want.append(t.reshape(cs[i].shape, order="F"))
        assert [k for k, _ in lt.legs[i]] == orders[i] and not np.array_equal(want[-1], cs[i])
    assert np.array_equal(new[0], f64(cs[0])) and np.array_equal(new[4], f64(cs[4]))
    assert_jobs(new[1:4], want, job_later_masks([w.shape for w in want]), "reorder_legs (leg_reorder_kernel)")


def test_apply_linear_operator_naive_fused_across_a_trip_boundary():
    """apply_site_kernel: operator bond 8 on sites 0, 2, 4 of a state of bond 64 and site dim 3.  Sites 1 and 3 are bridges, so gap and
    operator jobs share the launch: 1536 + 3 * 786 432 + 1536 = 2 362 368 outputs for 8192 * 256 threads; the trip boundary runs
    through site 3 and site 4 lies behind it."""
    sites, sb, ob = (0, 2, 4), (1, 64, 64, 64, 64, 1), (1, 8, 8, 1)
    x = [ints(1600 + i, (l, 3, r)) for i, (l, r) in enumerate(zip(sb[:-1], sb[1:]))]
    op = [ints(1610 + j, (l, 3, 3, r)) for j, (l, r) in enumerate(zip(ob[:-1], ob[1:]))]
    want = [np.rint(w).astype(np.int64) for w in A.np_naive(op, sites, x)]
    got, info = t4a_amd.apply_linear_operator(LinearOperator(MPO([f64(t) for t in op]), sites), SimpleTensorTrain([f64(c) for c in x]),
                                              ApplyOptions.naive(), route="fused", return_info=True)
    assert info["route"] == "fused"
    assert_jobs(got.site_tensors(), want, job_later_masks([w.shape for w in want]), "apply_linear_operator (apply_site_kernel)")


def test_partial_contract_naive_across_a_trip_boundary():
    """mpo_partial_site_kernel: two chains of bonds (1, 27, 27, 27, 1) and legs (2, 3), leg 0 diagonal and leg 1 summed on every site:
    result cores of 729 x 2 x 1 x 729 in the middle, 2 128 680 outputs for 8192 * 256 threads; the boundary runs through site 2 and
    site 3 lies behind it."""
    bonds = (1, 27, 27, 27, 1)
    a = [ints(1700 + i, (l, 2, 3, r)) for i, (l, r) in enumerate(zip(bonds[:-1], bonds[1:]))]
    b = [ints(1710 + i, (l, 2, 3, r)) for i, (l, r) in enumerate(zip(bonds[:-1], bonds[1:]))]
    cp = [((i, 1), (i, 1)) for i in range(4)]
    dp = [((i, 0), (i, 0)) for i in range(4)]
    plan = pn.plan_for(a, b, cp, dp)
    assert [(p.S, p.T) for p in plan] == [(2, 1)] * 4
    want = [pn.np_site(x, y, sp) for x, y, sp in zip(a, b, plan)]
    r = t4a_amd.partial_contract(MPO([f64(t) for t in a]), MPO([f64(t) for t in b]), Spec(cp, dp))
    assert_jobs(r.site_tensors(), want, job_later_masks([w.shape for w in want]), "partial_contract (mpo_partial_site_kernel)")


def test_linsolve_half_operators_past_the_cap():
    """linsolve_hl_kernel and linsolve_hr_kernel through the hook of tests/test_gpu_linsolve_exact.py: environments of 300, site dims 2
    and an operator bond of 6 make half operators of 3600 x 600 = 2 160 000 elements each, for launches of 8192 * 256 threads"""
    chi, d, w = 300, 2, 6
    ops = [ints(1800, (1, 2, 2, 1)), ints(1801, (1, d, d, w)), ints(1802, (w, d, d, 1)), ints(1803, (1, 2, 2, 1))]
    left, right, v = ints(1804, (chi, 1, chi)), ints(1805, (chi, 1, chi)), ints(1806, (chi, d, d, chi))
    want_l, want_r = ln.np_half_operators(left, right, ops[1], ops[2])
    assert want_l.size > lc.MULTI_JOB_OUTPUTS and want_r.size > lc.MULTI_JOB_OUTPUTS
    _, hl, hr = _apply_env(f64(left), f64(right), MPO([f64(t) for t in ops]), 1, f64(v), return_half_operators=True)
    assert_trips(hl, want_l, later_of(want_l.shape, lc.MULTI_JOB_OUTPUTS), "half operator HL (linsolve_hl_kernel)")
    assert_trips(hr, want_r, later_of(want_r.shape, lc.MULTI_JOB_OUTPUTS), "half operator HR (linsolve_hr_kernel)")
