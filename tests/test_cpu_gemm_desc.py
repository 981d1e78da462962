"""CPU-only checks around the GEMM descriptor hook (t4a_gpu_gemm_desc_f64, t4a_gpu_gemm_route): the numpy restatement the exact GPU tests
compare with (tests/gemm_desc_np.py) against plain numpy, the launch route against a table worked out by hand from the rule, and every
refusal of the hook -- all of which happen on the host, before the device is touched."""
import ctypes

import numpy as np
import pytest

import gemm_desc_np as gd


# ------------------------------------------------------------------------------------------------ the restatement
def _stored(buf, off, rows, cols, ld):
    """the stored rows x cols matrix at buf[off + row + ld col], by reshaping (not by the index arithmetic of gemm_desc_np)"""
    return buf[off:off + ld * cols].reshape(cols, ld).T[:rows]


def _plain(d, a, b, c):
    """the update with numpy slices and float64 matmul (exact on small integers); returns the list of (C_j before, C_j after)"""
    out = []
    for j in range(d["batch"]):
        ar, ac = (d["k"], d["m"]) if d["trans_a"] else (d["m"], d["k"])
        br, bc = (d["n"], d["k"]) if d["trans_b"] else (d["k"], d["n"])
        A = _stored(np.concatenate([a, np.zeros(d["lda"])]), d["off_a"] + j * d["stride_a"], ar, ac, d["lda"])
        B = _stored(np.concatenate([b, np.zeros(d["ldb"])]), d["off_b"] + j * d["stride_b"], br, bc, d["ldb"])
        C = _stored(np.concatenate([c, np.zeros(d["ldc"])]), d["off_c"] + j * d["stride_c"], d["m"], d["n"], d["ldc"])
        A = A.T if d["trans_a"] else A
        B = B.T if d["trans_b"] else B
        new = d["alpha"] * (A @ B)
        if d["beta"] != 0.0:
            new = new + d["beta"] * C
        out.append((C.copy(), new))
    return out


CASES = [(shape, t, ab, pad, sm) for shape in ((5, 3, 7, 1), (9, 6, 4, 3), (1, 1, 1, 2), (7, 2, 0, 2))
         for t in gd.TRANS for ab in gd.ALPHA_BETA for pad in gd.PADS for sm in (gd.STRIDE_MODES if shape[3] > 1 else ("dense",))]


def test_exact_restatement_against_plain_numpy():
    """all four transposes, ld > rows, offsets, zero and padded strides, k == 0: the result region is the plain update, everything else
    (the sentinel) comes back bit for bit, and with beta == 0 the sentinel in the result region is never read"""
    rng = np.random.default_rng(1)
    for (m, n, k, batch), (ta, tb), (alpha, beta), pad, sm in CASES:
        d, sizes = gd.make_desc(m, n, k, batch, ta, tb, alpha, beta, pad, sm)
        a, b, c = gd.fill_case(rng, d, sizes)
        ref = gd.gemm_desc_ref(d, a, b, c)
        mask = gd.c_mask(d, c.size)
        assert mask.sum() == m * n * batch
        assert np.array_equal(ref.view(np.uint64)[~mask], c.view(np.uint64)[~mask])
        assert np.all(ref.view(np.uint64)[~mask] == gd.SENTINEL_BITS)
        assert np.all(np.isfinite(ref[mask]))
        for j, (before, after) in enumerate(_plain(d, a, b, c)):
            got = _stored(np.concatenate([ref, np.zeros(d["ldc"])]), d["off_c"] + j * d["stride_c"], m, n, d["ldc"])
            assert np.array_equal(got, after), (m, n, k, batch, ta, tb, alpha, beta, pad, sm, j)
            assert np.all(np.isnan(before)) if beta == 0.0 else np.all(np.abs(before) <= 8)
        assert gd.check_exact(d, c, ref, ref) is None
        if mask.any():  # the checker notices one wrong element, one touched padding element, one NaN
            e = int(np.flatnonzero(mask)[-1])
            bad = ref.copy()
            bad[e] += 0.125
            assert "wrong results" in gd.check_exact(d, c, bad, ref)
            bad[e] = np.nan
            assert "non-finite" in gd.check_exact(d, c, bad, ref)
        if (~mask).any():
            bad = ref.copy()
            bad[int(np.flatnonzero(~mask)[0])] = 0.0
            assert "outside the result" in gd.check_exact(d, c, bad, ref)


def test_the_buffers_of_a_case_are_as_the_tests_describe_them():
    d, sizes = gd.make_desc(70, 40, 33, 3, 1, 0, -1.0, 1.0, True, "cpad")
    assert (d["lda"], d["ldb"], d["ldc"]) == (33 + 3, 33 + 5, 70 + 7) and (d["off_a"], d["off_b"], d["off_c"]) == (3, 5, 7)
    assert d["stride_c"] == 77 * 40 + 11 and sizes[2] == 7 + 2 * d["stride_c"] + 77 * 40 + 9
    d0, s0 = gd.make_desc(70, 40, 33, 3, 0, 1, 1.0, 0.0, False, "ab0")
    assert (d0["stride_a"], d0["stride_b"], d0["lda"], d0["ldb"]) == (0, 0, 70, 40) and s0[:2] == (70 * 33, 40 * 33)
    a, b, c = gd.fill_case(np.random.default_rng(0), d0, s0)
    assert np.all(np.abs(a) <= 3) and np.all(np.abs(b) <= 3) and np.all(c.view(np.uint64) == gd.SENTINEL_BITS)
    assert {v for v in np.unique(a)} == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}


def test_exact_mode_refuses_what_it_cannot_state_exactly():
    d, sizes = gd.make_desc(3, 2, 4, 1, 0, 0, 1.0, 1.0, False, "dense")
    a, b, c = gd.fill_case(np.random.default_rng(0), d, sizes)
    a[0] = 0.5
    with pytest.raises(ValueError):
        gd.gemm_desc_ref(d, a, b, c)
    with pytest.raises(ValueError):
        gd._pow2_scale(1.0 / 3.0, 0.0)
    assert gd._pow2_scale(0.5, 0.25) == (4, 2, 1) and gd._pow2_scale(-1.0, 0.0) == (1, -1, 0)


def test_tight_restatement():
    """on integers the tight value IS the exact one; on reals it agrees with float64 numpy within k roundings of the magnitude, and a sum
    that cancels to far below one rounding of its terms is still resolved"""
    rng = np.random.default_rng(2)
    for ta, tb in gd.TRANS:
        d, sizes = gd.make_desc(9, 6, 40, 2, ta, tb, -1.0, 1.0, True, "cpad")
        a, b, c = gd.fill_case(rng, d, sizes)
        val, mag = gd.gemm_desc_ref(d, a, b, c, mode="tight")
        mask = gd.c_mask(d, c.size)
        assert np.array_equal(val[mask].astype(np.float64), gd.gemm_desc_ref(d, a, b, c)[mask])
        assert np.all(mag[~mask] == 0) and np.all(np.isnan(val[~mask]))
        a, b, c = gd.fill_case(rng, d, sizes, real=True)
        val, mag = gd.gemm_desc_ref(d, a, b, c, mode="tight")
        for j, (before, after) in enumerate(_plain(d, a, b, c)):
            ci = gd.c_index(d, j)
            A, B = gd._ops(d, a, b, j)
            assert np.allclose(mag[ci].astype(np.float64), np.abs(A) @ np.abs(B) + np.abs(before), rtol=1e-14, atol=0)
            assert np.all(np.abs(val[ci] - after.astype(np.longdouble)) <= (40 + 3) * 2.0 ** -53 * mag[ci])
    # 1 + 2^-60 - 1: lost by a double sum in any order, kept by the tight one
    A = np.array([[1.0, 2.0 ** -30, -1.0]])
    B = np.array([[1.0], [2.0 ** -30], [1.0]])
    assert gd._tight_product(A, B)[0, 0] == np.longdouble(2.0) ** -60
    # a product that does not fit a double: (1 + 2^-30)^2 = 1 + 2^-29 + 2^-60
    A = np.array([[1.0 + 2.0 ** -30, -1.0, -(2.0 ** -29)]])
    B = np.array([[1.0 + 2.0 ** -30], [1.0], [1.0]])
    assert gd._tight_product(A, B)[0, 0] == np.longdouble(2.0) ** -60


# ------------------------------------------------------------------------------------------------ the route
# (m, n, k, batch) -> (bn, ksplit, grid_m, grid_n, remapped), by hand from the rule of gemm_launch as it stood before gemm_plan was
# factored out of it:
#   tiles64 = ceil(m / 64) ceil(n / 64) batch;  narrow (bn 32) iff tiles64 < 512 and n > 32;  grid = ceil(m / 64) x ceil(n / bn);
#   tiles = grid_m grid_n batch;  ktiles = ceil(k / 32);  ksplit = min(16, ktiles / 2, ceil(512 / tiles)) if tiles < 256 and ktiles >= 8,
#   else 1;  remapped iff grid_m grid_n is a multiple of 8.
ROUTES = {
    # the rows of tests/test_gpu_gemm_desc_exact.py
    (5, 3, 7, 1): (64, 1, 1, 1, False),
    (70, 40, 33, 1): (32, 1, 2, 2, False),
    (70, 40, 33, 3): (32, 1, 2, 2, False),
    (128, 64, 40, 1): (32, 1, 2, 2, False),
    (256, 128, 70, 1): (32, 1, 4, 4, True),
    (128, 128, 40, 128): (64, 1, 2, 2, False),        # tiles64 = 2 * 2 * 128 = 512: no longer narrow
    (256, 128, 40, 64): (64, 1, 4, 2, True),          # 4 * 2 * 64 = 512
    (64, 32, 256, 1): (64, 4, 1, 1, False),           # ktiles 8: min(16, 4, 512)
    (64, 32, 257, 1): (64, 4, 1, 1, False),           # ktiles 9: min(16, 4, 512); slices of 3 k-tiles, the fourth empty
    (64, 64, 512, 1): (32, 8, 1, 2, False),           # ktiles 16: min(16, 8, 256)
    (70, 70, 321, 5): (32, 5, 2, 3, False),           # tiles 30, ktiles 11: min(16, 5, 18); slices of 3, the fifth empty
    (100, 100, 289, 1): (32, 5, 2, 4, True),          # tiles 8, ktiles 10: min(16, 5, 64)
    (30, 20, 1000, 1): (64, 16, 1, 1, False),         # ktiles 32: min(16, 16, 512)
    # both sides of every threshold
    (1, 1, 0, 1): (64, 1, 1, 1, False),               # k = 0: no k-tile
    (64, 32, 10, 1): (64, 1, 1, 1, False),            # n = 32 stays wide
    (64, 33, 10, 1): (32, 1, 1, 2, False),            # n = 33 is narrow
    (128, 128, 40, 127): (32, 1, 2, 4, True),         # tiles64 = 508 < 512: narrow, 8 tiles per problem
    (64, 32, 224, 1): (64, 1, 1, 1, False),           # ktiles 7: no split
    (64, 32, 225, 1): (64, 4, 1, 1, False),           # ktiles 8
    (64, 32, 320, 1): (64, 5, 1, 1, False),           # ktiles 10
    (64, 32, 2000, 1): (64, 16, 1, 1, False),         # ktiles 63: the cap
    (64, 64, 512, 4): (32, 8, 1, 2, False),           # tiles 8: min(16, 8, 64)
    (512, 512, 512, 1): (32, 4, 8, 16, True),         # tiles 128: min(16, 8, 4)
    (256, 256, 1024, 1): (32, 16, 4, 8, True),        # tiles 32: min(16, 16, 16)
    (1024, 512, 512, 1): (32, 1, 16, 16, True),       # tiles 256: no split
    (1024, 480, 512, 1): (32, 3, 16, 15, True),       # tiles 240: min(16, 8, ceil(512 / 240) = 3)
    (1024, 1024, 1024, 1): (32, 1, 16, 32, True),     # tiles64 = 256: narrow
    (2048, 2048, 64, 1): (64, 1, 32, 32, True),       # tiles64 = 1024
    (192, 96, 64, 1): (32, 1, 3, 3, False),           # 9 tiles
    (65, 1, 1, 700): (64, 1, 2, 1, False),            # batch alone lifts a shape over 512 tiles
    # the largest int in every place: the rounding-up to tiles must not overflow
    (2 ** 31 - 1, 1, 1, 1): (64, 1, 2 ** 25, 1, True),
    (1, 2 ** 31 - 1, 1, 1): (64, 1, 1, 2 ** 25, True),
    (1, 1, 2 ** 31 - 1, 1): (64, 16, 1, 1, False),    # ktiles 2^26
    (64, 64, 64, 2 ** 31 - 1): (64, 1, 1, 1, False),
}


def test_gemm_route_against_the_table_worked_out_by_hand():
    import t4a_amd
    for shape, want in ROUTES.items():
        got = t4a_amd.gemm_route(*shape)
        assert tuple(got[key] for key in gd.ROUTE_KEYS) == want, (shape, got)
    # every row of the exact GPU tests is in the table, with the route those tests assert
    for shape, route, _ in gd.GPU_ROWS:
        assert ROUTES[shape] == route, shape
    assert t4a_amd.gemm_route(5, 3, 7) == t4a_amd.gemm_route(5, 3, 7, 1)


def test_gemm_route_refusals():
    import t4a_amd
    lib = t4a_amd._lib
    sz = ctypes.c_size_t
    out = [ctypes.c_int32(-7) for _ in range(5)]
    refs = [ctypes.byref(x) for x in out]
    for shape in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 1, 0)):
        assert lib.t4a_gpu_gemm_route(*[sz(v) for v in shape], *refs) == t4a_amd.INVALID_ARGUMENT
        assert "m, n and batch must be positive" in t4a_amd.last_error_message()
    for pos in range(4):
        shape = [1, 1, 1, 1]
        shape[pos] = 2 ** 31
        assert lib.t4a_gpu_gemm_route(*[sz(v) for v in shape], *refs) == t4a_amd.INVALID_ARGUMENT
        assert "32-bit index range" in t4a_amd.last_error_message()
    for pos in range(5):
        args = list(refs)
        args[pos] = None
        assert lib.t4a_gpu_gemm_route(sz(1), sz(1), sz(1), sz(1), *args) == t4a_amd.NULL_POINTER
    assert all(x.value == -7 for x in out)  # a refused call writes nothing


# ------------------------------------------------------------------------------------------------ the hook's refusals
BASE = dict(m=4, n=3, k=5, lda=4, ldb=5, ldc=4, trans_a=0, trans_b=0, alpha=1.0, beta=0.0, batch=2, stride_a=20, stride_b=15, stride_c=12,
            off_a=0, off_b=0, off_c=0)
NA, NB, NC = 40, 30, 24  # exactly what BASE needs
INT_MAX = 2 ** 31 - 1
NEG = "negative size, leading dimension, stride or offset"
BIG = "dimension exceeds the 32-bit index range of the device kernels"
TILE = "m, n and k must be at most INT_MAX - 63: the kernel rounds them up to whole tiles in 32-bit integers"
REFUSALS = [
    (dict(m=-1), NEG), (dict(n=-1), NEG), (dict(k=-1), NEG), (dict(batch=-1), NEG),
    (dict(lda=-4), NEG), (dict(stride_a=-20), NEG), (dict(stride_c=-12), NEG), (dict(off_b=-1), NEG),
    (dict(m=INT_MAX + 1), BIG), (dict(k=INT_MAX + 1), BIG), (dict(ldb=2 ** 40), BIG),
    (dict(batch=INT_MAX + 1), BIG),
    (dict(m=INT_MAX - 62), TILE), (dict(n=INT_MAX), TILE), (dict(k=INT_MAX - 62), TILE),
    (dict(trans_a=2), "trans_a and trans_b must be 0 or 1"), (dict(trans_b=-1), "trans_a and trans_b must be 0 or 1"),
    (dict(lda=3), "lda is smaller than the rows of the stored A"),
    (dict(trans_a=1, lda=4), "lda is smaller than the rows of the stored A"),  # stored k x m: 5 rows
    (dict(ldb=4), "ldb is smaller than the rows of the stored B"),
    (dict(trans_b=1, ldb=2), "ldb is smaller than the rows of the stored B"),  # stored n x k: 3 rows
    (dict(ldc=3), "ldc is smaller than the rows of C"),
    (dict(k=0, trans_a=1, lda=0), "lda is smaller than the rows of the stored A"),  # a leading dimension is at least 1
    (dict(off_a=1), "A runs past its buffer"), (dict(stride_a=21), "A runs past its buffer"), (dict(lda=5), "A runs past its buffer"),
    (dict(off_b=1), "B runs past its buffer"), (dict(stride_b=16), "B runs past its buffer"), (dict(k=6, lda=4, ldb=6), "A runs past its buffer"),
    (dict(off_c=1), "C runs past its buffer"), (dict(stride_c=13), "C runs past its buffer"), (dict(batch=3), "A runs past its buffer"),
    (dict(off_c=2 ** 62, stride_c=2 ** 62), "C runs past its buffer"),  # no wrap-around in the extent
    (dict(stride_c=0), "stride_c makes the results of two problems overlap"),
    (dict(stride_c=11), "stride_c makes the results of two problems overlap"),  # one element short of (n - 1) ldc + m
    (dict(stride_c=3), "stride_c makes the results of two problems overlap"),   # interleaved, but closer than m
    (dict(batch=65536, stride_a=0, stride_b=0, stride_c=0, n=1), "stride_c makes the results of two problems overlap"),
]


def _call(t4a, descs, na=NA, nb=NB, nc=NC):
    return t4a.gemm_desc(descs, np.zeros(na), np.zeros(nb), np.zeros(nc))


def test_every_refusal_and_its_message_come_before_the_device():
    """INVALID_ARGUMENT with the descriptor's index and the reason; without a device the valid descriptor gets as far as NO_DEVICE, the
    refused ones never do -- also behind a valid one: every descriptor is checked before the first is uploaded"""
    import t4a_amd
    no_device = t4a_amd.device_count() == 0
    if no_device:
        with pytest.raises(t4a_amd.T4aError) as e:
            _call(t4a_amd, [BASE])
        assert e.value.code == t4a_amd.NO_DEVICE
    for change, message in REFUSALS:
        d = dict(BASE, **change)
        for descs, index in (([d], 0), ([BASE, BASE, d], 2)):
            with pytest.raises(t4a_amd.T4aError) as e:
                _call(t4a_amd, descs)
            assert e.value.code == t4a_amd.INVALID_ARGUMENT, (change, e.value)
            assert e.value.message == f"gemm_desc[{index}]: " + message, (change, e.value)


def test_launch_limits_and_interleaved_results():
    """more problems x slices than a grid's z extent takes is refused; results interleaved inside ldc do not overlap and are accepted
    (as far as the device)"""
    import t4a_amd
    many = dict(m=1, n=1, k=1, batch=65536, stride_c=1)
    with pytest.raises(t4a_amd.T4aError) as e:
        _call(t4a_amd, [many], 1, 1, 65536)
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "65535" in e.value.message
    # (split-K needs fewer than 256 tiles, so slices never add to this: 255 problems x 16 slices at the most)
    assert t4a_amd.gemm_route(1, 1, 512, 255)["ksplit"] == 3 and t4a_amd.gemm_route(1, 1, 512, 256)["ksplit"] == 1
    if t4a_amd.device_count() == 0:
        inter = dict(BASE, ldc=8, stride_c=4)  # problem 1 in rows 4..7 of the same columns
        with pytest.raises(t4a_amd.T4aError) as e:
            _call(t4a_amd, [inter])
        assert e.value.code == t4a_amd.NO_DEVICE
        for empty in (dict(BASE, m=0), dict(BASE, n=0), dict(BASE, batch=0), dict(BASE, k=0)):
            with pytest.raises(t4a_amd.T4aError) as e:
                _call(t4a_amd, [empty])
            assert e.value.code == t4a_amd.NO_DEVICE


def test_null_pointers_and_unknown_fields():
    import t4a_amd
    lib = t4a_amd._lib
    sz = ctypes.c_size_t
    desc = (t4a_amd.GemmDescC * 1)(t4a_amd.gemm_desc_c(BASE))
    buf = (ctypes.c_double * 64)()
    assert lib.t4a_gpu_gemm_desc_f64(None, sz(1), buf, sz(NA), buf, sz(NB), buf, sz(NC)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gemm_desc_f64(desc, sz(1), None, sz(NA), buf, sz(NB), buf, sz(NC)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gemm_desc_f64(desc, sz(1), buf, sz(NA), None, sz(NB), buf, sz(NC)) == t4a_amd.NULL_POINTER
    assert lib.t4a_gpu_gemm_desc_f64(desc, sz(1), buf, sz(NA), buf, sz(NB), None, sz(NC)) == t4a_amd.NULL_POINTER
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.gemm_desc_c(dict(BASE, transa=1))
    assert e.value.code == t4a_amd.INVALID_ARGUMENT and "transa" in e.value.message
    c = t4a_amd.gemm_desc_c(dict(m=4, n=3, k=5, trans_a=1))
    assert (c.lda, c.ldb, c.ldc, c.alpha, c.beta, c.batch, c.stride_c) == (5, 5, 4, 1.0, 0.0, 1, 0)
    assert ctypes.sizeof(t4a_amd.GemmDescC) == 8 * 16  # the layout of t4a_gpu_gemm_desc: 6 + 1 (two int32) + 2 + 7 words
