"""LUCI factor VALUES and one-site site tensors on every device route, against answers that are exact by construction.

Pivot selection is pinned bitwise elsewhere; the factor values (left = A[:, J] P^-1, right = P^-1 A[I, :], the site tensors of every
sweep1site / make_canonical / final sweep) were only compared with the oracle at 1e-10 of the largest entry.  Here the matrices of
luci_exact_np.py go through matrix_luci_factors_from_matrix, and through TensorCI2 with a host callback: rank, pivot lists, both factors
and the cores must equal the construction bit for bit (np.array_equal everywhere).  The expected
values come from the construction and rational arithmetic alone; test_cpu_luci_exact.py shows, without a device, that the oracle returns
them too and that every sum the kernels form fits 52 bits, so that no summation order can change a bit.

Route of each case: Engine::build_factors_from (engine.hip) asks luci_factors_small_launch (kernels_dense.hip) first, which takes
1 <= rk <= 16 with M <= 1024 and N <= 1024 in ONE launch of ceil(max(M, N) / 256) workgroups; everything else takes the general path:
trsm_left_batched_launch(n = rk, nrhs = M - rk left-orthogonal | N - rk right-orthogonal; matrix cores iff n >= 64 and nrhs >= 16, no
launch for nrhs = 0) and gemm_launch (rk x N over k = rk | M x rk over k = rk; split-K iff ceil(k / 32) >= 8 and fewer than 256 tiles).
luci_exact_np.route_of() is that logic; test_cpu_luci_exact.py asserts it gives the routes of the table for every case.

  M x N        block ranks       rk   cap  left-orthogonal                   right-orthogonal                  there for
  8 x 6        [4]               4    -    one launch                        one launch
  33 x 20      [1]               1    -    one launch                        one launch                        rk = 1
  40 x 50      [16]              16   -    one launch                        one launch                        rk = 16, the kernel's last
  12 x 30      [12]              12   -    one launch                        one launch                        rk == M: no L21 rows
  30 x 12      [12]              12   -    one launch                        one launch                        rk == N: no U12 columns
  1024 x 40    [3, 2]            5    -    one launch, 4 workgroups          one launch, 4 workgroups          M = 1024, the last size
  40 x 1024    [3, 2]            5    -    one launch, 4 workgroups          one launch, 4 workgroups          N = 1024
  1025 x 40    [3, 2]            5    -    general: scalar trsm              general: scalar trsm              M > 1024
  40 x 1025    [3, 2]            5    -    general: scalar trsm              general: scalar trsm              N > 1024
  64 x 64      [17]              17   -    general: scalar trsm              general: scalar trsm              rk = 17 > 16
  70 x 90      [24]              24   -    general: scalar trsm              general: scalar trsm              47-bit sums
  20 x 20      [20]              20   -    general: no trsm                  general: no trsm                  rk == M == N
  79 x 100     [8] * 8           64   -    general: scalar trsm (15 rhs)     general: matrix-core trsm         M - rk = 15
  80 x 100     [8] * 8           64   -    general: matrix-core trsm (16)    general: matrix-core trsm         M - rk = 16
  100 x 79     [8] * 8           64   -    general: matrix-core trsm         general: scalar trsm (15 rhs)     N - rk = 15
  100 x 80     [8] * 8           64   -    general: matrix-core trsm         general: matrix-core trsm (16)    N - rk = 16
  100 x 100    [8] * 7 + [7]     63   -    general: scalar trsm              general: scalar trsm              rk = 63 < 64
  120 x 110    [16] * 5          80   -    general: matrix-core trsm         general: matrix-core trsm         nrhs 40 | 30: no multiple of 16
  100 x 90     [8] * 8           64   -    general: matrix-core trsm         general: matrix-core trsm
  130 x 150    [8] * 12          96   -    general: matrix-core trsm         general: matrix-core trsm
  120 x 110    [12,5,16,1,9,16,3] 62  -    general: scalar trsm              general: scalar trsm              mixed block ranks
  200 x 180    [16] * 6          96   -    general: matrix-core trsm         general: matrix-core trsm
  300 x 310    [15] * 16         240  -    general: mc trsm, split-K gemm    general: mc trsm, split-K gemm    ksplit = 4 in both products
  40 x 50      [16]              10   10   one launch                        one launch                        truncation
  70 x 90      [24]              16   16   one launch                        one launch                        rank 24 cut to the kernel's last
  100 x 90     [8] * 8           20   20   general: scalar trsm              general: scalar trsm              truncation

TensorCI2 (test_tci2_*): local dims [M, N], [M, N, 1] and [1, M, N] with f(i) = A[i_M, i_N] reach sweep1site_at_bond -> Engine::luci ->
build_factors -> set_core_from_left / set_core_from_right, the last-core pack, and both callback routes of tci2_fill.hip (one launch
for rk <= 16: 8x6, 40x50; general: 64x64 rk 17, 100x90 rk 64, 30x28 rk 19).  The product of the two cores is outside the bit budget:
`evaluate` is not asserted.

matrix_luci_factors_from_blocks is not here: t4a_gpu_luci_blocks_f64 (capi.hip) runs rook_luci, the lazy block-rook search, like the
reference (matrix_luci.rs:440).  It takes rook pivots, not the largest entry: on these matrices the oracle's rook search returns the
same pivots in another order on one block and stops at a lower rank on several (test_cpu_luci_exact.py
test_block_rook_takes_other_pivots), and it builds its factors from a partial-pivoting solve of A[I, J], outside the bit budget.  Its
selection and values stay with test_gpu_rook.py.

Not reached here either: luci_left_cores_batched_kernel (chained 1-site sweep) and the small engine's own left factor run only for built-in
functors, which cannot carry an arbitrary matrix.  tests/test_gpu_chain.py and tests/test_gpu_small.py hold both bitwise to the host path
tested here.
"""
import numpy as np
import pytest

import luci_exact_np as lx

pytestmark = pytest.mark.gpu

IDS = [lx.case_id(c) for c in lx.CASES]


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


def _assert_exact(f, case, left):
    rank, rows, cols, exp_l, exp_r = lx.expected(case, left)
    assert f.rank == rank
    assert np.array_equal(f.row_indices, rows)
    assert np.array_equal(f.col_indices, cols)
    assert f.left.shape == exp_l.shape and f.right.shape == exp_r.shape
    assert np.array_equal(f.left, exp_l), (case[:4], left, "left", int((f.left != exp_l).sum()), np.abs(f.left - exp_l).max())
    assert np.array_equal(f.right, exp_r), (case[:4], left, "right", int((f.right != exp_r).sum()), np.abs(f.right - exp_r).max())


@pytest.mark.parametrize("left", [True, False], ids=["left", "right"])
@pytest.mark.parametrize("case", lx.CASES, ids=IDS)
def test_factors_from_matrix_exact(t4a, case, left):
    a = lx.fixture(case).a
    f = t4a.matrix_luci_factors_from_matrix(a, max_bond_dim=case[3], rel_tol=lx.REL_TOL, abs_tol=lx.ABS_TOL, left_orthogonal=left)
    _assert_exact(f, case, left)


@pytest.mark.parametrize("tc", lx.TCI_CASES, ids=[lx.tci_case_id(t) for t in lx.TCI_CASES])
def test_tci2_site_tensors_exact(t4a, tc):
    """Bond sets equal to the constructed pivot lists in order, then (A[:, J] P^-1, A[I, :]) after fill_site_tensors, a forward
    sweep1site and make_canonical, (A[:, J], P^-1 A[I, :]) after a backward sweep1site; the trivial core is [[[1.0]]]."""
    fx = lx.tci_fixture(tc)
    tci = t4a.TensorCI2(lx.tci_dims(fx, tc[0]))
    lx.tci_check(tci, t4a.TCI2Options(tolerance=1e-15, nsearch=0, max_nglobal_pivot=0), fx, tc[0])
