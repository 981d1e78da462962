"""Soak of the LUCI factor kernels on matrices whose factors are exact by construction (tests/luci_exact_np.py): the assertions of
tests/test_gpu_luci_exact.py over random block profiles.  Per case: 1 - 12 blocks of rank 1 - 16 (one block: up to 24), M and N from the
rank up to 80 more (now and then 1024 or 1025 on one side), an optional rank cap; the bit budget of every sum is checked on the oracle's
factored buffer first and the block ranks lowered until it holds.  Then matrix_luci_factors_from_matrix in both orientations and, for
matrices of at most 120 x 120, TensorCI2 on [M, N], [M, N, 1] and [1, M, N]: np.array_equal everywhere.
usage: python3 tests/soak/soak_luci_exact.py N [seed0]     (test infrastructure; not collected by pytest)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import luci_exact_np as lx  # noqa: E402
import oracle_binding as ob  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
routes = {}


def within_budget(fx, cap):
    for left in (True, False):
        rank, rows, cols, el, er = fx.expected(left, cap)
        fac, rp, cp, npiv, _ = ob.rrlu(fx.a, max_bond_dim=cap, rel_tol=lx.REL_TOL, abs_tol=lx.ABS_TOL, left_orthogonal=left)
        if npiv != rank or not np.array_equal(rp[:rank], rows) or not np.array_equal(cp[:rank], cols):
            return False
        if lx.bit_budget(fac, rp, cp, rank, left, el, er) >= 52:
            return False
    return True


for seed in range(seed0, seed0 + N):
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(1, 13))
    ranks = [int(rng.integers(1, 25 if nb == 1 else 17)) for _ in range(nb)]
    while True:
        r = sum(ranks)
        m, n = r + int(rng.integers(0, 81)), r + int(rng.integers(0, 81))
        big = int(rng.integers(0, 12))
        if big < 2 and r <= 1024:
            m, n = ((1024 + big, n) if rng.integers(0, 2) else (m, 1024 + big))
        cap = int(rng.integers(1, r + 1)) if rng.integers(0, 3) == 0 else None
        fx = lx.build(m, n, ranks, seed)
        if within_budget(fx, cap):
            break
        ranks = [max(1, q - 1) for q in ranks]
    ctx = f"seed {seed} {m}x{n} ranks {ranks} cap {cap}"
    for left in (True, False):
        rank, rows, cols, el, er = fx.expected(left, cap)
        route = lx.route_of(m, n, rank, left)
        routes[route] = routes.get(route, 0) + 1
        f = t4a.matrix_luci_factors_from_matrix(fx.a, max_bond_dim=cap, rel_tol=lx.REL_TOL, abs_tol=lx.ABS_TOL, left_orthogonal=left)
        ok = (f.rank == rank and np.array_equal(f.row_indices, rows) and np.array_equal(f.col_indices, cols)
              and np.array_equal(f.left, el) and np.array_equal(f.right, er))
        if not ok:
            fails += 1
            print(f"FAIL {ctx} left={left} route {route}", flush=True)
    if cap is None and max(m, n) <= 120:
        for form in ("MN", "MN1", "1MN"):
            try:
                tci = t4a.TensorCI2(lx.tci_dims(fx, form))
                lx.tci_check(tci, t4a.TCI2Options(tolerance=1e-15, nsearch=0, max_nglobal_pivot=0), fx, form)
                routes["tci " + form] = routes.get("tci " + form, 0) + 1
            except AssertionError as e:
                fails += 1
                print(f"FAIL {ctx} TensorCI2 {form}: {e}", flush=True)
print(f"{N} cases, {fails} failures; routes: {routes}")
sys.exit(1 if fails else 0)
