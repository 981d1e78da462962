"""Every instantiated shape of the register-resident and of the one-workgroup rrLU kernel runs, in both tie orders, and agrees
with the oracle bitwise: a variant pruned from rrlu_shapes.hpp by mistake shows up as T4A_GPU_INTERNAL_ERROR from the launcher.

For every shape of the register table the matrix is the smallest one the planner sweep (tests/rrlu_plan_sweep.hip) reports for
it at 256 compute units, as the kernel sees it: a right-orthogonal factorisation runs on the transpose with the row-major tie
order, so it is given the transposed shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
from rrlu_plan_sweep import sweep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_shapes(t4a, shapes):
    """shapes: (M, N) as the kernel sees them.  Pivots, permutations, last error and pivot errors against the oracle, bitwise."""
    for (m, n) in shapes:
        rng = np.random.default_rng(31000 + 7 * m + n)
        for left in (True, False):
            a = rng.uniform(-1, 1, size=(m, n) if left else (n, m))
            opts = dict(max_bond_dim=8, left_orthogonal=left)
            lu = t4a.rrlu(a, **opts)
            f, rp, cp, npiv, err = ob.rrlu(a, **opts)
            ctx = f"kernel shape {m} x {n} left {left}"
            assert lu.npivots() == npiv, ctx
            assert np.array_equal(lu.row_permutation, rp) and np.array_equal(lu.col_permutation, cp), ctx
            assert np.array_equal(lu.factored.view(np.uint64), f.view(np.uint64)), ctx
            assert lu.error == err or (np.isnan(lu.error) and np.isnan(err)), ctx
            d = np.array([f[i, i] for i in range(npiv)])
            assert np.array_equal(lu.pivot_errors().view(np.uint64), np.concatenate([np.sqrt(d * d), [err]]).view(np.uint64)), ctx


def test_every_register_kernel_shape_in_a_child_process():
    """T4A_RRLU_IMPL=reg (read once per process) sends every matrix to the register-resident kernel."""
    s = sweep()
    witnesses = [s["reg"][256][k] for k in sorted(s["reg_table"])]
    assert len(witnesses) == len(s["reg_table"]) > 0
    code = (
        "import json, sys\n"
        "sys.path.insert(0, 'tests')\n"
        "import t4a_amd, test_gpu_rrlu_reg_variants as v\n"
        "v.check_shapes(t4a_amd, json.loads(sys.argv[1]))\n"
        "print('ok')\n")
    env = dict(os.environ, T4A_RRLU_IMPL="reg", PYTHONPATH=os.path.join(ROOT, "tensor4all-rs_amd", "python"))
    r = subprocess.run([sys.executable, "-c", code, json.dumps(witnesses)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_every_one_workgroup_kernel_shape():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    assert sweep()["wg_table"] == {(1, 8), (1, 16), (2, 8)}
    check_shapes(t4a_amd, [(60, 40), (60, 100), (100, 60)])
