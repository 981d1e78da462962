"""Soak of the GEMM descriptor (csrc/kernels_dense.hip gemm_launch through the test hook gemm_desc) over random cases -- the assertions
of tests/test_gpu_gemm_desc_exact.py:
  m, n in 1..200 and k in 0..1100, half of them drawn from the edges of the tiles (multiples of 32 and 64, one either side), batch 1
    or 2 - 6, every transpose, alpha from {1, -1, 2, 1/2}, beta from {0, 1, -1, 1/4}, dense or odd-padded leading dimensions and
    offsets, dense / zero / padded strides; operands integers in [-3, 3], C integers in [-8, 8], padding (and, for beta == 0, the
    result region) a NaN with a fixed payload: the whole c buffer must EQUAL the int64 restatement (tests/gemm_desc_np.py), padding
    bit for bit;
  every fourth case is queued twice more in the same call behind a product of another shape: the split-K workspace under work in
    flight, and the same bits three times.
usage: python3 tests/soak/soak_gemm_desc.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import gemm_desc_np as gd  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
EDGES_MN = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 200]
EDGES_K = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 223, 224, 225, 255, 256, 257, 287, 288, 289, 511, 512, 513, 1023, 1024, 1025, 1100]
fails = 0
counts = {}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def count(key, by=1):
    counts[key] = counts.get(key, 0) + by


def draw_dim(rng, edges, lo, hi):
    return int(edges[int(rng.integers(0, len(edges)))]) if rng.random() < 0.5 else int(rng.integers(lo, hi + 1))


def draw_case(rng):
    m, n, k = draw_dim(rng, EDGES_MN, 1, 200), draw_dim(rng, EDGES_MN, 1, 200), draw_dim(rng, EDGES_K, 0, 1100)
    batch = 1 if rng.random() < 0.5 else int(rng.integers(2, 7))
    ta, tb = gd.TRANS[int(rng.integers(0, 4))]
    alpha, beta = gd.ALPHAS[int(rng.integers(0, 4))], gd.BETAS[int(rng.integers(0, 4))]
    pad = bool(rng.integers(0, 2))
    mode = gd.STRIDE_MODES[int(rng.integers(0, 5))] if batch > 1 else "dense"
    d, sizes = gd.make_desc(m, n, k, batch, ta, tb, alpha, beta, pad, mode)
    return d, sizes, gd.fill_case(rng, d, sizes)


def shifted(d, off):
    return dict(d, off_a=d["off_a"] + off[0], off_b=d["off_b"] + off[1], off_c=d["off_c"] + off[2])


def one_case(rng, ctx, chained):
    d, sizes, (a, b, c) = draw_case(rng)
    route = t4a.gemm_route(d["m"], d["n"], d["k"], d["batch"])
    ctx = f"{ctx} {d} route {route}"
    count(f"bn{route['bn']}_{'split' if route['ksplit'] > 1 else 'whole'}{'_remapped' if route['remapped'] else ''}")
    want = gd.gemm_desc_ref(d, a, b, c)
    if not chained:
        problem = gd.check_exact(d, c, t4a.gemm_desc([d], a, b, c), want)
        if problem:
            fail(ctx, problem)
        return
    # the case, a product of another shape, the case again and once more: four launches (or pairs of them) queued back to back
    d2, sizes2, (a2, b2, c2) = draw_case(rng)
    want2 = gd.gemm_desc_ref(d2, a2, b2, c2)
    offs = [(0, 0, 0), sizes, (sizes[0] + sizes2[0], sizes[1] + sizes2[1], sizes[2] + sizes2[2]),
            (2 * sizes[0] + sizes2[0], 2 * sizes[1] + sizes2[1], 2 * sizes[2] + sizes2[2])]
    descs = [shifted(d, offs[0]), shifted(d2, offs[1]), shifted(d, offs[2]), shifted(d, offs[3])]
    got = t4a.gemm_desc(descs, np.concatenate([a, a2, a, a]), np.concatenate([b, b2, b, b]), np.concatenate([c, c2, c, c]))
    parts = np.split(got, [sizes[2], sizes[2] + sizes2[2], 2 * sizes[2] + sizes2[2]])
    for name, dd, before, part, ref in (("first", d, c, parts[0], want), ("other", d2, c2, parts[1], want2), ("second", d, c, parts[2], want),
                                        ("third", d, c, parts[3], want)):
        problem = gd.check_exact(dd, before, part, ref)
        if problem:
            fail(ctx, f"chained, {name} product ({dd}): {problem}")
    count("chained")


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    ctx = f"seed {seed0 + case}"
    try:
        one_case(rng, ctx, chained=case % 4 == 3)
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
print(f"{N} cases from seed {seed0}: {fails} failures; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
