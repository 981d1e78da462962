"""Times the device-resident MPO Contraction and contract_tci at one stated shape, next to a one-thread numpy run of the restatement
(tests/contraction_np.py) and to the device route that existed before: contract_naive(a, b, None) then MPO.evaluate, and contract_zipup.

Shape: two operators of `n` sites, site dims (2, 2), bonds `chi_a` and `chi_b` (the LCG fixtures of the tests).

    python tools/probe_contraction.py [n] [chi_a] [chi_b] [reps]          every step, each in a child process under its own `timeout`
    python tools/probe_contraction.py --step NAME [--route host|device] [n] [chi_a] [chi_b] [reps]

Steps: points (4096 random points), outer (one 512 x 512 outer-product batch split in the middle), naive_points / naive_outer (the same
batches through the materialised product), matrix (the same 512 x 512 outer product as ONE candidate matrix through evaluate_matrix:
no index buffer, no unique map, paired by contraction_pair_kernel — read its time under `rocprofv3 --kernel-trace --stats`), tci
(contract_tci at tolerance 1e-10 against contract_zipup, on the route given: "host" is the batch callback, "device" the contraction as
the device matrix source; the driver runs both at bonds 8 and 6 unless bonds are given), pairing (one outer batch and
one dense product of the pairing's shape, 512 x la*lb by la*lb x 512: run it under `rocprofv3 --kernel-trace --stats` to read
tt_env_dot_kernel next to gemm_kernel).  A time is the median of `reps` calls after a warm-up (reps = 0: one cold call); every call ends
with the synchronisation of its own stream, so the device work is inside the window.  The driver stops at the first step that fails."""
import os

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the numpy side runs on one thread
    os.environ[v] = "1"

import json  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tensor4all-rs_amd", "python"), os.path.join(ROOT, "tests")]

STEPS = [("points", 240), ("outer", 240), ("matrix", 240), ("pairing", 240), ("naive_points", 420), ("naive_outer", 540), ("tci", 540),
         ("tci:device", 540)]
TCI_DEFAULT_BONDS = (8, 6)  # the driver's tci step when no bonds are given: at 32 and 24 (rank 768) one call takes minutes
ORACLE_MAX_RANK = 64  # the one-thread reference run of the tci step is skipped above this la * lb (minutes of numpy callbacks)


def median_ms(call, reps):
    if reps == 0:  # one cold call, for shapes where a call takes minutes
        t0 = time.perf_counter()
        call()
        ms = round((time.perf_counter() - t0) * 1e3, 3)
        return ms, ms, ms
    call()  # warm-up (allocations, first launches)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 3), round(min(times), 3), round(max(times), 3)


def once_ms(call):
    t0 = time.perf_counter()
    r = call()
    return r, round((time.perf_counter() - t0) * 1e3, 1)


def rel_dev(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(want).max()))


def step(name, n, chi_a, chi_b, reps, route="host"):
    import t4a_amd
    import contraction_np as cnp
    a = cnp.random_tensors([1] + [chi_a] * (n - 1) + [1], 2, 2, cnp.SEED)
    b = cnp.random_tensors([1] + [chi_b] * (n - 1) + [1], 2, 2, cnp.SEED ^ 0x5555)
    A, B = t4a_amd.MPO(a), t4a_amd.MPO(b)
    ref = cnp.ContractionNP(a, b)
    points = cnp.lcg_points(4096, [[2, 2]] * n, 21)
    h = n // 2
    rows, cols = cnp.lcg_points(512, [[2, 2]] * h, 22), cnp.lcg_points(512, [[2, 2]] * (n - h), 23)
    outer = np.concatenate([np.repeat(rows, 512, axis=0), np.tile(cols, (512, 1, 1))], axis=1)
    out = {"step": name, "n": n, "chi_a": chi_a, "chi_b": chi_b, "reps": reps}
    if name in ("points", "outer"):
        batch, split = (points, None) if name == "points" else (outer, h)
        c = t4a_amd.Contraction(A, B)
        med, best, worst = median_ms(lambda: c.evaluate_many(batch, split=split), reps)
        vals, used = c.evaluate_many(batch, split=split)
        want, np_ms = once_ms(lambda: ref.evaluate_many(batch, used))  # the same scheme: unique halves once, then the pairing
        out.update({"n_pts": len(batch), "split": used, "gpu_ms_median": med, "gpu_ms_min": best, "gpu_ms_max": worst,
                    "numpy_1thread_ms": np_ms, "max_rel_dev": rel_dev(vals, want)})
    elif name == "matrix":
        c = t4a_amd.Contraction(A, B)
        med, best, worst = median_ms(lambda: c.evaluate_matrix(h, rows, cols), reps)
        vals = c.evaluate_matrix(h, rows, cols)
        want, np_ms = once_ms(lambda: ref.evaluate_many(outer, h))
        out.update({"shape": list(vals.shape), "cut": h, "gpu_ms_median": med, "gpu_ms_min": best, "gpu_ms_max": worst,
                    "numpy_1thread_ms": np_ms, "max_rel_dev": rel_dev(vals.reshape(-1), want)})
    elif name in ("naive_points", "naive_outer"):
        batch = points if name == "naive_points" else outer
        flat = batch.reshape(len(batch), -1)
        med_c, _, _ = median_ms(lambda: t4a_amd.contract_naive(A, B, None), reps)
        prod = t4a_amd.contract_naive(A, B, None)
        med_e, best_e, _ = median_ms(lambda: prod.evaluate(flat), reps)
        c = t4a_amd.Contraction(A, B)
        out.update({"n_pts": len(batch), "contract_naive_ms_median": med_c, "evaluate_ms_median": med_e, "evaluate_ms_min": best_e,
                    "route_ms": round(med_c + med_e, 3), "max_rel_dev_vs_contraction": rel_dev(c.evaluate_many(batch)[0], prod.evaluate(flat))})
    elif name == "tci":
        opts = t4a_amd.TCI2Options(tolerance=1e-10, max_nglobal_pivot=0, nsearch=0)
        zopt = t4a_amd.ContractionOptions(tolerance=1e-10)
        keep = {}
        tci = (lambda: t4a_amd.contract_tci(A, B, opts)) if route == "host" else (lambda: t4a_amd.contract_tci(A, B, opts, route=route))
        med, best, worst = median_ms(lambda: keep.__setitem__("m", tci()), reps)
        medz, bestz, _ = median_ms(lambda: keep.__setitem__("z", t4a_amd.contract_zipup(A, B, zopt)), reps)
        m, z = keep["m"], keep["z"]
        flat = points.reshape(len(points), -1)
        want = ref.evaluate(points)
        o_ms = "skipped: la * lb above %d" % ORACLE_MAX_RANK
        try:  # the reference algorithm on one CPU thread, fed by the numpy restatement
            if route != "host":  # the oracle column belongs to the host row of the table: one minute of numpy callbacks, not repeated
                o_ms = "skipped: reported with route host"
                raise OverflowError
            if chi_a * chi_b > ORACLE_MAX_RANK:
                raise OverflowError
            import oracle_binding as ob
            o = ob.OracleTCI2(ref.fused_dims())
            o.set_function(ref.fused_function())
            # like the device run: the first pivot by opt_first_pivot from the all-zero index, inside the timed window
            _, o_ms = once_ms(lambda: o.crossinterpolate2([ob.opt_first_pivot(ref.fused_function(), ref.fused_dims(), [0] * n)], opts))
        except OverflowError:
            pass
        except Exception as e:  # the oracle is a test fixture: the probe runs without it
            o_ms = f"unavailable: {e}"
        out.update({"route": route, "tci_ms_median": med, "tci_ms_min": best, "tci_ms_max": worst, "tci_link_dims": m.link_dims(), "tci_info": m.tci_info,
                    "tci_max_rel_dev": rel_dev(m.evaluate(flat), want), "zipup_ms_median": medz, "zipup_ms_min": bestz,
                    "zipup_link_dims": z.link_dims(), "zipup_max_rel_dev": rel_dev(z.evaluate(flat), want),
                    "oracle_tci_numpy_1thread_ms": o_ms})
    elif name == "pairing":
        c = t4a_amd.Contraction(A, B)
        c.evaluate_many(outer, split=h)
        left = c.evaluate_left(h, outer[::512]).reshape(512, -1)       # 512 x la*lb
        right = c.evaluate_right(h, outer[:512]).reshape(512, -1).T    # la*lb x 512
        med, best, _ = median_ms(lambda: t4a_amd.mat_mul(left, right), reps)
        out.update({"pairing_shape": [left.shape[0], left.shape[1], right.shape[1]], "mat_mul_with_copies_ms_median": med,
                    "max_rel_dev": rel_dev(t4a_amd.mat_mul(left, right).reshape(-1), c.evaluate_many(outer, split=h)[0])})
    else:
        raise SystemExit(f"unknown step {name}")
    print(json.dumps(out), flush=True)


def main():
    argv = sys.argv[1:]
    name = None
    route = "host"
    if argv[:1] == ["--step"]:
        name, argv = argv[1], argv[2:]
    if argv[:1] == ["--route"]:
        route, argv = argv[1], argv[2:]
    a = [int(x) for x in argv]
    n, chi_a, chi_b, reps = (a + [16, 32, 24, 5][len(a):])[:4]
    if name is not None:
        return step(name, n, chi_a, chi_b, reps, route)
    for s, limit in STEPS:
        s, _, r = s.partition(":")
        ca, cb = TCI_DEFAULT_BONDS if s == "tci" and len(a) < 3 else (chi_a, chi_b)
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s, "--route", r or "host",
                              str(n), str(ca), str(cb), str(reps)])
        if rc != 0:
            raise SystemExit(f"step {s} ended with status {rc}: nothing further is started")


if __name__ == "__main__":
    main()
