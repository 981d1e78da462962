"""Builds and runs tests/rrlu_plan_sweep.hip (host code only: the planners of the register-resident and the one-workgroup rrLU
kernel over every shape they can take) and parses what it prints.  Shared by test_cpu_rrlu_plans.py and
test_gpu_rrlu_reg_variants.py; the program runs once per process."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def sweep():
    """{"reg_table": {(rpt, cpt, single, uni)}, "reg": {cus: {(rpt, cpt, single, uni): (M, N)}}, "wg_table": {(rpt, cpw)},
    "wg": {(rpt, cpw): (M, N)}, "hash": str}; (M, N) is the smallest matrix, as the kernel sees it, that selects the shape."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rrlu_plan_sweep")
        subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "rrlu_plan_sweep.hip"),
                        os.path.join(ROOT, "tensor4all-rs_amd", "csrc", "rrlu_plan.hip"), "-o", exe], check=True, capture_output=True, text=True)
        env = {k: v for k, v in os.environ.items() if k != "T4A_NO_WG"}
        out = subprocess.run([exe], check=True, capture_output=True, text=True, env=env).stdout
    res = {"reg_table": set(), "reg": {}, "wg_table": set(), "wg": {}, "hash": None}
    for line in out.splitlines():
        tag, *f = line.split()
        if tag == "hash":
            res["hash"] = f[0]
            continue
        v = [int(x) for x in f]
        if tag == "reg-table":
            res["reg_table"].add(tuple(v))
        elif tag == "reg":
            res["reg"].setdefault(v[0], {})[tuple(v[1:5])] = (v[5], v[6])
        elif tag == "wg-table":
            res["wg_table"].add(tuple(v))
        elif tag == "wg":
            res["wg"][tuple(v[:2])] = (v[2], v[3])
        else:
            raise ValueError("unexpected line from rrlu_plan_sweep: " + line)
    return res
