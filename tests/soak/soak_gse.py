"""Soak of the global subspace expansion (csrc/gse.hip, kernels_gse.hip) on random small problems against the numpy restatement
(tests/gse_np.py): 2 - 6 sites, site dimensions 2 or 3 drawn per site, a random start of bond 1 - 3, 1 - 3 random references of bond
1 - 4, any centre.  A case is EXCLUDED, and counted, when the restatement misses the gap condition of tests/test_cpu_gse.py (a normalised
eigenvalue of an edge inside (1e-14, 1e-8), or a child whose smallest singular value is not above 1e-6 of its largest): there the eigen and
the SVD selection may keep different directions.  Nothing else is skipped, and more than 5 % excluded cases is a failure.  Per case: bond
dimensions and counters equal the restatement's, the dense state is within max(100 x the restatement's own preservation error, 1e-12) of
the start, the projectors of all bonds within max(100 spread, 1e-12) of the restatement's (gse_np.spread_tolerance), the non-centre cores are
isometries to 1e-12, the references are contained to the projector tolerance, and a second run gives the same bits.
usage: python3 tests/soak/soak_gse.py N [seed0]     (test infrastructure: numpy is the checker; not collected by pytest)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import gse_np as g  # noqa: E402
from linsolve_np import np_state_full  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
counts = {"cases": 0, "excluded": 0, "edges": 0, "rows_added": 0}


def fail(ctx, what):
    global fails
    fails += 1
    print(f"FAIL {ctx}: {what}", flush=True)


def bonds_of(dims, chi):
    n = len(dims)
    return [1] + [int(min(chi, np.prod(dims[:i]), np.prod(dims[i:]))) for i in range(1, n)] + [1]


t0 = time.perf_counter()
for case in range(N):
    rng = np.random.default_rng(seed0 + case)
    n = int(rng.integers(2, 7))
    dims = [int(rng.integers(2, 4)) for _ in range(n)]
    center = int(rng.integers(0, n))
    sb = bonds_of(dims, int(rng.integers(1, 4)))
    init = [rng.standard_normal((sb[k], d, sb[k + 1])) for k, d in enumerate(dims)]
    refs = []
    for _ in range(int(rng.integers(1, 4))):
        rb = bonds_of(dims, int(rng.integers(1, 5)))
        refs.append([rng.standard_normal((rb[k], d, rb[k + 1])) for k, d in enumerate(dims)])
    ctx = f"seed {seed0 + case} dims {dims} center {center} bonds {sb} refs {[g.link_dims(r) for r in refs]}"
    try:
        want = g.np_gse_with_references(init, refs, center)
        inside, ratio = g.gap_report(want)
        if inside or ratio <= 1e-6:
            counts["excluded"] += 1
            print(f"excluded {ctx}: eigenvalues in the gap {inside}, singular-value ratio {ratio}", flush=True)
            continue
        x0, rs = t4a.SimpleTensorTrain(init), [t4a.SimpleTensorTrain(r) for r in refs]
        r = t4a.global_subspace_expand_with_references(x0, rs, center)
        cores = r.state.site_tensors()
        if g.link_dims(cores) != g.link_dims(want["state"]):
            fail(ctx, f"bonds {g.link_dims(cores)}, restatement {g.link_dims(want['state'])}")
            continue
        got = (r.references_built, r.edges_processed, r.bonds_expanded, r.max_added_basis)
        exp = (len(refs), want["edges_processed"], want["bonds_expanded"], want["max_added_basis"])
        if got != exp:
            fail(ctx, f"counters {got}, restatement {exp}")
        psi0 = np_state_full(init)
        own = g.relative_distance(np_state_full(want["state"]), psi0)
        dist = g.relative_distance(np_state_full(cores), psi0)
        if dist > max(100.0 * own, 1e-12):
            fail(ctx, f"preservation {dist}, the restatement's {own}")
        tol, spread = g.spread_tolerance(lambda s: g.projector_vector(g.np_gse_with_references(s, refs, center)["state"], center), init)
        pdist = g.relative_distance(g.projector_vector(cores, center), g.projector_vector(want["state"], center))
        if pdist > tol:
            fail(ctx, f"projector distance {pdist}, tolerance {tol} (spread {spread})")
        if g.row_defect(cores, center) > 1e-12:
            fail(ctx, f"isometry defect {g.row_defect(cores, center)}")
        if g.containment_residual(cores, refs, center) > tol:
            fail(ctx, f"containment {g.containment_residual(cores, refs, center)}, tolerance {tol}")
        r2 = t4a.global_subspace_expand_with_references(x0, rs, center)
        if any(p.tobytes() != s.tobytes() for p, s in zip(cores, r2.state.site_tensors())):
            fail(ctx, "a second run gave other bits")
        counts["cases"] += 1
        counts["edges"] += r.edges_processed
        counts["rows_added"] += sum(a - b for a, b in zip(g.link_dims(cores), g.link_dims(g.np_canonicalize(init, center))))
    except Exception as exc:  # noqa: BLE001 (no mismatch but an error: the device may be in a failed state, nothing more is started on it)
        fail(ctx, f"exception {type(exc).__name__}: {exc}; stopped after {case + 1} of {N} cases")
        break
if counts["excluded"] > 0.05 * N:
    fail("the whole run", f"{counts['excluded']} of {N} cases excluded by the gap condition: more than 5 %")
print(f"{N} cases from seed {seed0}: {fails} failures; {counts['excluded']} excluded by the gap condition; {counts}; {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
