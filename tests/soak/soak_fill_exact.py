"""Soak of fill_site_tensors on ragged batches whose cores are exact by construction (tests/fill_exact_np.py): the assertions of
tests/test_gpu_fill_exact.py over random profiles.  Per case: 3 - 6 sites, bond sizes drawn around the switches of the launchers
(31 / 32 / 33, 255 / 256 / 257, 511 / 512 / 513; one case in twelve around 1024 / 1025) beside small ones, local dimensions large
enough for the nested I sets and the disjoint J sets, a zero pivot matrix at a random site in one case of four, small=True (the
pivot-sensitive bounds) in one case of three and np.array_equal otherwise; the bit budget is asserted before the device runs.
usage: python3 tests/soak/soak_fill_exact.py N [seed0]     (test infrastructure; not collected by pytest)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tensor4all-rs_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import t4a_amd as t4a  # noqa: E402
import fill_exact_np as fx  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fails = 0
routes = {}


def draw_profile(rng):
    n = int(rng.integers(3, 7))
    centres = [32, 256, 512] + ([1024] if rng.integers(0, 12) == 0 else [])
    bonds = []
    for b in range(n - 1):
        if rng.integers(0, 2):
            bonds.append(int(rng.choice(centres)) + int(rng.integers(-1, 2)) + (1 if rng.integers(0, 8) == 0 else 0))
        else:
            bonds.append(int(rng.integers(1, 24)))
    # the ends of a chain stay small: bond b cannot exceed the product of the dimensions on either side
    dims = []
    left = 1
    for b in range(n - 1):
        d = max(2, -(-bonds[b] // left) + int(rng.integers(0, 3)))  # |I_b| d_b >= bonds[b]
        dims.append(d)
        left = bonds[b]
    dims.append(0)
    # J_b: bonds[b] suffixes over b+1 .. n-1 with the last coordinate = b (mod n-1): d_last / (n-1) values times the sites between
    need = 1
    for b in range(n - 1):
        mid = int(np.prod(dims[b + 1:n - 1], dtype=np.int64))
        need = max(need, -(-bonds[b] // mid))
    dims[-1] = (need + int(rng.integers(0, 2))) * (n - 1)
    return dims, bonds


for seed in range(seed0, seed0 + N):
    rng = np.random.default_rng(seed)
    dims, bonds = draw_profile(rng)
    zero_site = int(rng.integers(0, len(bonds))) if rng.integers(0, 4) == 0 else None
    small = rng.integers(0, 3) == 0
    ctx = f"seed {seed} dims {dims} bonds {bonds} zero_site {zero_site} small {bool(small)}"
    c = fx.build(dims, bonds, seed, zero_site, bool(small))
    if not small:
        fx.assert_bit_budget(c)
    route = fx.fill_route(c.max_n(), c.max_nrhs())
    routes[route] = routes.get(route, 0) + 1
    g = t4a.TensorCI2(dims)
    g.set_function(c.f)
    fx.apply_sets(g, c)
    try:
        g.fill_site_tensors()
        if small:
            cores = [g.site_tensor(s) for s in range(len(dims))]
            for b, (fwd, back) in fx.pivot_sensitive_ratios(c, cores).items():
                assert fwd <= 1.0 and back <= 1.0, (b, fwd, back)
            if zero_site is not None:
                assert not cores[zero_site].any(), "zero site"
            fx.assert_cores_exact(g, c, sites=[len(dims) - 1])
        else:
            fx.assert_cores_exact(g, c)
    except AssertionError as e:
        fails += 1
        print(f"FAIL {ctx} route {route}: {e}", flush=True)
print(f"{N} cases, {fails} failures; routes: {routes}")
sys.exit(1 if fails else 0)
