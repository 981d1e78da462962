"""The two launches of an edge of the global subspace expansion (csrc/kernels_gse.hip), exactly.  On small-integer operands every
product and partial sum is an integer far below 2^53, so the results must EQUAL int64 arithmetic whatever the order of a sum: project,
N_j = R_j - (R_j B^T) B stacked over the references with the trace sum |R_j|_F^2, with B made of rows of signed unit vectors (exactly
orthonormal), and absorb, parent_j (C_j B'^T).  Bonds and q run over the edges of the 16-wide tiles of the matrix-core path and of the
16-row tiles of a workgroup (1, 2, 15, 16, 17, 33), in both orientations, with 1, 3 and 8 references of ragged bonds, k = q (nothing is
missing), r > q (the bond shrinks), a reference of zero trace; every launch runs twice and must give the same bits, and the GEMM
composition the driver may route a shape through must give the same integers."""
import numpy as np
import pytest

from t4a_amd.gse import _project, _absorb, ROUTE_FUSED, ROUTE_GEMM

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 15, 16, 17, 33)
RAGGED = {1: None, 3: (1, 17, 2), 8: (1, 17, 1, 17, 33, 15, 16, 2)}  # None: one reference, its bond cycles through SIZES


def signed_unit_rows(rng, kb, q):
    """kb rows of +-e_p for kb distinct positions p"""
    b = np.zeros((kb, q))
    b[np.arange(kb), rng.permutation(q)[:kb]] = rng.choice((-1.0, 1.0), kb)
    return b


def orient_of(mats, orient):
    return [m.T.copy() for m in mats] if orient else mats


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def project_case(rng, q, kb, rhos, zero=None):
    refs = [rng.integers(-3, 4, (rho, q)).astype(np.float64) for rho in rhos]
    if zero is not None:
        refs[zero][:] = 0.0
    basis = signed_unit_rows(rng, kb, q)
    ri, bi = [r.astype(np.int64) for r in refs], basis.astype(np.int64)
    want = np.concatenate([r - (r @ bi.T) @ bi for r in ri])
    return refs, basis, want, int(sum((r * r).sum() for r in ri))


def check_project(refs, basis, want, trace, orient):
    got = {}
    for route in (ROUTE_FUSED, ROUTE_GEMM):
        stack, t = _project(orient_of(refs, orient), orient_of([basis], orient)[0], orient, route)
        again, t2 = _project(orient_of(refs, orient), orient_of([basis], orient)[0], orient, route)
        assert same_bits(stack, again) and t == t2, route
        got[route] = stack.T if orient else stack
        assert np.array_equal(got[route], want.astype(np.float64)), (route, orient)
        assert t == float(trace), (route, orient)
    return got[ROUTE_FUSED]


@pytest.mark.parametrize("orient", (0, 1))
@pytest.mark.parametrize("q", SIZES)
def test_project_equals_int64_arithmetic(q, orient):
    """|R| <= 3 and B of signed unit rows: |R B^T| <= 3, every entry of N an integer of at most 6, the trace at most 9 * 89 * 33"""
    for i, kb in enumerate(k for k in SIZES if k <= q):
        rng = np.random.default_rng(1000 * q + 10 * kb + orient)
        for n_refs, rhos in RAGGED.items():
            rhos = (SIZES[(i + SIZES.index(q)) % len(SIZES)],) if rhos is None else rhos
            refs, basis, want, trace = project_case(rng, q, kb, rhos)
            stack = check_project(refs, basis, want, trace, orient)
            if kb == q:  # B spans everything: nothing is missing
                assert not stack.any()


@pytest.mark.parametrize("orient", (0, 1))
def test_project_of_a_reference_with_zero_trace(orient):
    rng = np.random.default_rng(77 + orient)
    refs, basis, want, trace = project_case(rng, 17, 5, (17, 1, 16), zero=0)
    stack = check_project(refs, basis, want, trace, orient)
    assert not stack[:17].any() and stack[17:].any()
    refs, basis, want, trace = project_case(rng, 33, 16, (2,), zero=0)  # all of them: the trace is exactly zero
    assert trace == 0
    assert not check_project(refs, basis, want, trace, orient).any()


def test_project_of_references_inside_the_span():
    """rows of B itself, recombined with integers: N must be exactly zero although k < q"""
    rng = np.random.default_rng(5)
    for q, kb, rho in ((33, 17, 16), (17, 16, 33), (16, 2, 1)):
        basis = signed_unit_rows(rng, kb, q)
        ref = rng.integers(-3, 4, (rho, kb)).astype(np.float64) @ basis
        for orient in (0, 1):
            stack, t = _project(orient_of([ref], orient), orient_of([basis], orient)[0], orient)
            assert not stack.any() and t == float((ref * ref).sum())


def absorb_case(rng, q, kn, rs, ls):
    children = [rng.integers(-2, 3, (r, q)).astype(np.float64) for r in rs]
    parents = [rng.integers(-2, 3, (lj, r)).astype(np.float64) for lj, r in zip(ls, rs)]
    basis = rng.integers(-2, 3, (kn, q)).astype(np.float64)
    bi = basis.astype(np.int64)
    want = [p.astype(np.int64) @ (c.astype(np.int64) @ bi.T) for p, c in zip(parents, children)]
    return children, parents, basis, want


@pytest.mark.parametrize("orient", (0, 1))
@pytest.mark.parametrize("q", SIZES)
def test_absorb_equals_int64_arithmetic(q, orient):
    """entries in [-2, 2]: |C B'^T| <= 4 q <= 132, |parent (C B'^T)| <= 2 * 33 * 132: integers far below 2^53.  The bonds r of the
    trains include r > q (the bond shrinks to k <= q)."""
    for i, kn in enumerate(k for k in SIZES if k <= q):
        rng = np.random.default_rng(2000 * q + 10 * kn + orient)
        for n_trains in (2, 4, 9):
            rs = [SIZES[(i + j) % len(SIZES)] for j in range(n_trains)]
            rs[0] = 33 if q < 33 else 17  # the target: r > q where q allows it
            ls = [SIZES[(2 * i + 3 * j + 1) % len(SIZES)] for j in range(n_trains)]
            children, parents, basis, want = absorb_case(rng, q, kn, rs, ls)
            for route in (ROUTE_FUSED, ROUTE_GEMM):
                args = (orient_of(children, orient), orient_of(parents, orient), orient_of([basis], orient)[0], orient, route)
                got, again = _absorb(*args), _absorb(*args)
                for j, (a, b, w) in enumerate(zip(got, again, want)):
                    assert same_bits(a, b), (route, j)
                    assert np.array_equal(a.T if orient else a, w.astype(np.float64)), (route, orient, kn, n_trains, j)
