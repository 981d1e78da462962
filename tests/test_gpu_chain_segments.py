"""Segments of the launched bond chain (tci2_chain.hip chain_plan_segments / chain_launch, kernels_chain.hip chain_walk_kernel): a
half-sweep whose middle bonds outgrow 64 x 32 is launched bond by bond, but each maximal run of consecutive bonds that fit — the two
ends of the chain — runs as one persistent workgroup between the launches of its neighbours.  A segment must change nothing: every
test compares index sets, link dimensions, bond errors and max_sample_value with the CPU oracle exactly, and the counter
t4a_gpu_tci2_chain_segments says whether the route under test was taken.

The split itself is a pure host function (t4a_gpu_tci2_chain_plan_segments): its cases need no device and are not marked gpu.

Reference: update_pivots / sweep2site / optimize_with_finder, crates/tensor4all-tensorci/src/tensorci2.rs:746-798, 1626-1802,
1821-2007; kronecker_i / kronecker_j :1224-1246; the history extras :1675-1689, :1833-1846."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = dict(nsearch=0, max_nglobal_pivot=0)
FORWARD, BACKWARD, BACK_AND_FORTH = 0, 1, 2
WALK_DEP, WALK_IND = 64, 32   # what the one-wave kernel of a walk takes: rows of the dependent, columns of the independent side


@pytest.fixture(scope="module")
def t4a():
    import t4a_amd
    if t4a_amd.device_count() < 1:
        pytest.fail("no MI355X visible: the product path has no CPU fallback")
    return t4a_amd


# ------------------------------------------------------------------------------------------------ helpers
def mixed_radix_weights(dims, n_acc):
    """Site s feeds accumulator s % n_acc with its digit times the product of the later sites' dimensions of the same accumulator:
    the accumulators are mixed-radix integers, most significant site first."""
    w = np.zeros((n_acc, sum(dims)), dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(dims)[:-1]])
    place = [1] * n_acc
    for s in range(len(dims) - 1, -1, -1):
        a = s % n_acc
        for v in range(dims[s]):
            w[a, off[s] + v] = v * place[a]
        place[a] *= dims[s]
    return w


def mixed_osc2d(dims):
    """The 2-variable oscillatory integrand of quantics_osc2d on sites of mixed local dimension (x and y are 10-bit fractions)."""
    from t4a_amd.functions import FnSpec, FN_QUANTICS_OSC2D
    return FnSpec(FN_QUANTICS_OSC2D, [37, 53, 211, 0.5, 1641, 0.5, 10, 10], mixed_radix_weights(dims, 2), dims)


def mixed_trig_exp(dims, n_bits):
    """cos(10 x) exp(-x), x = (mixed-radix position) / 2^n_bits: x is a sum over the sites, so every unfolding has exact rank 2."""
    from t4a_amd.functions import FnSpec, FN_QUANTICS_TRIG_EXP
    return FnSpec(FN_QUANTICS_TRIG_EXP, [10.0, 1.0, 1.0, 0.0, n_bits], mixed_radix_weights(dims, 1), dims)


def planned_bounds(dims, link, chi, forward):
    """Upper bounds of every bond's shape as the chain plans a 2-site half-sweep WITHOUT history extras from the set sizes alone
    (|I_{b+1}| = |J_b| = link[b]): rows kron(I_b, d_b), columns kron(d_{b+1}, J_{b+1}), and a bond leaves at most min(rows, columns,
    chi) pivots to the next one.  -> (dep_ub, ind_ub, order): the dependent side is the rows sweeping forward, the columns backward."""
    nb = len(dims) - 1
    c_i, c_j = [1] + list(link), list(link) + [1]
    dep, ind = [0] * nb, [0] * nb
    order = list(range(nb)) if forward else list(range(nb - 1, -1, -1))
    for b in order:
        m, n = c_i[b] * dims[b], c_j[b + 1] * dims[b + 1]
        m, n = min(m, int(np.prod(dims[:b + 1]))), min(n, int(np.prod(dims[b + 1:])))   # (never more entries than the index space)
        c_i[b + 1] = c_j[b] = max(min(m, n, chi), 1)
        dep[b], ind[b] = (m, n) if forward else (n, m)
    return dep, ind, order


def launched(t4a, spec, dims, verify=False):
    g = t4a.TensorCI2(dims)
    g.set_function(spec)
    g.set_chain(True, verify=verify, small_engine=False)   # the bond chain, not the one-launch engine for small problems
    return g


def oracle(spec, dims):
    o = ob.OracleTCI2(dims)
    o.set_function(spec)
    return o


def assert_same_state(g, o, n, what):
    for p in range(n):
        assert np.array_equal(g.i_set(p), o.i_set(p)), (what, "I", p)
        assert np.array_equal(g.j_set(p), o.j_set(p)), (what, "J", p)
    assert list(g.link_dims()) == list(o.link_dims()), what
    assert np.array_equal(g.bond_errors(), o.bond_errors()), what
    assert g.max_sample_value() == o.max_sample_value(), what


def assert_chained(g, what):
    st = g.chain_stats()
    assert st["fell_back"] == 0 and st["not_eligible"] == 0 and st["half_sweeps"] > 0, (what, st)


# ------------------------------------------------------------------------------------------------ every iteration against the oracle
N12, CHI12, ITERS12 = 12, 64, 6
OSC12 = dict(k1=3, k2=5, k3=7, eps=0.1, k4=11, delta=0.3)


def options12(t4a, k, strategy, nested):
    return t4a.TCI2Options(tolerance=1e-12, max_bond_dim=CHI12, max_iter=k, sweep_strategy=strategy, strictly_nested=nested,
                           ncheck_history=20, **PARITY)


@pytest.fixture(scope="module")
def oracle12(t4a):
    """The oracle's state after k = 1 .. 6 iterations from one pivot, per sweep strategy and nesting (a run of k iterations ends in
    the state a longer run passes through after its k-th iteration).  Computed once on the CPU, before any device run; the middle
    link dimension passes 32 on the oracle alone, so the middle bond outgrows 64 x 32 from some iteration on."""
    from t4a_amd.functions import quantics_osc2d
    spec = quantics_osc2d(N12, **OSC12)
    runs = {}
    for strategy in (FORWARD, BACKWARD, BACK_AND_FORTH):
        for nested in (False, True):
            for k in range(1, ITERS12 + 1):
                o = oracle(spec, [2] * N12)
                o.add_global_pivots([[0] * N12])
                o.optimize(options12(t4a, k, strategy, nested), final_sweep1site=False)
                runs[strategy, nested, k] = o
            mid = [runs[strategy, nested, k].link_dims()[N12 // 2 - 1] for k in range(1, ITERS12 + 1)]
            assert mid[0] <= 16 and mid[-1] > 32, (strategy, nested, mid)
    return spec, runs


@pytest.mark.gpu
@pytest.mark.parametrize("nested", [False, True], ids=["extras", "strictly_nested"])
@pytest.mark.parametrize("strategy", [FORWARD, BACKWARD, BACK_AND_FORTH], ids=["forward", "backward", "back_and_forth"])
def test_every_iteration_matches_oracle(t4a, oracle12, strategy, nested):
    """d = 12 binary sites, chi = 64, from one pivot: the first iterations are whole walks (every bond at most 64 x 32), the later
    ones launched chains with a walked head and a walked tail around the middle bonds; without strictly_nested the previous
    iteration's sets are merged as extras.  After EVERY iteration the state equals the oracle's exactly."""
    spec, runs = oracle12
    walked, segments, bonds = [], [], []
    for k in range(1, ITERS12 + 1):
        g = launched(t4a, spec, [2] * N12)
        g.add_global_pivots([[0] * N12])
        g.optimize(options12(t4a, k, strategy, nested), final_sweep1site=False)
        o = runs[strategy, nested, k]
        assert_same_state(g, o, N12, k)
        assert np.array_equal(g.pivot_errors(), o.pivot_errors()), k
        assert np.array_equal(g.last_sweep_shapes(), o.last_sweep_shapes()), k
        assert_chained(g, k)
        assert g.chain_stats()["half_sweeps"] == k, k
        walked.append(g.chain_stats()["walked_sweeps"])
        segments.append(g.chain_segments()["segments"])
        bonds.append(g.chain_segments()["bonds"])
    print("walked sweeps", walked, "segments", segments, "bonds in them", bonds)
    # precondition: the middle bond of the last sweep was wider than a walk takes, whichever side is the dependent one (its planned
    # bounds are no smaller than its shape)
    m, n, _ = g.last_sweep_shapes()[N12 // 2 - 1]
    assert max(m, n) > WALK_DEP or min(m, n) > WALK_IND, (m, n)
    # both kinds of half-sweep occurred: the counters of the k-iteration runs are those of one run after its k-th iteration
    per_iter_walked = np.diff([0] + walked).tolist()
    per_iter_segments = np.diff([0] + segments).tolist()
    assert per_iter_walked[0] == 1 and per_iter_segments[0] == 0, (walked, segments)     # a whole walk
    assert per_iter_walked[-1] == 0 and per_iter_segments[-1] == 2, (walked, segments)   # a head and a tail around the middle
    for w, s in zip(per_iter_walked, per_iter_segments):                                 # every half-sweep is one or the other
        assert (w == 1 and s == 0) or (w == 0 and s >= 1), (walked, segments)
    assert all(b >= s for b, s in zip(bonds, segments)), (bonds, segments)


@pytest.mark.gpu
def test_every_iteration_with_table_verification(t4a, oracle12):
    """The same run with set_chain(verify): after every chain the host's mirror must decode to the index sets and equal the device
    tables — the segments write their own part of both, the launched preparations the rest."""
    spec, runs = oracle12
    for strategy, nested in ((BACK_AND_FORTH, False), (FORWARD, True)):
        g = launched(t4a, spec, [2] * N12, verify=True)
        g.add_global_pivots([[0] * N12])
        g.optimize(options12(t4a, ITERS12, strategy, nested), final_sweep1site=False)
        assert_same_state(g, runs[strategy, nested, ITERS12], N12, (strategy, nested))
        assert_chained(g, (strategy, nested))
        assert g.chain_segments()["segments"] > 0


# ------------------------------------------------------------------------------------------------ edges of the split
def grown(t4a, dims, chi, iters, verify=False, nested=False):
    """Device handle and oracle after `iters` iterations from one pivot (compared), ready for single half-sweeps."""
    spec = mixed_osc2d(dims)
    n = len(dims)
    opts = t4a.TCI2Options(tolerance=1e-12, max_bond_dim=chi, max_iter=iters, strictly_nested=nested, ncheck_history=20, **PARITY)
    g, o = launched(t4a, spec, dims, verify=verify), oracle(spec, dims)
    for t in (g, o):
        t.add_global_pivots([[0] * n])
        t.optimize(opts, final_sweep1site=False)
    assert_same_state(g, o, n, "grown")
    return g, o


def half_sweep_and_plan(t4a, g, o, dims, chi, forward):
    """One sweep2site on both (no history extras: the plan follows from the link dimensions alone) -> the planned segments in sweep
    order and the counters this half-sweep added: (plan, walked sweeps, segments, bonds in segments)."""
    dep, ind, order = planned_bounds(dims, g.link_dims(), chi, forward)
    plan = t4a.chain_plan_segments(dep, ind, order)
    before = (g.chain_stats()["walked_sweeps"], g.chain_segments()["segments"], g.chain_segments()["bonds"])
    opts = t4a.TCI2Options(tolerance=1e-12, max_bond_dim=chi, **PARITY)
    g.sweep2site(forward, opts)
    o.sweep2site(forward, opts)
    assert_same_state(g, o, len(dims), ("sweep2site", forward))
    assert_chained(g, ("sweep2site", forward))
    after = (g.chain_stats()["walked_sweeps"], g.chain_segments()["segments"], g.chain_segments()["bonds"])
    return plan, tuple(a - b for a, b in zip(after, before))


def check_counters(plan, added):
    walked_runs = [s for s in plan if s[2]]
    if len(plan) == 1 and plan[0][2]:
        assert added == (1, 0, 0), (plan, added)     # everything fits: the whole half-sweep is one walk, no segment
    else:
        assert added == (0, len(walked_runs), sum(s[1] for s in walked_runs)), (plan, added)


@pytest.mark.gpu
def test_head_and_tail_of_one_bond(t4a):
    """Local dimensions 4, 2, 3, 2, 2, 3, 4, 2 at chi = 48: only the first and the last bond fit a walk — a head of one bond (its
    dependent list goes out to the launched bond behind it) and a tail of one bond (it starts from a launched bond's result block
    and ends the half-sweep), in both directions."""
    dims, chi = [4, 2, 3, 2, 2, 3, 4, 2], 48
    g, o = grown(t4a, dims, chi, 4, verify=True)
    for forward in (True, False, True):
        plan, added = half_sweep_and_plan(t4a, g, o, dims, chi, forward)
        assert [(s[1], s[2]) for s in plan] == [(1, True), (5, False), (1, True)], plan
        check_counters(plan, added)


@pytest.mark.gpu
def test_no_walkable_head_no_walkable_tail_and_a_walk_in_the_middle(t4a):
    """Chains that start or end with a launched bond, and a walked run between two launched runs."""
    seen = set()
    for dims, chi, iters in (([4, 4, 3, 2, 2, 3, 4, 4], 64, 2), ([4, 4, 3, 2, 2, 3, 4, 4], 64, 3), ([4, 4, 4, 3, 2, 2, 3, 2, 2], 48, 3),
                             ([2, 2, 3, 2, 2, 3, 6, 6], 64, 4)):
        g, o = grown(t4a, dims, chi, iters)
        for forward in (True, False):
            plan, added = half_sweep_and_plan(t4a, g, o, dims, chi, forward)
            check_counters(plan, added)
            kinds = [s[2] for s in plan]
            if len(kinds) > 1:
                seen.add("no head" if not kinds[0] else "head")
                seen.add("no tail" if not kinds[-1] else "tail")
                if any(kinds[1:-1]):
                    seen.add("middle")
            print(dims, chi, iters, "forward" if forward else "backward", plan, added)
    assert {"head", "no head", "tail", "no tail", "middle"} <= seen, seen


@pytest.mark.gpu
def test_everything_walkable_is_a_whole_walk(t4a):
    """max_bond_dim = 8, strictly nested (no extras: a side is at most 8 x 4 = 32 entries): every bond fits, the half-sweeps stay whole
    walks and the segment counter stays 0."""
    dims, chi = [4, 2, 3, 2, 2, 3, 4, 2], 8
    g, o = grown(t4a, dims, chi, 5, nested=True)
    st = g.chain_stats()
    assert st["walked_sweeps"] == st["half_sweeps"] == 5 and g.chain_segments() == dict(segments=0, bonds=0), (st, g.chain_segments())
    for forward in (True, False):
        plan, added = half_sweep_and_plan(t4a, g, o, dims, chi, forward)
        assert len(plan) == 1 and plan[0][2] and added == (1, 0, 0), (plan, added)


@pytest.mark.gpu
def test_exact_rank_two_stops_on_tolerance_inside_a_segment(t4a):
    """cos(10 x) exp(-x) has exact rank 2 across every bond.  Forty global pivots make the middle sets large, so the middle bonds are
    planned wide and launched while the ends are walked: inside the segments — and everywhere else — the factorisation stops on the
    tolerance at rank 2 with max_bond_dim = 64 far away."""
    dims, chi = [4, 2, 3, 2, 2, 3, 4, 2], 64
    n = len(dims)
    spec = mixed_trig_exp(dims, 12)
    rng = np.random.default_rng(5)
    pivots = np.unique(np.stack([rng.integers(0, d, size=60) for d in dims], axis=1), axis=0)[:40].tolist()
    pts = np.stack([rng.integers(0, d, size=64) for d in dims], axis=1)
    for strategy in (FORWARD, BACKWARD):   # (the first half-sweep meets the large sets: its first bonds are the walked end)
        opts = t4a.TCI2Options(tolerance=1e-10, max_bond_dim=chi, max_iter=2, sweep_strategy=strategy, ncheck_history=20, **PARITY)
        g, o = launched(t4a, spec, dims, verify=True), oracle(spec, dims)
        for t in (g, o):
            t.add_global_pivots(pivots)
        assert max(o.link_dims()) > 32, o.link_dims()   # (planned wide in the middle)
        for t in (g, o):
            t.optimize(opts, final_sweep1site=False)
        assert_same_state(g, o, n, ("rank 2", strategy))
        assert_chained(g, ("rank 2", strategy))
        assert max(g.link_dims()) == 2, g.link_dims()
        assert g.chain_segments()["segments"] >= 1 and g.chain_stats()["walked_sweeps"] <= 1, (g.chain_segments(), g.chain_stats())
        g.fill_site_tensors()
        o.fill_site_tensors()
        assert np.abs(g.evaluate(pts) - o.evaluate(pts)).max() <= 1e-10


# ------------------------------------------------------------------------------------------------ unaffected routes
def digest(t, n):
    h = hashlib.sha256()
    for p in range(n):
        h.update(np.ascontiguousarray(t.i_set(p)).tobytes())
        h.update(np.ascontiguousarray(t.j_set(p)).tobytes())
    h.update(np.ascontiguousarray(t.bond_errors()).tobytes())
    h.update(np.ascontiguousarray(t.pivot_errors()).tobytes())
    h.update(np.float64(t.max_sample_value()).tobytes())
    t.fill_site_tensors()
    for p in range(n):
        h.update(np.ascontiguousarray(t.site_tensor(p)).tobytes())
    return h.hexdigest()


CHILD = r'''
import sys
sys.path.insert(0, "tensor4all-rs_amd/python")
sys.path.insert(0, "tests")
import t4a_amd as t4a
import test_gpu_chain_segments as m
n = m.N12
g = m.launched(t4a, t4a.quantics_osc2d(n, **m.OSC12), [2] * n)
g.add_global_pivots([[0] * n])
g.optimize(m.options12(t4a, m.ITERS12, m.BACK_AND_FORTH, False), final_sweep1site=False)
print("digest", m.digest(g, n), g.chain_stats()["walked_sweeps"], g.chain_segments()["segments"], g.chain_stats()["fell_back"])
'''


@pytest.mark.gpu
def test_no_walk_switch_covers_segments_and_gives_identical_results(t4a, oracle12):
    """T4A_NO_WALK=1 (read once per process: a fresh child) launches every bond; index sets, errors and the filled site tensors are
    those of the run with walks and segments, byte for byte."""
    spec, runs = oracle12
    g = launched(t4a, spec, [2] * N12)
    g.add_global_pivots([[0] * N12])
    g.optimize(options12(t4a, ITERS12, BACK_AND_FORTH, False), final_sweep1site=False)
    assert_same_state(g, runs[BACK_AND_FORTH, False, ITERS12], N12, "here")
    assert g.chain_segments()["segments"] > 0 and g.chain_stats()["walked_sweeps"] > 0
    here = digest(g, N12)
    env = dict(os.environ, T4A_NO_WALK="1")
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("digest ")][-1].split()
    assert line[2:] == ["0", "0", "0"], line   # no walk, no segment, nothing fell back
    assert line[1] == here


@pytest.mark.gpu
def test_group_chain_has_no_segments(t4a):
    """optimize_group of two handles: the group chain launches every bond for both; results equal one handle at a time (whose chains
    have segments), the segment counter of the grouped handles stays 0."""
    from t4a_amd.functions import quantics_osc2d
    specs = [quantics_osc2d(N12, **OSC12), quantics_osc2d(N12, k1=2, k2=7, k3=5, eps=0.2, k4=13, delta=0.4)]
    opts = options12(t4a, ITERS12, BACK_AND_FORTH, False)
    solo, grouped = [], []
    for spec in specs:
        for into in (solo, grouped):
            g = launched(t4a, spec, [2] * N12)
            g.add_global_pivots([[0] * N12])
            into.append(g)
    for g in solo:
        g.optimize(opts, final_sweep1site=False)
    t4a.optimize_group(grouped, opts, final_sweep1site=False)
    for a, b in zip(solo, grouped):
        for p in range(N12):
            assert np.array_equal(a.i_set(p), b.i_set(p)) and np.array_equal(a.j_set(p), b.j_set(p)), p
        assert np.array_equal(a.bond_errors(), b.bond_errors()) and a.max_sample_value() == b.max_sample_value()
        assert a.chain_segments()["segments"] > 0
        assert b.chain_stats()["group_half_sweeps"] > 0 and b.chain_stats()["fell_back"] == 0
        assert b.chain_segments() == dict(segments=0, bonds=0)


# ------------------------------------------------------------------------------------------------ the planner (host only)
def plan(dep, ind, order=None):
    import t4a_amd
    return t4a_amd.chain_plan_segments(dep, ind, list(range(len(dep))) if order is None else order)


def test_planner_empty_chain():
    assert plan([], []) == []


def test_planner_all_walkable_and_none_walkable():
    assert plan([2, 8, 16, 8], [8, 16, 8, 2]) == [(0, 4, True)]
    assert plan([128, 512, 512], [64, 512, 128]) == [(0, 3, False)]
    assert plan([1], [1]) == [(0, 1, True)]
    assert plan([1], [33]) == [(0, 1, False)]


def test_planner_runs_are_maximal_and_in_sweep_order():
    dep = [8, 16, 128, 32, 16, 256, 64, 8]
    ind = [16, 32, 64, 8, 16, 256, 16, 2]
    assert plan(dep, ind) == [(0, 2, True), (2, 1, False), (3, 2, True), (5, 1, False), (6, 2, True)]   # a walkable run in the middle
    back = list(range(len(dep) - 1, -1, -1))
    assert plan(dep, ind, back) == [(0, 2, True), (2, 1, False), (3, 2, True), (5, 1, False), (6, 2, True)]
    assert plan(dep[:6], ind[:6], back[2:]) == [(0, 1, False), (1, 2, True), (3, 1, False), (4, 2, True)]  # positions, not bonds


def test_planner_bounds_are_inclusive_at_64_and_32():
    assert plan([64], [32]) == [(0, 1, True)]
    assert plan([65], [32]) == [(0, 1, False)]
    assert plan([64], [33]) == [(0, 1, False)]
    assert plan([64, 65, 64, 64], [32, 32, 33, 32]) == [(0, 1, True), (1, 2, False), (3, 1, True)]


def test_planner_rejects_an_order_that_is_no_bond():
    import t4a_amd
    with pytest.raises(t4a_amd.T4aError):
        plan([1, 1], [1, 1], [0, 2])
