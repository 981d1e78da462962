"""fuse_to, split_to and restructure_to on the device with random operands, against the dense tensor and the numpy restatement
(tests/restructure_np.py): at most 8 sites, bonds up to 40.

FUSE.  A group of k cores A_1 .. A_k with inner bonds m_1 .. m_{k-1} is contracted left to right.  Round t forms, per element, a sum
of m_t products of the accumulated core with A_{t+1}; multiply and add are rounded separately (or, on the matrix cores, in chunks of
four in ascending order), so by the standard bound for an inner product of length m_t the round adds at most m_t * u * (|acc| |A_{t+1}|)
to the error it inherits, u = 2^-53, and the inherited error of the accumulated core is carried through the same nonnegative
product.  By induction the error of the result is at most ((1 + u)^(m_1 + .. + m_{k-1}) - 1) (|A_1| .. |A_k|) componentwise; the
second-order terms of that expansion are far below one u for the bonds used here and are covered by adding k.  The leg permutation
of the last round moves elements and rounds nothing.  Hence
    |out - exact| <= (sum_t m_t + k) * 2^-53 * (|A_1| .. |A_k|)    componentwise,
with `exact` evaluated in extended precision (its own error is 2^-11 of the unit of this bound).

SPLIT.  |dense(out) - dense(in)|_F <= C_SPLIT * n_qr * eps * |T|_F with C_SPLIT = 8 * 2.14: 2.14 is the restatement's own largest
deviation over the split cases and seeds 0 .. 19 (tests/test_cpu_restructure.py asserts it), 8 the margin swap's C_DENSE gives a
different QR implementation.  See tests/restructure_np.py; the number was not tuned to the device's output.

The dense tensor of a result is evaluated by numpy from the result's cores, and the fuse phase of restructure_to works on the cores
the earlier phase left; both round like a fuse.  Their share of a tolerance is gamma * | |A_1| .. |A_n| |_F with the cores the
restatement hands to its fuse phase and gamma = (all bonds of that train + its sites + the result's sites) * 2^-53."""
import numpy as np
import pytest

import restructure_np as rn
import swap_np as sn
import t4a_amd
from t4a_amd import (LegTrain, MPO, RestructureOptions, SimpleTensorTrain, SplitOptions, SvdTruncationPolicy, T4aError, fuse_quantics,
                     fuse_to, restructure_to, split_to, unfuse_quantics)
from t4a_amd.mpo import truncate_many

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def leg_train(cores, legs):
    return LegTrain(SimpleTensorTrain(cores), legs)


def abs_chain_norm(cores, legs):
    return float(np.linalg.norm(sn.to_dense([np.abs(c) for c in cores], legs)))


def rounding_share(cores, legs, n_out):
    """the share of evaluating and fusing: see the module docstring"""
    gamma = (sum(c.shape[2] for c in cores[:-1]) + len(cores) + n_out) * U
    return gamma * abs_chain_norm(cores, legs)


_FUSE = {}


def fuse_inputs():
    """a train whose groups have 1, 2, 3 and 4 members, made once"""
    if not _FUSE:
        rng = np.random.default_rng(0)
        legs = [[("a", 2)], [("b", 3)], [("c", 2), ("d", 2)], [], [("e", 3)], [("f", 2)], [("g", 2)], [("h", 3)]]
        cores = sn.random_train(rng, legs, [2, 6, 24, 17, 40, 16, 3])
        target = [["a"], ["c", "b", "d"], ["e", "g", "h", "f"]]
        _FUSE.update(legs=legs, cores=cores, target=target)
    return _FUSE["cores"], _FUSE["legs"], _FUSE["target"]


def test_fuse_error_is_within_the_componentwise_bound():
    cores, legs, target = fuse_inputs()
    out = fuse_to(leg_train(cores, legs), target, as_legs=True)
    fp = rn.fuse_plan(legs, target)
    assert fp["members"] == [[0], [1, 2, 3], [4, 5, 6, 7]]
    exact, _ = rn.fuse([c.astype(np.longdouble) for c in cores], legs, target)
    bound, _ = rn.fuse([np.abs(c) for c in cores], legs, target)
    got = out._tt.site_tensors()
    for g, members in enumerate(fp["members"]):
        k = len(members)
        m_sum = sum(cores[s].shape[2] for s in members[:-1])
        err = np.abs(got[g].astype(np.longdouble) - exact[g]).astype(np.float64)
        lim = (m_sum + k) * U * bound[g] if k > 1 else np.zeros_like(bound[g])
        print(f"group {g}: k = {k}, sum m = {m_sum}, max err / unit = {float((err / (U * bound[g])).max()):.3f} of {m_sum + k}")
        assert got[g].shape == exact[g].shape and np.all(err <= lim)
    assert out.legs == [[(k, d) for k, d in g] for g in fp["legs"]]


_SPLIT = {}


def split_inputs(name):
    if name not in _SPLIT:
        legs, bonds, target = rn.split_cases()[name]
        cores = sn.random_train(np.random.default_rng(0), legs, bonds)
        _SPLIT[name] = (cores, legs, target, sn.to_dense(cores, legs))
    return _SPLIT[name]


@pytest.mark.parametrize("name", sorted(rn.split_cases()))
def test_split_equals_the_dense_input_and_peels_isometries(name):
    cores, legs, target, dense = split_inputs(name)
    ref_cores, ref_legs, info = rn.split(cores, legs, target)
    out = split_to(leg_train(cores, legs), target, as_legs=True)
    assert out.legs == ref_legs and out.center is None
    got = out._tt.site_tensors()
    # bonds equal min(rows, cols) of every unfolding on generic inputs
    assert all(k == min(rows, cols) for rows, cols, k in info["qr_shapes"])
    assert [c.shape for c in got] == [c.shape for c in ref_cores]
    exact = sn.permuted(dense, sn.keys_of(legs), out.keys())
    err = np.linalg.norm(out.to_dense() - exact)
    unit = info["n_qr"] * rn.EPS * np.linalg.norm(dense)
    print(f"{name}: |out - exact| = {err / unit:.3f} n_qr eps |T| (allowed {rn.C_SPLIT:.2f})")
    assert err <= rn.C_SPLIT * unit
    for f in info["fragments"]:  # every peeled fragment is left-orthogonal to the same scale
        q = got[f].reshape(-1, got[f].shape[2], order="F")
        dev = np.linalg.norm(q.T @ q - np.eye(q.shape[1]))
        print(f"  fragment {f}: |Q^T Q - 1| = {dev / (rn.EPS * np.sqrt(q.shape[1])):.3f} eps sqrt(k)")
        assert dev <= rn.C_SPLIT * rn.EPS * np.sqrt(q.shape[1])


@pytest.mark.parametrize("name", ["mpo_sites", "three_fragments_reordered"])
def test_fuse_of_split_gives_the_dense_tensor_back(name):
    cores, legs, target, dense = split_inputs(name)
    lt = leg_train(cores, legs)
    parts = split_to(lt, target, as_legs=True)
    back = fuse_to(parts, [[k for k, _ in site] for site in legs], as_legs=True)
    assert back.legs == [list(s) for s in legs]
    n_qr = rn.split_plan(legs, target)["n_qr"]
    ref_parts, ref_legs, _ = rn.split(cores, legs, target)
    tol = rn.C_SPLIT * n_qr * rn.EPS * np.linalg.norm(dense) + rounding_share(ref_parts, ref_legs, len(legs))
    assert np.linalg.norm(back.to_dense() - dense) <= tol


def test_quantics_round_trip_three_bits_two_variables():
    rng = np.random.default_rng(1)
    legs = sn.train_legs([2] * 6)
    cores = sn.random_train(rng, legs, [2, 4, 8, 4, 2])
    dense = sn.to_dense(cores, legs)  # axes x1 y1 x2 y2 x3 y3
    tt = SimpleTensorTrain(cores)
    fused = fuse_quantics(tt, 2)
    assert isinstance(fused, SimpleTensorTrain) and fused.site_dims() == [4, 4, 4] and fused.link_dims() == [4, 4]
    fd = sn.to_dense(fused.site_tensors(), sn.train_legs([4] * 3))
    # site index x + 2 y, the first variable least significant: a reshape of the dense tensor
    share = rounding_share(cores, legs, 3)
    assert np.linalg.norm(fd - dense.reshape(4, 4, 4, order="F")) <= share
    again = unfuse_quantics(fused, 2)
    assert isinstance(again, SimpleTensorTrain) and again.site_dims() == [2] * 6
    ad = sn.to_dense(again.site_tensors(), legs)
    assert np.linalg.norm(ad - dense) <= rn.C_SPLIT * 3 * rn.EPS * np.linalg.norm(dense) + share
    # variable-major order of the bits of a fused site: the transposed dense tensor is what swapping x and y gives
    swapped = fuse_to(LegTrain.from_train(tt), [[(2 * b + 1, 0), (2 * b, 0)] for b in range(3)], as_legs=True)
    sd = sn.to_dense(swapped._tt.site_tensors(), sn.train_legs([4] * 3))
    assert np.linalg.norm(sd - np.transpose(dense, [1, 0, 3, 2, 5, 4]).reshape(4, 4, 4, order="F")) <= share


_CASES = {}


def case_inputs(name):
    if name not in _CASES:
        legs, bonds, target, kind = rn.restructure_cases()[name]
        cores = sn.random_train(np.random.default_rng(0), legs, bonds)
        _CASES[name] = (cores, legs, target, kind, sn.to_dense(cores, legs))
    return _CASES[name]


def fuse_operands(cores, legs, target):
    """the train the restatement hands to its fuse phase"""
    p = rn.plan(legs, target)
    if p["kind"] in ("SwapOnly", "SwapThenFuse"):
        c, lg, _, _ = sn.swap(cores, legs, p["swap_target"])
        return c, lg
    if p["kind"] == "SplitThenFuse":
        c, lg, _ = rn.split(cores, legs, p["split_target"], keep_legless=True)
        return c, lg
    return cores, legs


@pytest.mark.parametrize("name", sorted(rn.restructure_cases()))
def test_restructure_equals_the_regrouped_dense_tensor(name):
    cores, legs, target, kind, dense = case_inputs(name)
    _, ref_legs, ref = rn.restructure(cores, legs, target)
    out, info = restructure_to(leg_train(cores, legs), target, as_legs=True, info=True)
    assert info["kind"] == kind == ref["kind"]
    dim = {k: d for s in legs for k, d in s}
    assert out.legs == ref_legs == [[(k, dim[k]) for k in g] for g in target]
    assert (info["n_swap_steps"], info["n_qr"]) == (ref["n_steps"], ref["n_qr"])
    exact = sn.permuted(dense, sn.keys_of(legs), out.keys())
    fc, fl = fuse_operands(cores, legs, target)
    tol = (sn.C_DENSE * ref["n_steps"] + rn.C_SPLIT * ref["n_qr"]) * rn.EPS * np.linalg.norm(dense) + rounding_share(fc, fl, len(target))
    err = np.linalg.norm(out.to_dense() - exact)
    print(f"{name}: {kind}, |out - exact| = {err / (rn.EPS * np.linalg.norm(dense)):.3f} eps |T|, allowed {tol / (rn.EPS * np.linalg.norm(dense)):.1f}")
    assert err <= tol


def as_sites_s1(tt):
    """the chain seen as an MPO with sites (s, 1)"""
    return MPO.from_tensor_train(tt)


@pytest.mark.parametrize("policy,cap", [(SvdTruncationPolicy(1e-3), None), (None, 3)])
def test_final_sweep_and_final_truncation_have_the_bits_of_the_serial_truncation_stage(policy, cap):
    cores, legs, target, _ = split_inputs("fused_quantics_3x2")
    lt = leg_train(cores, legs)
    plain = split_to(lt, target, as_legs=True)
    ref = truncate_many([as_sites_s1(plain._tt)], policy, cap, route="serial")[0].site_tensors()
    swept = split_to(lt, target, SplitOptions(policy=policy, max_bond_dim=cap, final_sweep=True), as_legs=True)
    got = swept._tt.site_tensors()
    assert [g.shape for g in got] == [(r.shape[0], r.shape[1], r.shape[3]) for r in ref]
    assert all(np.array_equal(g.view(np.uint64), r.reshape(g.shape, order="F").view(np.uint64)) for g, r in zip(got, ref))
    if cap is not None:
        assert max(swept.link_dims()) <= cap < max(plain.link_dims())
    # restructure_to: the same stage after the phases of the kind
    c2, l2, t2, _, _ = case_inputs("split_then_fuse")
    lt2 = leg_train(c2, l2)
    plain2 = restructure_to(lt2, t2, as_legs=True)
    ref2 = truncate_many([as_sites_s1(plain2._tt)], SvdTruncationPolicy() if policy is None else policy, cap, route="serial")[0].site_tensors()
    cut = restructure_to(lt2, t2, RestructureOptions(final_truncation=(SvdTruncationPolicy() if policy is None else policy, cap)), as_legs=True)
    got2 = cut._tt.site_tensors()
    assert [g.shape for g in got2] == [(r.shape[0], r.shape[1], r.shape[3]) for r in ref2]
    assert all(np.array_equal(g.view(np.uint64), r.reshape(g.shape, order="F").view(np.uint64)) for g, r in zip(got2, ref2))
    assert cut.center is None


def test_result_types_follow_the_rule_of_swap():
    rng = np.random.default_rng(2)
    sd = [(2, 3), (3, 2), (2, 2), (2, 3)]
    cores = [rng.standard_normal((l, a, b, r)) for (a, b), l, r in zip(sd, [1, 5, 17, 4], [5, 17, 4, 1])]
    m = MPO(cores)
    # an MPO in, an MPO out when every result site has two legs: the rows of sites 0 and 1 and their columns as two sites
    out = restructure_to(m, [[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(2, 0), (2, 1)], [(3, 1), (3, 0)]])
    assert isinstance(out, MPO) and out.site_dims() == [(2, 3), (3, 2), (2, 2), (3, 2)]
    parts = split_to(m, [[(i, q)] for i in range(4) for q in (0, 1)])
    assert isinstance(parts, SimpleTensorTrain) and parts.site_dims() == [2, 3, 3, 2, 2, 2, 2, 3]
    fused = fuse_to(m, [[(0, 0), (0, 1), (1, 0), (1, 1)], [(2, 0), (2, 1)], [(3, 0), (3, 1)]])
    assert isinstance(fused, LegTrain) and [len(s) for s in fused.legs] == [4, 2, 2]
    dense = LegTrain.from_mpo(m).to_dense()
    lt = LegTrain.from_mpo(m)
    assert np.linalg.norm(fused.to_dense() - dense) <= rounding_share(lt._tt.site_tensors(), lt.legs, 3)


def test_refusals_reach_the_caller_before_any_work():
    cores, legs, target, _ = split_inputs("mpo_sites")
    lt = leg_train(cores, legs)
    with pytest.raises(T4aError) as e:
        split_to(lt, target, SplitOptions(form="lu"))
    assert e.value.code == t4a_amd.NOT_IMPLEMENTED
    with pytest.raises(T4aError, match="spans multiple current nodes; use restructure_to for mixed regrouping"):
        split_to(lt, [[(0, 0)], [(0, 1), (1, 0)], [(1, 1)], [(2, 0), (2, 1)]])
    with pytest.raises(T4aError, match="restructure_to can move them"):
        fuse_to(lt, [[(1, 0), (1, 1)], [(0, 0), (0, 1)], [(2, 0), (2, 1)]])
    with pytest.raises(T4aError, match="planner placeholder only"):
        restructure_to(lt, [[(0, 0), (2, 0)], [(0, 1), (1, 0), (1, 1), (2, 1)]])
