"""The budgeted-truncation kernels (mpo.truncate_many: bt_qr_step_kernel, bt_svd_step_kernel in both directions) pinned exactly, through
the trace hook that returns per item the squared norm the QR sweep found and per SVD step the singular values and the rank.

The items are those of tests/patching_cases_np.py: chains of two and three sites whose cores are signed partial permutations times
diag(2^-k), so that every singular value and every sum of squares is exactly representable; bonds 1, 2, 15, 16, 17, 33 and 64 on the
kernels and 65 on the serial stage of the same call; tall, square and wide steps; site dims 2 and 3 and fused ones; a threshold and a
cap of its own per item.  tests/test_cpu_patching.py checks that every threshold sits between two of the quantities the rule compares
(relative distance > 0.05 at every one of the 2 (n - 1) truncations) and that the model of the expected values is the restatement."""
import numpy as np
import pytest

import t4a_amd
from t4a_amd import MPO, T4aError, INVALID_ARGUMENT, SvdTruncationPolicy, svd_retained_rank
from t4a_amd import mpo as M

import patching_np as R
import patching_cases_np as C

pytestmark = pytest.mark.gpu


def run(batch, route="batched"):
    ops = [MPO(t) for _, t, _, _, _ in batch]
    pols = [SvdTruncationPolicy(*p) for _, _, _, p, _ in batch]
    caps = [c for _, _, _, _, c in batch]
    return ops, pols, caps, M._truncate_many(ops, pols, caps, route, True, trace=True)


@pytest.mark.parametrize("smr", C.POLICIES)
@pytest.mark.parametrize("n", [2, 3])
def test_singular_values_ranks_and_norms_are_exact_under_every_policy(n, smr):
    batch = C.exact_batch(n, smr)
    ops, pols, caps, (_, bonds, counts, tr) = run(batch)
    names = [b[0] for b in batch]
    assert counts["n_serial"] == sum("serial" in nm for nm in names) == 1 and counts["n_batched"] == len(batch) - 1
    assert counts["launches"] == 3 * (n - 1) and counts["syncs"] == 1
    for k, (name, tensors, values, policy, cap) in enumerate(batch):
        norm2, steps = C.model(values, n, policy, cap)
        if "serial" in name:
            assert abs(tr["norm2"][k] - norm2) <= 1e-13 * norm2, (name, tr["norm2"][k], norm2)
        else:
            assert tr["norm2"][k] == norm2, (name, tr["norm2"][k], norm2)
        for t, (want, rank, _) in enumerate(steps):
            got = tr["sv"][k, t]
            if "serial" in name:  # the serial stage computes its own values: it is held to its own rule, and to the model's rank
                m = min(len(want), 64)  # (the hook records 64 values per step)
                assert np.allclose(got[:m], want[:m], rtol=1e-13, atol=0.0), (name, t)
            else:
                assert np.array_equal(got[:len(want)], want) and not got[len(want):].any(), (name, t, got[:len(want) + 2], want)
            # the device rule against the host's on the values the step itself computed, then the cap and the floor (the serial
            # stage IS the host's rule; its 65 values do not fit the hook's 64, so it is held to the model alone)
            if "serial" not in name:
                host = svd_retained_rank(got, pols[k])
                host = max(1, host if cap is None else min(host, cap))
                assert tr["ranks"][k, t] == host, (name, t, tr["ranks"][k, t], host)
            assert tr["ranks"][k, t] == rank, (name, t, tr["ranks"][k, t], rank)
        # the bonds of the result are the ranks of the way back
        assert bonds[k] == [1] + [int(r) for r in tr["ranks"][k, n - 1:]] + [1], name


@pytest.mark.parametrize("n", [2, 3])
def test_a_zero_item_stays_where_the_serial_svd_leaves_a_zero_matrix(n):
    batch = [b for b in C.exact_batch(n, (1, 1, 1)) if b[0] == "zero"] * 2
    for route in ("batched", "serial"):
        _, _, _, (_, bonds, counts, tr) = run(batch, route)
        assert bonds == [[1] * (n + 1)] * 2 and not tr["sv"].any() and not tr["norm2"].any() and (tr["ranks"] == 1).all(), route
    res, bonds, _ = M._truncate_many([MPO(batch[0][1])], [SvdTruncationPolicy(*batch[0][3])], None, "batched", False)
    assert bonds == [[1] * (n + 1)] and not res[0].full_tensor().any()


def test_an_inf_fails_the_call_with_the_lowest_item_index():
    batch = C.exact_batch(3, (0, 0, 0))[:5]
    tensors = [[x.copy() for x in t] for _, t, _, _, _ in batch]
    tensors[3][1][0, 0, 0, 0] = np.inf
    tensors[1][2][0, 1, 0, 0] = np.inf
    for route in ("batched", "serial"):
        with pytest.raises(T4aError) as e:
            M.truncate_many([MPO(t) for t in tensors], None, None, route)
        assert e.value.code == INVALID_ARGUMENT and "truncate_many: item 1: SVD computation failed: non-finite input" in str(e.value)


def bits(m):
    return [t.view(np.uint64).copy() for t in m.site_tensors()]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [2, 3])
def test_the_same_bits_twice_and_alone_or_inside_a_batch_of_seven(n):
    rng = np.random.default_rng(n)
    sds = [C.M23] * n
    items = [C.random_chain(rng, sds, [1] + [int(b) for b in rng.integers(2, 18, n - 1)] + [1]) for _ in range(7)]
    ops = [MPO(t) for t in items]
    pols = [SvdTruncationPolicy(10.0 ** -(k + 1), k % 2, (k // 2) % 2, (k // 4) % 2) for k in range(7)]
    caps = [None, 3, None, 5, 2, None, 4]
    first = M.truncate_many(ops, pols, caps, "batched")
    again = M.truncate_many(ops, pols, caps, "batched")
    for k in range(7):
        assert same(bits(first[k]), bits(again[k])), k
        alone = M.truncate_many([ops[k]], [pols[k]], [caps[k]], "batched")
        assert same(bits(first[k]), bits(alone[0])), k


@pytest.mark.parametrize("n", [2, 3])
def test_ranks_only_returns_the_bonds_of_the_full_call_and_the_counts_are_the_plan(n):
    batch = C.exact_batch(n, (1, 1, 1))
    ops = [MPO(t) for _, t, _, _, _ in batch]
    pols = [SvdTruncationPolicy(*p) for _, _, _, p, _ in batch]
    caps = [c for _, _, _, _, c in batch]
    res, bonds, counts = M._truncate_many(ops, pols, caps, "batched", False)
    none, only, counts_only = M._truncate_many(ops, pols, caps, "batched", True)
    assert none is None and only == bonds and counts_only == counts
    assert [[1] + m.link_dims() + [1] for m in res] == bonds
    plan = M.truncate_many_plan([[tuple(int(x) for x in s.shape) for s in t] for _, t, _, _, _ in batch], caps, "batched")
    assert (counts["launches"], counts["syncs"], counts["n_batched"]) == (plan["launches"], plan["syncs"], plan["n_batched"])
    assert plan["routes"] == ["serial" if "serial" in b[0] else "batched" for b in batch]
    for b, bound in zip(bonds, plan["bonds"]):
        assert all(x <= y for x, y in zip(b, bound))
    # the tensors: what the model says survives, to rounding (the values are exact, the products of the factors are not pinned)
    for (name, t, values, policy, cap), m in zip(batch, res):
        _, steps = C.model(values, n, policy, cap)
        kept = values[:steps[-1][1]] if values else []
        F = R.dense(t)
        err = np.linalg.norm(m.full_tensor() - F)
        want = np.sqrt(max(sum(v * v for v in values) - sum(v * v for v in kept), 0.0))
        assert abs(err - want) <= 1e-13 * max(np.linalg.norm(F), 1.0), (name, err, want)
