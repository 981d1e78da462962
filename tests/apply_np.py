"""numpy restatement of an operator applied on a subset of a state's sites (t4a_gpu_linop_*): the plan with its refusals, the dense
reference (identities (x) O) x by einsum for n <= 8, and the three methods.  The state is a list of cores X_i[b, x, b'], the operator a
list of site tensors O_j[a, y, x, a'] (leg 0 the output, leg 1 the input), ``sites`` the state positions of the operator's sites.
Result bonds are fused with the operator index slow and the state index fast.  The restated zip-up and fit are the recursion and the
sweeps of tests/fit_np.py run on the operator with its gap sites written out (a bridge site is delta_{aa'} delta_{yx}, an outside site
the identity with bond 1) and the state as an MPO with s2 = 1; nothing of the code under test is used.

The module also holds the operand sets of the GPU driver tests (CASES): tests/test_cpu_linop.py asserts the gap condition for exactly
these, tests/test_gpu_linop.py runs them on the device."""
import numpy as np

import fit_np
from fit_np import SEED, Options, random_tensors, np_full, links  # noqa: F401  (re-exported)
from partial_np import GapLog


class PlanError(ValueError):
    """INVALID_ARGUMENT of the plan"""


def np_plan(op_dims, sites, state_dims):
    """op_dims: (left, out, in, right) per operator site; state_dims: (left, site, right) per state site ->
    {"kinds", "bonds", "result_dims"} as t4a_amd.apply_plan; the checks and their order are those of apply_plan (csrc/linop.hip)"""
    k, n = len(op_dims), len(state_dims)
    sites = [int(s) for s in sites]
    if k == 0:
        raise PlanError("apply_linear_operator: the operator has no sites")
    if len(sites) != k:
        raise PlanError(f"apply_linear_operator: the operator has {k} sites, `sites` names {len(sites)} positions")
    if any(a >= b for a, b in zip(sites[:-1], sites[1:])):
        raise PlanError(f"apply_linear_operator: sites must be strictly ascending, got {sites}")
    if sites[-1] >= n:
        raise PlanError(f"Operator nodes {sites} are not a subset of state nodes {list(range(n))}")
    for j, s in enumerate(sites):
        if op_dims[j][2] != state_dims[s][1]:
            raise PlanError(f"Shared shape mismatch at site {s}: operator has input dim {op_dims[j][2]}, the state has site dim {state_dims[s][1]}")
    kinds, bonds, res = [], [], []
    j = 0
    for i in range(n):
        lb, d, rb = state_dims[i]
        if j < k and sites[j] == i:
            kinds.append("op")
            ml, dout, _, mr = op_dims[j]
            j += 1
        else:
            kinds.append("outside" if j in (0, k) else "bridge")
            ml = mr = op_dims[j][0] if kinds[-1] == "bridge" else 1
            dout = d
        for m, b in ((ml, lb), (mr, rb)):
            if m * b > 65535:
                raise PlanError(f"apply_linear_operator: site {i}: the fused bond {m} * {b} is above 65535")
        if ml * lb * dout * mr * rb > 2 ** 31 - 1:
            raise PlanError(f"apply_linear_operator: site {i}: the result's core holds more than INT_MAX elements")
        bonds.append((ml, mr))
        res.append((ml * lb, dout, mr * rb))
    return {"kinds": kinds, "bonds": bonds, "result_dims": res}


def np_extend(op, sites, site_dims):
    """the full-length operator: bridge sites delta_{aa'} delta_{yx} of shape (m, d, d, m), outside sites (1, d, d, 1) identities"""
    plan = np_plan([t.shape for t in op], sites, [(1, d, 1) for d in site_dims])
    out, j = [], 0
    for i, d in enumerate(site_dims):
        if plan["kinds"][i] == "op":
            out.append(op[j])
            j += 1
        else:
            m = plan["bonds"][i][0]
            out.append(np.einsum("ab,yx->ayxb", np.eye(m), np.eye(d)))
    return out


def as_mpo(x):
    return [c.reshape(c.shape + (1,)).transpose(0, 1, 3, 2) for c in x]  # [b, x, 1, b']


def as_train(ts):
    return [t[:, :, 0, :] for t in ts]


def np_dense_state(x):
    acc = x[0][0]
    for c in x[1:]:
        acc = np.tensordot(acc, c, axes=([-1], [0]))
    return acc[..., 0]


def np_dense_apply(op, sites, x):
    """(identities (x) O) x as a dense tensor indexed by the result's site indices, n <= 8"""
    assert len(x) <= 8
    psi = np_dense_state(x)
    o = np_full(op)  # [y_0, x_0, y_1, x_1, ...]
    k = len(op)
    r = np.tensordot(o, psi, axes=([2 * j + 1 for j in range(k)], list(sites)))  # [y_0 .. y_{k-1}, the other state legs in order]
    rest = [i for i in range(len(x)) if i not in sites]
    return np.moveaxis(r, list(range(len(x))), list(sites) + rest)


def np_naive(op, sites, x):
    """the exact site-wise product: Y[(a lb + b), y, (a' rb + b')] = sum_x O[a, y, x, a'] X[b, x, b']"""
    full = np_extend(op, sites, [c.shape[1] for c in x])
    out = []
    for o, c in zip(full, x):
        y = np.einsum("ayxr,bxq->bayqr", o, c)
        out.append(y.reshape((c.shape[0] * o.shape[0], o.shape[1], c.shape[2] * o.shape[3]), order="F"))
    return out


def np_zipup(op, sites, x, options):
    return as_train(fit_np.np_zipup(np_extend(op, sites, [c.shape[1] for c in x]), as_mpo(x), options))


def np_fit(op, sites, x, options, initial=None):
    """-> (cores, {"n_sweeps", "norms"})"""
    ts, info = fit_np.np_fit(np_extend(op, sites, [c.shape[1] for c in x]), as_mpo(x), options, None if initial is None else as_mpo(initial))
    return as_train(ts), info


def np_gap_half(env, x, right):
    """left: P[n, x, a, d] = sum_b L[n, a, b] X[b, x, d]; right: Q[a, b, x, n] = sum_d X[b, x, d] R[a, d, n]"""
    return np.einsum("bxd,adn->abxn", x, env) if right else np.einsum("nab,bxd->nxad", env, x)


# ------------------------------------------------------------------------------------------------ the gap condition
def gap_violations(log, factor=1e3, cap_ratio=1.01):
    """At every factorize of a recorded restatement run: no singular value that can decide lies within `factor` of tolerance * s_max,
    and a cap does not cut between two values closer than `cap_ratio`.  The ranks of a correct device run are then determined."""
    bad = []
    for k, (s, tol, cap) in enumerate(log.splits):
        if s.size == 0 or s.max() == 0.0:
            continue
        cut = tol * s.max()
        if tol > 0.0:
            for v in s if cap is None else s[:cap]:
                if cut / factor < v < cut * factor:
                    bad.append((k, "tolerance", float(v / cut)))
        kept = int((s >= cut).sum()) if tol > 0.0 else s.size
        if cap is not None and cap < kept and s[cap] > 0.0 and s[cap - 1] / s[cap] < cap_ratio:
            bad.append((k, "cap", float(s[cap - 1] / s[cap])))
    return bad


# ------------------------------------------------------------------------------------------------ the operand sets of the GPU driver tests
TOLERANCE = 1e-9
# name -> (state site dims, state bonds, sites, (out, in) per operator site, operator bonds, cap below the exact bond)
CASES = {
    "full": ((2, 2, 2, 2), (1, 2, 4, 2, 1), (0, 1, 2, 3), ((2, 2),) * 4, (1, 2, 3, 2, 1), 3),
    "k1": ((2, 2, 2, 2), (1, 2, 4, 2, 1), (2,), ((2, 2),), (1, 1), 2),
    "inner": ((2, 2, 2, 2, 2), (1, 2, 4, 4, 2, 1), (1, 2, 3), ((2, 2),) * 3, (1, 2, 2, 1), 3),
    "interleaved": ((2,) * 8, (1, 2, 3, 4, 4, 4, 3, 2, 1), (0, 2, 4, 6), ((2, 2),) * 4, (1, 2, 2, 2, 1), 4),
    "mixed_dims": ((2, 3, 2, 3, 2), (1, 2, 4, 5, 2, 1), (0, 3), ((2, 2), (3, 3)), (1, 3, 1), 4),
    "s1_ne_s2": ((2, 2, 2, 2), (1, 2, 4, 2, 1), (1, 2), ((3, 2), (3, 2)), (1, 3, 1), 3),
}


def case_operands(name):
    """-> (operator site tensors, sites, state cores, cap)"""
    dims, bonds, sites, od, ob, cap = CASES[name]
    seed = SEED ^ (0x51 + 7 * sorted(CASES).index(name))
    x = [random_tensors([l, r], d, 1, seed + 11 * i)[0][:, :, 0, :] for i, (d, l, r) in enumerate(zip(dims, bonds[:-1], bonds[1:]))]
    op = [random_tensors([l, r], s1, s2, (seed ^ 0xABCD) + 13 * j)[0] for j, ((s1, s2), l, r) in enumerate(zip(od, ob[:-1], ob[1:]))]
    return op, sites, x, cap


def options_for(cap, sweeps=2):
    return Options(tolerance=TOLERANCE, max_bond_dim=cap, max_sweeps=sweeps, convergence_tol=0.0)


def initial_fit_case():
    """the fit of "interleaved" from a start of bond 2 with a stop test -> (op, sites, x, start, options)"""
    op, sites, x, cap = case_operands("interleaved")
    start = np_zipup(op, sites, x, options_for(2))
    return op, sites, x, start, Options(tolerance=TOLERANCE, max_bond_dim=cap, max_sweeps=6, convergence_tol=1e-3)


def record(fn):
    """run a restatement with every factorize recorded -> (result, GapLog)"""
    log = GapLog()
    with log.recording():
        out = fn()
    return out, log
