"""numpy restatement of one-site TDVP (t4a_gpu_tdvp_one_site): the one-site region plan of tensor4all-treetn's tdvp (tdvp/plan.rs:97-111,
first_order_sweep with nsite = 1) on a chain rooted at any site, the sweeps of tdvp/mod.rs:639-914 (update_one_site_tensor,
apply_one_site_bond_correction, evolve_edge_center) and the bond-centre operator, on the pieces of tests/tdvp_np.py (the Krylov
exponential, the environments, the full-rank centre move).  It follows the reference literally: after a bond correction the site
holds Q C' and the next centre move factorises it again, where the device leaves Q and absorbs C' into the neighbour (the same state,
another gauge on that bond).  Local exponentials are exact (eigh of the dense projected operator) or by the restated Krylov solver.

One rule is the project's, not the reference's: in a reversed substep the bond correction at the jump between the two arms of an inner
centre goes to the LAST edge of the path to the next node (the centre is moved to the neighbour of that node first), where the
reference corrects the first edge.  literal_jump=True restates the reference there; it is not a projector splitting (percents away from
the dense exponential at full bonds, tests/test_cpu_tdvp_one_site.py) and the device does not run it.  Paths of one edge are untouched."""
import numpy as np

from fit_np import SEED
from linsolve_np import np_canonicalize, np_left_env, np_right_env, np_operator_full, np_state_full  # noqa: F401
from dmrg_np import tfim, symmetric_integer_operator, random_state  # noqa: F401
from tdvp_np import (Options, KrylovOptions, applyexp_sub_steps, np_krylov_expm, np_one_site_apply, _left, _right, _move_center,  # noqa: F401
                     relative_distance, spread_tolerance, perturbed, full_bonds)

ONE = 2  # the kind of a one-site plan step, as t4a_gpu_tdvp_one_site_plan reports it


# ------------------------------------------------------------------------------------------------ the plan
def post_order(n, center):
    """the nodes in post order from `center`: the left arm leaf first, then the right arm leaf first, then the centre"""
    return list(range(0, center)) + list(range(n - 1, center, -1)) + [center]


def one_site_plan(n, center, order, tau):
    """-> [(ONE, (node,), node, exponent)]: every substep carries tau * weight, every even substep (1-based) is the reversed list"""
    if n < 1 or not 0 <= center < n:
        raise ValueError("center is not a state node")
    nodes = post_order(n, center)
    steps = []
    for k, weight in enumerate(applyexp_sub_steps(order)):
        part = nodes if (k + 1) % 2 else nodes[::-1]
        steps.extend((ONE, (c,), c, tau * weight) for c in part)
    return steps


# ------------------------------------------------------------------------------------------------ the bond-centre operator
def np_bond_apply(la, rb, c):
    """Y[b, b'] = sum_w sum_a sum_a' La[b, w, a] C[a, a'] Rb[b', w, a']"""
    return np.einsum("bwa,ac,dwc->bd", la, c, rb)


def np_bond_apply_int(la, rb, c):
    """the same in int64 arithmetic, for operands with integer values"""
    return np.einsum("bwa,ac,dwc->bd", la.astype(np.int64), c.astype(np.int64), rb.astype(np.int64))


def factorize_towards(x, toward_right):
    """the full-rank thin QR of a centre move -> (Q as a site tensor, C): x = Q C (to the right) or C Q (to the left)"""
    l, s, r = x.shape
    if toward_right:
        q, c = np.linalg.qr(x.reshape((l * s, r), order="F"))
        return q.reshape((l, s, q.shape[1]), order="F"), c
    q, c = np.linalg.qr(x.reshape((l, s * r), order="F").T)
    return q.T.reshape((q.shape[1], s, r), order="F"), c.T


# ------------------------------------------------------------------------------------------------ the sweeps
def np_tdvp_one_site(ops, init, center=0, options=None, exact_local=False, literal_jump=False):
    """-> dict(state, sweeps_completed, local_updates, max_error_estimate, max_krylov_iterations, one_site_steps, bond_corrections,
    krylov_steps, max_time_splits)"""
    o = Options() if options is None else options
    n = len(ops)
    if o.nsweeps == 0:
        raise ValueError("invalid TDVP option nsweeps: must be greater than zero")
    if o.max_bond_dim is not None:
        raise ValueError("invalid TDVP option max_bond_dim: one-site TDVP has fixed ranks; use nsite=2 for truncation")
    plan = one_site_plan(n, center, o.order, o.exponent_step)
    x = np_canonicalize(init, center)
    cur = center
    out = {"local_updates": 0, "max_error_estimate": 0.0, "max_krylov_iterations": 0, "one_site_steps": 0, "bond_corrections": 0, "krylov_steps": 0,
           "max_time_splits": 1}

    def evolve(apply, v, exponent):
        if exact_local:
            h = np.stack([apply(e) for e in np.eye(v.size)], axis=1)
            lams, q = np.linalg.eigh(0.5 * (h + h.T))
            res = (q @ (np.exp(exponent * lams) * (q.T @ v)), 0, 0.0, True, 1)
        else:
            res = np_krylov_expm(apply, exponent, v, o.krylov, o.cgs2)
        out["local_updates"] += 1
        out["krylov_steps"] += res[1]
        out["max_error_estimate"] = max(out["max_error_estimate"], res[2])
        out["max_krylov_iterations"] = max(out["max_krylov_iterations"], res[1])
        out["max_time_splits"] = max(out["max_time_splits"], res[4])
        return res[0]

    sweeps = 0
    for sweep in range(o.nsweeps):
        for k, (_, nodes, new_center, exponent) in enumerate(plan):
            c = nodes[0]
            cur = _move_center(x, cur, c)
            left, right = _left(ops, x, c), _right(ops, x, c + 1)
            shape = x[c].shape

            def apply1(v):
                return np_one_site_apply(left, right, ops[c], v.reshape(shape, order="F")).reshape(-1, order="F")
            x[c] = evolve(apply1, x[c].reshape(-1, order="F"), exponent).reshape(shape, order="F")
            out["one_site_steps"] += 1
            if k + 1 < len(plan) and plan[k + 1][1] != nodes:  # the bond correction towards the next node
                t = plan[k + 1][1][0]
                toward_right = t > c
                if (k // n) % 2 == 1 and not literal_jump:  # a reversed substep: the correction on the LAST edge of the path
                    c = cur = _move_center(x, c, t - 1 if toward_right else t + 1)
                    left, right = _left(ops, x, c), _right(ops, x, c + 1)
                q, cm = factorize_towards(x[c], toward_right)
                la = np_left_env(left, ops[c], q) if toward_right else left
                rb = right if toward_right else np_right_env(right, ops[c], q)
                cs = cm.shape

                def apply0(v):
                    return np_bond_apply(la, rb, v.reshape(cs, order="F")).reshape(-1, order="F")
                cm = evolve(apply0, cm.reshape(-1, order="F"), -exponent).reshape(cs, order="F")
                x[c] = np.einsum("lsk,kr->lsr", q, cm) if toward_right else np.einsum("lk,ksr->lsr", cm, q)
                out["bond_corrections"] += 1
            cur = c
        sweeps = sweep + 1
    out["state"] = x
    out["sweeps_completed"] = sweeps
    return out


# ------------------------------------------------------------------------------------------------ the cases the CPU and the device tests share
TAU = -0.05
_CACHE = {}


def bonds_case(dims, bonds, which="sym"):
    """-> (operator sites, random start with the given bonds): a symmetric integer MPO of bond 3 or the Ising chain at g = 0.7"""
    n = len(dims)
    ops = symmetric_integer_operator(dims, 3, SEED ^ 0x151 ^ n) if which == "sym" else tfim(n, 0.7)
    return ops, random_state(dims, list(bonds), SEED ^ 0x1510 ^ n ^ (sum(bonds) << 4))


def case_tau(ops):
    """The step of the dense comparisons: tau = -1 / (2 ||H||_2).  A one-site sweep evolves forwards (sites) and backwards (bonds) in
    turn; each of the 2n - 1 local exponentials amplifies the rounding errors before it by up to exp(|tau| ||H||), so the error of a sweep
    is eps exp(O(n |tau| ||H||)).  The symmetric integer operators have ||H||_2 of several hundred: at tau = -0.05 that factor exceeds 1e13,
    at |tau| ||H|| = 1/2 it is below 1e2 and the comparison measures the splitting, not the conditioning of the test input."""
    return -0.5 / float(np.linalg.norm(np_operator_full(ops), 2))


def dense_exponential(ops, init, tau):
    h = np_operator_full(ops)
    lams, q = np.linalg.eigh(0.5 * (h + h.T))
    return q @ (np.exp(tau * lams) * (q.T @ np_state_full(init)))


THIN = {"dims": (2,) * 5, "bonds": (1, 2, 3, 3, 2, 1), "nsweeps": 2, "order": 2, "center": 2}


def thin_case():
    return bonds_case(THIN["dims"], THIN["bonds"], "tfim")


def thin_restated(cgs2=True):
    key = ("thin", cgs2)
    if key not in _CACHE:
        ops, init = thin_case()
        _CACHE[key] = np_tdvp_one_site(ops, init, THIN["center"], Options(nsweeps=THIN["nsweeps"], order=THIN["order"], exponent_step=TAU, cgs2=cgs2))
    return _CACHE[key]
