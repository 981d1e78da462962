"""numpy restatement of fuse_to, split_to and restructure_to on a chain (tensor4all-treetn, treetn/transform.rs and
treetn/restructure/mod.rs) by position: the plan (kinds and precedence of build_plan, absorption of sites without legs, the
swap-then-fuse assignment, the messages), fuse by einsum in the project's association (left to right inside a group, the legs of
the result in the target's order), split by np.linalg.qr (fragment-major legs, fragments peeled from the left, the rank rule of
qr_retained_rank at rtol 0).  Also the shared cases of tests/test_cpu_restructure.py and tests/test_gpu_restructure.py.

A leg train is (cores, legs) as in tests/swap_np.py; a target is a list of groups of keys, group j = site j of the result, first key
fastest.  Refusals are ValueError (NotImplementedError for the planner's placeholder) with the library's text.
"""
import numpy as np

import swap_np as sn

EPS = sn.EPS
KINDS = ("FuseOnly", "SwapThenFuse", "SplitOnly", "SwapOnly", "SplitThenFuse")
PLACEHOLDER = "restructure_to: planner placeholder only; split/move/mixed restructure planning is not implemented yet"
FUSE_MAX_LEGS = 16
DIM_MAX = 65535
INT_MAX = 2 ** 31 - 1

# The dense tolerance of the device's split_to is C_SPLIT * n_qr * eps * |T|_F.  The restatement itself (numpy's Householder QR)
# deviates from the exact tensor by at most SPLIT_RESTATEMENT_DEVIATION of these units over split_cases() with seeds 0 .. 19
# (tests/test_cpu_restructure.py asserts it); another Householder QR rounds differently, which is given the margin of 8 that swap's
# C_DENSE uses: C_SPLIT = 8 * SPLIT_RESTATEMENT_DEVIATION.  The same scale bounds the left-orthogonality of a peeled fragment Q with k
# columns, one QR each: |Q^T Q - 1|_F <= C_SPLIT * eps * |Q|_F = C_SPLIT * eps * sqrt(k) (the restatement's own largest value over the
# same cases and seeds is 3.34 of these units).  Neither number was taken from the device's output.
SPLIT_RESTATEMENT_DEVIATION = 2.14
C_SPLIT = 8.0 * SPLIT_RESTATEMENT_DEVIATION


# ------------------------------------------------------------------------------------------------ plan
def check_target(op, legs, target):
    """(site_of, group_of, dim): the refusals every entry point shares"""
    site_of, group_of, dim = {}, {}, {}
    for i, site in enumerate(legs):
        for k, d in site:
            if k in site_of:
                raise ValueError(f"{op}: site index {k!r} appears in both current nodes {site_of[k]} and {i}")
            site_of[k], dim[k] = i, d
    for j, g in enumerate(target):
        if not g:
            raise ValueError(f"{op}: target node {j} has no site indices")
        for k in g:
            if k in group_of:
                raise ValueError(f"{op}: site index {k!r} appears in both target nodes {group_of[k]} and {j}")
            group_of[k] = j
    for k, j in group_of.items():
        if k not in site_of:
            if op == "fuse_to":
                raise ValueError(f"fuse_to: incompatible target structure: target node {j} has site indices not found in the current train")
            if op == "split_to":
                raise ValueError(f"split_to: target site index {k!r} is missing from the current network")
            raise ValueError(f"{op}: current and target must contain the same site indices")
    for k, i in site_of.items():
        if k not in group_of:
            if op == "fuse_to":
                raise ValueError(f"fuse_to: missing target for current node {i}: it has site indices but no corresponding target node")
            if op == "split_to":
                raise ValueError(f"split_to: incompatible target structure: site index {k!r} in current node {i} has no corresponding target node")
            raise ValueError(f"{op}: current and target must contain the same site indices")
    return site_of, group_of, dim


def groups_of_site(site, group_of):
    return sorted({group_of[k] for k, _ in site})


def fuse_assign(legs, target, group_of):
    """fuse_to steps 2 - 4b and the connectivity of contract_node_group on a chain: the group of every site"""
    n = len(legs)
    group = [None] * n
    for i, site in enumerate(legs):
        gs = groups_of_site(site, group_of)
        if len(gs) > 1:
            raise ValueError(f"fuse_to: ambiguous mapping: current node {i} maps to multiple target nodes: {gs[0]} and {gs[1]}")
        if gs:
            group[i] = gs[0]
    for g in range(len(target)):  # step 4: between two members of a group
        members = [i for i in range(n) if group[i] == g]
        for i in range(members[0], members[-1] + 1):
            if not legs[i] and group[i] is None:
                group[i] = g
    while True:  # step 4b, to a fixed point
        additions = []
        for i in range(n):
            if group[i] is not None or legs[i]:
                continue
            near = {group[j] for j in (i - 1, i + 1) if 0 <= j < n and group[j] is not None}
            if len(near) == 1:
                additions.append((i, near.pop()))
            elif len(near) == 2 and max(near) - min(near) == 1:  # neighbours in the target: the smaller index
                additions.append((i, min(near)))
        if not additions:
            break
        for i, g in additions:
            group[i] = g
    for i in range(n):
        if group[i] is None:
            raise ValueError(f"fuse_to: current node {i} has no site indices and lies between target nodes that are no neighbours: it cannot be absorbed")
    for g in range(len(target)):
        members = [i for i in range(n) if group[i] == g]
        if members != list(range(members[0], members[-1] + 1)):
            raise ValueError(f"fuse_to: failed to contract nodes for target {g}: Nodes to contract do not form a connected subtree")
    for i in range(n - 1):
        if group[i + 1] < group[i]:
            raise ValueError("fuse_to: the groups of the target are contiguous on the chain but not in chain order (target node "
                             f"{group[i]} lies left of target node {group[i + 1]}); restructure_to can move them")
    return group


def fuse_plan(legs, target, link_dims=None):
    """{"members", "legs", "rounds", "launches"} with the plan-time refusals"""
    _, group_of, dim = check_target("fuse_to", legs, target)
    group = fuse_assign(legs, target, group_of)
    members = [[i for i in range(len(legs)) if group[i] == g] for g in range(len(target))]
    reorder = 0
    for g, keys in enumerate(target):
        if len(keys) > FUSE_MAX_LEGS:
            raise ValueError(f"fuse_to: target node {g} holds {len(keys)} legs; a fused site holds at most {FUSE_MAX_LEGS}")
        if int(np.prod([dim[k] for k in keys], dtype=object)) > DIM_MAX:
            raise ValueError(f"fuse_to: target node {g} would hold a fused site dimension above 65535")
        if link_dims is not None:
            bonds = [1] + list(link_dims) + [1]
            x = 1
            for s in members[g]:
                x *= int(np.prod([d for _, d in legs[s]], dtype=object))
                if bonds[members[g][0]] * x * bonds[s + 1] > INT_MAX:
                    raise ValueError(f"fuse_to: target node {g}: the result core would hold more than INT_MAX elements")
        if len(members[g]) == 1 and [k for k, _ in legs[members[g][0]]] != list(keys):
            reorder = 1
    rounds = max(len(m) for m in members) - 1
    return {"members": members, "legs": [[(k, dim[k]) for k in g] for g in target], "rounds": rounds, "launches": rounds + reorder}


def split_assign(legs, target, site_of, keep_legless=False):
    site = []
    for j, g in enumerate(target):
        sites = {site_of[k] for k in g}
        if len(sites) != 1:
            raise ValueError(f"split_to: target node {j} spans multiple current nodes; use restructure_to for mixed regrouping")
        site.append(sites.pop())
    if not keep_legless:
        for i, s in enumerate(legs):
            if not s:
                raise ValueError(f"split_to: current node {i} has no site indices and so has no corresponding target node; fuse_to absorbs such nodes")
    for j in range(len(target) - 1):
        if site[j + 1] < site[j]:
            raise ValueError(f"split_to: the target is not in chain order (target node {j} lies on current node {site[j]}, target node "
                             f"{j + 1} on current node {site[j + 1]}); use restructure_to for mixed regrouping")
    return site


def split_plan(legs, target, keep_legless=False):
    """{"groups": per site its target groups, "legs", "n_qr", "launches"}"""
    site_of, _, dim = check_target("split_to", legs, target)
    site = split_assign(legs, target, site_of, keep_legless)
    groups = [[j for j in range(len(target)) if site[j] == i] for i in range(len(legs))]
    out, n_qr, launches = [], 0, 0
    for i, gs in enumerate(groups):
        if not gs:
            out.append([])
            continue
        out += [[(k, dim[k]) for k in target[j]] for j in gs]
        n_qr += len(gs) - 1
        if [k for j in gs for k in target[j]] != [k for k, _ in legs[i]]:
            launches = 1
    return {"groups": groups, "legs": out, "n_qr": n_qr, "launches": launches}


def swap_then_fuse_assignment(legs, target, group_of):
    """build_path_swap_then_fuse_assignment by position: {key: site} or None"""
    contributors = [0] * len(target)
    for site in legs:
        gs = groups_of_site(site, group_of)
        if len(gs) != 1:
            return None
        contributors[gs[0]] += 1
    out, cursor = {}, 0
    for j, g in enumerate(target):
        n = contributors[j]
        if n == 0 or cursor + n > len(legs) or len(g) < n:
            return None
        for pos, k in enumerate(sorted(g)):
            out[k] = cursor + min(pos, n - 1)
        cursor += n
    return out if cursor == len(legs) else None


def legs_after_swap(legs, assignment):
    """sites a step touches end in ascending key order, the others keep theirs"""
    dim = {k: d for site in legs for k, d in site}
    steps = sn.schedule(len(legs), {k: i for i, site in enumerate(legs) for k, _ in site}, dict(assignment), 0)
    touched = {s[1] for s in steps} | {s[2] for s in steps}
    return [[(k, dim[k]) for k in sorted(k for k, v in assignment.items() if v == i)] if i in touched else list(legs[i])
            for i in range(len(legs))]


def plan(legs, target, link_dims=None):
    """restructure_plan: {"kind", "legs", "fuse_rounds", "fuse_launches", "n_qr", "swap_target", "split_target"}"""
    site_of, group_of, dim = check_target("restructure_to", legs, target)
    p = {"kind": None, "legs": None, "fuse_rounds": 0, "fuse_launches": 0, "n_qr": 0, "swap_target": {}, "split_target": None}

    def take_fuse(before, links):
        fp = fuse_plan(before, target, links)
        p.update(legs=fp["legs"], fuse_rounds=fp["rounds"], fuse_launches=fp["launches"])
        return p

    unique = all(len(groups_of_site(s, group_of)) <= 1 for s in legs)
    if unique:
        try:
            fuse_assign(legs, target, group_of)
            ok = True
        except ValueError:
            ok = False
        if ok:
            p["kind"] = "FuseOnly"
            return take_fuse(legs, link_dims)
        a = swap_then_fuse_assignment(legs, target, group_of)
        if a is not None:
            p["kind"], p["swap_target"] = "SwapThenFuse", a
            return take_fuse(legs_after_swap(legs, a), None)
    try:
        split_assign(legs, target, site_of)
        ok = True
    except ValueError:
        ok = False
    if ok:
        sp = split_plan(legs, target)
        p.update(kind="SplitOnly", legs=sp["legs"], n_qr=sp["n_qr"])
        return p
    if len(target) == len(legs):
        p["kind"], p["swap_target"] = "SwapOnly", {k: j for j, g in enumerate(target) for k in g}
        return take_fuse(legs_after_swap(legs, p["swap_target"]), None)
    order = [g for site in legs for g in groups_of_site(site, group_of)]
    if all(a <= b for a, b in zip(order[:-1], order[1:])):
        p["kind"] = "SplitThenFuse"
        p["split_target"] = [[k for k in target[g] if site_of[k] == i] for i, site in enumerate(legs) for g in groups_of_site(site, group_of)]
        sp = split_plan(legs, p["split_target"], keep_legless=True)
        p["n_qr"] = sp["n_qr"]
        return take_fuse(sp["legs"], None)
    raise NotImplementedError(PLACEHOLDER)


# ------------------------------------------------------------------------------------------------ drivers
def reorder(core, site, order):
    """the legs of a core (l, s, r) in another order"""
    l, _, r = core.shape
    keys = [k for k, _ in site]
    t = core.reshape([l] + [d for _, d in site] + [r], order="F")
    t = np.transpose(t, [0] + [1 + keys.index(k) for k in order] + [len(site) + 1])
    return np.ascontiguousarray(t).reshape(core.shape, order="F"), [site[keys.index(k)] for k in order]


def fuse(cores, legs, target):
    """fuse_to: left to right inside a group, the legs of the result in the target's order.  Works on any dtype (int64: exact)."""
    fp = fuse_plan(legs, target, [c.shape[2] for c in cores[:-1]])
    out = []
    for g, members in enumerate(fp["members"]):
        acc, chain = cores[members[0]], list(legs[members[0]])
        for s in members[1:]:
            acc = np.einsum("lxm,myr->lxyr", acc, cores[s]).reshape(acc.shape[0], -1, cores[s].shape[2], order="F")
            chain += legs[s]
        acc, _ = reorder(acc, chain, list(target[g]))
        out.append(acc)
    return out, fp["legs"]


def split(cores, legs, target, keep_legless=False):
    """split_to, phase 1.  Returns (cores, legs, info); info["fragments"]: the indices of the result sites that are a Q,
    info["qr_shapes"]: (rows, cols, retained rank) of every QR."""
    sp = split_plan(legs, target, keep_legless)
    out, info = [], {"n_qr": 0, "fragments": [], "qr_shapes": []}
    for i, gs in enumerate(sp["groups"]):
        rem = np.array(cores[i], dtype=np.float64)
        if gs:
            rem, _ = reorder(rem, legs[i], [k for j in gs for k in target[j]])
        for j in gs[:-1]:
            f = int(np.prod([d for _, d in sp["legs"][len(out)]], dtype=np.int64))
            l, s, r = rem.shape
            q, rr = np.linalg.qr(rem.reshape(l * f, (s // f) * r, order="F"))
            k = q.shape[1]
            if not np.any(rr):
                k = 1  # qr_retained_rank: at least one
            info["fragments"].append(len(out))
            info["qr_shapes"].append((l * f, (s // f) * r, k))
            out.append(q[:, :k].reshape(l, f, k, order="F"))
            rem = rr[:k].reshape(k, s // f, r, order="F")
            info["n_qr"] += 1
        out.append(rem)
    return out, sp["legs"], info


def restructure(cores, legs, target):
    """restructure_to without truncation.  Returns (cores, legs, info) with info = {"kind", "n_steps", "n_qr"}."""
    p = plan(legs, target, [c.shape[2] for c in cores[:-1]])
    info = {"kind": p["kind"], "n_steps": 0, "n_qr": 0}
    if p["kind"] == "FuseOnly":
        cores, legs = fuse(cores, legs, target)
    elif p["kind"] == "SplitOnly":
        cores, legs, si = split(cores, legs, target)
        info["n_qr"] = si["n_qr"]
    elif p["kind"] in ("SwapOnly", "SwapThenFuse"):
        cores, legs, _, si = sn.swap(cores, legs, p["swap_target"])
        info["n_steps"] = si["n_steps"]
        cores, legs = fuse(cores, legs, target)
    else:
        cores, legs, si = split(cores, legs, p["split_target"], keep_legless=True)
        info["n_qr"] = si["n_qr"]
        cores, legs = fuse(cores, legs, target)
    return cores, legs, info


# ------------------------------------------------------------------------------------------------ shared cases
def int_train(rng, legs, bonds):
    """cores with integer entries in -2 .. 2 (as float64): every product and sum of a fuse is exact"""
    b = [1] + list(bonds) + [1]
    return [rng.integers(-2, 3, size=(b[i], int(np.prod([d for _, d in site], dtype=np.int64)), b[i + 1])).astype(np.float64)
            for i, site in enumerate(legs)]


def split_cases():
    """name -> (legs, bonds, target): split_to on generic inputs, at most 8 sites in the result, bonds <= 40"""
    c = {}
    c["fused_quantics_3x2"] = ([[((2 * b, 0), 2), ((2 * b + 1, 0), 2)] for b in range(3)], [4, 4],
                               [[(i, 0)] for i in range(6)])
    c["mpo_sites"] = (sn.mpo_legs([(2, 3), (3, 2), (2, 2)]), [7, 5], [[(0, 0)], [(0, 1)], [(1, 0), (1, 1)], [(2, 1)], [(2, 0)]])
    c["three_fragments_reordered"] = ([[("a", 2), ("b", 3), ("c", 2), ("d", 3)], [("e", 3), ("f", 2)]], [40],
                                      [["c"], ["a", "d"], ["b"], ["f", "e"]])
    c["wide_bonds"] = ([[("a", 2), ("b", 2)], [("c", 3), ("d", 2), ("e", 2)], [("f", 2)]], [33, 17], [["a"], ["b"], ["d"], ["c", "e"], ["f"]])
    return c


def restructure_cases():
    """name -> (legs, bonds, target, kind): one case per kind, plus the widened SplitThenFuse (2-bit sites into 3-bit sites)"""
    t = sn.train_legs
    c = {}
    c["fuse_only"] = (t([2, 3, 2, 2, 3, 2]), [2, 6, 9, 6, 3], [[(0, 0), (1, 0)], [(3, 0), (2, 0)], [(4, 0)], [(5, 0)]], "FuseOnly")
    c["swap_then_fuse"] = (t([2, 2, 2, 2, 2, 2]), [2, 4, 7, 4, 2], [[(0, 0), (2, 0), (4, 0)], [(1, 0), (3, 0), (5, 0)]], "SwapThenFuse")
    c["split_only"] = (sn.mpo_legs([(2, 3), (3, 2), (2, 2)]), [6, 4], [[(0, 0)], [(0, 1)], [(1, 1), (1, 0)], [(2, 0)], [(2, 1)]], "SplitOnly")
    c["swap_only"] = (sn.mpo_legs([(2, 3), (3, 2), (2, 2)]), [6, 4], [[(0, 0), (1, 0)], [(1, 1), (2, 1)], [(0, 1), (2, 0)]], "SwapOnly")
    c["split_then_fuse"] = (sn.mpo_legs([(2, 3), (3, 2), (2, 2)]), [6, 4], [[(0, 0)], [(0, 1), (1, 0)], [(1, 1)], [(2, 1), (2, 0)]],
                            "SplitThenFuse")
    bits2 = [[((2 * s, 0), 2), ((2 * s + 1, 0), 2)] for s in range(3)]
    c["bits_2_to_3"] = (bits2, [4, 4], [[(0, 0), (1, 0), (2, 0)], [(3, 0), (4, 0), (5, 0)]], "SplitThenFuse")
    return c
