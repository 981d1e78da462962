"""numpy restatement of crates/tensor4all-partitionedtt/src/patching.rs, followed literally, with dense SVDs: TensorTrain::truncate
(canonicalise onto the last site, then the two-site Euler tour from it: every bond is truncated twice with the same rule),
svd_retained_rank for the eight policies, patch_stats / the volume budgets / the drop, truncate_adaptive, and add_with_patching with
both split strategies, and contract_adaptive over the products of tests/pmpo_np.py.  ONE DEVIATION is shared with the library (DESIGN.md
§8) and can therefore not show up as a disagreement: with an empty patch_order a leg of dimension 1 is no split candidate (it is the
absent s2 of a train).  A patch is a list of site tensors (l, s1, s2, r) (a train has s2 = 1), a projector a dict {(site, leg): value}.
Patches keep their insertion order (the reference iterates a hash map).  No device, no library."""
import functools

import numpy as np

import pmpo_np as PM

RELATIVE, ABSOLUTE = 0, 1
VALUE, SQUARED = 0, 1
PER_VALUE, TAIL_SUM = 0, 1
DEFAULT_POLICY = (1e-12, RELATIVE, VALUE, PER_VALUE)


def budget_policy(budget):
    return (budget, ABSOLUTE, SQUARED, TAIL_SUM)


def svd_retained_rank(s, policy):
    """compute_retained_rank (defaults/svd.rs:150-211) on non-increasing singular values"""
    thr, scale, measure, rule = policy
    s = np.asarray(s, dtype=np.float64)
    n = len(s)
    if n == 0:
        return 1
    m = s if measure == VALUE else s * s
    if not np.any(m != 0.0):
        return 1
    keep = 0
    if rule == PER_VALUE:
        if scale == RELATIVE:
            ref = float(m.max())
            while keep < n and ref > 0.0 and m[keep] / ref > thr:
                keep += 1
        else:
            while keep < n and m[keep] > thr:
                keep += 1
    else:
        total = 0.0
        for v in m:
            total += v
        if scale == RELATIVE and total == 0.0:
            return 1
        discarded, keep = 0.0, n
        for i in range(n - 1, -1, -1):
            t = discarded + m[i]
            ok = (t / total <= thr) if scale == RELATIVE else (t <= thr)
            if not ok:
                break
            discarded, keep = t, i
    return max(keep, 1)


def margin(s, policy):
    """how close the rule's decision is to flipping: the smallest relative distance |x / thr - 1| over the quantities it compares with
    the threshold (inf for a zero threshold or a zero matrix)"""
    thr, scale, measure, rule = policy
    s = np.asarray(s, dtype=np.float64)
    m = s if measure == VALUE else s * s
    if thr == 0.0 or not np.any(m != 0.0):
        return np.inf
    if rule == PER_VALUE:
        x = m / m.max() if scale == RELATIVE else m
    else:
        x = np.cumsum(m[::-1])
        x = x / m.sum() if scale == RELATIVE else x
    return float(np.min(np.abs(x / thr - 1.0)))


def fuse(t):
    t = np.asarray(t, dtype=np.float64)
    return t.reshape((t.shape[0], t.shape[1] * t.shape[2], t.shape[3]), order="F")


def unfuse(c, sd):
    return c.reshape((c.shape[0], sd[0], sd[1], c.shape[2]), order="F")


def dense(tensors):
    """the dense operator of shape (s1_1, s2_1, s1_2, s2_2, ...)"""
    acc = np.ones((1, 1))
    shape = []
    for t in tensors:
        l, s1, s2, r = t.shape
        acc = (acc @ t.reshape((l, s1 * s2 * r), order="F")).reshape((-1, r), order="F")
        shape += [s1, s2]
    return acc.reshape(shape, order="F")


def truncate_chain(tensors, policy=DEFAULT_POLICY, cap=None, log=None):
    """TensorTrain::truncate.  log (a list) receives per truncation (singular values, rank, margin)."""
    sds = [t.shape[1:3] for t in tensors]
    c = [fuse(t).copy() for t in tensors]
    n = len(c)
    for i in range(n - 1):  # canonicalise onto the last site
        l, s, r = c[i].shape
        q, rr = np.linalg.qr(c[i].reshape((l * s, r), order="F"))
        c[i] = q.reshape((l, s, q.shape[1]), order="F")
        c[i + 1] = np.einsum("ab,bsr->asr", rr, c[i + 1])

    def two_site(i, to_left):
        a, b = c[i], c[i + 1]
        theta = np.einsum("lsm,mtr->lstr", a, b).reshape((a.shape[0] * a.shape[1], b.shape[1] * b.shape[2]), order="F")
        u, s, vt = np.linalg.svd(theta, full_matrices=False)
        keep = svd_retained_rank(s, policy)
        if cap is not None:
            keep = min(keep, cap)
        keep = min(max(keep, 1), len(s))
        if log is not None:
            log.append((s.copy(), keep, margin(s, policy)))
        u, s, vt = u[:, :keep], s[:keep], vt[:keep]
        if to_left:
            u = u * s
        else:
            vt = s[:, None] * vt
        c[i] = u.reshape((a.shape[0], a.shape[1], keep), order="F")
        c[i + 1] = vt.reshape((keep, b.shape[1], b.shape[2]), order="F")

    for i in range(n - 2, -1, -1):
        two_site(i, True)
    for i in range(n - 1):
        two_site(i, False)
    return [unfuse(x, sd) for x, sd in zip(c, sds)]


def link_dims(tensors):
    return [t.shape[3] for t in tensors[:-1]]


def max_bond(tensors):
    return max([1] + link_dims(tensors))


def norm2(tensors):
    return float(np.sum(dense(tensors) ** 2))


def project(tensors, proj):
    """SubDomainTT::project: zeros outside the subdomain"""
    out = []
    for i, t in enumerate(tensors):
        t = np.array(t, dtype=np.float64)
        for leg in (0, 1):
            if (i, leg) in proj:
                keep = np.zeros(t.shape[1 + leg], dtype=bool)
                keep[proj[(i, leg)]] = True
                if leg == 0:
                    t[:, ~keep, :, :] = 0.0
                else:
                    t[:, :, ~keep, :] = 0.0
        out.append(t)
    return out


def volume(proj, site_dims):
    v = 1
    for i, sd in enumerate(site_dims):
        for leg in (0, 1):
            v *= 1 if (i, leg) in proj else sd[leg]
    return v


def budgets(volumes, norms2, rtol):
    """(budgets, drop), or None for the empty result"""
    total_volume = sum(volumes)
    if not volumes or total_volume == 0:
        return None
    total = 0.0
    for v in norms2:
        total += v
    g = rtol * rtol * total
    b = [g * (v / total_volume) for v in volumes]
    return b, [n2 <= x for n2, x in zip(norms2, b)]


def split_candidates(proj, site_dims, patch_order):
    raw = list(patch_order) if patch_order else [(i, leg) for i, sd in enumerate(site_dims) for leg in (0, 1) if sd[leg] != 1]
    out = []
    for leg in raw:
        if leg in proj or leg[0] >= len(site_dims) or leg in out:
            continue
        out.append(leg)
    return out


def _assign_and_truncate(work, site_dims, rtol, cap, log):
    """patch_stats, budgets, drop, truncate: [(proj, tensors, budget)] of the survivors"""
    masked = [project(t, p) for p, t, _ in work]
    vols = [volume(p, site_dims) for p, _, _ in work]
    n2 = [norm2(t) for t in masked]
    b = budgets(vols, n2, rtol)
    if b is None:
        return []
    out = []
    for (p, _, _), t, budget, drop in zip(work, masked, b[0], b[1]):
        if drop:
            continue
        out.append((p, truncate_chain(t, budget_policy(budget), cap, log), budget))
    return out


def truncate_adaptive(patches, projectors, site_dims, rtol, cap=None, log=None):
    """[(projector, tensors, budget_squared)] of the survivors, in order"""
    return _assign_and_truncate([(dict(p), t, None) for p, t in zip(projectors, patches)], site_dims, rtol, cap, log)


def parameter_count(tensors):
    return sum(int(np.prod(t.shape)) for t in tensors)


def split_child_parameter_count(proj, tensors, budget, leg, site_dims, cap, log=None):
    dim = site_dims[leg[0]][leg[1]]
    total = 0
    for v in range(dim):
        q = dict(proj)
        q[leg] = v
        child = project(tensors, q)
        if norm2(child) <= budget / dim:
            continue
        total += parameter_count(truncate_chain(child, budget_policy(budget / dim), cap, log))
    return total


SEQUENTIAL, EXACT_PARAMETER_GAIN = 0, 1


def add_with_patching(patches, projectors, site_dims, rtol=1e-12, cap=100, patch_order=(), strategy=EXACT_PARAMETER_GAIN, log=None,
                      chosen=None, counts=None):
    """the loop of patching.rs:154-198; chosen (a list) receives the leg of every split, counts (a list) the candidates' parameter
    counts of every ExactParameterGain decision"""
    work = [(dict(p), t, None) for p, t in zip(projectors, patches)]
    while True:
        work = _assign_and_truncate(work, site_dims, rtol, None, log)
        nxt, split_any = [], False
        for p, t, budget in work:
            if cap is not None and max_bond(t) > cap:
                cands = split_candidates(p, site_dims, patch_order)
                if cands:
                    if strategy == SEQUENTIAL:
                        leg = cands[0]
                    else:
                        cs = [split_child_parameter_count(p, t, budget, c, site_dims, cap, log) for c in cands]
                        if counts is not None:
                            counts.append(list(zip(cands, cs)))
                        leg = cands[int(np.argmin(cs))]  # the first of the smallest
                    if chosen is not None:
                        chosen.append(leg)
                    for v in range(site_dims[leg[0]][leg[1]]):
                        q = dict(p)
                        q[leg] = v
                        nxt.append((q, project(t, q), None))
                    split_any = True
                    continue
            nxt.append((p, t, budget))
        work = nxt
        if not split_any:
            return _assign_and_truncate(work, site_dims, rtol, cap, log)


def dense_sum(result, site_dims):
    shape = [d for sd in site_dims for d in sd]
    acc = np.zeros(shape)
    for _, t, _ in result:
        acc = acc + dense(t)
    return acc


# ---------------------------------------------------------------------------------------------- contract_adaptive (:282-412)
PROJECTION_POLICY = (64.0 * np.finfo(np.float64).eps, RELATIVE, VALUE, PER_VALUE)


def _pair_contract(pa, ta, pb, tb, tol, cap):
    """SubDomainTT::contract: (result projector, product) or None when the shared legs disagree"""
    if any(leg == 1 and pb.get((site, 0), v) != v for (site, leg), v in pa.items()):
        return None
    r = {k: v for k, v in pa.items() if k[1] == 0}
    r.update({k: v for k, v in pb.items() if k[1] == 1})
    c = [PM.site_product(u, v) for u, v in zip(PM.mask(ta, pa), PM.mask(tb, pb))]
    return r, PM.compress(c, tol, cap)


def _project_if_present(p, t, is_left, leg, value, log):
    if (leg[1] == 0) != is_left:
        return p, t
    if p.get(leg, value) != value:
        return None
    q = dict(p)
    q[leg] = value
    return q, truncate_chain(project(t, q), PROJECTION_POLICY, None, log)


def _contract_group(pairs, pre, rsd, tol, ccap, rtol, cap, patch_order, strategy, log, chosen):
    contributions = pre if pre is not None else [c for c in (_pair_contract(pa, ta, pb, tb, tol, ccap) for (pa, ta), (pb, tb) in pairs)
                                                   if c is not None]
    if not contributions:
        return []
    proj, total = contributions[0]
    for _, c in contributions[1:]:
        total = PM.add_truncate(total, c, PM.truncates(tol, ccap), tol, ccap)
    if cap is None:
        return [(proj, total, None)]
    if not (max_bond(total) >= cap or any(max_bond(c) >= cap for _, c in contributions)):
        return [(proj, total, None)]
    total = project(total, proj)
    budget = budgets([volume(proj, rsd)], [norm2(total)], rtol)[0][0]
    cands = split_candidates(proj, rsd, patch_order)
    if not cands:
        return [(proj, total, budget)]
    if strategy == SEQUENTIAL:
        leg = cands[0]
    else:
        leg = cands[int(np.argmin([split_child_parameter_count(proj, total, budget, c, rsd, cap, log) for c in cands]))]
    if chosen is not None:
        chosen.append(leg)
    out = []
    for value in range(rsd[leg[0]][leg[1]]):
        left, right, child = {}, {}, []
        for (pa, ta), (pb, tb) in pairs:
            ka, kb = tuple(sorted(pa.items())), tuple(sorted(pb.items()))
            if ka not in left:
                left[ka] = _project_if_present(pa, ta, True, leg, value, log)
            if kb not in right:
                right[kb] = _project_if_present(pb, tb, False, leg, value, log)
            if left[ka] is not None and right[kb] is not None:
                child.append((left[ka], right[kb]))
        out += _contract_group(child, None, rsd, tol, ccap, rtol, cap, patch_order, strategy, log, chosen)
    return out


def contract_adaptive(pa, ta, pb, tb, sda, sdb, tol=1e-12, ccap=None, rtol=1e-12, cap=100, patch_order=(), strategy=EXACT_PARAMETER_GAIN,
                      log=None, chosen=None):
    """[(projector, tensors, budget_squared)]; tol / ccap are the contraction's rank rule, rtol / cap / patch_order / strategy the patching
    options (legs of the result: (i, 0) is A's s1 leg, (i, 1) B's s2 leg)"""
    rsd = [(a[0], b[1]) for a, b in zip(sda, sdb)]
    key = functools.cmp_to_key(lambda x, y: PM.compare(x[0], y[0]))
    left, right = sorted(zip(pa, ta), key=key), sorted(zip(pb, tb), key=key)
    groups = []
    for p, t in left:
        for q, u in right:
            c = _pair_contract(p, t, q, u, tol, ccap)
            if c is None:
                continue
            for g in groups:
                if g[0] == c[0]:
                    break
            else:
                g = (c[0], [], [])
                groups.append(g)
            g[1].append(((p, t), (q, u)))
            g[2].append(c)
    groups.sort(key=key)
    subs = []
    for _, pairs, contributions in groups:
        subs += _contract_group(pairs, contributions, rsd, tol, ccap, rtol, cap, patch_order, strategy, log, chosen)
    return _assign_and_truncate(subs, rsd, rtol, cap, log)
