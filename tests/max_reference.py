"""numpy restatement of `jtp_max_marginals` (`engine.Plan.max_marginals`): max-propagation as include/jtprop.h defines it, operation
by operation.

Same schedule (describe()["sample"], read as `sample_reference.schedule` reads it), same multiplication order - the clique's entry
widened to float64, then the parent's downward message, then the children's upward messages in ascending ABI clique number, left to
right -, the same power-of-two scaling of every message (`np.frexp` for the exponent of its largest entry, `np.ldexp` to take it
out: both exact) and the same integer bookkeeping of the exponents.  A maximum is exact whatever the order, so every number is
made of single IEEE operations on float64 in a fixed order: the device must agree bit for bit, tables and exponents."""
import numpy as np

from sample_reference import schedule


def _onto(table, its_vars, names, card):
    """`table` over `its_vars` (a subset of `names`, any order) shaped to broadcast against an array whose axes are `names`"""
    its_vars = list(its_vars)
    order = sorted(range(len(its_vars)), key=lambda i: names.index(its_vars[i]))
    t = np.transpose(np.asarray(table).reshape([card[v] for v in its_vars]), order)
    return t.reshape([card[v] if v in its_vars else 1 for v in names])


def _max_onto(w, looked, names, keep, card):
    """the largest looked-at entry of `w` (axes `names`) per assignment of `keep`, in the axis order of `keep`; 0 where there is none"""
    w = np.where(looked & ~np.isnan(w), w, -1.0)               # (-1: not looked at, never the maximum where an entry counts)
    drop = tuple(i for i, v in enumerate(names) if v not in keep)
    best = w.max(axis=drop) if drop else w
    left = [v for v in names if v in keep]
    best = np.transpose(best, [left.index(v) for v in keep])
    return np.abs(np.where(best >= 0, best, 0.0)).reshape([card[v] for v in keep])


def _exponent(table):
    """(ilogb of the largest entry, whether it is one a set fails on)"""
    top = table.max() if table.size else 0.0
    if not (top > 0 and np.isfinite(top)):
        return 0, True
    return int(np.frexp(top)[1]) - 1, False


def max_reference(plan, pots, requests, evidence=None):
    """`plan`: any plan of the tree (a `plan_only` one will do: only its schedule and labels are read); `pots[c]`: the table of clique
    c (caller's index) in the clique's axis order, in the numbers the device holds (float32 tables: float32 values, widened here);
    `requests`: [(clique, labels)]; `evidence`: {label: state}.
    Returns (tables, log2_scale, log_value): `tables[i]` float64 of the request's shape, the true max-marginal times
    2**-log2_scale[i]; a set that fails: tables of zeros, exponents 0, -inf."""
    evidence = dict(evidence or {})
    sched = schedule(plan)
    axes = plan.node_vars
    card = {lab: plan.node_shape[c][i] for c in plan.cliques for i, lab in enumerate(axes[c])}
    children = {c: [] for c, *_ in sched}
    parent_of = {}
    for c, parent, *_ in sched:
        parent_of[c] = parent
        if parent != -1:
            children[parent].append(c)
    for c in children:
        children[c].sort(key=lambda d: plan.abi_of[d])
    K_of = {c: list(K) for c, _, _, K, F, _ in sched}
    psi, looked = {}, {}
    failed = False
    for c, *_ in sched:
        names = list(axes[c])
        psi[c] = np.asarray(pots[c]).reshape(plan.node_shape[c]).astype(np.float64)
        seen = np.ones(psi[c].shape, dtype=bool)
        for i, v in enumerate(names):
            if v in evidence:
                sel = np.zeros(card[v], dtype=bool)
                sel[evidence[v]] = True
                seen = seen & sel.reshape([card[v] if j == i else 1 for j in range(len(names))])
        looked[c] = seen
        if np.any(seen & ~(psi[c] >= 0)):                                  # a negative or NaN entry that counts
            failed = True

    def times(w, c, table, exponent, its_vars):
        return w * _onto(np.ldexp(table, -exponent), its_vars, list(axes[c]), card)

    # upward, deepest first: jtp_map's pass
    raw, e = {}, {}
    for c, *_ in reversed(sched):
        w = psi[c].copy()
        for d in children[c]:
            w = times(w, c, raw[d], e[d], K_of[d])
        raw[c] = _max_onto(w, looked[c], list(axes[c]), K_of[c], card)
        e[c], bad = _exponent(raw[c])
        failed = failed or bad
    # downward, shallowest first
    rawdn, f = {}, {}
    for c, *_ in sched:
        for d in children[c]:
            w = psi[c].copy()
            if parent_of[c] != -1:
                w = times(w, c, rawdn[c], f[c], K_of[c])
            for x in children[c]:
                if x != d:
                    w = times(w, c, raw[x], e[x], K_of[x])
            rawdn[d] = _max_onto(w, looked[c], list(axes[c]), K_of[d], card)
            f[d], bad = _exponent(rawdn[d])
            failed = failed or bad
    shapes = [tuple(card[v] for v in labels) for _, labels in requests]
    if failed:
        return [np.zeros(s) for s in shapes], [0] * len(requests), -np.inf
    # the exponents: integers
    U, V, S = {}, {}, {}
    for c, *_ in reversed(sched):
        U[c] = e[c] + sum(U[x] for x in children[c])
    for c, *_ in sched:
        if parent_of[c] == -1:
            V[c] = 0
        else:
            p = parent_of[c]
            V[c] = V[p] + sum(U[s] for s in children[p] if s != c) + f[c]
    for c, *_ in sched:
        S[c] = V[c] + sum(U[d] for d in children[c])
    tables, scales = [], []
    for c, labels in requests:
        w = psi[c].copy()
        if parent_of[c] != -1:
            w = times(w, c, rawdn[c], f[c], K_of[c])
        for d in children[c]:
            w = times(w, c, raw[d], e[d], K_of[d])
        tables.append(_max_onto(w, looked[c], list(axes[c]), list(labels), card))
        scales.append(S[c])
    root = sched[0][0]
    log_value = np.log(raw[root].max()) + np.log(2.0) * float(sum(x for c, x in e.items() if c != root))
    return tables, scales, float(log_value)


def factor_requests(plan):
    """the requests of the GPU tests: every clique onto its first one and its first two variables, and onto its separator to the parent"""
    sched = schedule(plan)
    out = []
    for c, parent, depth, K, F, R in sched:
        vs = list(plan.node_vars[c])
        out.append((c, vs[:1]))
        out.append((c, vs[:2]))
        out.append((c, list(K)))
    return out


def log_of(table, scale):
    """log of the true max-marginal: np.log(table) + scale * np.log(2.0)"""
    with np.errstate(divide="ignore"):
        return np.log(table) + float(scale) * np.log(2.0)
