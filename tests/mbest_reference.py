"""numpy restatement of `jtp_map_best` (`engine.Plan.map_best`): the list-valued max-product sweep of include/jtprop.h, operation
by operation.

Same schedule as `map_reference` (describe()["sample"], read as `sample_reference.schedule` reads it), the same power-of-two scaling
of every message (`np.frexp` for the exponent of the largest first element, `np.ldexp` to take it out: both exact), and per entry
the fold over the children in ascending ABI clique number: the products E[a] * m[b] are formed - all M x M of them on request, by
default those with (a + 1) * (b + 1) <= M, as on the device: the others cannot be among the M largest -, the positive ones put in
descending value with equal values in ascending (a, b) by a stable sort of the products laid out in (a, b) order, and the first
M kept.  Per k the same over the (r, t) of the entries' lists.  Every step is one IEEE operation on float64, so the device must agree bit for bit: the tests
compare states exactly."""
import numpy as np

from sample_reference import schedule


def _largest(values, m):
    """rows of candidates, laid out in the order that decides among equals: (the m largest positive ones per row in descending
    value, zero past their count; their places in the row)"""
    keyed = np.where(values > 0, values, -1.0)                                    # (zero, negative, NaN: not listed)
    order = np.argsort(-keyed, axis=1, kind="stable")[:, :m]
    best = np.take_along_axis(keyed, order, axis=1)
    return np.where(best > 0, best, 0.0), np.where(best > 0, order, 0)


def mbest_reference(plan, pots, m, evidence=None, with_values=False, all_pairs=False):
    """`plan`, `pots`, `evidence`: as `map_reference` takes them; `m`: the length of every list; `all_pairs`: every step of a fold
    forms all m x m products, not only those with (a + 1) * (b + 1) <= m - the same result (tests/test_mbest_host.py), five times
    the work at m = 16.
    Returns (list of n_found dicts {label: int}, best first, float64 array of their log values), or (None, None) where the set
    fails; `with_values`: a third item, the values themselves - the root's list times two to the exponents taken out, exact
    unless that leaves float64."""
    evidence = dict(evidence or {})
    sched = schedule(plan)
    axes = plan.node_vars
    card = {lab: plan.node_shape[c][i] for c in plan.cliques for i, lab in enumerate(axes[c])}
    children = {c: [] for c, *_ in sched}
    for c, parent, *_ in sched:
        if parent != -1:
            children[parent].append(c)
    for c in children:
        children[c].sort(key=lambda d: plan.abi_of[d])
    info = {c: (K, F) for c, _, _, K, F, _ in sched}
    raw, arg, exps, back = {}, {}, {}, {}
    failed = False
    pairs = [(a, b) for a in range(m) for b in range(m) if all_pairs or (a + 1) * (b + 1) <= m]
    pair_a, pair_b = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    for c, parent, depth, K, F, R in reversed(sched):                     # (deepest first: every child before its parent)
        order = [axes[c].index(v) for v in K] + [axes[c].index(v) for v in F]
        tab = np.transpose(np.asarray(pots[c]).reshape(plan.node_shape[c]), order)
        shape = tab.shape
        psi = tab.astype(np.float64)
        names = list(K) + list(F)
        looked = np.ones(shape, dtype=bool)
        for i, v in enumerate(names):
            if v in evidence:
                sel = np.zeros(card[v], dtype=bool)
                sel[evidence[v]] = True
                looked = looked & sel.reshape([card[v] if j == i else 1 for j in range(len(names))])
        if np.any(looked & ~(psi >= 0)):                                           # a negative or NaN entry that counts
            failed = True
        nk = int(np.prod(shape[:len(K)], dtype=np.int64))
        n = nk * R
        E = np.zeros((n, m))
        E[:, 0] = np.where(looked & (psi > 0), psi, 0.0).reshape(n)                # E_0: one element, none where the entry is 0
        back[c] = []
        for d in children[c]:
            kd = list(info[d][0])
            at = np.zeros(shape, dtype=np.int64)                                   # k_d of every entry of c
            radix = 1
            for v in reversed(kd):
                i = names.index(v)
                at = at + np.arange(card[v]).reshape([card[v] if j == i else 1 for j in range(len(names))]) * radix
                radix *= card[v]
            msg = np.ldexp(raw[d], -exps[d])[at.reshape(n)]                        # (n, m)
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                prod = E[:, pair_a] * msg[:, pair_b]                               # [entry, (a, b) in lexicographic order]
            E, place = _largest(prod, m)
            back[c].append((pair_a * m + pair_b)[place].astype(np.int16))          # a * m + b
        best, place = _largest(E.reshape(nk, R * m), m)
        raw[c] = best
        arg[c] = place                                                             # r * m + t
        top = raw[c][:, 0].max()
        if not (top > 0 and np.isfinite(top)):
            failed = True
            exps[c] = 0
        else:
            exps[c] = int(np.frexp(top)[1]) - 1                                    # ilogb
    if failed:
        return (None, None, None) if with_values else (None, None)
    root = sched[0][0]
    scale = np.log(2.0) * float(sum(e for c, e in exps.items() if c != root))
    found = int(np.count_nonzero(raw[root][0] > 0))
    solutions, values = [], []
    for s in range(found):
        rank = {root: s}
        states = {}
        for c, parent, depth, K, F, R in sched:
            k = 0
            for v in K:
                k = k * card[v] + states[v]
            r, t = divmod(int(arg[c][k, rank[c]]), m)
            for v, digit in zip(F, np.unravel_index(r, [card[v] for v in F]) if F else []):
                states[v] = int(digit)
            for d, place in zip(reversed(children[c]), reversed(back[c])):        # back through the fold of entry (k, r)
                t, rank[d] = divmod(int(place[k * R + r, t]), m)
        solutions.append(states)
        values.append(np.log(raw[root][0][s]) + scale)
    values = np.array(values, dtype=np.float64)
    if with_values:
        return solutions, values, np.ldexp(raw[root][0][:found], sum(e for c, e in exps.items() if c != root))
    return solutions, values


def states_rows(plan, solutions):
    """the dicts as the rows of `engine.Plan.map_best`'s array"""
    return np.array([[st[lab] for lab in plan.var_labels] for st in solutions], dtype=np.int32).reshape(len(solutions), len(plan.var_labels))
