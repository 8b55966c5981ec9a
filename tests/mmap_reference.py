"""numpy restatement of `jtp_marginal_map` (`engine.Plan.marginal_map`): the sum-then-max sweep of include/jtprop.h.

Same schedule as `map_reference` (describe()["sample"], read as `sample_reference.schedule` reads it), same multiplication order -
the clique's entry widened to float64, then the children's messages in ascending ABI clique number, left to right -, the same
power-of-two scaling of every message, the smallest rm among equal maxima.  What differs from the device is the ORDER of the sum
over rs: numpy's own (`ndarray.sum`), where the device adds blocks per lane and a butterfly.  With integer potentials every sum is
exact and the two agree bit for bit; otherwise they agree to `parity_bound`.  With every variable in the query every sum has one
term and this is `map_reference`, exactly."""
import itertools

import numpy as np

from sample_reference import schedule


def split(plan, query):
    """[(clique, K, FM, FS, Rs, number of children)] in visit order: F cut into the query's variables and the others"""
    query = set(query)
    sched = schedule(plan)
    card = {lab: plan.node_shape[c][i] for c in plan.cliques for i, lab in enumerate(plan.node_vars[c])}
    kids = {c: 0 for c, *_ in sched}
    for c, parent, *_ in sched:
        if parent != -1:
            kids[parent] += 1
    out = []
    for c, parent, depth, K, F, R in sched:
        fs = [v for v in F if v not in query]
        out.append((c, list(K), [v for v in F if v in query], fs, int(np.prod([card[v] for v in fs], dtype=np.int64)), kids[c]))
    return out


def parity_bound(plan, query):
    """Relative bound between two evaluations of max raw_root that add the same non-negative terms in different orders:
    4 x 2^-53 x sum over the cliques of (Rs_c + m_c + 2), m_c the children of c.

    As `joint_reference.parity_bound`: with u = 2^-53, an entry w = ((psi * m_1) * ...) * m_d takes one rounding per child (ldexp is
    exact), a sum of Rs_c non-negative terms in ANY order is within (Rs_c - 1) u of the exact sum relatively, and a maximum is exact -
    the maximum of values each within a relative eps of their true ones is within eps of the true maximum.  All terms are
    non-negative, so the relative errors of the messages a clique reads add up and nothing is amplified: one evaluation is within
    (1 + u)^(sum_c (Rs_c - 1 + m_c)) - 1 of the exact value, two evaluations within twice that of each other.  The +2 per clique and
    the factor 4 instead of 2 pay for the second-order terms (sum_c (Rs_c + m_c) stays far below 2^26 here)."""
    return 4 * 2.0 ** -53 * sum(rs + m + 2 for _, _, _, _, rs, m in split(plan, query))


def mmap_reference(plan, pots, query, evidence=None):
    """`plan`: any plan of the tree (a `plan_only` one will do: only its schedule and labels are read); `pots[c]`: the table of
    clique c (caller's index) in the clique's axis order, in the numbers the device holds; `query`: labels; `evidence`: {label: state}.
    Returns (states {label: int} over the query or None where the set fails, log_value or -inf)."""
    evidence = dict(evidence or {})
    query = list(query)
    axes = plan.node_vars
    card = {lab: plan.node_shape[c][i] for c in plan.cliques for i, lab in enumerate(axes[c])}
    parts = split(plan, query)
    sched = schedule(plan)
    children = {c: [] for c, *_ in sched}
    for c, parent, *_ in sched:
        if parent != -1:
            children[parent].append(c)
    for c in children:
        children[c].sort(key=lambda d: plan.abi_of[d])
    k_of = {c: K for c, K, _, _, _, _ in parts}
    raw, arg, exps = {}, {}, {}
    failed = False
    for c, K, FM, FS, Rs, _ in reversed(parts):                            # (deepest first: every child before its parent)
        names = K + FM + FS
        tab = np.transpose(np.asarray(pots[c]).reshape(plan.node_shape[c]), [axes[c].index(v) for v in names])
        psi = tab.astype(np.float64)
        w = psi.copy()
        for d in children[c]:
            kd = list(k_of[d])
            m = np.ldexp(raw[d], -exps[d]).reshape([card[v] for v in kd])      # over K_d, the child's axis order
            m = np.transpose(m, sorted(range(len(kd)), key=lambda i: names.index(kd[i])))
            m = m.reshape([card[v] if v in kd else 1 for v in names])
            w = w * m
        looked = np.ones(psi.shape, dtype=bool)
        for i, v in enumerate(names):
            if v in evidence:
                sel = np.zeros(card[v], dtype=bool)
                sel[evidence[v]] = True
                looked &= sel.reshape([card[v] if j == i else 1 for j in range(len(names))])
        if np.any(looked & ~(psi >= 0)):                                   # a negative or NaN entry that counts
            failed = True
        nk = int(np.prod([card[v] for v in K], dtype=np.int64))
        rm = int(np.prod([card[v] for v in FM], dtype=np.int64))
        looked = looked.reshape(nk, rm, Rs)
        with np.errstate(invalid="ignore"):
            u = np.where(looked, w.reshape(nk, rm, Rs), 0.0).sum(axis=2)
        u = np.where(looked.any(axis=2) & ~np.isnan(u), u, -1.0)           # (-1: not looked at, never the maximum of a row that has one)
        a = np.argmax(u, axis=1)
        best = u[np.arange(nk), a]
        arg[c] = np.where(best >= 0, a, 0)
        raw[c] = np.abs(np.where(best >= 0, best, 0.0))
        top = raw[c].max()
        if not (top > 0 and np.isfinite(top)):
            failed = True
            exps[c] = 0
        else:
            exps[c] = int(np.frexp(top)[1]) - 1                            # ilogb
    if failed:
        return None, -np.inf
    states = {}
    for c, K, FM, FS, Rs, _ in parts:
        if not FM:
            continue
        k = 0
        for v in K:
            k = k * card[v] + states[v]
        for v, digit in zip(FM, np.unravel_index(int(arg[c][k]), [card[v] for v in FM])):
            states[v] = int(digit)
    root = parts[0][0]
    log_value = np.log(raw[root].max()) + np.log(2.0) * float(sum(e for c, e in exps.items() if c != root))
    return {v: states[v] for v in query}, float(log_value)


def brute_force(node_vars, pots, sizes, query, evidence=None):
    """sum over the other variables of the product of the clique tables, as an array over `query` (in that order), in extended
    precision so that its own rounding does not count; entries that contradict `evidence` are -1"""
    labels = sorted(sizes, key=str)
    ids = {lab: i for i, lab in enumerate(labels)}
    ops = []
    for vs, p in zip(node_vars, pots):
        ops += [np.asarray(p, dtype=np.longdouble), [ids[v] for v in vs]]
    for lab, st in (evidence or {}).items():
        mask = np.zeros(sizes[lab], dtype=np.longdouble)
        mask[st] = 1
        ops += [mask, [ids[lab]]]
    table = np.einsum(*ops, [ids[v] for v in query], optimize="greedy")
    for ax, lab in enumerate(query):
        if lab in (evidence or {}):
            keep = np.zeros(sizes[lab], dtype=bool)
            keep[evidence[lab]] = True
            table = np.where(keep.reshape([sizes[lab] if j == ax else 1 for j in range(len(query))]), table, -1)
    return table


def two_best(table):
    """(best, second best) entries of a brute-force table (second: -1 if it has one entry)"""
    flat = np.sort(np.asarray(table).reshape(-1))
    return flat[-1], (flat[-2] if flat.size > 1 else type(flat[-1])(-1))


def is_rip(parent, node_vars):
    """the running-intersection property: the cliques that hold a variable are connected in the tree"""
    for v in set(itertools.chain.from_iterable(node_vars)):
        holders = [c for c, vs in enumerate(node_vars) if v in vs]
        tops = [c for c in holders if parent[c] < 0 or v not in node_vars[parent[c]]]
        if len(tops) != 1:
            return False
    return True


def strong_model(factors, sizes, query):
    """(tree, node_vars, parent list, maxcliques, factor_to_maxclique) of the strong junction tree of a factor graph"""
    from junctiontree_amd import construction, engine
    maxcliques, f2m, tree, separators = construction.strong_junction_tree(factors, sizes, query)
    node_vars = [list(c) for c in maxcliques] + [list(s) for s in separators]
    _, parent, _, _ = engine.flatten_tree(tree) if maxcliques else ([], {}, {}, {})
    return tree, node_vars, [parent[c] for c in range(len(maxcliques))], maxcliques, f2m
