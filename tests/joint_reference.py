"""numpy restatement of `jtp_joint` (`engine.Plan.joint`): the joint of variables of different cliques from the clique beliefs.

The definition (include/jtprop.h), on the sampling schedule (`sample_reference.schedule`: per clique its parent, depth,
K = the variables shared with the parent, F = the others in axis order, R = prod card(F)):
  home of a query variable   the shallowest clique that holds it
  top                        the deepest clique whose subtree holds every home
  active cliques             those on the paths from the homes up to the top
  C_c, Q_c                   the query variables whose home lies in the subtree of c (in the order of the query) / is c itself
upward, deepest first, for every active clique but the top
  sigma_c[k] = sum_r beta_c[k, r]
  U_c[k, x]  = sum_r' beta_c[k, x|Q_c, r'] * M_d1 * M_d2 ...     active children in ascending clique number, left to right
  M_c[k, x]  = U_c[k, x] / sigma_c[k], 0 where sigma_c[k] = 0
and the top sums over everything outside the query, K_top included, without dividing.  Sums are numpy's (pairwise): the device adds
the same non-negative terms in another order, so the two agree to a summation bound, not bit for bit."""
import numpy as np


def _expand(array, labels, all_labels):
    """`array` with axes `labels` as a view broadcastable over `all_labels` (a superset, any order)"""
    order = [labels.index(lab) for lab in all_labels if lab in labels]
    shape = [array.shape[labels.index(lab)] if lab in labels else 1 for lab in all_labels]
    return np.transpose(array, order).reshape(shape)


def joint_reference(beliefs, sched, query, node_vars):
    """`beliefs`: {clique: float64 table}, its axes `node_vars[clique]`; `sched`: `sample_reference.schedule(plan)`; `query`: distinct
    labels.  Returns (joint over the query's variables in that axis order, [(clique, R_c, R'_c, m_c)] over the active cliques in
    visit order, the top first: m_c = the number of active children)."""
    query = list(query)
    assert len(set(query)) == len(query) and query
    by = {s[0]: s for s in sched}
    order = [s[0] for s in sched]                        # visit order: by depth, then clique number
    home = {}
    for q in query:
        home[q] = next(c for c in order if q in by[c][4])          # (the shallowest clique that holds q has it in F)
    paths = []
    for q in query:                                      # from the home up to the root
        p = [home[q]]
        while by[p[-1]][1] >= 0:
            p.append(by[p[-1]][1])
        paths.append(p)
    common = set(paths[0]).intersection(*[set(p) for p in paths[1:]])
    top = max(common, key=lambda c: by[c][2])
    active = set()
    for p in paths:
        active.update(p[:p.index(top) + 1])
    active = [c for c in order if c in active]
    assert active[0] == top
    carried = {c: [q for q, p in zip(query, paths) if c in p[:p.index(top) + 1]] for c in active}
    msgs, report = {}, {}
    sizes = {}
    for c in active:
        for lab, n in zip(node_vars[c], np.shape(beliefs[c])):
            sizes[lab] = n
    for c in reversed(active):
        _, parent, depth, K, F, R = by[c]
        axes = list(node_vars[c])
        beta = np.asarray(beliefs[c], dtype=np.float64)
        own = [q for q in carried[c] if home[q] == c]
        kids = sorted(d for d in active if by[d][1] == c)
        K = list(K) if c != top else []
        rest = [lab for lab in axes if lab not in K and lab not in own]            # F'_c (the top: its K as well), axis order
        brought = [q for q in carried[c] if q not in own]
        every = K + own + rest + brought
        w = _expand(beta, axes, every)
        for d in kids:                                                              # ascending clique number, left to right
            w = w * _expand(msgs[d][0], msgs[d][1], every)
        rest_axes = tuple(every.index(lab) for lab in rest)
        u = w.sum(axis=rest_axes) if rest_axes else w
        u_labels = K + own + brought
        out_labels = K + carried[c]
        u = np.transpose(u, [u_labels.index(lab) for lab in out_labels])
        r_prime = int(np.prod([sizes[lab] for lab in rest], dtype=np.int64))
        report[c] = (c, int(R), r_prime, len(kids))
        if c == top:
            assert carried[c] == query
            return u, [report[a] for a in active]
        sigma = _expand(beta, axes, K + [lab for lab in axes if lab not in K]).sum(axis=tuple(range(len(K), len(axes))))
        sig = sigma.reshape(sigma.shape + (1,) * len(carried[c]))
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(sig == 0.0, 0.0, u / sig)
        msgs[c] = (m, out_labels)
    raise AssertionError("unreachable")


def parity_bound(report):
    """B of the tests: 2^-53 x sum over the active cliques of (R_c + m_c + 2)"""
    return 2.0 ** -53 * sum(r + m + 2 for _, r, _, m in report)


def brute_force_joint(factors, sizes, values, evidence, query):
    """The unnormalised joint of `query` from the einsum of all factors, entries that contradict `evidence` zeroed."""
    labels = list(sizes)
    ids = {lab: i for i, lab in enumerate(labels)}
    ops = []
    for f, v in zip(factors, values):
        ops += [np.asarray(v, dtype=np.float64), [ids[lab] for lab in f]]
    for lab, st in (evidence or {}).items():
        mask = np.zeros(sizes[lab])
        mask[st] = 1.0
        ops += [mask, [ids[lab]]]
    return np.einsum(*ops, [ids[lab] for lab in query])
