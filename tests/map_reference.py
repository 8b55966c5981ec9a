"""numpy restatement of `jtp_map` (`engine.Plan.map`): the max-product sweep of include/jtprop.h, operation by operation.

Same schedule (describe()["sample"], read as `sample_reference.schedule` reads it), same multiplication order - the clique's entry
widened to float64, then the children's messages in ascending ABI clique number, left to right -, the same power-of-two scaling of
every message (`np.frexp` for the exponent of its largest entry, `np.ldexp` to take it out: both exact), and the smallest r among
equal maxima (`np.argmax` returns the first).  Every step is one IEEE operation on float64, so the device must agree bit for bit:
the tests compare states exactly."""
import numpy as np

from sample_reference import schedule


def map_reference(plan, pots, evidence=None):
    """`plan`: any plan of the tree (a `plan_only` one will do: only its schedule and labels are read); `pots[c]`: the table of
    clique c (caller's index) in the clique's axis order, in the numbers the device holds (float32 tables: float32 values, widened
    here); `evidence`: {label: state}.
    Returns (states {label: int} or None where the set fails, log_value or -inf)."""
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
    raw, arg, exps = {}, {}, {}
    failed = False
    for c, parent, depth, K, F, R in reversed(sched):                     # (deepest first: every child before its parent)
        order = [axes[c].index(v) for v in K] + [axes[c].index(v) for v in F]
        tab = np.transpose(np.asarray(pots[c]).reshape(plan.node_shape[c]), order)
        shape = tab.shape
        psi = tab.astype(np.float64)
        w = psi.copy()
        names = list(K) + list(F)
        for d in children[c]:
            e = exps[d]
            m = np.ldexp(raw[d], -e).reshape([card[v] for v in info[d][0]])       # over K_d, the child's axis order
            kd = list(info[d][0])
            m = np.transpose(m, sorted(range(len(kd)), key=lambda i: names.index(kd[i])))
            kd_sorted = sorted(kd, key=names.index)
            m = m.reshape([card[v] if v in kd_sorted else 1 for v in names])
            w = w * m
        looked = np.ones(shape, dtype=bool)
        for i, v in enumerate(names):
            if v in evidence:
                sel = np.zeros(card[v], dtype=bool)
                sel[evidence[v]] = True
                looked &= sel.reshape([card[v] if j == i else 1 for j in range(len(names))])
        if np.any(looked & ~(psi >= 0)):                                           # a negative or NaN entry that counts
            failed = True
        nk = int(np.prod(shape[:len(K)], dtype=np.int64))
        w = np.where(looked & ~np.isnan(w), w, -1.0).reshape(nk, R)                # (-1: not looked at, never the maximum of a row that has one)
        a = np.argmax(w, axis=1)
        best = w[np.arange(nk), a]
        a = np.where(best >= 0, a, 0)
        raw[c] = np.abs(np.where(best >= 0, best, 0.0))
        arg[c] = a
        top = raw[c].max()
        if not (top > 0 and np.isfinite(top)):
            failed = True
            exps[c] = 0
        else:
            exps[c] = int(np.frexp(top)[1]) - 1                                    # ilogb
    if failed:
        return None, -np.inf
    states = {}
    for c, parent, depth, K, F, R in sched:
        k = 0
        for v in K:
            k = k * card[v] + states[v]
        r = int(arg[c][k])
        for v, digit in zip(F, np.unravel_index(r, [card[v] for v in F]) if F else []):
            states[v] = int(digit)
    root = sched[0][0]
    log_value = np.log(raw[root].max()) + np.log(2.0) * float(sum(e for c, e in exps.items() if c != root))
    return states, float(log_value)


def states_row(plan, states):
    """the dict as a row of `engine.Plan.map`'s array"""
    return np.array([states[lab] for lab in plan.var_labels], dtype=np.int32)


def value_of(pots, node_vars, states):
    """the product of the clique entries at an assignment, float64"""
    v = 1.0
    for p, vs in zip(pots, node_vars):
        v = v * float(np.asarray(p, dtype=np.float64)[tuple(states[lab] for lab in vs)])
    return v
