"""numpy restatement of `jtp_entropy` (`engine.Plan.entropy`) and the bound its device result is held to.

`entropy_reference` applies the definition of include/jtprop.h to clique beliefs handed to it - in long double by default, so that
its own rounding (2^-64 a step) does not count beside the device's float64.  `parity_bound` is the distance, per clique and in nats,
within which the device's h_c must lie of it; it is derived from the order the kernels add in (csrc/jtp_entropy.hip), not tuned."""
import math

import numpy as np

EPS = 2.0 ** -53
SEG = 1024            # JT_QUERY_SEG
# The roundings a term meets between the table entry and h_c that are not additions of the chain: the logarithm (the device's float64
# log: at most 1 ulp), its product with beta (1/2), the same pair for the sigma ln sigma that is taken off (1 + 1/2), that
# subtraction (1/2), the division by S (1/2) and the last rounding of S itself (1/2), the rounding of the reference to float64 for
# the comparison (1/2): 5; the sign change is exact.  One more for the logarithm of a float32 entry widened to float64, whose last
# bits the reference sees as they are: 6.
C0 = 6.0


def _nseg(n):
    return min(4096, n // SEG) if n >= 2 * SEG else 1


def chain(R, nk):
    """Additions on the longest path from an entry to the clique's sum, as the kernels add (csrc/jtp_entropy.hip): the entries a
    lane adds one after the other, the shuffle tree over the lanes; where r is cut into segments, the segment sums a lane adds and
    the tree again; over k, what a thread (a wave where there are segments) adds one after the other, the tree of a wave, the
    four waves."""
    lanes = 1
    while lanes < 64 and lanes < R:
        lanes *= 2
    nseg = _nseg(R)
    seg_len = -(-R // nseg)
    n = -(-seg_len // lanes) + int(math.log2(lanes))
    if nseg > 1:
        n += -(-nseg // 64) + 6 + -(-nk // 4)
    else:
        n += -(-nk // 256) + 6
    return n + 3


def _rows(table, axes, K, F, dtype):
    """the table as (assignments of K, assignments of F)"""
    table = np.asarray(table)
    order = [axes.index(v) for v in K] + [axes.index(v) for v in F]
    assert sorted(order) == list(range(len(axes)))
    tab = np.transpose(table, order)
    nk = int(np.prod(tab.shape[:len(K)], dtype=np.int64)) if K else 1
    return np.ascontiguousarray(tab).reshape(nk, -1).astype(dtype)


def _plogq(p, q):
    """sum of p ln q over the entries with p > 0, and whether some of them has q = 0 (those are left out of the sum)"""
    live = p > 0
    hole = bool(np.any(live & (q == 0)))
    use = live & (q > 0)
    return (p[use] * np.log(q[use])).sum(dtype=p.dtype), hole


def entropy_reference(beliefs, sched, node_vars, ref_beliefs=None, dtype=np.longdouble):
    """(H, X, {clique: h_c}) of the beliefs `beliefs[clique]` (axes `node_vars[clique]`) on the schedule `sched`
    (`sample_reference.schedule`): H = sum of h_c = -t_c(a, a) / S_c; X = sum of -t_c(a, b) / S_c against `ref_beliefs` - inf where a
    positive entry meets a zero of the reference -, None without one.  Sums and logarithms in `dtype`; the results are floats."""
    H, X, per, holes = dtype(0), dtype(0), {}, False
    for clique, parent, depth, K, F, R in sched:
        a = _rows(beliefs[clique], list(node_vars[clique]), K, F, dtype)
        sig = a.sum(axis=1, dtype=dtype)
        S = sig.sum(dtype=dtype)
        t = _plogq(a, a)[0] - _plogq(sig, sig)[0]
        h = -t / S
        per[clique] = float(h)
        H = H + h
        if ref_beliefs is not None:
            b = _rows(ref_beliefs[clique], list(node_vars[clique]), K, F, dtype)
            inner, hole = _plogq(a, b)
            outer, hole_k = _plogq(sig, b.sum(axis=1, dtype=dtype))
            holes = holes or hole or hole_k
            X = X + -(inner - outer) / S
    if ref_beliefs is None:
        return float(H), None, per
    return float(H), float("inf") if holes else float(X), per


def parity_bound(beliefs, sched, node_vars, ref_beliefs=None):
    """{clique: bound in nats on |h_c (device) - h_c (reference)|, and on x_c with a reference}:
        EPS (C0 + chain_c) (L_c + ln n_c + 1),   EPS = 2^-53.
    Every product beta ln beta carries the few ulps counted in C0 and is at most beta L_c, L_c = max |ln beta| over the positive
    entries of the clique (and of the reference's table); a sum adds one ulp per addition on the longest chain a term passes
    (`chain`); sigma ln sigma is bounded by sigma (L_c + ln n_c), n_c the clique's entries, and moves by (ln sigma + 1) d sigma -
    the 1.  Dividing by S_c = sum beta turns the weights beta and sigma into fractions that sum to 1."""
    out = {}
    for clique, parent, depth, K, F, R in sched:
        tabs = [np.asarray(beliefs[clique], dtype=np.float64)] + ([np.asarray(ref_beliefs[clique], dtype=np.float64)] if ref_beliefs is not None else [])
        L = 0.0
        for t in tabs:
            pos = t[t > 0]
            if pos.size:
                L = max(L, float(np.max(np.abs(np.log(pos.astype(np.longdouble))))))
        n = tabs[0].size
        out[clique] = EPS * (C0 + chain(int(R), n // int(R))) * (L + math.log(n) + 1.0)
    return out


def belief_rounding(beliefs, sched, eps=EPS):
    """delta: a bound on the relative distance of any belief entry (and of any sum of entries) that a propagate in arithmetic of
    unit roundoff `eps` leaves from the exact one, non-negative tables.  A belief is the clique's potential times one message per
    neighbour.  An entry of a message out of clique d over a separator of m entries is a sum of n_d / m non-negative products -
    in whatever order, a term passes at most n_d / m - 1 additions -, each product made of the potential, the evidence and the
    other deg_d - 1 messages, and it carries the relative error of those messages.  So a clique adds at most terms_d + deg_d + 1
    roundings to whatever depends on it, terms_d = n_d over its smallest separator, and a belief depends on every clique:
        delta = eps x sum over the cliques of (terms_d + deg_d + 1)."""
    entries = {s[0]: int(np.asarray(beliefs[s[0]]).size) for s in sched}
    sep = {s[0]: entries[s[0]] // int(s[5]) for s in sched}                   # entries of the separator towards the parent (1 at the root)
    deg = {s[0]: (1 if s[1] >= 0 else 0) for s in sched}
    smallest = {s[0]: (sep[s[0]] if s[1] >= 0 else entries[s[0]]) for s in sched}
    for clique, parent, depth, K, F, R in sched:
        if parent >= 0:
            deg[parent] += 1
            smallest[parent] = min(smallest[parent], sep[clique])
    return eps * sum(entries[c] // smallest[c] + deg[c] + 1 for c in entries)


def calibration_slack(beliefs, sched, node_vars, ref_beliefs=None, eps=EPS):
    """How far H (with `ref_beliefs`: X) of rounded beliefs may lie from that of the exact ones, in nats; for comparisons with
    something NOT formed from the plan's own beliefs (enumeration, another plan, log Z).  With delta = `belief_rounding`:
    h_c = -sum p ln(beta / sigma), p = beta / S.  Each of the two logarithms moves by at most delta, and the weights sum to 1:
    2 delta.  Each weight moves by at most 2 delta of itself, and |ln(beta / sigma)| <= L_c + ln n_c (L_c, n_c as in
    `parity_bound`): 2 delta (L_c + ln n_c).  Together, over the cliques: sum_c 2 delta (1 + L_c + ln n_c); the same holds for x_c
    with the reference's tables in the logarithms and L_c taken over both."""
    delta = belief_rounding(beliefs, sched, eps)
    if ref_beliefs is not None:
        delta = max(delta, belief_rounding(ref_beliefs, sched, eps))
    out = 0.0
    for clique, parent, depth, K, F, R in sched:
        tabs = [np.asarray(beliefs[clique], dtype=np.float64)] + ([np.asarray(ref_beliefs[clique], dtype=np.float64)] if ref_beliefs is not None else [])
        L = 0.0
        for t in tabs:
            pos = t[t > 0]
            if pos.size:
                L = max(L, float(np.max(np.abs(np.log(pos.astype(np.longdouble))))))
        out += 2.0 * delta * (1.0 + L + math.log(tabs[0].size))
    return out


def brute_force_entropy(factors, sizes, values, evidence=None, values_q=None):
    """(H, log Z, KL) by enumeration of the joint: the entropy of the posterior given `evidence` ({variable: state}), the log of its
    normaliser, and - with `values_q` - KL(posterior under `values` || posterior under `values_q`), inf where the second lacks support"""
    labels = sorted(sizes, key=str)
    letters = {lab: chr(ord("a") + i) for i, lab in enumerate(labels)}
    expr = ",".join("".join(letters[v] for v in f) for f in factors) + "->" + "".join(letters[v] for v in labels)

    def posterior(vals):
        joint = np.einsum(expr, *[np.asarray(v, dtype=np.float64) for v in vals]).astype(np.longdouble)
        for lab, st in (evidence or {}).items():
            mask = np.zeros(sizes[lab])
            mask[st] = 1.0
            shape = [1] * len(labels)
            shape[labels.index(lab)] = sizes[lab]
            joint = joint * mask.reshape(shape)
        z = joint.sum()
        return joint / z, z

    p, z = posterior(values)
    live = p > 0
    H = float(-(p[live] * np.log(p[live])).sum())
    kl = None
    if values_q is not None:
        q, _ = posterior(values_q)
        kl = float("inf") if np.any(live & (q == 0)) else float((p[live] * (np.log(p[live]) - np.log(q[live]))).sum())
    return H, float(np.log(z)), kl
