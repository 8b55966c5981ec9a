"""numpy reference for `jtp_sample` (`engine.Plan.sample`): what the draw of one clique must satisfy, from the host's side.

Nothing here runs the sweep: given the beliefs a plan holds, the states it returned and the uniforms it used
(`synthetic.sample_uniform`), `clique_draws` rebuilds, per sample, the slice of the clique's belief the kernel conditioned on and
where in its cumulative sum the drawn entry lies.  The tests assert the inverse-CDF property on that."""
import numpy as np


def schedule(plan):
    """describe()["sample"] of a plan with variable ids turned into the plan's labels and ABI clique numbers into the caller's:
    [(clique, parent, depth, K labels, F labels, R)] in visit order."""
    d = plan.describe()["sample"]
    lab = plan.var_labels
    out = []
    for c in d["cliques"]:
        parent = plan.node_ids[c["parent"]] if c["parent"] >= 0 else -1
        out.append((plan.node_ids[c["clique"]], parent, c["depth"], [lab[v] for v in c["K"]], [lab[v] for v in c["F"]], int(c["R"])))
    return out


def clique_draws(belief, axes, K, F, states, columns):
    """`belief`: the clique's table (float64) with axes labelled `axes`; `K` / `F`: the conditioning and the drawn variables (F in
    the clique's axis order); `states`: int array (N, n columns), column `columns[label]` the state of a variable.
    Returns a dict of arrays over the N samples:
      slice (N, R)  the entries w_r the sample chose among, r in C order over F
      r             the entry the states name
      w             its weight
      lo, hi        the cumulative sums (float64, in r order) before and including it
      total         the sum of the slice"""
    belief = np.asarray(belief, dtype=np.float64)
    assert [a for a in axes if a in F] == list(F), "F must be in the clique's axis order"
    order = [axes.index(v) for v in K] + [axes.index(v) for v in F]
    assert sorted(order) == list(range(len(axes)))
    tab = np.transpose(belief, order)
    k_shape, f_shape = tab.shape[:len(K)], tab.shape[len(K):]
    n_k = int(np.prod(k_shape, dtype=np.int64)) if K else 1
    n_f = int(np.prod(f_shape, dtype=np.int64)) if F else 1
    tab = np.ascontiguousarray(tab).reshape(n_k, n_f)
    n = states.shape[0]
    k_idx = np.zeros(n, dtype=np.int64)
    for v, size in zip(K, k_shape):
        k_idx = k_idx * size + states[:, columns[v]]
    r = np.zeros(n, dtype=np.int64)
    for v, size in zip(F, f_shape):
        r = r * size + states[:, columns[v]]
    sl = tab[k_idx]
    cs = np.cumsum(sl, axis=1)
    rows = np.arange(n)
    hi = cs[rows, r]
    lo = np.where(r > 0, cs[rows, np.maximum(r - 1, 0)], 0.0)
    return {"slice": sl, "r": r, "w": sl[rows, r], "lo": lo, "hi": hi, "total": cs[:, -1]}
