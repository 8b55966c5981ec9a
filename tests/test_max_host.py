"""Max-propagation (`jtp_max_marginals`), the part that needs no GPU: the entry point, and the numpy restatement of the sweep
(`tests/max_reference.py`) against brute force - the einsum joint of the factors, then `np.max` over the axes a request drops - on
models small enough to enumerate (under 2^16 joint assignments).

Tolerance, relative on values: 4 (n_cliques + n_factors) 2^-53.  A value of the sweep is one entry per clique multiplied through at
most n_cliques - 1 message multiplications, the brute force has its own n_factors multiplications, each rounding 2^-53; the factor
2 on top covers second-order terms.  On logarithms 4 spacings of |log_value| are added (the `log`, the multiply and the add that
form it, on either side).  Derived, not measured."""
import numpy as np
import pytest

import junctiontree_amd as jt
from junctiontree_amd import _capi, engine, synthetic
from max_reference import factor_requests, log_of, max_reference

README_FACTORS = [["cloudy"], ["cloudy", "sprinkler"], ["cloudy", "rain"], ["rain", "sprinkler", "wet_grass"]]
README_SIZES = {"cloudy": 2, "sprinkler": 2, "rain": 2, "wet_grass": 2}
README_VALUES = [np.array([0.5, 0.5]), np.array([[0.5, 0.5], [0.9, 0.1]]), np.array([[0.8, 0.2], [0.2, 0.8]]),
                 np.array([[[1.0, 0.0], [0.1, 0.9]], [[0.1, 0.9], [0.01, 0.99]]])]
IMPOSSIBLE = {"sprinkler": 0, "rain": 0, "wet_grass": 1}


def readme_model():
    """(tree, clique tables, node_vars, sizes, n_cliques, factors, factor values)"""
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    ct = tree.clique_tree
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]
    pots = [np.broadcast_to(p, [README_SIZES[v] for v in vs]).copy() for p, vs in zip(ct.evaluate(README_VALUES), ct.maxcliques)]
    return tree.tree, pots, node_vars, README_SIZES, len(ct.maxcliques), README_FACTORS, README_VALUES


def five_cliques():
    """two children under the root, two under the first of them; cardinalities 2 and 3, clique tables of very different sizes"""
    rng = np.random.default_rng(21)
    node_vars = [["a", "b", "c"], ["b", "d"], ["c", "e"], ["d", "f"], ["d", "g"], ["b"], ["c"], ["d"], ["d"]]
    sizes = {"a": 2, "b": 3, "c": 2, "d": 3, "e": 2, "f": 3, "g": 2}
    tree = [0, (5, [1, (7, [3]), (8, [4])]), (6, [2])]
    scale = [1e30, 1e-25, 3.0, 1e12, 1e-40]
    pots = [rng.uniform(0.5, 1.5, [sizes[v] for v in vs]) * s for vs, s in zip(node_vars[:5], scale)]
    return tree, pots, node_vars, sizes, 5, node_vars[:5], pots


def chain():
    spec = synthetic.chain_tree(4, 3, 3)
    pots = synthetic.potentials_for(spec, seed=5)
    n = spec["n_cliques"]
    return spec["tree"], pots[:n], spec["node_vars"], spec["sizes"], n, spec["node_vars"][:n], pots[:n]


MODELS = {"readme": readme_model, "five_cliques": five_cliques, "chain4_card3": chain}
EVIDENCE = {
    "readme": [None, {"wet_grass": 1}, {"cloudy": 0, "sprinkler": 1}],
    "five_cliques": [None, {"d": 2}, {"b": 1, "g": 0}],
    "chain4_card3": [None, {1: 2, 5: 1}],
}
RUNS = [(name, i) for name in MODELS for i in range(len(EVIDENCE[name]))]


def brute_force(factors, sizes, values, evidence):
    """(labels, the joint with the entries that contradict the evidence at 0)"""
    labels = sorted(sizes, key=str)
    assert np.prod([sizes[v] for v in labels], dtype=np.int64) < 1 << 16
    letters = {lab: chr(ord("a") + i) for i, lab in enumerate(labels)}
    expr = ",".join("".join(letters[v] for v in f) for f in factors) + "->" + "".join(letters[v] for v in labels)
    joint = np.einsum(expr, *[np.asarray(v, dtype=np.float64) for v in values])
    for lab, st in (evidence or {}).items():
        keep = np.zeros(sizes[lab], dtype=bool)
        keep[st] = True
        joint = np.where(keep.reshape([sizes[u] if u == lab else 1 for u in labels]), joint, 0.0)
    return labels, joint


def max_onto(labels, joint, keep):
    drop = tuple(i for i, v in enumerate(labels) if v not in keep)
    best = joint.max(axis=drop) if drop else joint
    left = [v for v in labels if v in keep]
    return np.transpose(best, [left.index(v) for v in keep])


def test_jtp_max_marginals_is_exported_and_bound_and_plan_only_plans_raise():
    assert "jtp_max_marginals" in _capi.SYMBOLS
    fn = _capi.lib().jtp_max_marginals
    assert fn.argtypes is not None and len(fn.argtypes) == 12
    spec = synthetic.wide_binary_tree(3, 6, 3)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], plan_only=True)
    with pytest.raises(_capi.JtpError):
        plan.max_marginals([(0, spec["node_vars"][0][:1])])


@pytest.mark.parametrize("name,which", RUNS, ids=["%s-%d" % r for r in RUNS])
def test_the_restatement_gives_the_brute_force_max_marginals(name, which):
    tree, pots, node_vars, sizes, n, factors, values = MODELS[name]()
    evidence = EVIDENCE[name][which]
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    requests = factor_requests(plan) + [(c, list(node_vars[c])) for c in range(n)]
    tables, scales, log_value = max_reference(plan, pots, requests, evidence)
    labels, joint = brute_force(factors, sizes, values, evidence)
    best = joint.max()
    tol = 4 * (n + len(factors)) * 2.0 ** -53
    log_tol = tol + 4 * np.spacing(abs(log_value))
    assert best > 0 and np.isfinite(log_value)
    print("%s %r: log_value %.17g, brute force %.17g (bound %.3g)" % (name, evidence, log_value, np.log(best), log_tol))
    assert abs(log_value - np.log(best)) <= log_tol
    worst = 0.0
    for (c, keep), table, scale in zip(requests, tables, scales):
        want = max_onto(labels, joint, keep)
        assert table.shape == want.shape and table.dtype == np.float64
        got = np.ldexp(table, scale)
        assert np.all(got[want == 0] == 0), "request %r: a value where the brute force has none" % ((c, keep),)
        nz = want > 0
        if nz.any():
            worst = max(worst, float(np.max(np.abs(got[nz] - want[nz]) / want[nz])))
        assert np.all(np.abs(got - want) <= tol * want), (c, keep)
        # every table's largest entry is the value of the most probable assignment
        assert abs(log_of(table, scale).max() - log_value) <= log_tol
    print("worst relative difference of a value %.3g (bound %.3g)" % (worst, tol))
    for lab, st in (evidence or {}).items():                 # observed variables: nothing off the observed state
        c = next(c for c in range(n) if lab in node_vars[c])
        (table,), _, _ = max_reference(plan, pots, [(c, [lab])], evidence)
        assert table[st] > 0 and np.all(np.delete(table, st) == 0)


def test_evidence_of_probability_zero_fails_in_the_restatement_as_brute_force_says():
    tree, pots, node_vars, sizes, n, factors, values = readme_model()
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    labels, joint = brute_force(factors, sizes, values, IMPOSSIBLE)
    assert joint.max() == 0.0
    requests = factor_requests(plan)
    tables, scales, log_value = max_reference(plan, pots, requests, IMPOSSIBLE)
    assert log_value == -np.inf and all(s == 0 for s in scales)
    for (c, keep), table in zip(requests, tables):
        assert table.shape == tuple(sizes[v] for v in keep) and not table.any()
    negative = [np.array(p) for p in pots]
    negative[0].flat[0] = -1.0
    assert max_reference(plan, negative, requests)[2] == -np.inf


def test_entries_far_apart_keep_their_logarithms():
    """clique tables near 10^200, 10^150, 10^180, 10^-100 and 10^120: the value of an assignment, about 10^550, leaves float64; the
    scaled tables and integer exponents do not.  Against a brute force in logarithms (sums of logs, exact to a few spacings of the
    largest term)"""
    tree, pots, node_vars, sizes, n, _, _ = five_cliques()
    rng = np.random.default_rng(4)
    huge = [rng.uniform(0.5, 1.5, np.shape(p)) * 10.0 ** x for p, x in zip(pots, (200, 150, 180, -100, 120))]
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    requests = factor_requests(plan)
    evidence = {"d": 1}
    tables, scales, log_value = max_reference(plan, huge, requests, evidence)
    labels = sorted(sizes)
    log_joint = np.zeros([sizes[v] for v in labels])
    for p, vs in zip(huge, node_vars[:n]):
        order = sorted(range(len(vs)), key=lambda i: labels.index(vs[i]))
        log_joint = log_joint + np.transpose(np.log(p), order).reshape([sizes[v] if v in vs else 1 for v in labels])
    keep = np.zeros(sizes["d"], dtype=bool)
    keep[1] = True
    log_joint = np.where(keep.reshape([sizes[u] if u == "d" else 1 for u in labels]), log_joint, -np.inf)
    # n logs of up to 200 ln 10 = 461 each and their sum, against the sweep's 2 n roundings and the final log, multiply and add
    tol = 4 * (2 * n) * 2.0 ** -53 + (n + 4) * np.spacing(n * 461.0)
    assert log_value > 1200 and abs(log_value - log_joint.max()) <= tol
    for (c, keep_vars), table, scale in zip(requests, tables, scales):
        want = max_onto(labels, log_joint, keep_vars)
        got = log_of(table, scale)
        assert np.all((got == -np.inf) == (want == -np.inf))
        fin = np.isfinite(want)
        assert np.all(np.abs(got[fin] - want[fin]) <= tol), (c, keep_vars)
