"""The most probable assignment (`jtp_map`), the part that needs no GPU: the entry point, and the numpy restatement of the sweep
(`tests/map_reference.py`) against brute force on models small enough to enumerate.

VALUES are compared, not assignments, so that ties can neither hide nor fake a failure: the product of the clique entries at the
restatement's assignment against the largest entry of the enumerated joint.  Tolerance, relative: (cliques + messages) x 2^-52 -
the sweep takes its maxima over products of one rounding per clique table and per message, the enumeration rounds once per clique,
each rounding 2^-53 on either side."""
import numpy as np
import pytest

from junctiontree_amd import _capi, engine, synthetic
from map_reference import map_reference, value_of
from test_planner_emulated import star


def spec_case(spec, seed=5):
    return spec["tree"], synthetic.potentials_for(spec, seed=seed), spec["node_vars"], spec["sizes"], spec["n_cliques"]


def star_case(n_children):
    tree, pots, node_vars, sizes = star(n_children, card=2, seed=n_children)
    return tree, pots, node_vars, sizes, n_children + 1


def contained_case():
    rng = np.random.default_rng(8)
    node_vars = [[0, 1, 2, 3], [1, 2], [2, 3, 4], [4, 2], [1, 2], [2, 3], [2, 4]]
    sizes = {0: 3, 1: 2, 2: 3, 3: 2, 4: 5}
    tree = [0, (4, [1]), (5, [2, (6, [3])])]
    pots = [rng.uniform(0.5, 1.5, [sizes[v] for v in vs]) for vs in node_vars[:4]] + [np.ones([sizes[v] for v in vs]) for vs in node_vars[4:]]
    return tree, pots, node_vars, sizes, 4


SMALL = {
    "wide7": lambda: spec_case(synthetic.wide_binary_tree(7, 4, 2)),            # 16 binary variables: 2^16 joint states
    "chain5_card3": lambda: spec_case(synthetic.chain_tree(5, 3, 3)),
    "random8_card3": lambda: spec_case(synthetic.random_tree(8, 3, 2, card=3)),
    "random4_card5": lambda: spec_case(synthetic.random_tree(4, 3, 2, card=5)),
    "star5": lambda: star_case(5),
    "contained": contained_case,
}


def brute_force(pots, node_vars, sizes, n, evidence):
    labels = sorted(sizes)
    assert np.prod([sizes[v] for v in labels], dtype=np.int64) <= 1 << 16
    joint = np.ones([sizes[v] for v in labels])
    for p, vs in zip(pots[:n], node_vars[:n]):
        order = sorted(range(len(vs)), key=lambda i: labels.index(vs[i]))
        t = np.transpose(np.asarray(p, dtype=np.float64), order)
        joint = joint * t.reshape([sizes[v] if v in vs else 1 for v in labels])
    for v, st in (evidence or {}).items():
        keep = np.zeros(sizes[v], dtype=bool)
        keep[st] = True
        joint = np.where(keep.reshape([sizes[u] if u == v else 1 for u in labels]), joint, -1.0)
    return float(joint.max())


def test_jtp_map_is_exported_and_bound():
    assert "jtp_map" in _capi.SYMBOLS
    fn = _capi.lib().jtp_map
    assert fn.argtypes is not None and len(fn.argtypes) == 5


def test_a_plan_only_plan_raises_and_does_not_crash():
    spec = synthetic.wide_binary_tree(3, 6, 3)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], plan_only=True)
    with pytest.raises(_capi.JtpError):
        plan.map()


@pytest.mark.parametrize("with_evidence", [False, True], ids=["free", "evidence"])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_restatements_assignment_has_the_largest_joint_value(name, with_evidence):
    tree, pots, node_vars, sizes, n = SMALL[name]()
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    labels = sorted(sizes)
    evidence = None
    if with_evidence:                                        # two observed variables, states away from 0
        evidence = {labels[1]: sizes[labels[1]] - 1, labels[-1]: sizes[labels[-1]] // 2}
    states, log_value = map_reference(plan, pots, evidence)
    assert sorted(states) == labels
    for v, st in (evidence or {}).items():
        assert states[v] == st
    assert all(0 <= states[v] < sizes[v] for v in labels)
    got = value_of(pots[:n], node_vars[:n], states)
    want = brute_force(pots, node_vars, sizes, n, evidence)
    roundings = n + (n - 1)
    tol = roundings * 2.0 ** -52
    print("%s: value %.17g, brute force %.17g, relative difference %.3g (bound %.3g)" % (name, got, want, abs(got - want) / want, tol))
    assert want > 0 and abs(got - want) <= tol * want
    # log_value is the logarithm of that value: the bound above, and one log, one multiply and one add
    assert abs(log_value - np.log(want)) <= tol + 8 * 2.0 ** -53 * max(1.0, abs(np.log(want)))


def test_ties_go_to_the_smallest_r_and_impossible_evidence_fails():
    tree, pots, node_vars, sizes, n = SMALL["random8_card3"]()
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    ones = [np.ones_like(p) for p in pots]
    states, log_value = map_reference(plan, ones)
    assert all(st == 0 for st in states.values()) and log_value == 0.0
    v = sorted(sizes)[3]
    states, log_value = map_reference(plan, ones, {v: 1})
    assert states == {u: (1 if u == v else 0) for u in sizes} and log_value == 0.0
    zero = [np.array(p) for p in pots]
    c = next(c for c in range(n) if v in node_vars[c])
    zero[c][tuple(slice(1, 2) if u == v else slice(None) for u in node_vars[c])] = 0.0
    assert map_reference(plan, zero, {v: 1}) == (None, -np.inf)
    assert map_reference(plan, zero, {v: 0})[0] is not None
    negative = [np.array(p) for p in pots]
    negative[0].flat[0] = -1.0
    assert map_reference(plan, negative) == (None, -np.inf)
