"""The M most probable assignments (`jtp_map_best`), the part that needs no GPU: the entry point, and the numpy restatement of the
sweep (`tests/mbest_reference.py`) against brute-force enumeration on the models of `test_map_host.py`.

ASSIGNMENTS are compared here, in order.  That is fair only where the enumerated values are further apart than the two
computations can differ: a value of the sweep is one entry per clique multiplied through at most n - 1 message multiplications,
the enumeration rounds once per clique - (2n - 1) roundings of 2^-53 on either side, (2n - 1) x 2^-52 relative.  Every run asserts
that its 17 largest enumerated values are separated by more than twice that, so a change of seeds cannot hide a failure."""
import numpy as np
import pytest

from junctiontree_amd import _capi, engine, synthetic
from map_reference import map_reference
from mbest_reference import mbest_reference
from test_map_host import SMALL
from test_max_host import README_FACTORS, README_SIZES, README_VALUES, brute_force as readme_joint, readme_model


def joint_of(pots, node_vars, sizes, n, evidence):
    """(labels, the enumerated joint, -1 where an assignment contradicts the evidence)"""
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
    return labels, joint


def largest(labels, joint, count):
    """the `count` largest entries of the joint, best first: ([{label: state}], values)"""
    flat = joint.reshape(-1)
    order = np.argsort(-flat, kind="stable")[:count]
    digits = np.unravel_index(order, joint.shape)
    return [{lab: int(digits[i][j]) for i, lab in enumerate(labels)} for j in range(len(order))], flat[order]


def evidence_of(sizes, with_evidence):
    labels = sorted(sizes)                                   # two observed variables, states away from 0: test_map_host's
    return {labels[1]: sizes[labels[1]] - 1, labels[-1]: sizes[labels[-1]] // 2} if with_evidence else None


def test_jtp_map_best_is_exported_and_bound():
    assert "jtp_map_best" in _capi.SYMBOLS
    fn = _capi.lib().jtp_map_best
    assert fn.argtypes is not None and len(fn.argtypes) == 6


def test_a_plan_only_plan_raises_and_does_not_crash():
    spec = synthetic.wide_binary_tree(3, 6, 3)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], plan_only=True)
    with pytest.raises(_capi.JtpError):
        plan.map_best(4)


_runs = {}


def run(name, with_evidence):
    """the restatement with m = 16, once per (model, evidence)"""
    if (name, with_evidence) not in _runs:
        tree, pots, node_vars, sizes, n = SMALL[name]()
        plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
        evidence = evidence_of(sizes, with_evidence)
        _runs[name, with_evidence] = (plan, pots, node_vars, sizes, n, evidence, mbest_reference(plan, pots, 16, evidence, with_values=True))
    return _runs[name, with_evidence]


@pytest.mark.parametrize("with_evidence", [False, True], ids=["free", "evidence"])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_restatement_lists_the_sixteen_largest_of_the_enumerated_joint_in_order(name, with_evidence):
    plan, pots, node_vars, sizes, n, evidence, (solutions, values, products) = run(name, with_evidence)
    labels, joint = joint_of(pots, node_vars, sizes, n, evidence)
    want, want_values = largest(labels, joint, 17)
    tol = (2 * n - 1) * 2.0 ** -52
    gaps = (want_values[:-1] - want_values[1:]) / want_values[:-1]
    print("%s: smallest relative gap among the 17 largest values %.3g, bound %.3g" % (name, gaps.min(), tol))
    assert want_values[-1] > 0 and gaps.min() > 2 * tol
    assert len(solutions) == 16 and values.shape == (16,)
    for s in range(16):
        assert solutions[s] == want[s], "solution %d" % s
        assert abs(products[s] - want_values[s]) <= tol * want_values[s]
        # log_value is the logarithm of that value: the bound above, and one log, one multiply and one add
        assert abs(values[s] - np.log(want_values[s])) <= tol + 8 * 2.0 ** -53 * max(1.0, abs(np.log(want_values[s])))
        direct = float(joint[tuple(solutions[s][lab] for lab in labels)])
        assert direct == want_values[s]
    for v, st in (evidence or {}).items():
        assert all(sol[v] == st for sol in solutions)
    # forming every product of a fold's step, not only those with (a + 1) * (b + 1) <= 16, changes nothing
    full, full_values = mbest_reference(plan, pots, 16, evidence, all_pairs=True)
    assert full == solutions
    np.testing.assert_array_equal(full_values, values)


@pytest.mark.parametrize("with_evidence", [False, True], ids=["free", "evidence"])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_one_solution_is_map_references_and_three_are_the_head_of_sixteen(name, with_evidence):
    plan, pots, node_vars, sizes, n, evidence, (solutions, values, _) = run(name, with_evidence)
    one, one_value = mbest_reference(plan, pots, 1, evidence)
    states, log_value = map_reference(plan, pots, evidence)
    assert one == [states] and one_value[0] == log_value
    three, three_values = mbest_reference(plan, pots, 3, evidence)
    assert three == solutions[:3]
    np.testing.assert_array_equal(three_values, values[:3])


def test_ties_come_out_in_the_order_of_the_definition():
    tree, pots, node_vars, sizes, n = SMALL["random8_card3"]()
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    ones = [np.ones_like(p) for p in pots]
    solutions, values = mbest_reference(plan, ones, 4)
    assert len(solutions) == 4 and np.all(values == 0.0)
    assert all(st == 0 for st in solutions[0].values())
    assert len({tuple(sorted(sol.items())) for sol in solutions}) == 4
    assert solutions[0] == map_reference(plan, ones)[0]


def test_fewer_assignments_of_positive_value_than_asked_for():
    tree, pots, node_vars, sizes, n, factors, values = readme_model()
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    evidence = {"sprinkler": 0, "rain": 0}
    labels, joint = readme_joint(README_FACTORS, README_SIZES, README_VALUES, evidence)
    assert np.count_nonzero(joint > 0) == 2                  # wet_grass = 1 has value 0 there
    solutions, log_values = mbest_reference(plan, pots, 4, evidence)
    assert len(solutions) == 2 and log_values.shape == (2,)
    want, want_values = largest(labels, joint, 2)
    assert solutions == want
    assert all(sol["wet_grass"] == 0 for sol in solutions)
    np.testing.assert_allclose(np.exp(log_values), want_values, rtol=16 * 2.0 ** -52, atol=0)
    assert mbest_reference(plan, pots, 4, {"sprinkler": 0, "rain": 0, "wet_grass": 1}) == (None, None)
