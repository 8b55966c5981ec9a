"""Joints over variables of different cliques (`jtp_joint`), the part that needs no GPU: the numpy restatement of the definition
(`tests/joint_reference.py`) applied to the oracle's beliefs equals the brute-force joint, and `JunctionTree.joint` refuses bad
variable lists before any device work."""
import numpy as np
import pytest

import jt_oracle as oracle
import junctiontree_amd as jt
from joint_reference import brute_force_joint, joint_reference, parity_bound
from junctiontree_amd import _capi, engine, synthetic
from sample_reference import schedule

README_FACTORS = [["cloudy"], ["cloudy", "sprinkler"], ["cloudy", "rain"], ["rain", "sprinkler", "wet_grass"]]
README_SIZES = {"cloudy": 2, "sprinkler": 2, "rain": 2, "wet_grass": 2}
README_VALUES = [np.array([0.5, 0.5]), np.array([[0.5, 0.5], [0.9, 0.1]]), np.array([[0.8, 0.2], [0.2, 0.8]]),
                 np.array([[[1, 0], [0.1, 0.9]], [[0.1, 0.9], [0.01, 0.99]]])]


def with_evidence(pots, node_vars, n_cliques, evidence):
    """the clique potentials with the entries that contradict the evidence zeroed (in one clique per observed variable)"""
    pots = [np.array(p, dtype=np.float64) for p in pots]
    for lab, st in (evidence or {}).items():
        c = next(c for c in range(n_cliques) if lab in node_vars[c])
        mask = np.zeros(pots[c].shape[node_vars[c].index(lab)])
        mask[st] = 1.0
        shape = [1] * pots[c].ndim
        shape[node_vars[c].index(lab)] = len(mask)
        pots[c] = pots[c] * mask.reshape(shape)
    return pots


def readme_case():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    ct = tree.clique_tree
    cliques = [list(c) for c in ct.maxcliques]
    node_vars = cliques + [list(s) for s in tree.separators]
    psi = oracle.evaluate(README_FACTORS, ct.factor_to_maxclique, cliques, README_VALUES)
    pots = [np.broadcast_to(p, [README_SIZES[v] for v in c]).copy() for p, c in zip(psi, cliques)] + [np.ones([README_SIZES[v] for v in s]) for s in tree.separators]
    return tree.tree, pots, node_vars, README_SIZES, len(cliques), README_FACTORS, README_VALUES


def chain_case():
    spec = synthetic.chain_tree(3, card=2, width=3)
    pots = synthetic.potentials_for(spec, seed=7)
    n = spec["n_cliques"]
    return spec["tree"], pots, spec["node_vars"], spec["sizes"], n, spec["node_vars"][:n], pots[:n]


RUNS = [("readme", None, ["cloudy", "wet_grass"]), ("readme", None, ["wet_grass", "cloudy"]), ("readme", None, ["sprinkler", "rain"]),
        ("readme", None, ["wet_grass", "rain", "cloudy", "sprinkler"]), ("readme", {"wet_grass": 1}, ["cloudy", "wet_grass"]),
        ("readme", {"wet_grass": 1}, ["sprinkler", "rain"]), ("readme", {"rain": 0}, ["cloudy", "wet_grass"]),
        ("chain", None, [0, 4]), ("chain", None, [4, 0]), ("chain", None, [4, 1, 0]), ("chain", None, [1, 2]), ("chain", None, [3]),
        ("chain", None, [3, 4]), ("chain", {2: 1}, [0, 4]), ("chain", {2: 1}, [4, 2, 0]), ("chain", {4: 0}, [1, 2])]


@pytest.mark.parametrize("name,evidence,query", RUNS, ids=["%s-%s-%s" % (n, "ev" if e else "free", "_".join(map(str, q))) for n, e, q in RUNS])
def test_the_restatement_on_the_oracles_beliefs_is_the_brute_force_joint(name, evidence, query):
    tree, pots, node_vars, sizes, n, factors, values = readme_case() if name == "readme" else chain_case()
    beliefs = oracle.beliefs_exact(tree, with_evidence(pots, node_vars, n, evidence), node_vars)
    plan = engine.Plan(tree, node_vars, sizes, plan_only=True)
    got, report = joint_reference({c: beliefs[c] for c in range(n)}, schedule(plan), query, node_vars)
    want = brute_force_joint(factors, sizes, values, evidence, query)
    assert got.shape == want.shape == tuple(sizes[v] for v in query)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0)
    assert np.all((got == 0.0) == (want == 0.0))
    for lab, st in (evidence or {}).items():               # zero off an observed state
        if lab in query:
            off = np.delete(got, st, axis=query.index(lab))
            assert np.all(off == 0.0) and got.sum() > 0.0
    # what the report says of the active set
    cliques = [r[0] for r in report]
    assert len(set(cliques)) == len(cliques) and all(1 <= rp <= r or c == cliques[0] for c, r, rp, m in report)
    shared = any(all(v in node_vars[c] for v in query) for c in range(n))
    homes = {next(c for c, _, _, _, F, _ in schedule(plan) if v in F) for v in query}
    if len(homes) == 1:
        assert len(report) == 1 and report[0][3] == 0          # one clique: its marginal
    assert sum(m for _, _, _, m in report) == len(report) - 1  # every active clique but the top is some active clique's child
    assert parity_bound(report) < 1e-12 and (shared or len(report) > 1)


def test_junction_tree_joint_refuses_bad_variable_lists_before_any_device_work():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    with pytest.raises(ValueError, match="not a variable"):
        tree.joint(README_VALUES, ["cloudy", "snow"])
    with pytest.raises(ValueError, match="twice"):
        tree.joint(README_VALUES, ["cloudy", "rain", "cloudy"])
    with pytest.raises(ValueError, match="at least one"):
        tree.joint(README_VALUES, [])
    assert not any(k.startswith("plan") for k in tree._memo)       # (no plan was made)


def test_jtp_joint_is_exported_and_bound_and_plan_only_plans_raise():
    assert "jtp_joint" in _capi.SYMBOLS
    fn = _capi.lib().jtp_joint
    assert fn.argtypes is not None and len(fn.argtypes) == 6
    spec = synthetic.wide_binary_tree(3, 6, 3)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], plan_only=True)
    with pytest.raises(_capi.JtpError):
        plan.joint([0, 1])
    with pytest.raises(ValueError, match="twice"):
        plan.joint([0, 0])
    with pytest.raises(ValueError, match="no clique"):
        plan.joint([0, "nobody"])
