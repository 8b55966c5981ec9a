"""Expected counts (`jtp_accumulate_marginals`), the part that needs no GPU: the reference the device tests compare with
(`tests/counts_reference.py`) against a brute-force joint, the entry point, and the arguments that are refused before any device work."""
import numpy as np
import pytest

import junctiontree_amd as jt
from counts_reference import bruteforce_counts, expected_counts_reference
from junctiontree_amd import _capi, engine, synthetic


def _requests(spec, rng):
    out = []
    for c in range(spec["n_cliques"]):
        labels = list(spec["node_vars"][c])
        out.append((c, [labels[int(rng.integers(0, len(labels)))]]))
        out.append((c, labels[:2][::-1]))
    out.append((0, []))
    out.append((1, list(spec["node_vars"][1])))
    return out


def _evidence_sets(spec, n_sets, seed):
    labels = sorted(spec["sizes"])
    sets = []
    for b in range(n_sets):
        rng = np.random.default_rng(seed + b)
        k = min(len(labels), b % 4)
        sets.append({labels[i]: int(rng.integers(0, spec["sizes"][labels[i]])) for i in rng.choice(len(labels), size=k, replace=False)})
    return sets


SPECS = {"card 3": lambda: synthetic.random_tree(n_cliques=5, width=4, sep=2, card=3, seed=3),
         "binary": lambda: synthetic.wide_binary_tree(n_cliques=4, width=5, sep=3, card=2, seed=5)}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_the_reference_matches_a_bruteforce_joint(name):
    spec = SPECS[name]()
    assert len(spec["sizes"]) <= 12
    pots = synthetic.potentials_for(spec, seed=2)
    rng = np.random.default_rng(1)
    requests, sets = _requests(spec, rng), _evidence_sets(spec, 7, 40)
    weights = rng.uniform(0.5, 2.0, len(sets))
    got, log_z = expected_counts_reference(spec, pots, requests, sets, weights)
    want, want_log_z = bruteforce_counts(spec, pots, requests, sets, weights)
    for (c, labels), g, w in zip(requests, got, want):
        assert g.shape == tuple(spec["sizes"][v] for v in labels)
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=0.0, err_msg="clique %d labels %r" % (c, labels))
        np.testing.assert_allclose(g.sum(), weights.sum(), rtol=1e-12)       # (every set adds a table that sums to its weight)
    np.testing.assert_allclose(log_z, want_log_z, rtol=0.0, atol=1e-12)


def test_a_set_of_weight_zero_contributes_nothing_to_the_reference():
    spec = SPECS["card 3"]()
    pots = synthetic.potentials_for(spec, seed=2)
    rng = np.random.default_rng(2)
    requests, sets = _requests(spec, rng), _evidence_sets(spec, 5, 60)
    weights = np.array([1.0, 0.0, 2.0, 0.0, 0.5])
    got, log_z = expected_counts_reference(spec, pots, requests, sets, weights)
    kept = [0, 2, 4]
    want, kept_log_z = expected_counts_reference(spec, pots, requests, [sets[i] for i in kept], weights[kept])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(log_z[kept], kept_log_z) and np.isfinite(log_z).all()     # (log Z is reported whatever the weight)


def test_jtp_accumulate_marginals_is_exported_and_bound():
    assert "jtp_accumulate_marginals" in _capi.SYMBOLS
    fn = _capi.lib().jtp_accumulate_marginals
    assert len(fn.argtypes) == 12
    for name in ("accumulate_marginals", "factor_counts"):
        assert callable(getattr(engine.Plan, name))
    assert callable(jt.JunctionTree.expected_counts)


def _plan_only(spec, **opts):
    return engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], plan_only=True, **opts)


def test_a_plan_only_plan_raises_from_accumulate_marginals():
    spec = synthetic.wide_binary_tree(3, 6, 3)
    plan = _plan_only(spec, n_batch=2, share_potentials=True)
    with pytest.raises(_capi.JtpError, match="JTP_PLAN_ONLY"):
        plan.accumulate_marginals([(0, spec["node_vars"][0][:2])])
    plan.close()


def test_plans_of_several_ranks_are_refused():
    spec = synthetic.wide_binary_tree(n_cliques=7, width=6, sep=3)
    plan = _plan_only(spec, n_ranks=2, rank=0, owner=[0, 0, 1, 0, 0, 1, 1])
    with pytest.raises(_capi.UnsupportedStructure, match="ranks"):
        plan.accumulate_marginals([(0, spec["node_vars"][0][:2])])
    plan.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_weights_that_are_not_finite_are_refused_before_any_device_work(bad):
    spec = synthetic.wide_binary_tree(3, 6, 3)
    plan = _plan_only(spec, n_batch=2, share_potentials=True)
    with pytest.raises(ValueError, match="finite"):
        plan.accumulate_marginals([(0, spec["node_vars"][0][:2])], weights=[1.0, bad])
    with pytest.raises(ValueError, match="2 evidence sets"):
        plan.accumulate_marginals([(0, spec["node_vars"][0][:2])], weights=[1.0])
    plan.close()
    tree = jt.create_junction_tree([["a"], ["a", "b"]], {"a": 2, "b": 3})
    values = [np.array([0.5, 0.5]), np.ones((2, 3))]
    with pytest.raises(ValueError, match="finite"):                  # (no plan is made: this runs without a device)
        tree.expected_counts(values, [{}, {"b": 1}], weights=[bad, 1.0])
    with pytest.raises(ValueError, match="weights"):
        tree.expected_counts(values, [{}, {"b": 1}], weights=[1.0])


def test_no_evidence_sets_give_zero_arrays_without_a_device():
    tree = jt.create_junction_tree([["a"], ["a", "b"]], {"a": 2, "b": 3})
    values = [np.array([0.5, 0.5]), np.ones((2, 3), dtype=np.float32)]
    out = tree.expected_counts(values, [])
    assert [o.shape for o in out] == [(2,), (2, 3)] and all(o.dtype == np.float64 and not o.any() for o in out)
    assert len(tree.log_z_sets) == 0
