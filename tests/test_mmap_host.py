"""Host side of marginal MAP: the strong junction tree (`construction.strong_junction_tree`, `construction.is_strong`) and the numpy
restatement of the sweep (`tests/mmap_reference.py`) against brute-force enumeration.  No GPU: plans are made `plan_only`."""
import numpy as np
import pytest

from junctiontree_amd import construction, engine
from map_reference import map_reference
from mmap_reference import brute_force, is_rip, mmap_reference, parity_bound, strong_model


def random_model(seed):
    """a factor graph of at most 10 variables of cardinality 1 to 4, and a query: empty for seed 0, everything for seed 1"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(3, 11))
    sizes = {"v%d" % i: int(rng.integers(1, 5)) for i in range(n)}
    names = list(sizes)
    factors = [[names[i]] for i in range(n)]                               # (every variable is in a factor)
    for _ in range(int(rng.integers(n - 1, 2 * n))):
        factors.append([names[i] for i in rng.choice(n, size=int(rng.integers(2, 4)), replace=False)])
    if seed == 0:
        query = []
    elif seed == 1:
        query = list(names)
    else:
        query = [v for v in names if rng.random() < 0.5]
    return factors, sizes, query


MODELS = [random_model(seed) for seed in range(30)]


def clique_tables(rng, maxcliques, sizes, low=0.5, high=1.5):
    return [rng.uniform(low, high, [sizes[v] for v in vs]) for vs in maxcliques]


@pytest.mark.parametrize("seed", range(30))
def test_the_strong_tree_is_strong_and_a_junction_tree(seed):
    factors, sizes, query = MODELS[seed]
    tree, node_vars, parent, maxcliques, f2m = strong_model(factors, sizes, query)
    assert parent.count(-1) == 1
    assert construction.is_strong(parent, maxcliques, query)
    assert is_rip(parent, maxcliques)
    for f, c in zip(factors, f2m):
        assert set(f) <= set(maxcliques[c])
    for c, p in enumerate(parent):                                          # (no clique left inside its parent or its child)
        assert p < 0 or not (set(maxcliques[c]) <= set(maxcliques[p]) or set(maxcliques[p]) <= set(maxcliques[c]))
    assert set().union(*map(set, maxcliques)) == set(sizes)
    order, _, parent_sep, _ = engine.flatten_tree(tree)
    for c in order:
        if parent[c] >= 0:
            assert set(node_vars[parent_sep[c]]) == set(maxcliques[c]) & set(maxcliques[parent[c]])


def test_queries_cover_both_ends():
    assert MODELS[0][2] == [] and set(MODELS[1][2]) == set(MODELS[1][1])
    assert any(0 < len(q) < len(s) for _, s, q in MODELS)


def test_is_strong_rejects_a_tree_that_maximises_below_a_summed_separator():
    node_vars = [["a", "s"], ["s", "m"]]                                    # the child maximises m and shares the summed s with its parent
    assert not construction.is_strong([-1, 0], node_vars, ["a", "m"])
    assert construction.is_strong([-1, 0], node_vars, ["a", "s", "m"])      # (s maximised too: a plain MAP)
    assert construction.is_strong([-1, 0], node_vars, ["a"])                # (the child only sums)
    assert construction.is_strong([-1, 0], node_vars, [])
    assert construction.is_strong([1, -1], node_vars, ["m"])                # (hung from the other end: m is the root's)
    assert not construction.is_strong([1, -1], node_vars, ["a"])


@pytest.mark.parametrize("seed", range(30))
def test_the_restatement_agrees_with_enumeration(seed):
    factors, sizes, query = MODELS[seed]
    tree, node_vars, parent, maxcliques, _ = strong_model(factors, sizes, query)
    rng = np.random.default_rng(seed)
    pots = clique_tables(rng, maxcliques, sizes)
    probe = engine.Plan(tree, node_vars, sizes, plan_only=True)
    evidence = {}
    if seed % 3 == 2:                                                       # one observed variable, in or outside the query
        lab = sorted(sizes)[seed % len(sizes)]
        evidence = {lab: sizes[lab] - 1}
    states, log_value = mmap_reference(probe, pots, query, evidence)
    table = brute_force(maxcliques, pots, sizes, query, evidence)
    bound = parity_bound(probe, query)
    best = float(table.max())
    print("seed %d: %d cliques, query %d of %d, value %.17g, enumeration %.17g, bound %.3g" % (seed, len(maxcliques), len(query), len(sizes), np.exp(log_value), best, bound))
    assert sorted(states) == sorted(query)
    for lab, st in evidence.items():
        if lab in states:
            assert states[lab] == st
    assert abs(np.exp(log_value) - best) <= (bound + 8 * 2.0 ** -53 * max(1.0, abs(log_value))) * best
    at = float(table[tuple(states[v] for v in query)])
    assert abs(at - best) <= bound * best


@pytest.mark.parametrize("seed", [1, 4, 9])
def test_with_every_variable_in_the_query_the_restatement_is_map_reference(seed):
    factors, sizes, _ = MODELS[seed]
    query = list(sizes)
    tree, node_vars, parent, maxcliques, _ = strong_model(factors, sizes, query)
    rng = np.random.default_rng(50 + seed)
    ties = [rng.integers(1, 3, [sizes[v] for v in vs]).astype(np.float64) for vs in maxcliques]
    probe = engine.Plan(tree, node_vars, sizes, plan_only=True)
    for pots in (clique_tables(rng, maxcliques, sizes), ties):
        assert mmap_reference(probe, pots, query) == map_reference(probe, pots)
        lab = sorted(sizes)[0]
        assert mmap_reference(probe, pots, query, {lab: 0}) == map_reference(probe, pots, {lab: 0})


def test_a_failed_set_has_no_states():
    factors, sizes, query = MODELS[5]
    tree, node_vars, parent, maxcliques, _ = strong_model(factors, sizes, query)
    pots = [np.zeros([sizes[v] for v in vs]) for vs in maxcliques]
    probe = engine.Plan(tree, node_vars, sizes, plan_only=True)
    assert mmap_reference(probe, pots, query) == (None, -np.inf)
