"""Marginal MAP on the device (`jtp_marginal_map`: kernels `jt_mmap_level`, `jt_mmap_merge`, and jtp_map's where a clique sums nothing)
on a real MI355X, against the numpy restatement of the sweep (`tests/mmap_reference.py`) and against brute-force enumeration.

Every model is a small factor graph whose strong junction tree (`construction.strong_junction_tree`) is handed to `engine.Plan`
as it is; the clique tables are drawn per clique.  With integer tables every product and sum is exact, so the device's states
must EQUAL the restatement's, ties included, and `log_value` may differ by the one `log`, one multiply and one add that end it:
8 x 2^-53 x max(1, |log_value|), `test_gpu_map`'s bound.  With real tables device and numpy add the same terms in different orders:
the bound is `mmap_reference.parity_bound`, and states are compared where the best and the second-best query assignment lie more
than twice the bound apart."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

import junctiontree_amd as jt
from junctiontree_amd import _capi, engine
from mmap_reference import brute_force, mmap_reference, parity_bound, strong_model, two_best
from test_gpu_sample import LAYOUTS, README_FACTORS, README_SIZES, README_VALUES, variants_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


# ---------------------------------------------------------------------------------------------- models

def chain_model(seed, n_vars, cards, extra, keep=0.5):
    """variables 0 .. n_vars - 1 with cardinalities drawn from `cards`, a factor per neighbouring pair and `extra` factors over three
    variables at most four apart; about `keep` of the variables in the query"""
    rng = np.random.default_rng(seed)
    sizes = {v: int(cards[i % len(cards)]) for i, v in enumerate(range(n_vars))}
    factors = [[v, v + 1] for v in range(n_vars - 1)]
    for _ in range(extra):
        a = int(rng.integers(0, n_vars - 4))
        factors.append([a] + sorted(int(x) for x in a + 1 + rng.choice(4, size=2, replace=False)))
    query = [v for v in range(n_vars) if rng.random() < keep]
    return factors, sizes, query


MODELS = {
    "cards2356": lambda: chain_model(5, 11, (2, 3, 5, 6), 3),
    "cards6532": lambda: chain_model(8, 14, (6, 5, 3, 2, 3), 5, keep=0.4),
    "cards2356b": lambda: chain_model(4, 12, (2, 3, 5, 6), 6, keep=0.4),
}
_cases = {}


def case(name, query=None):
    """(tree, node_vars, sizes, number of cliques, query, parent list) of a model's strong tree; `query`: instead of the model's"""
    key = (name, None if query is None else tuple(query))
    if key not in _cases:
        factors, sizes, q = MODELS[name]()
        q = q if query is None else list(query)
        tree, node_vars, parent, maxcliques, _ = strong_model(factors, sizes, q)
        _cases[key] = (tree, node_vars, sizes, len(maxcliques), q, parent)
    return _cases[key]


def tables(cs, kind, seed, dtype="f64"):
    """clique tables in the numbers a plan of `dtype` holds: "int" small integers 1..4, "real" uniform in [0.5, 1.5)"""
    tree, node_vars, sizes, n, _, _ = cs
    rng = np.random.default_rng(seed)
    np_t = np.float32 if dtype == "f32" else np.float64
    shapes = [[sizes[v] for v in vs] for vs in node_vars[:n]]
    if kind == "int":
        return [rng.integers(1, 5, sh).astype(np_t) for sh in shapes]
    return [rng.uniform(0.5, 1.5, sh).astype(np_t) for sh in shapes]


def make(cs, pots, dtype="f64", n_batch=1, per_set=None, **opts):
    """a plan with its potentials staged and NOT propagated; `per_set[b]`: the tables of set b (plans whose sets own their tables)"""
    tree, node_vars, sizes, n, _, _ = cs
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, n_batch=n_batch, **opts)
    for b in range(n_batch if per_set is not None else 1):
        mine = per_set[b] if per_set is not None else pots
        for c in range(n):
            plan.set_potential(c, mine[c], batch=b)
    return plan


def probe_of(cs):
    return engine.Plan(cs[0], cs[1], cs[2], plan_only=True)


def row(states, query):
    return np.array([states[v] for v in query], dtype=np.int32)


def close_enough(got, want):
    return abs(got - want) <= 8 * 2.0 ** -53 * max(1.0, abs(want))


_refs = {}


def reference(name, kind, seed, dtype="f64", evidence=None):
    """(states row, log_value, brute-force table) computed once per case, shared by the tests that need it"""
    key = (name, kind, seed, dtype, tuple(sorted((evidence or {}).items())))
    if key not in _refs:
        cs = case(name)
        pots = tables(cs, kind, seed, dtype)
        states, value = mmap_reference(probe_of(cs), pots, cs[4], evidence)
        _refs[key] = (row(states, cs[4]), value, brute_force(cs[1][:cs[3]], pots, cs[2], cs[4], evidence))
    return _refs[key]


# ---------------------------------------------------------------------------------------------- 1. exact arithmetic, exact answer

def test_the_models_are_what_the_tests_need():
    """(CPU) 4 to 12 cliques; cardinalities 2, 3, 5 and 6; cliques that sum and maximise, that only sum, that only maximise; some plan
    stores mixed-radix rows with a split variable; an integer case has a tie at the maximum"""
    cards, kinds, split, mixed, tie = set(), set(), False, False, False
    for name in MODELS:
        cs = case(name)
        tree, node_vars, sizes, n, query, parent = cs
        assert 4 <= n <= 12, (name, n)
        assert 0 < len(query) < len(sizes)
        cards |= set(sizes.values())
        for c in range(n):
            own = set(node_vars[c]) - (set(node_vars[parent[c]]) if parent[c] >= 0 else set())
            kinds.add((bool(own & set(query)), bool(own - set(query))))
        for dtype in ("f64", "f32"):
            d = engine.Plan(tree, node_vars, sizes, dtype=dtype, plan_only=True).describe()
            split = split or any(p["split_var"] >= 0 for p in d["pack"])
            mixed = mixed or d["tmix"] == 1
        for seed in (1, 2):
            table = reference(name, "int", seed)[2]
            assert float(table.max()) < 2.0 ** 53
            tie = tie or int((table == table.max()).sum()) > 1
    assert {2, 3, 5, 6} <= cards
    assert {(True, True), (False, True), (True, False)} <= kinds
    assert split and mixed and tie


@pytest.mark.parametrize("name", list(MODELS))
def test_integer_tables_give_the_restatements_states_in_every_layout_and_type(name):
    cs = case(name)
    query = cs[4]
    variants = variants_of({"no_compact": dict(no_compact=True)})
    assert set(LAYOUTS) <= set(variants)
    for seed in (1, 2):
        want_states, want_value, table = reference(name, "int", seed)
        assert float(table[tuple(want_states)]) == float(table.max())      # (exact arithmetic: the restatement's answer IS a best one)
        assert abs(np.exp(want_value) - float(table.max())) <= 16 * 2.0 ** -53 * float(table.max()) * max(1.0, abs(want_value))
        for dtype in ("f64", "f32"):
            pots = tables(cs, "int", seed, dtype)
            for key, opts in variants.items():
                if seed == 2 and key.endswith("+level"):
                    continue                                               # (the launch mode of the propagate: once is enough)
                plan = make(cs, pots, dtype, **opts)
                states, value = plan.marginal_map(query)
                plan.close()
                assert states.dtype == np.int32 and states.shape == (1, len(query)) and value.shape == (1,)
                np.testing.assert_array_equal(states[0], want_states, err_msg="%s %s seed %d" % (key, dtype, seed))
                assert close_enough(value[0], want_value), (key, dtype, value[0], want_value)


# ---------------------------------------------------------------------------------------------- 2. real values

REAL_SEEDS = {"cards2356": 21, "cards6532": 22, "cards2356b": 24}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(MODELS))
def test_real_tables_agree_with_enumeration_to_the_bound(name, dtype):
    cs = case(name)
    query, seed = cs[4], REAL_SEEDS[name]
    bound = parity_bound(probe_of(cs), query)
    want_states, want_value, table = reference(name, "real", seed, dtype)
    best, second = (float(x) for x in two_best(table))
    assert best - second > 2 * bound * best, "seed %d of %s: the two best query assignments are too close to compare states" % (seed, name)
    plan = make(cs, tables(cs, "real", seed, dtype), dtype)
    states, value = plan.marginal_map(query)
    plan.close()
    at = float(table[tuple(states[0])])
    print("%s %s: exp(log_value) %.17g, enumeration %.17g, at the states %.17g, bound %.3g" % (name, dtype, np.exp(value[0]), best, at, bound))
    log_slack = 8 * 2.0 ** -53 * max(1.0, abs(value[0]))                    # (the log, multiply and add that end log_value, and this exp)
    assert abs(np.exp(value[0]) - best) <= (bound + log_slack) * best
    assert abs(at - best) <= bound * best
    np.testing.assert_array_equal(states[0], want_states)


# ---------------------------------------------------------------------------------------------- 3. the two ends

@pytest.mark.parametrize("kind", ["int", "real"])
def test_a_query_of_all_variables_is_map_bit_for_bit(kind):
    factors, sizes, _ = MODELS["cards2356"]()
    cs = case("cards2356", query=sorted(sizes))
    pots = tables(cs, kind, 5)
    plan = make(cs, pots, n_batch=3, share_potentials=True)
    plan.set_evidence({2: 1}, batch=1)
    plan.set_evidence({0: 0, 7: sizes[7] - 1}, batch=2)
    want_states, want_value = plan.map()
    states, value = plan.marginal_map(plan.var_labels)
    np.testing.assert_array_equal(states, want_states)
    np.testing.assert_array_equal(value, want_value)                       # bit for bit
    states, value = plan.marginal_map(list(reversed(plan.var_labels)))      # (the order of the query is the order of the columns)
    np.testing.assert_array_equal(states[:, ::-1], want_states)
    plan.close()
    if kind == "int":
        ones = [np.ones_like(p) for p in pots]                              # every assignment ties: the smallest r everywhere
        plan = make(cs, ones)
        states, value = plan.marginal_map(plan.var_labels)
        np.testing.assert_array_equal(states, plan.map()[0])
        assert np.all(states == 0) and value[0] == 0.0
        plan.close()


@pytest.mark.parametrize("name", ["cards2356", "cards2356b"])
def test_an_empty_query_gives_log_z(name):
    cs = case(name)
    pots = tables(cs, "real", 6)
    plan = make(cs, pots, n_batch=2, share_potentials=True)
    plan.set_evidence({1: 0, 4: 1}, batch=1)
    states, value = plan.marginal_map([])
    assert states.shape == (2, 0)
    plan.propagate()
    bound = parity_bound(probe_of(cs), [])
    for b in range(2):
        sign, log_z = plan.log_z(batch=b)
        print("%s set %d: log_value %.17g, log Z %.17g, bound %.3g" % (name, b, value[b], log_z, bound))
        assert sign == 1 and abs(value[b] - log_z) <= bound + 16 * 2.0 ** -53 * max(1.0, abs(log_z))     # (a relative bound on Z is an absolute one on log Z)
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. determinism

def test_results_do_not_depend_on_calls_knobs_layout_or_how_the_sets_hold_their_tables():
    cs = case("cards6532")
    query = cs[4]
    pots = tables(cs, "real", 31, "f32")                                    # float32 numbers in every plan: float64 and float32 storage hold the same
    sets = [{}, {query[0]: 1}, {1: 0, 5: 1}, {query[-1]: 0, 3: 1}, {}]
    want = None
    for key, opts in dict(variants_of({"no_compact": dict(no_compact=True)}), n_batch=dict(own_tables=True)).items():
        for dtype in ("f64", "f32"):
            mine = [p.astype(np.float64) for p in pots] if dtype == "f64" else pots
            if opts.get("own_tables"):
                plan = make(cs, None, dtype, n_batch=5, per_set=[mine] * 5)
            else:
                plan = make(cs, mine, dtype, n_batch=5, share_potentials=True, **opts)
            for b, obs in enumerate(sets):
                plan.set_evidence(obs, batch=b)
            got = plan.marginal_map(query)
            if want is None:
                want = got
                again = plan.marginal_map(query)                            # two calls
                np.testing.assert_array_equal(again[0], want[0])
                np.testing.assert_array_equal(again[1], want[1])
                for knob, values in (("map_chunk", (1, 3, 0)), ("map_seg", (1, 4, 0))):
                    for v in values:
                        plan.debug_set(knob, v)
                        other = plan.marginal_map(query)
                        np.testing.assert_array_equal(other[0], want[0], err_msg="%s = %d" % (knob, v))
                        np.testing.assert_array_equal(other[1], want[1], err_msg="%s = %d" % (knob, v))
                part = plan.marginal_map(query, 1, 4)
                np.testing.assert_array_equal(part[0], want[0][1:4])
                np.testing.assert_array_equal(part[1], want[1][1:4])
            plan.close()
            np.testing.assert_array_equal(got[0], want[0], err_msg="%s %s" % (key, dtype))
            np.testing.assert_array_equal(got[1], want[1], err_msg="%s %s" % (key, dtype))
    probe = probe_of(cs)
    for b, obs in enumerate(sets):                                          # ... and they are the right ones
        ref_states, ref_value = mmap_reference(probe, pots, query, obs)
        assert abs(want[1][b] - ref_value) <= parity_bound(probe, query) + 16 * 2.0 ** -53 * max(1.0, abs(ref_value))
        for lab, st in obs.items():
            if lab in query:
                assert want[0][b, query.index(lab)] == st


# ---------------------------------------------------------------------------------------------- 5. sum segments

@pytest.mark.parametrize("n_vars,n_query,seed", [(12, 1, 41), (13, 2, 43)])
def test_a_sum_cut_into_segments(n_vars, n_query, seed):
    """one clique of binary variables: Rs = 2^(n_vars - n_query) >= 2048, so every sum is cut into segments and jt_mmap_merge adds them"""
    sizes = {v: 2 for v in range(n_vars)}
    query = [5, 9][:n_query]
    tree, node_vars, parent, maxcliques, _ = strong_model([list(range(n_vars))], sizes, query)
    assert len(maxcliques) == 1
    cs = (tree, node_vars, sizes, 1, query, parent)
    rng = np.random.default_rng(seed)
    pots = [rng.uniform(0.5, 1.5, [2] * n_vars)]
    table = brute_force(node_vars[:1], pots, sizes, query)                 # (numpy's sum over the other axes, in extended precision)
    rs = 2 ** (n_vars - n_query)
    assert rs >= 2048 and rs // 1024 >= 2
    bound = parity_bound(probe_of(cs), query)
    assert bound == 4 * 2.0 ** -53 * (rs + 2)
    best, second = (float(x) for x in two_best(table))
    assert best - second > 2 * bound * best
    want_states, want_value = mmap_reference(probe_of(cs), pots, query)
    assert tuple(row(want_states, query)) == np.unravel_index(int(np.argmax(table)), table.shape)
    assert abs(np.exp(want_value) - best) <= (bound + 8 * 2.0 ** -53 * max(1.0, abs(want_value))) * best
    for dtype in ("f64", "f32"):
        plan = make(cs, [pots[0].astype(np.float32)] if dtype == "f32" else pots, dtype)
        states, value = plan.marginal_map(query)
        if dtype == "f64":
            print("%d variables, %d in the query: exp(log_value) %.17g, numpy %.17g, bound %.3g" % (n_vars, n_query, np.exp(value[0]), best, bound))
            assert abs(np.exp(value[0]) - best) <= (bound + 8 * 2.0 ** -53 * max(1.0, abs(value[0]))) * best
            np.testing.assert_array_equal(states[0], row(want_states, query))
            plan.set_evidence({0: 1, 5: 0})                                 # a summed variable sliced, a query variable observed
            states, value = plan.marginal_map(query)
            ref_states, ref_value = mmap_reference(probe_of(cs), pots, query, {0: 1, 5: 0})
            assert states[0, 0] == 0 and abs(value[0] - ref_value) <= bound + 16 * 2.0 ** -53 * max(1.0, abs(ref_value))
        else:                                                               # (float32 numbers: another table, the same path)
            ref_states, ref_value = mmap_reference(probe_of(cs), [pots[0].astype(np.float32)], query)
            assert abs(value[0] - ref_value) <= bound + 16 * 2.0 ** -53 * max(1.0, abs(ref_value))
        plan.close()


def test_a_sum_wider_than_a_wave_in_mixed_radix():
    """one clique of cardinalities 3, 5, 2, 3, 6, 2 with the first and the last variable in the query: Rs = 180, so each of the 64
    lanes walks a block of three entries across digit carries and the last lanes have none"""
    sizes = dict(enumerate((3, 5, 2, 3, 6, 2)))
    query = [5, 0]
    tree, node_vars, parent, maxcliques, _ = strong_model([list(sizes)], sizes, query)
    cs = (tree, node_vars, sizes, 1, query, parent)
    probe = probe_of(cs)
    bound = parity_bound(probe, query)
    assert bound == 4 * 2.0 ** -53 * (180 + 2)
    rng = np.random.default_rng(44)
    for kind, pots in (("int", [rng.integers(1, 5, [sizes[v] for v in node_vars[0]]).astype(np.float64)]), ("real", [rng.uniform(0.5, 1.5, [sizes[v] for v in node_vars[0]])])):
        table = brute_force(node_vars[:1], pots, sizes, query)
        best, second = (float(x) for x in two_best(table))
        want_states, want_value = mmap_reference(probe, pots, query)
        for evidence in ({}, {2: 1, 4: 5}):
            want_states, want_value = mmap_reference(probe, pots, query, evidence)
            plan = make(cs, pots)
            plan.set_evidence(evidence)
            states, value = plan.marginal_map(query)
            plan.close()
            if kind == "int":
                np.testing.assert_array_equal(states[0], row(want_states, query))
                assert close_enough(value[0], want_value)
            else:
                assert abs(value[0] - want_value) <= bound + 16 * 2.0 ** -53 * max(1.0, abs(want_value))
                if not evidence:
                    assert best - second > 2 * bound * best
                    np.testing.assert_array_equal(states[0], row(want_states, query))


# ---------------------------------------------------------------------------------------------- 6. evidence

def test_evidence_is_slicing():
    cs = case("cards2356")
    tree, node_vars, sizes, n, query, parent = cs
    summed = [v for v in sorted(sizes) if v not in query and sizes[v] > 1]
    pots = tables(cs, "int", 9)
    sets = [{query[1]: sizes[query[1]] - 1}, {summed[0]: 1}, {query[0]: 0, summed[-1]: 0, summed[1]: 1}]
    plan = make(cs, pots, n_batch=3, share_potentials=True)
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    states, value = plan.marginal_map(query)
    probe = probe_of(cs)
    for b, obs in enumerate(sets):
        for lab, st in obs.items():
            if lab in query:
                assert states[b, query.index(lab)] == st                    # an observed query variable comes out observed
        want_states, want_value = mmap_reference(probe, pots, query, obs)   # (integer tables: exact, so the states are the restatement's)
        np.testing.assert_array_equal(states[b], row(want_states, query), err_msg="set %d" % b)
        assert close_enough(value[b], want_value)
        table = brute_force(node_vars[:n], pots, sizes, query, obs)
        assert float(table[tuple(states[b])]) == float(table.max())
    # NaN and inf in entries that contradict the evidence change nothing, bit for bit
    poisoned = [np.array(p) for p in pots]
    for c in range(n):
        for lab, st in sets[2].items():
            if lab in node_vars[c]:
                idx = [slice(None)] * len(node_vars[c])
                for bad_state in range(sizes[lab]):
                    if bad_state != st:
                        idx[node_vars[c].index(lab)] = bad_state
                        poisoned[c][tuple(idx)] = np.nan if (c + bad_state) % 2 else np.inf
    assert any(not np.all(np.isfinite(p)) for p in poisoned)
    plan.close()
    plan = make(cs, poisoned)
    plan.set_evidence(sets[2])
    got_states, got_value = plan.marginal_map(query)
    np.testing.assert_array_equal(got_states[0], states[2])
    assert got_value[0] == value[2]
    plan.close()


def test_a_set_of_probability_zero_fails_among_healthy_ones():
    cs = case("cards2356b")
    tree, node_vars, sizes, n, query, parent = cs
    pots = tables(cs, "real", 12)
    home = next(c for c in range(n) if 0 in node_vars[c])
    idx = [slice(None)] * len(node_vars[home])
    idx[node_vars[home].index(0)] = 1
    pots[home][tuple(idx)] = 0.0                                            # variable 0 is never in state 1
    sets = [{3: 1}, {0: 1}, {}]
    plan = make(cs, pots, n_batch=3, share_potentials=True)
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    with pytest.raises(_capi.JtpError, match=r"1 of 3 evidence sets.*first set 1") as err:
        plan.marginal_map(query)
    states, value = err.value.states, err.value.log_value
    assert np.all(states[1] == -1) and value[1] == -np.inf
    assert mmap_reference(probe_of(cs), pots, query, sets[1]) == (None, -np.inf)
    for b in (0, 2):
        alone_states, alone_value = plan.marginal_map(query, b, b + 1)      # as if run alone
        np.testing.assert_array_equal(states[b], alone_states[0])
        assert value[b] == alone_value[0] and np.isfinite(value[b]) and states[b].min() >= 0
    plan.close()


# ---------------------------------------------------------------------------------------------- 7. depth

def test_a_deep_chain_beyond_float64_has_a_finite_log_value():
    """600 factors of 4 x 4 along a chain, every other variable in the query: the strong tree is a chain of 300 cliques (two factors
    and the summed variable between two query variables each), 299 deep.  Entries near 1e30 make every number that matters lie
    far outside float64's range - the value is about 1e18000 - so only the exponent arithmetic of the sweep is being checked here,
    against an evaluation in the log domain (log-sum-exp over the summed variable, then a Viterbi pass in logs): 1e-9 relative."""
    n_f = 600
    sizes = {v: 4 for v in range(n_f + 1)}
    factors = [[v, v + 1] for v in range(n_f)]
    query = list(range(0, n_f + 1, 2))
    tree, node_vars, parent, maxcliques, f2m = strong_model(factors, sizes, query)
    assert len(maxcliques) == 300 and all(len(c) == 3 for c in maxcliques)
    depth = [0] * 300
    order, par, _, _ = engine.flatten_tree(tree)
    for c in order:                                                         # (pre-order: a parent before its children)
        depth[c] = depth[par[c]] + 1 if par[c] >= 0 else 0
    assert max(depth) == 299
    rng = np.random.default_rng(17)
    values = [rng.uniform(0.5, 1.5, (4, 4)) * 1e30 for _ in range(n_f)]
    pots = []
    for c, vs in enumerate(maxcliques):
        members = [f for f in range(n_f) if f2m[f] == c]
        pots.append(jt.einsum([values[f] for f in members], [factors[f] for f in members], vs))
    cs = (tree, node_vars, sizes, 300, query, parent)
    plan = make(cs, pots)
    states, value = plan.marginal_map(query)
    plan.close()
    logs = [np.log(v) for v in values]
    score = np.zeros(4)
    for j in range(0, n_f, 2):                                              # g(m, m') = sum_s f(m, s) f'(s, m'), in logs
        pair = logs[j][:, :, None] + logs[j + 1][None, :, :]
        top = pair.max(axis=1)
        g = top + np.log(np.exp(pair - top[:, None, :]).sum(axis=1))
        score = (score[:, None] + g).max(axis=0)
    want = float(score.max())
    print("log_value %.17g, log-domain evaluation %.17g" % (value[0], want))
    assert np.isfinite(value[0]) and value[0] > 600 * np.log(0.5e30)
    assert abs(value[0] - want) <= 1e-9 * abs(want)
    assert states.min() >= 0 and states.max() < 4


# ---------------------------------------------------------------------------------------------- 8. refusals and errors

def live_bytes():
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().jtp_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def test_a_tree_that_is_not_strong_is_refused_before_any_device_work():
    node_vars = [["a", "s"], ["s", "m"], ["s"]]
    sizes = {"a": 2, "s": 3, "m": 2}
    plan = engine.Plan([0, (2, [1])], node_vars, sizes)
    rng = np.random.default_rng(2)
    for c in range(2):
        plan.set_potential(c, rng.uniform(0.5, 1.5, [sizes[v] for v in node_vars[c]]))
    ids = plan.var_id
    before = live_bytes()
    words = "the tree is not strong for this query: clique 1 maximises variable %d below variable %d, which is summed and shared with its parent clique 0" % (ids["m"], ids["s"])
    with pytest.raises(ValueError, match=words):
        plan.marginal_map(["a", "m"])
    assert live_bytes() == before
    states, value = plan.marginal_map(["a"])                                # the same tree is strong for these
    assert states.shape == (1, 1)
    states, value = plan.marginal_map(["m", "s", "a"])
    np.testing.assert_array_equal(states[0], plan.map()[0][0][[plan.var_labels.index(v) for v in ("m", "s", "a")]])
    plan.close()


def test_plans_without_every_table_refuse_in_maps_words_and_bad_queries_are_invalid():
    cs = case("cards2356")
    tree, node_vars, sizes, n, query, parent = cs
    pots = tables(cs, "real", 3)
    multi = engine.Plan(tree, node_vars, sizes, multiset=True, n_batch=8)
    for c in range(n):
        multi.set_potential(c, pots[c])
    with pytest.raises(_capi.UnsupportedStructure, match="jtp_marginal_map: a multi-set plan"):
        multi.marginal_map(query)
    multi.close()
    lean = engine.Plan(tree, node_vars, sizes, cover=[[] for _ in range(n)])
    assert lean.describe()["has_unit"] == 1
    with pytest.raises(_capi.UnsupportedStructure, match="keeps no table on the device: make the plan without `cover`"):
        lean.marginal_map(query)
    lean.close()
    plan = make(cs, pots)
    lib, handle = _capi.lib(), plan._handle
    out, value = np.zeros(4, dtype=np.int32), np.zeros(1)

    def call(ids, states=out, begin=0, end=1):
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        rc = lib.jtp_marginal_map(handle, begin, end, len(ids), C.cast(arr, C.c_void_p), None if states is None else states.ctypes.data_as(C.c_void_p),
                                  value.ctypes.data_as(C.c_void_p))
        return rc, lib.jtp_last_error().decode()

    before = live_bytes()
    assert call([0, 1, 0]) == (_capi.JTP_EINVAL, "jtp_marginal_map: variable 0 listed twice")
    assert call([0, len(sizes)])[0] == _capi.JTP_EINVAL and "out of range" in call([0, len(sizes)])[1]
    assert call([-1])[0] == _capi.JTP_EINVAL
    assert call([0], states=None) == (_capi.JTP_EINVAL, "null argument")
    assert call([0], begin=0, end=2)[0] == _capi.JTP_EINVAL and "bad batch range" in call([0], begin=0, end=2)[1]
    assert call([0], begin=0, end=0)[0] == _capi.JTP_EINVAL
    assert live_bytes() == before
    with pytest.raises(ValueError, match="listed twice"):
        plan.marginal_map([query[0], query[0]])
    with pytest.raises(ValueError, match="in no clique"):
        plan.marginal_map(["nobody"])
    plan.close()


# ---------------------------------------------------------------------------------------------- 9. side effects

@pytest.mark.parametrize("opts", [{}, dict(level_launches=True), dict(scaled=True)], ids=["flow", "level", "scaled"])
def test_marginal_map_leaves_beliefs_and_messages_alone(opts):
    cs = case("cards6532")
    tree, node_vars, sizes, n, query, parent = cs
    plan = make(cs, tables(cs, "real", 8), **opts)
    free, _ = plan.marginal_map(query)                                      # before any propagate: staged potentials are all it needs
    plan.set_evidence({query[0]: 1})
    plan.propagate()
    before = [plan.belief(node) for node in range(len(node_vars))]
    z = plan.log_z()
    observed, _ = plan.marginal_map(query)
    assert free.min() >= 0 and observed[0, 0] == 1
    for a, b in zip(before, [plan.belief(node) for node in range(len(node_vars))]):
        np.testing.assert_array_equal(a, b)
    assert plan.log_z() == z
    plan.propagate()                                                        # ... and the next propagate finds its messages as it left them
    for a, b in zip(before, [plan.belief(node) for node in range(len(node_vars))]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(plan.marginal_map(query)[0], observed)
    plan.close()


def test_the_first_call_survives_the_failure_of_each_of_its_allocations():
    gc.collect()
    cs = case("cards6532")
    query = cs[4]
    pots = tables(cs, "real", 8)
    fresh = make(cs, pots, n_batch=3, share_potentials=True)
    want = fresh.marginal_map(query)
    fresh.close()
    plan = make(cs, pots, n_batch=3, share_potentials=True)
    failed = 0
    for n in range(1, 16):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            got = plan.marginal_map(query, 0, 1)
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    assert failed == n - 1 and failed >= 5, (failed, n)        # records, their extensions, child lists, depth table, work area
    plan.debug_set("fail_alloc", 0)
    np.testing.assert_array_equal(got[0], want[0][:1])
    # the work area grows with the sets of a call: that allocation failing leaves the smaller one in place
    before = live_bytes()
    plan.debug_set("fail_alloc", 1)
    with pytest.raises(MemoryError):
        plan.marginal_map(query)
    assert live_bytes() == before
    plan.debug_set("fail_alloc", 0)
    got = plan.marginal_map(query)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    # another query (the empty one: every tree is strong for it): new records, the work area stays; their first allocation failing
    # leaves the old query's records in place
    before = live_bytes()
    plan.debug_set("fail_alloc", 1)
    with pytest.raises(MemoryError):
        plan.marginal_map([])
    assert live_bytes() == before
    plan.debug_set("fail_alloc", 0)
    np.testing.assert_array_equal(plan.marginal_map(query)[0], want[0])
    plan.close()


# ---------------------------------------------------------------------------------------------- 10. API

def test_junction_tree_marginal_map_on_the_readme_network():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    before = tree.propagate(README_VALUES)
    labels = sorted(README_SIZES)
    for k in range(1, len(labels) + 1):
        for query in itertools.combinations(labels, k):
            for evidence in (None, {"wet_grass": 1}):
                states, value = tree.marginal_map(README_VALUES, list(query), evidence=evidence)
                table = brute_force(README_FACTORS, README_VALUES, README_SIZES, list(query), evidence)
                best = float(table.max())
                assert sorted(states) == list(query) and all(isinstance(st, int) for st in states.values())
                for lab, st in (evidence or {}).items():
                    if lab in states:
                        assert states[lab] == st
                assert abs(float(table[tuple(states[v] for v in query)]) - best) <= 64 * 2.0 ** -53 * best      # values, not assignments
                assert abs(value - np.log(best)) <= 64 * 2.0 ** -53
    sets = [{}, {"wet_grass": 1}, {"cloudy": 0, "sprinkler": 1}]
    cols, values = tree.marginal_map_evidence_sets(README_VALUES, ["rain", "cloudy"], sets)
    assert list(cols) == ["rain", "cloudy"] and values.shape == (3,) and all(col.dtype == np.int32 and col.shape == (3,) for col in cols.values())
    for b, evidence in enumerate(sets):
        states, value = tree.marginal_map(README_VALUES, ["rain", "cloudy"], evidence=evidence)
        assert {lab: int(col[b]) for lab, col in cols.items()} == states and values[b] == value
    # the empty query: log Z
    states, value = tree.marginal_map(README_VALUES, [])
    tree.propagate(README_VALUES, normalize=True)
    assert states == {} and abs(value - tree.log_z) <= 64 * 2.0 ** -53
    with pytest.raises(ValueError, match="not a variable of the model"):
        tree.marginal_map(README_VALUES, ["snow"])
    with pytest.raises(ValueError, match="listed twice"):
        tree.marginal_map(README_VALUES, ["rain", "rain"])
    with pytest.raises(_capi.JtpError) as err:                                    # wet grass without sprinkler or rain: probability zero
        tree.marginal_map_evidence_sets(README_VALUES, ["cloudy"], [{}, {"sprinkler": 0, "rain": 0, "wet_grass": 1}])
    assert err.value.states["cloudy"][1] == -1 and err.value.states["cloudy"][0] >= 0 and err.value.log_value[1] == -np.inf
    for a, b in zip(before, tree.propagate(README_VALUES)):
        np.testing.assert_array_equal(a, b)


def test_one_state_variables_in_the_query_come_back_as_zero():
    factors = [["a", "t"], ["t", "b"], ["b", "u", "c"]]
    sizes = {"a": 3, "t": 1, "b": 2, "u": 1, "c": 3}
    rng = np.random.default_rng(4)
    values = [rng.uniform(0.5, 1.5, [sizes[v] for v in f]) for f in factors]
    tree = jt.create_junction_tree(factors, sizes)
    states, value = tree.marginal_map(values, ["t", "a", "u"])
    table = brute_force(factors, values, sizes, ["t", "a", "u"])
    assert states["t"] == 0 and states["u"] == 0 and states["a"] == int(np.argmax(table[0, :, 0]))
    assert abs(value - np.log(float(table.max()))) <= 64 * 2.0 ** -53
