"""The most probable assignment on the device (`jtp_map`: kernels `jt_map_collect_level`, `jt_map_merge`, `jt_map_decode`) on a real
MI355X, against the numpy restatement of the sweep (`tests/map_reference.py`).

The definition is made of single IEEE operations in a fixed order, so the device's states must EQUAL the restatement's, ties
included, for float64 and for float32 tables (float32 potentials are drawn as float32 and widened); `log_value` may differ by the
one `log`, one multiply and one add that end it: 8 x 2^-53 x max(1, |log_value|)."""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import junctiontree_amd as jt
from junctiontree_amd import _capi, engine, synthetic
from map_reference import map_reference, states_row, value_of
from sample_reference import schedule
from test_gpu_sample import LAYOUTS, README_FACTORS, README_SIZES, README_VALUES, case_of, spec_case, star_case

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = star_case(12) if name == "star12" else case_of(name)
    return _cases[name]


def tables(cs, dtype, seed=None):
    """the case's clique tables in the numbers a plan of `dtype` holds (float32: drawn as float32), separators all ones"""
    tree, pots, node_vars, sizes, n = cs
    if seed is not None:
        rng = np.random.default_rng(seed)
        pots = [rng.uniform(0.5, 1.5, np.shape(p)) if c < n else p for c, p in enumerate(pots)]
    np_t = np.float32 if dtype == "f32" else np.float64
    return [np.asarray(p, dtype=np_t) for p in pots]


def make(cs, dtype="f64", pots=None, n_batch=1, per_set=None, **opts):
    """a plan with its potentials staged and NOT propagated; `per_set[b]`: the tables of set b (plans whose sets own their tables)"""
    tree, _, node_vars, sizes, n = cs
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, n_batch=n_batch, **opts)
    for b in range(n_batch if per_set is not None else 1):
        mine = per_set[b] if per_set is not None else (tables(cs, dtype) if pots is None else pots)
        for c in range(n):
            plan.set_potential(c, mine[c], batch=b)
    return plan


def close_enough(got, want):
    return abs(got - want) <= 8 * 2.0 ** -53 * max(1.0, abs(want))


_refs = {}


def reference(name, dtype):
    """computed once per (case, number format), shared by the tests that need it"""
    if (name, dtype) not in _refs:
        cs = case(name)
        probe = engine.Plan(cs[0], cs[2], cs[3], plan_only=True)
        states, value = map_reference(probe, tables(cs, dtype))
        _refs[name, dtype] = (states_row(probe, states), value)
    return _refs[name, dtype]


# ---------------------------------------------------------------------------------------------- 1. exact match

NAMES = ["random16_card3", "random16_card5", "random16_card6", "random16_card7", "contained", "root64k", "chain6", "star5", "star12"]
RUNS = [(n, d, {}) for n in NAMES for d in ("f64", "f32")] + [("random16_card3", "f64", dict(no_compact=True)), ("random16_card5", "f32", dict(no_compact=True)),
                                                              ("random16_card6", "f64", dict(no_compact=True)), ("random16_card7", "f32", dict(no_compact=True))]


@pytest.mark.parametrize("name,dtype,opts", RUNS, ids=["%s-%s%s" % (n, d, "-no_compact" if o else "") for n, d, o in RUNS])
def test_states_equal_the_restatements(name, dtype, opts):
    cs = case(name)
    plan = make(cs, dtype, **opts)
    sched = plan.describe()["sample"]["cliques"]
    if name == "contained":
        assert sorted(c["R"] for c in sched)[:2] == [1, 1]
    if name == "root64k":
        assert max(c["R"] for c in sched) == 1 << 16                    # (cut into segments: jt_map_merge runs)
    if name == "star12":
        assert sum(1 for c in sched if c["parent"] == sched[0]["clique"]) == 12
    if name.startswith("random16") and not opts:
        assert plan.describe()["compact"] == 1
    states, value = plan.map()
    want_states, want_value = reference(name, dtype)
    assert states.dtype == np.int32 and states.shape == (1, len(plan.var_labels)) and value.shape == (1,)
    np.testing.assert_array_equal(states[0], want_states)
    print("%s %s: log_value %.17g, restatement %.17g" % (name, dtype, value[0], want_value))
    assert close_enough(value[0], want_value)
    # the value is that of the assignment returned: the product of the entries, one rounding per clique and message
    tabs = tables(cs, dtype)
    direct = value_of(tabs[:cs[4]], cs[2][:cs[4]], dict(zip(plan.var_labels, states[0])))
    assert abs(value[0] - np.log(direct)) <= 2 * cs[4] * 2.0 ** -52 + 8 * 2.0 ** -53 * max(1.0, abs(value[0]))
    plan.close()


# ---------------------------------------------------------------------------------------------- 2. layout independence

@pytest.mark.parametrize("name", ["wide7", "random16_card6"])
def test_equal_potentials_give_equal_states_in_every_layout(name):
    """float32 numbers in every plan, so that float64 and float32 storage hold the same potentials"""
    cs = case(name)
    pots32 = tables(cs, "f32")
    want, want_value = None, None
    variants = dict(LAYOUTS, no_compact=dict(no_compact=True), no_compact_keep_root=dict(no_compact=True, keep_root=True), policy1_no_compact=dict(no_compact=True, layout_policy=1))
    for key, opts in variants.items():
        for dtype in ("f64", "f32"):
            plan = make(cs, dtype, pots=[p.astype(np.float64) for p in pots32] if dtype == "f64" else pots32, **opts)
            order = [plan.var_labels.index(lab) for lab in sorted(plan.var_labels)]
            states, value = plan.map()
            plan.close()
            if want is None:
                want, want_value = states[0, order], value[0]
            np.testing.assert_array_equal(states[0, order], want, err_msg="%s %s" % (key, dtype))
            assert value[0] == want_value, (key, dtype)


# ---------------------------------------------------------------------------------------------- 3. ties

def test_ties_go_to_the_smallest_r():
    cs = case("random16_card5")
    tree, _, node_vars, sizes, n = cs
    ones = [np.ones(np.shape(p)) for p in cs[1]]
    plan = make(cs, "f64", pots=ones)
    states, value = plan.map()
    assert np.all(states == 0) and value[0] == 0.0
    v = sorted(sizes)[7]
    plan.set_evidence({v: 1})
    states, value = plan.map()
    want = np.zeros(len(plan.var_labels), dtype=np.int32)
    want[plan.var_labels.index(v)] = 1
    np.testing.assert_array_equal(states[0], want)
    assert value[0] == 0.0
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. evidence sets

def five_sets(cs):
    probe = engine.Plan(cs[0], cs[2], cs[3], plan_only=True)
    sched = schedule(probe)
    parents = {s[1] for s in sched}
    leaf = next(s for s in reversed(sched) if s[0] not in parents and s[4])
    in_k = sorted({v for s in sched for v in s[3]})
    sizes = cs[3]
    return probe, [{leaf[4][-1]: sizes[leaf[4][-1]] - 1}, {}, {in_k[0]: 1, leaf[4][0]: 0}, {in_k[-1]: sizes[in_k[-1]] - 1}, {in_k[1]: 0, in_k[2]: 1, sched[0][4][0]: 1}]


@pytest.mark.parametrize("kind", ["share_potentials", "n_batch"])
@pytest.mark.parametrize("name,dtype", [("random16_card3", "f64"), ("wide7", "f32")])
def test_evidence_sets_go_through_the_same_launches(name, dtype, kind):
    cs = case(name)
    probe, sets = five_sets(cs)
    if kind == "share_potentials":
        per_set = None
        plan = make(cs, dtype, n_batch=5, share_potentials=True)
        tabs = [tables(cs, dtype)] * 5
    else:
        tabs = [tables(cs, dtype, seed=40 + b) for b in range(5)]            # distinct tables per set
        plan = make(cs, dtype, n_batch=5, per_set=tabs)
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    states, value = plan.map()
    assert states.shape == (5, len(plan.var_labels)) and value.shape == (5,)
    col = {lab: j for j, lab in enumerate(plan.var_labels)}
    for b, obs in enumerate(sets):
        for lab, st in obs.items():
            assert states[b, col[lab]] == st
        want_states, want_value = map_reference(probe, tabs[b], obs)
        np.testing.assert_array_equal(states[b], states_row(plan, want_states), err_msg="set %d" % b)
        assert close_enough(value[b], want_value)
        one_states, one_value = plan.map(b, b + 1)                                # a one-set call per set: the same row
        np.testing.assert_array_equal(one_states[0], states[b])
        assert one_value[0] == value[b]
    part_states, part_value = plan.map(1, 4)
    np.testing.assert_array_equal(part_states, states[1:4])
    np.testing.assert_array_equal(part_value, value[1:4])
    plan.debug_set("map_chunk", 2)                                                # three chunks: 2 + 2 + 1 sets
    chunk_states, chunk_value = plan.map()
    np.testing.assert_array_equal(chunk_states, states)
    np.testing.assert_array_equal(chunk_value, value)
    plan.close()


# ---------------------------------------------------------------------------------------------- 5. overflow

def test_a_chain_whose_z_is_beyond_float64_has_a_finite_log_value():
    spec = synthetic.chain_tree(300, card=3, width=3)
    cs = spec_case(spec)
    tree, pots, node_vars, sizes, n = cs
    rng = np.random.default_rng(17)
    big = [rng.uniform(0.5, 1.5, np.shape(p)) * 1e30 if c < n else p for c, p in enumerate(pots)]      # Z is about 1e9000
    plan = make(cs, "f64", pots=big)
    states, value = plan.map()
    want_states, want_value = map_reference(plan, big)
    assert np.isfinite(value[0]) and value[0] > 300 * np.log(0.5e30)
    np.testing.assert_array_equal(states[0], states_row(plan, want_states))
    assert close_enough(value[0], want_value)
    plan.close()


# ---------------------------------------------------------------------------------------------- 6. failure

def test_a_set_of_probability_zero_fails_among_healthy_ones():
    spec = synthetic.chain_tree(4, card=3, width=3)
    cs = spec_case(spec, seed=3)
    tree, pots, node_vars, sizes, n = cs
    pots = [np.array(p) for p in pots]
    pots[0][2, :, :] = 0.0                                   # variable 0 is never in state 2
    plan = make(cs, "f64", pots=pots, n_batch=3, share_potentials=True)
    sets = [{1: 1}, {0: 2}, {}]
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    with pytest.raises(_capi.JtpError) as err:
        plan.map()
    m = re.search(r"(\d+) of (\d+) evidence sets.*first set (\d+)", str(err.value))
    assert m and [int(g) for g in m.groups()] == [1, 3, 1], str(err.value)
    states, value = err.value.states, err.value.log_value
    assert np.all(states[1] == -1) and value[1] == -np.inf
    for b in (0, 2):
        want_states, want_value = map_reference(plan, pots, sets[b])
        np.testing.assert_array_equal(states[b], states_row(plan, want_states))
        assert close_enough(value[b], want_value)
    assert map_reference(plan, pots, sets[1]) == (None, -np.inf)
    # the evidence gone, the same plan answers for every set
    plan.set_evidence({}, batch=1)
    states, value = plan.map()
    assert states.min() >= 0 and np.all(np.isfinite(value))
    plan.close()


def test_a_negative_entry_fails():
    spec = synthetic.chain_tree(4, card=3, width=3)
    cs = spec_case(spec, seed=3)
    pots = [np.array(p) for p in cs[1]]
    pots[2][1, 0, 2] = -pots[2][1, 0, 2]
    plan = make(cs, "f32", pots=[p.astype(np.float32) for p in pots], n_batch=2, share_potentials=True)
    plan.set_evidence({3: 1}, batch=1)                       # (clique 2 holds variables 2, 3, 4: the entry disagrees with set 1's evidence)
    with pytest.raises(_capi.JtpError) as err:
        plan.map()
    assert np.all(err.value.states[0] == -1) and err.value.log_value[0] == -np.inf
    want_states, want_value = map_reference(plan, [p.astype(np.float32) for p in pots], {3: 1})
    np.testing.assert_array_equal(err.value.states[1], states_row(plan, want_states))      # an entry that is not looked at fails nothing
    assert close_enough(err.value.log_value[1], want_value)
    plan.close()


# ---------------------------------------------------------------------------------------------- 7. no side effects

@pytest.mark.parametrize("opts", [{}, dict(level_launches=True), dict(scaled=True)], ids=["flow", "level", "scaled"])
def test_map_leaves_beliefs_and_messages_alone(opts):
    cs = case("wide7")
    plan = make(cs, "f64", **opts)
    free, _ = plan.map()                                     # before any propagate: staged potentials are all it needs
    plan.set_evidence({sorted(cs[3])[2]: 1})
    plan.propagate()
    before = [plan.belief(node) for node in range(len(cs[2]))]
    z = plan.log_z()
    observed, _ = plan.map()
    assert free.min() >= 0 and observed[0, plan.var_labels.index(sorted(cs[3])[2])] == 1
    after = [plan.belief(node) for node in range(len(cs[2]))]
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert plan.log_z() == z
    plan.propagate()                                         # ... and the next propagate finds its messages as it left them
    for a, b in zip(before, [plan.belief(node) for node in range(len(cs[2]))]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(plan.map()[0], observed)
    plan.close()


# ---------------------------------------------------------------------------------------------- 8. refusals and API

def test_plans_without_every_table_refuse_and_say_why():
    spec = synthetic.wide_binary_tree(7, 8, 4)
    cs = spec_case(spec)
    tree, pots, node_vars, sizes, n = cs
    multi = engine.Plan(tree, node_vars, sizes, multiset=True, n_batch=8)
    for c in range(n):
        multi.set_potential(c, pots[c])
    with pytest.raises(_capi.UnsupportedStructure, match="multi-set"):
        multi.map()
    multi.close()
    lean = engine.Plan(tree, node_vars, sizes, cover=[[] for _ in range(n)])
    assert lean.describe()["has_unit"] == 1
    with pytest.raises(_capi.UnsupportedStructure, match="without `cover`"):
        lean.map()
    lean.close()
    plan = make(cs)
    with pytest.raises(ValueError, match="bad batch range"):
        plan.map(0, 2)
    with pytest.raises(ValueError, match="bad batch range"):
        plan.map(0, 0)
    plan.close()


def brute_force_value(factors, sizes, values, evidence):
    labels = sorted(sizes, key=str)
    letters = {lab: chr(ord("a") + i) for i, lab in enumerate(labels)}
    expr = ",".join("".join(letters[v] for v in f) for f in factors) + "->" + "".join(letters[v] for v in labels)
    joint = np.einsum(expr, *[np.asarray(v, dtype=np.float64) for v in values])
    for lab, st in (evidence or {}).items():
        keep = np.zeros(sizes[lab], dtype=bool)
        keep[st] = True
        joint = np.where(keep.reshape([sizes[u] if u == lab else 1 for u in labels]), joint, -1.0)
    return labels, joint


def test_junction_tree_map():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    before = tree.propagate(README_VALUES)
    sets = [None, {"wet_grass": 1}, {"cloudy": 0, "sprinkler": 1}]
    for evidence in sets:
        states, value = tree.map(README_VALUES, evidence=evidence)
        labels, joint = brute_force_value(README_FACTORS, README_SIZES, README_VALUES, evidence)
        assert sorted(states, key=str) == labels and all(isinstance(st, int) for st in states.values())
        for lab, st in (evidence or {}).items():
            assert states[lab] == st
        at = joint[tuple(states[lab] for lab in labels)]
        assert abs(at - joint.max()) <= 8 * 2.0 ** -52 * joint.max()                 # values, not assignments
        assert abs(value - np.log(joint.max())) <= 16 * 2.0 ** -52
    cols, values = tree.map_evidence_sets(README_VALUES, [e or {} for e in sets])
    assert values.shape == (3,) and all(col.dtype == np.int32 and col.shape == (3,) for col in cols.values())
    for b, evidence in enumerate(sets):
        states, value = tree.map(README_VALUES, evidence=evidence)
        assert {lab: int(col[b]) for lab, col in cols.items()} == states and values[b] == value
    again, _ = tree.map(README_VALUES)                                            # the evidence does not stick to the cached plan
    assert again == tree.map(README_VALUES, evidence=None)[0]
    with pytest.raises(_capi.JtpError) as err:                                    # wet grass without sprinkler or rain: probability zero
        tree.map_evidence_sets(README_VALUES, [{}, {"sprinkler": 0, "rain": 0, "wet_grass": 1}])
    assert all(col[1] == -1 and col[0] >= 0 for col in err.value.states.values()) and err.value.log_value[1] == -np.inf
    for a, b in zip(before, tree.propagate(README_VALUES)):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 9. allocation failures

def live_bytes():
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().jtp_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def test_the_first_call_survives_the_failure_of_each_of_its_allocations():
    gc.collect()
    cs = case("wide7")
    fresh = make(cs, n_batch=3, share_potentials=True)
    want = fresh.map()
    fresh.close()
    plan = make(cs, n_batch=3, share_potentials=True)
    failed = 0
    for n in range(1, 16):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            got = plan.map(0, 1)
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    assert failed == n - 1 and failed >= 4, (failed, n)      # records, child lists, depth table, work area
    plan.debug_set("fail_alloc", 0)
    np.testing.assert_array_equal(got[0], want[0][:1])
    # the work area grows with the sets of a call: that allocation failing leaves the smaller one in place
    before = live_bytes()
    plan.debug_set("fail_alloc", 1)
    with pytest.raises(MemoryError):
        plan.map()
    assert live_bytes() == before
    plan.debug_set("fail_alloc", 0)
    got = plan.map()
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    plan.close()
