"""The M most probable assignments on the device (`jtp_map_best`: kernels `jt_mbest_level`, `jt_mbest_merge`, `jt_mbest_decode`) on a
real MI355X, against the numpy restatement of the sweep (`tests/mbest_reference.py`).

The definition is made of single IEEE operations in a fixed order and of a total order on every list, so the device's states must
EQUAL the restatement's, ties included, for float64 and for float32 tables (float32 potentials are drawn as float32 and widened);
`log_value` may differ by the one `log`, one multiply and one add that end it: 8 x 2^-53 x max(1, |log_value|), as for `jtp_map`."""
import ctypes as C
import gc

import numpy as np
import pytest

import junctiontree_amd as jt
from junctiontree_amd import _capi, engine, synthetic
from map_reference import value_of
from mbest_reference import mbest_reference, states_rows
from test_gpu_map import case, close_enough, five_sets, make, tables
from test_gpu_sample import LAYOUTS, README_FACTORS, README_SIZES, README_VALUES, spec_case
from test_map_host import SMALL
from test_max_host import brute_force as readme_joint, readme_model
from test_mbest_host import evidence_of, joint_of, largest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


_refs = {}


def reference(name, dtype):
    """the restatement with m = 16, computed once per (case, number format), shared by the tests that need it"""
    if (name, dtype) not in _refs:
        cs = case(name)
        probe = engine.Plan(cs[0], cs[2], cs[3], plan_only=True)
        solutions, values = mbest_reference(probe, tables(cs, dtype), 16)
        _refs[name, dtype] = (states_rows(probe, solutions), values)
    return _refs[name, dtype]


def value_bound(n_cliques, value):
    """the log of the product of an assignment's entries against its log_value: test_gpu_map.test_states_equal_the_restatements'"""
    return 2 * n_cliques * 2.0 ** -52 + 8 * 2.0 ** -53 * max(1.0, abs(value))


# ---------------------------------------------------------------------------------------------- 1. exact match

NAMES = ["random16_card3", "random16_card5", "random16_card6", "random16_card7", "contained", "chain6", "star12", "root64k"]
RUNS = [(n, d, {}) for n in NAMES for d in ("f64", "f32")] + [("random16_card3", "f64", dict(no_compact=True)), ("random16_card5", "f32", dict(no_compact=True)),
                                                              ("random16_card6", "f64", dict(no_compact=True)), ("random16_card7", "f32", dict(no_compact=True))]
RUN_IDS = ["%s-%s%s" % (n, d, "-no_compact" if o else "") for n, d, o in RUNS]


@pytest.mark.parametrize("name,dtype,opts", RUNS, ids=RUN_IDS)
def test_states_equal_the_restatements(name, dtype, opts):
    cs = case(name)
    plan = make(cs, dtype, **opts)
    sched = plan.describe()["sample"]["cliques"]
    if name == "contained":
        assert sorted(c["R"] for c in sched)[:2] == [1, 1]
    if name == "root64k":
        assert max(c["R"] for c in sched) == 1 << 16                    # (cut into segments: jt_mbest_merge runs)
    if name == "star12":
        assert sum(1 for c in sched if c["parent"] == sched[0]["clique"]) == 12      # (more than the staged children)
    if name.startswith("random16") and not opts:
        assert plan.describe()["compact"] == 1
    states, value = plan.map_best(16)
    want_states, want_value = reference(name, dtype)
    assert states.dtype == np.int32 and states.shape == (16, len(plan.var_labels)) and value.shape == (16,)
    np.testing.assert_array_equal(states, want_states)
    assert len({row.tobytes() for row in states}) == 16
    assert np.all(value[:-1] >= value[1:])
    for s in range(16):
        print("%s %s solution %d: log_value %.17g, restatement %.17g" % (name, dtype, s, value[s], want_value[s]))
        assert close_enough(value[s], want_value[s])
    if name == "root64k":                                               # another cut of r: the same bits
        plan.debug_set("map_seg", 64)
        again, again_value = plan.map_best(16)
        np.testing.assert_array_equal(again, states)
        np.testing.assert_array_equal(again_value, value)
    plan.close()


# ---------------------------------------------------------------------------------------------- 2. m = 1 is jtp_map, 3. prefixes

@pytest.mark.parametrize("name,dtype,opts", RUNS, ids=RUN_IDS)
def test_one_solution_is_maps_and_five_are_the_head_of_sixteen(name, dtype, opts):
    cs = case(name)
    plan = make(cs, dtype, **opts)
    map_states, map_value = plan.map()
    one, one_value = plan.map_best(1)
    assert one.shape == (1, len(plan.var_labels))
    np.testing.assert_array_equal(one, map_states)
    np.testing.assert_array_equal(one_value, map_value)                 # (bit for bit)
    sixteen, sixteen_value = plan.map_best(16)
    five, five_value = plan.map_best(5)
    np.testing.assert_array_equal(five, sixteen[:5])
    np.testing.assert_array_equal(five_value, sixteen_value[:5])
    np.testing.assert_array_equal(one, sixteen[:1])
    np.testing.assert_array_equal(one_value, sixteen_value[:1])
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. layout independence

@pytest.mark.parametrize("name", ["wide7", "random16_card6"])
def test_equal_potentials_give_equal_solutions_in_every_layout(name):
    """float32 numbers in every plan, so that float64 and float32 storage hold the same potentials"""
    cs = case(name)
    pots32 = tables(cs, "f32")
    want, want_value = None, None
    variants = dict(LAYOUTS, no_compact=dict(no_compact=True), no_compact_keep_root=dict(no_compact=True, keep_root=True), policy1_no_compact=dict(no_compact=True, layout_policy=1))
    for key, opts in variants.items():
        for dtype in ("f64", "f32"):
            plan = make(cs, dtype, pots=[p.astype(np.float64) for p in pots32] if dtype == "f64" else pots32, **opts)
            order = [plan.var_labels.index(lab) for lab in sorted(plan.var_labels)]
            states, value = plan.map_best(8)
            plan.close()
            assert states.shape[0] == 8
            if want is None:
                want, want_value = states[:, order], value
            np.testing.assert_array_equal(states[:, order], want, err_msg="%s %s" % (key, dtype))
            np.testing.assert_array_equal(value, want_value, err_msg="%s %s" % (key, dtype))


# ---------------------------------------------------------------------------------------------- 5. brute force

@pytest.mark.parametrize("with_evidence", [False, True], ids=["free", "evidence"])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_device_lists_the_sixteen_largest_of_the_enumerated_joint_in_order(name, with_evidence):
    cs = SMALL[name]()
    tree, pots, node_vars, sizes, n = cs
    evidence = evidence_of(sizes, with_evidence)
    plan = make(cs, "f64", pots=pots)
    if evidence:
        plan.set_evidence(evidence)
    states, value = plan.map_best(16)
    plan.close()
    labels, joint = joint_of(pots, node_vars, sizes, n, evidence)
    want, want_values = largest(labels, joint, 16)
    assert states.shape == (16, len(plan.var_labels))
    assert len({row.tobytes() for row in states}) == 16
    for s in range(16):
        got = dict(zip(plan.var_labels, (int(x) for x in states[s])))
        assert got == want[s], "solution %d" % s
        direct = value_of(pots[:n], node_vars[:n], got)
        print("%s solution %d: log_value %.17g, log of the product of its entries %.17g" % (name, s, value[s], np.log(direct)))
        assert abs(value[s] - np.log(direct)) <= value_bound(n, value[s])


# ---------------------------------------------------------------------------------------------- 6. ties, short lists, failure

def test_ties_come_out_in_the_order_of_the_definition():
    cs = SMALL["random8_card3"]()
    ones = [np.ones(np.shape(p)) for p in cs[1]]
    plan = make(cs, "f64", pots=ones)
    states, value = plan.map_best(4)
    probe = engine.Plan(cs[0], cs[2], cs[3], plan_only=True)
    want, want_value = mbest_reference(probe, ones, 4)
    assert states.shape[0] == 4 and np.all(value == 0.0) and np.all(states[0] == 0)
    assert len({row.tobytes() for row in states}) == 4
    np.testing.assert_array_equal(states, states_rows(probe, want))
    plan.close()


def test_fewer_assignments_of_positive_value_than_asked_for():
    tree, pots, node_vars, sizes, n, factors, values = readme_model()
    cs = (tree, pots, node_vars, sizes, n)
    plan = make(cs, "f64", pots=pots)
    evidence = {"sprinkler": 0, "rain": 0}
    plan.set_evidence(evidence)
    labels, joint = readme_joint(README_FACTORS, README_SIZES, README_VALUES, evidence)
    assert np.count_nonzero(joint > 0) == 2                  # wet_grass = 1 has value 0 there
    states, value = plan.map_best(4)
    assert states.shape == (2, len(plan.var_labels)) and value.shape == (2,)
    want, want_values = largest(labels, joint, 2)
    for s in range(2):
        assert dict(zip(plan.var_labels, (int(x) for x in states[s]))) == want[s]
        assert abs(value[s] - np.log(want_values[s])) <= value_bound(n, value[s])
    # the raw call: the two remaining rows are absent
    raw_states = np.zeros((4, len(plan.var_labels)), dtype=np.int32)
    raw_value = np.zeros(4)
    found = C.c_int32(-1)
    _capi.check(_capi.lib().jtp_map_best(plan._handle, 0, 4, raw_states.ctypes.data_as(C.c_void_p), raw_value.ctypes.data_as(C.c_void_p), C.byref(found)))
    assert found.value == 2 and np.all(raw_states[2:] == -1) and np.all(np.isneginf(raw_value[2:]))
    np.testing.assert_array_equal(raw_states[:2], states)
    # evidence of probability zero: nothing to list
    plan.set_evidence({"sprinkler": 0, "rain": 0, "wet_grass": 1})
    with pytest.raises(_capi.JtpError, match="no assignment of positive finite value") as err:
        plan.map_best(4)
    assert err.value.states.shape == (4, len(plan.var_labels)) and np.all(err.value.states == -1) and np.all(np.isneginf(err.value.log_value))
    plan.set_evidence({})
    assert plan.map_best(4)[0].shape[0] == 4
    plan.close()


def test_a_negative_entry_fails():
    spec = synthetic.chain_tree(4, card=3, width=3)
    cs = spec_case(spec, seed=3)
    pots = [np.array(p) for p in cs[1]]
    pots[2][1, 0, 2] = -pots[2][1, 0, 2]
    pots32 = [p.astype(np.float32) for p in pots]
    plan = make(cs, "f32", pots=pots32, n_batch=2, share_potentials=True)
    plan.set_evidence({3: 1}, batch=1)                       # (clique 2 holds variables 2, 3, 4: the entry disagrees with set 1's evidence)
    with pytest.raises(_capi.JtpError) as err:
        plan.map_best(3)
    assert np.all(err.value.states == -1) and np.all(np.isneginf(err.value.log_value))
    states, value = plan.map_best(3, batch=1)                # an entry that is not looked at fails nothing
    want, want_value = mbest_reference(plan, pots32, 3, {3: 1})
    np.testing.assert_array_equal(states, states_rows(plan, want))
    assert all(close_enough(g, w) for g, w in zip(value, want_value))
    plan.close()


# ---------------------------------------------------------------------------------------------- 7. evidence sets

def test_every_evidence_set_sees_its_own_evidence():
    cs = case("random16_card3")
    probe, sets = five_sets(cs)
    sets = [sets[0], sets[2], sets[4]]
    plan = make(cs, "f64", n_batch=3, share_potentials=True)
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    col = {lab: j for j, lab in enumerate(plan.var_labels)}
    tabs = tables(cs, "f64")
    for b, obs in enumerate(sets):
        states, value = plan.map_best(16, batch=b)
        for lab, st in obs.items():
            assert np.all(states[:, col[lab]] == st)
        want, want_value = mbest_reference(probe, tabs, 16, obs)
        np.testing.assert_array_equal(states, states_rows(plan, want), err_msg="set %d" % b)
        assert all(close_enough(g, w) for g, w in zip(value, want_value))
    with pytest.raises(ValueError, match="out of range"):
        plan.map_best(2, batch=3)
    plan.close()


# ---------------------------------------------------------------------------------------------- 8. no side effects

@pytest.mark.parametrize("opts", [{}, dict(level_launches=True), dict(scaled=True)], ids=["flow", "level", "scaled"])
def test_map_best_leaves_beliefs_and_messages_alone(opts):
    cs = case("wide7")
    plan = make(cs, "f64", **opts)
    free, _ = plan.map_best(6)                               # before any propagate: staged potentials are all it needs
    plan.set_evidence({sorted(cs[3])[2]: 1})
    plan.propagate()
    before = [plan.belief(node) for node in range(len(cs[2]))]
    z = plan.log_z()
    observed, observed_value = plan.map_best(6)
    assert free.shape[0] == 6 and np.all(observed[:, plan.var_labels.index(sorted(cs[3])[2])] == 1)
    after = [plan.belief(node) for node in range(len(cs[2]))]
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert plan.log_z() == z
    plan.propagate()                                         # ... and the next propagate finds its messages as it left them
    for a, b in zip(before, [plan.belief(node) for node in range(len(cs[2]))]):
        np.testing.assert_array_equal(a, b)
    again, again_value = plan.map_best(6)
    np.testing.assert_array_equal(again, observed)
    np.testing.assert_array_equal(again_value, observed_value)
    np.testing.assert_array_equal(plan.map()[0], observed[:1])
    plan.close()


# ---------------------------------------------------------------------------------------------- 9. refusals

def test_plans_without_every_table_refuse_and_say_why():
    spec = synthetic.wide_binary_tree(7, 8, 4)
    cs = spec_case(spec)
    tree, pots, node_vars, sizes, n = cs
    multi = engine.Plan(tree, node_vars, sizes, multiset=True, n_batch=8)
    for c in range(n):
        multi.set_potential(c, pots[c])
    with pytest.raises(_capi.UnsupportedStructure, match="multi-set plan runs eight evidence sets per pass of the propagate and nothing else"):
        multi.map_best(2)
    multi.close()
    lean = engine.Plan(tree, node_vars, sizes, cover=[[] for _ in range(n)])
    assert lean.describe()["has_unit"] == 1
    with pytest.raises(_capi.UnsupportedStructure, match="keeps no table on the device: make the plan without `cover`"):
        lean.map_best(2)
    lean.close()
    plan = make(cs)
    for m in (0, 17, -3):
        with pytest.raises(ValueError, match="not in"):
            plan.map_best(m)
    assert plan.map_best(16)[0].shape[0] == 16
    plan.close()


# ---------------------------------------------------------------------------------------------- 10. allocation failures

def live_bytes():
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().jtp_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def test_the_first_call_survives_the_failure_of_each_of_its_allocations():
    gc.collect()
    cs = case("wide7")
    fresh = make(cs)
    want = fresh.map_best(4)
    want_map = fresh.map()
    fresh.close()
    plan = make(cs)
    failed = 0
    for n in range(1, 16):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            got = plan.map_best(4)
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    assert failed == n - 1 and failed >= 4, (failed, n)      # records, child lists, depth table, work area
    plan.debug_set("fail_alloc", 0)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    # the work area grows with the lists of a call: that allocation failing leaves the smaller one in place
    before = live_bytes()
    plan.debug_set("fail_alloc", 1)
    with pytest.raises(MemoryError):
        plan.map_best(16)
    assert live_bytes() == before
    plan.debug_set("fail_alloc", 0)
    np.testing.assert_array_equal(plan.map_best(4)[0], want[0])
    np.testing.assert_array_equal(plan.map_best(16)[0][:4], want[0])
    # jtp_map finds the records this call made and allocates a work area of its own
    got_map = plan.map()
    np.testing.assert_array_equal(got_map[0], want_map[0])
    np.testing.assert_array_equal(got_map[1], want_map[1])
    plan.close()


# ---------------------------------------------------------------------------------------------- 11. through the package

def test_junction_tree_map_best():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    before = tree.propagate(README_VALUES)
    evidence = {"wet_grass": 1}
    got = tree.map_best(README_VALUES, 3, evidence=evidence)
    labels, joint = readme_joint(README_FACTORS, README_SIZES, README_VALUES, evidence)
    want, want_values = largest(labels, joint, 4)
    assert want_values[3] > 0 and np.min((want_values[:-1] - want_values[1:]) / want_values[:-1]) > 1e-9      # (no ties: assignments compare)
    assert len(got) == 3
    for s, (states, value) in enumerate(got):
        assert states == want[s] and all(isinstance(st, int) for st in states.values())
        assert abs(value - np.log(want_values[s])) <= 16 * 2.0 ** -52
    assert got[0] == tree.map(README_VALUES, evidence=evidence)
    free = tree.map_best(README_VALUES, 2)                                        # the evidence does not stick to the cached plan
    assert free[0] == tree.map(README_VALUES)
    with pytest.raises(_capi.JtpError) as err:                                    # wet grass without sprinkler or rain: probability zero
        tree.map_best(README_VALUES, 2, evidence={"sprinkler": 0, "rain": 0, "wet_grass": 1})
    assert all(np.all(col == -1) for col in err.value.states.values()) and np.all(np.isneginf(err.value.log_value))
    assert tree.map_best(README_VALUES, 2) == free
    for a, b in zip(before, tree.propagate(README_VALUES)):
        np.testing.assert_array_equal(a, b)
