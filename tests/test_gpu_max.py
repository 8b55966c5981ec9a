"""Max-propagation on the device (`jtp_max_marginals`: jtp_map's upward kernels, then `jt_max_level` / `jt_max_merge`) on a real
MI355X, against the numpy restatement of the sweep (`tests/max_reference.py`).

The definition is made of single IEEE operations in a fixed order and of exact maxima, so the device's tables and exponents must
EQUAL the restatement's, for float64 and for float32 tables (float32 potentials are drawn as float32 and widened); `log_value` may
differ by the one `log`, one multiply and one add that end it: 8 x 2^-53 x max(1, |log_value|), as for `jtp_map`.  Where two
computations that round differently are compared (the clamping identity, the value of the most probable assignment), the
tolerance is the one derived in tests/test_max_host.py: 4 (n_cliques + n_factors) 2^-53 relative on values, and on logarithms
4 spacings of |log_value| more."""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import junctiontree_amd as jt
from junctiontree_amd import _capi, engine, synthetic
from max_reference import factor_requests, log_of, max_reference
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


def make(cs, dtype="f64", pots=None, n_batch=1, **opts):
    """a plan with its potentials staged (set 0: shared plans) and NOT propagated"""
    tree, _, node_vars, sizes, n = cs
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, n_batch=n_batch, **opts)
    mine = tables(cs, dtype) if pots is None else pots
    for c in range(n):
        plan.set_potential(c, mine[c])
    return plan


def probe_of(cs):
    return engine.Plan(cs[0], cs[2], cs[3], plan_only=True)


def close_enough(got, want):
    return abs(got - want) <= 8 * 2.0 ** -53 * max(1.0, abs(want))


def log_tol(n_cliques, n_factors, log_value):
    return 4 * (n_cliques + n_factors) * 2.0 ** -53 + 4 * np.spacing(abs(log_value))


def assert_equal_results(got, want, what=""):
    """tables and exponents bit for bit; `got` / `want`: (tables of one set, exponents of one set)"""
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        np.testing.assert_array_equal(a, b, err_msg="%s request %d" % (what, i))
    np.testing.assert_array_equal(np.asarray(got[1]), np.asarray(want[1]), err_msg=what)


_refs = {}


def reference(name, dtype):
    """(requests, tables, exponents, log_value) of the restatement, computed once per (case, number format)"""
    if (name, dtype) not in _refs:
        cs = case(name)
        probe = probe_of(cs)
        requests = factor_requests(probe)
        _refs[name, dtype] = (requests,) + max_reference(probe, tables(cs, dtype), requests)
    return _refs[name, dtype]


def variable_requests(cs):
    """one request per variable, on the first clique that holds it: [(clique, [variable])]"""
    node_vars, n = cs[2], cs[4]
    return [(next(c for c in range(n) if v in node_vars[c]), [v]) for v in sorted(cs[3])]


# ---------------------------------------------------------------------------------------------- 1. exact match, 6. consistency

NAMES = ["wide7", "chain6", "random16_card3", "random16_card5", "random16_card6", "random16_card7", "star5", "star12", "contained", "root64k"]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_tables_and_exponents_equal_the_restatements(name, dtype):
    cs = case(name)
    plan = make(cs, dtype)
    sched = plan.describe()["sample"]["cliques"]
    if name == "contained":
        assert sorted(c["R"] for c in sched)[:2] == [1, 1]
    if name == "root64k":
        assert max(c["R"] for c in sched) == 1 << 16                    # (cut into segments: jt_max_merge runs)
    if name == "star12":
        assert sum(1 for c in sched if c["parent"] == sched[0]["clique"]) == 12       # (more inputs than are staged)
    if name.startswith("random16"):
        assert plan.describe()["compact"] == 1
    requests, want_tables, want_scale, want_value = reference(name, dtype)
    got_tables, got_scale, got_value = plan.max_marginals(requests)
    assert got_scale.dtype == np.int64 and got_scale.shape == (1, len(requests)) and got_value.shape == (1,)
    for (c, labels), t in zip(requests, got_tables[0]):
        assert t.dtype == np.float64 and t.shape == tuple(cs[3][v] for v in labels)
    assert_equal_results((got_tables[0], got_scale[0]), (want_tables, want_scale), name)
    print("%s %s: log_value %.17g, restatement %.17g" % (name, dtype, got_value[0], want_value))
    assert close_enough(got_value[0], want_value)
    # every table's largest entry, scaled back, is the value of the most probable assignment - and jtp_map reports the same number
    _, map_value = plan.map()
    assert got_value[0] == map_value[0]
    tol = log_tol(cs[4], cs[4], got_value[0])
    worst = max(abs(log_of(t, e).max() - got_value[0]) for t, e in zip(got_tables[0], got_scale[0]))
    print("largest |log max - log_value| %.3g (bound %.3g)" % (worst, tol))
    assert worst <= tol
    plan.close()


# ---------------------------------------------------------------------------------------------- 2. layout independence

@pytest.mark.parametrize("name", ["wide7", "random16_card6"])
def test_equal_potentials_give_equal_tables_in_every_layout(name):
    """float32 numbers in every plan, so that float64 and float32 storage hold the same potentials"""
    cs = case(name)
    pots32 = tables(cs, "f32")
    requests = factor_requests(probe_of(cs))
    want = None
    for key, opts in LAYOUTS.items():
        for dtype in ("f64", "f32"):
            plan = make(cs, dtype, pots=[p.astype(np.float64) for p in pots32] if dtype == "f64" else pots32, **opts)
            got_tables, got_scale, got_value = plan.max_marginals(requests)
            plan.close()
            if want is None:
                want = (got_tables[0], got_scale[0], got_value[0])
            assert_equal_results((got_tables[0], got_scale[0]), want, "%s %s" % (key, dtype))
            assert got_value[0] == want[2], (key, dtype)


# ---------------------------------------------------------------------------------------------- 3. segments and chunks

@pytest.mark.parametrize("name", ["root64k", "wide7"])
def test_the_cut_into_segments_changes_nothing(name):
    cs = case(name)
    plan = make(cs, "f64")
    requests = factor_requests(probe_of(cs))
    want_tables, want_scale, want_value = plan.max_marginals(requests)
    plan.debug_set("map_seg", 4)
    got_tables, got_scale, got_value = plan.max_marginals(requests)
    assert_equal_results((got_tables[0], got_scale[0]), (want_tables[0], want_scale[0]), "map_seg 4")
    assert got_value[0] == want_value[0]
    plan.debug_set("map_seg", 0)
    got_tables, got_scale, got_value = plan.max_marginals(requests)
    assert_equal_results((got_tables[0], got_scale[0]), (want_tables[0], want_scale[0]), "map_seg 0")
    assert_equal_results((got_tables[0], got_scale[0]), reference(name, "f64")[1:3], "restatement")
    plan.close()


def five_sets(cs):
    probe = probe_of(cs)
    sched = [(c["clique"], c["K"], c["F"]) for c in probe.describe()["sample"]["cliques"]]
    lab = probe.var_labels
    in_k = sorted({lab[v] for s in sched for v in s[1]})
    leaf_f = [lab[v] for v in sched[-1][2]]
    sizes = cs[3]
    return probe, [{leaf_f[-1]: sizes[leaf_f[-1]] - 1}, {}, {in_k[0]: 1, leaf_f[0]: 0}, {in_k[-1]: sizes[in_k[-1]] - 1}, {in_k[1]: 0, in_k[2]: 1, lab[sched[0][2][0]]: 1}]


@pytest.mark.parametrize("name,dtype", [("random16_card3", "f64"), ("wide7", "f32")])
def test_evidence_sets_go_through_the_same_launches(name, dtype):
    cs = case(name)
    probe, sets = five_sets(cs)
    requests = factor_requests(probe)
    plan = make(cs, dtype, n_batch=5, share_potentials=True)
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    got_tables, got_scale, got_value = plan.max_marginals(requests)
    assert got_scale.shape == (5, len(requests)) and got_value.shape == (5,) and len(got_tables) == 5
    for b, obs in enumerate(sets):
        want_tables, want_scale, want_value = max_reference(probe, tables(cs, dtype), requests, obs)
        assert_equal_results((got_tables[b], got_scale[b]), (want_tables, want_scale), "set %d" % b)
        assert close_enough(got_value[b], want_value)
        one_tables, one_scale, one_value = plan.max_marginals(requests, b, b + 1)        # a one-set call per set: the same
        assert_equal_results((one_tables[0], one_scale[0]), (got_tables[b], got_scale[b]), "single call, set %d" % b)
        assert one_value[0] == got_value[b]
    plan.debug_set("map_chunk", 1)                                                     # five chunks of one set
    chunk_tables, chunk_scale, chunk_value = plan.max_marginals(requests)
    for b in range(5):
        assert_equal_results((chunk_tables[b], chunk_scale[b]), (got_tables[b], got_scale[b]), "map_chunk 1, set %d" % b)
    np.testing.assert_array_equal(chunk_value, got_value)
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. the clamping identity

@pytest.mark.parametrize("name", ["star5", "chain6"])
def test_a_variables_max_marginal_is_jtp_map_with_the_variable_clamped(name):
    cs = case(name)
    tree, _, node_vars, sizes, n = cs
    pots = [np.array(p) for p in tables(cs, "f64")]
    dead = sorted(sizes)[2]                                  # one variable never in its last state: that clamp has probability zero
    c0 = next(c for c in range(n) if dead in node_vars[c])
    pots[c0][tuple(slice(sizes[dead] - 1, None) if u == dead else slice(None) for u in node_vars[c0])] = 0.0
    requests = variable_requests(cs)
    clamps = [(v, s) for _, (v,) in requests for s in range(sizes[v])]
    plan = make(cs, "f64", pots=pots, n_batch=len(clamps), share_potentials=True)
    got_tables, got_scale, got_value = plan.max_marginals(requests, 0, 1)
    _, free_value = plan.map(0, 1)
    assert got_value[0] == free_value[0]                     # bit for bit: the same computation
    for b, (v, s) in enumerate(clamps):
        plan.set_evidence({v: s}, batch=b)
    with pytest.raises(_capi.JtpError) as err:
        plan.map()
    clamped = err.value.log_value
    tol = log_tol(n, n, got_value[0])
    mm = {v: log_of(t, e) for (_, (v,)), t, e in zip(requests, got_tables[0], got_scale[0])}
    worst = 0.0
    for b, (v, s) in enumerate(clamps):
        if (v, s) == (dead, sizes[dead] - 1):
            assert clamped[b] == -np.inf and mm[v][s] == -np.inf
            continue
        assert np.isfinite(clamped[b])
        worst = max(worst, abs(mm[v][s] - clamped[b]))
    print("%s: largest |log mm_v[s] - log_value of the clamped jtp_map| %.3g over %d clamps (bound %.3g)" % (name, worst, len(clamps), tol))
    assert worst <= tol
    assert int(np.isneginf(clamped).sum()) == 1
    plan.close()


def test_the_clamping_identity_on_the_readme_network():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    mm = tree.max_marginals(README_VALUES)
    tables, value = tree.max_propagate(README_VALUES)
    _, map_value = tree.map(README_VALUES)
    assert value == map_value
    clamps = [(v, s) for v in sorted(README_SIZES) for s in range(README_SIZES[v])]
    _, clamped = tree.map_evidence_sets(README_VALUES, [{v: s} for v, s in clamps])
    n = len(tree.clique_tree.maxcliques)
    tol = log_tol(n, len(README_FACTORS), value)
    for b, (v, s) in enumerate(clamps):
        assert mm[v].shape == (README_SIZES[v],)
        print("%s = %d: log max-marginal %.17g, clamped map %.17g" % (v, s, mm[v][s], clamped[b]))
        assert abs(mm[v][s] - clamped[b]) <= tol
    for labels, t in zip(README_FACTORS, tables):
        assert t.shape == tuple(README_SIZES[v] for v in labels) and abs(t.max() - value) <= tol


# ---------------------------------------------------------------------------------------------- 5. decode agrees

def runner_up_gap(logs):
    top = np.sort(logs)[::-1]
    return top[0] - top[1]


def test_argmax_of_the_max_marginals_is_the_map_assignment_readme():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    evidence = {"wet_grass": 1}
    mm = tree.max_marginals(README_VALUES, evidence=evidence)
    states, value = tree.map(README_VALUES, evidence=evidence)
    tol = log_tol(len(tree.clique_tree.maxcliques), len(README_FACTORS), value)
    for v, logs in mm.items():
        assert runner_up_gap(logs) > tol, "variable %r: no unique best state - a condition of this test" % (v,)
        assert int(np.argmax(logs)) == states[v]
    assert mm["wet_grass"][0] == -np.inf


def test_argmax_of_the_max_marginals_is_the_map_assignment_wide7():
    cs = case("wide7")
    requests = variable_requests(cs)
    pots = tables(cs, "f64", seed=3)
    want_tables, want_scale, want_value = max_reference(probe_of(cs), pots, requests)
    tol = log_tol(cs[4], cs[4], want_value)
    for (c, (v,)), t, e in zip(requests, want_tables, want_scale):       # from the restatement: every variable has one best state
        assert runner_up_gap(log_of(t, e)) > tol, "variable %r: no unique best state - a condition of this test" % (v,)
    plan = make(cs, "f64", pots=pots)
    got_tables, got_scale, _ = plan.max_marginals(requests)
    states, _ = plan.map()
    col = {lab: j for j, lab in enumerate(plan.var_labels)}
    for (c, (v,)), t in zip(requests, got_tables[0]):
        assert int(np.argmax(t)) == states[0, col[v]]
    plan.close()


# ---------------------------------------------------------------------------------------------- 7. range

@pytest.mark.parametrize("power", [600, -600])
def test_a_chain_whose_values_lie_beyond_float64_has_finite_logarithms(power):
    spec = synthetic.chain_tree(64, card=3, width=3)
    cs = spec_case(spec)
    tree, pots, node_vars, sizes, n = cs
    rng = np.random.default_rng(17)
    big = [np.ldexp(rng.uniform(0.5, 1.5, np.shape(p)), power) if c < n else p for c, p in enumerate(pots)]
    plan = make(cs, "f64", pots=big)
    requests = factor_requests(probe_of(cs))
    got_tables, got_scale, got_value = plan.max_marginals(requests)
    want_tables, want_scale, want_value = max_reference(plan, big, requests)
    assert_equal_results((got_tables[0], got_scale[0]), (want_tables, want_scale))
    centre = 64 * power * np.log(2.0)
    assert np.isfinite(got_value[0]) and abs(got_value[0] - centre) <= 64 * np.log(2.0)        # (every entry within [0.5, 1.5) of 2^power)
    assert close_enough(got_value[0], want_value)
    tol = log_tol(n, n, got_value[0])
    for t, e in zip(got_tables[0], got_scale[0]):
        logs = log_of(t, e)
        assert np.all(np.isfinite(logs)) and abs(logs.max() - got_value[0]) <= tol
    plan.close()


# ---------------------------------------------------------------------------------------------- 8. evidence

def test_observed_variables_are_minus_infinity_off_their_state_and_contradicted_entries_are_never_read():
    cs = case("random16_card3")
    tree, _, node_vars, sizes, n = cs
    probe, sets = five_sets(cs)
    obs = sets[4]
    requests = factor_requests(probe) + variable_requests(cs)
    clean = tables(cs, "f64")
    plan = make(cs, "f64", pots=clean)
    plan.set_evidence(obs)
    want_tables, want_scale, want_value = plan.max_marginals(requests)
    for (c, labels), t, e in zip(requests, want_tables[0], want_scale[0]):
        logs = log_of(t, e)
        for ax, v in enumerate(labels):
            if v in obs:
                assert np.all(np.delete(logs, obs[v], axis=ax) == -np.inf), (c, labels)
                assert np.any(np.isfinite(np.take(logs, obs[v], axis=ax))), (c, labels)
    plan.close()
    poison = [np.inf, np.nan, -1.0]
    dirty = [np.array(p) for p in clean]
    k = 0
    for c in range(n):
        for v, st in obs.items():
            if v in node_vars[c]:
                for s in range(sizes[v]):
                    if s != st:
                        dirty[c][tuple(slice(s, s + 1) if u == v else slice(None) for u in node_vars[c])] = poison[k % 3]
                        k += 1
    assert k >= 6
    plan = make(cs, "f64", pots=dirty)
    plan.set_evidence(obs)
    got_tables, got_scale, got_value = plan.max_marginals(requests)
    assert_equal_results((got_tables[0], got_scale[0]), (want_tables[0], want_scale[0]), "poisoned")
    assert got_value[0] == want_value[0]
    plan.close()


# ---------------------------------------------------------------------------------------------- 9. failures

def test_a_set_of_probability_zero_fails_among_healthy_ones():
    spec = synthetic.chain_tree(4, card=3, width=3)
    cs = spec_case(spec, seed=3)
    tree, pots, node_vars, sizes, n = cs
    pots = [np.array(p) for p in pots]
    pots[0][2, :, :] = 0.0                                   # variable 0 is never in state 2
    plan = make(cs, "f64", pots=pots, n_batch=3, share_potentials=True)
    requests = factor_requests(probe_of(cs))
    sets = [{1: 1}, {0: 2}, {}]
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    with pytest.raises(_capi.JtpError) as err:
        plan.max_marginals(requests)
    m = re.search(r"(\d+) of (\d+) evidence sets.*first set (\d+)", str(err.value))
    assert m and [int(g) for g in m.groups()] == [1, 3, 1], str(err.value)
    got_tables, got_scale, got_value = err.value.tables, err.value.log2_scale, err.value.log_value
    assert got_value[1] == -np.inf and not got_scale[1].any() and not any(t.any() for t in got_tables[1])
    for b in (0, 2):
        want_tables, want_scale, want_value = max_reference(plan, pots, requests, sets[b])
        assert_equal_results((got_tables[b], got_scale[b]), (want_tables, want_scale), "set %d" % b)
        assert close_enough(got_value[b], want_value)
    assert max_reference(plan, pots, requests, sets[1])[2] == -np.inf
    plan.set_evidence({}, batch=1)                           # the evidence gone, the same plan answers for every set
    _, _, value = plan.max_marginals(requests)
    assert np.all(np.isfinite(value))
    plan.close()


def test_a_negative_entry_that_counts_fails_its_set():
    spec = synthetic.chain_tree(4, card=3, width=3)
    cs = spec_case(spec, seed=3)
    pots = [np.array(p) for p in cs[1]]
    pots[2][1, 0, 2] = -pots[2][1, 0, 2]
    pots32 = [p.astype(np.float32) for p in pots]
    plan = make(cs, "f32", pots=pots32, n_batch=2, share_potentials=True)
    requests = factor_requests(probe_of(cs))
    plan.set_evidence({3: 1}, batch=1)                       # (clique 2 holds variables 2, 3, 4: the entry disagrees with set 1's evidence)
    with pytest.raises(_capi.JtpError) as err:
        plan.max_marginals(requests)
    assert err.value.log_value[0] == -np.inf and not any(t.any() for t in err.value.tables[0])
    want_tables, want_scale, want_value = max_reference(plan, pots32, requests, {3: 1})
    assert_equal_results((err.value.tables[1], err.value.log2_scale[1]), (want_tables, want_scale))      # an entry that is not looked at fails nothing
    assert close_enough(err.value.log_value[1], want_value)
    plan.close()


# ---------------------------------------------------------------------------------------------- 10. refusals

def test_plans_without_every_table_refuse_with_jtp_maps_words():
    spec = synthetic.wide_binary_tree(7, 8, 4)
    cs = spec_case(spec)
    tree, pots, node_vars, sizes, n = cs
    requests = [(0, node_vars[0][:2])]

    def same_words(plan, kind):
        with pytest.raises(kind) as of_map:
            plan.map()
        with pytest.raises(kind) as of_max:
            plan.max_marginals(requests)
        assert str(of_max.value).replace("jtp_max_marginals", "jtp_map") == str(of_map.value)
        return str(of_max.value)

    multi = engine.Plan(tree, node_vars, sizes, multiset=True, n_batch=8)
    for c in range(n):
        multi.set_potential(c, pots[c])
    assert "multi-set" in same_words(multi, _capi.UnsupportedStructure)
    multi.close()
    lean = engine.Plan(tree, node_vars, sizes, cover=[[] for _ in range(n)])
    assert lean.describe()["has_unit"] == 1
    assert "without `cover`" in same_words(lean, _capi.UnsupportedStructure)
    lean.close()
    plan = make(cs)
    for begin, end in ((0, 2), (0, 0)):
        with pytest.raises(ValueError, match="bad batch range") as of_max:
            plan.max_marginals(requests, begin, end)
        with pytest.raises(ValueError, match="bad batch range") as of_map:
            plan.map(begin, end)
        assert str(of_max.value) == str(of_map.value)
    stranger = next(v for v in sorted(sizes) if v not in node_vars[0])
    with pytest.raises(ValueError, match="is not in clique"):
        plan.max_marginals([(0, [node_vars[0][0], stranger])])
    with pytest.raises(ValueError, match="listed twice"):
        plan.max_marginals([(0, [node_vars[0][0], node_vars[0][0]])])
    tables_, _, _ = plan.max_marginals(requests)             # ... and the plan still answers
    assert tables_[0][0].shape == (2, 2)
    plan.close()


# ---------------------------------------------------------------------------------------------- 11. allocation failures

def live_bytes():
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().jtp_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def test_the_first_call_survives_the_failure_of_each_of_its_allocations():
    gc.collect()
    cs = case("wide7")
    requests = factor_requests(probe_of(cs))
    fresh = make(cs, n_batch=3, share_potentials=True)
    want = fresh.max_marginals(requests)
    fresh.close()
    plan = make(cs, n_batch=3, share_potentials=True)
    failed = 0
    for n in range(1, 24):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            got = plan.max_marginals(requests, 0, 1)
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    # upward records, child lists, depth table; downward records and inputs; request records and inputs; the work area
    assert failed == n - 1 and failed >= 8, (failed, n)
    plan.debug_set("fail_alloc", 0)
    assert_equal_results((got[0][0], got[1][0]), (want[0][0], want[1][0]))
    # the work area grows with the sets of a call: that allocation failing leaves the smaller one in place
    before = live_bytes()
    plan.debug_set("fail_alloc", 1)
    with pytest.raises(MemoryError):
        plan.max_marginals(requests)
    assert live_bytes() == before
    plan.debug_set("fail_alloc", 0)
    got = plan.max_marginals(requests)
    for b in range(3):
        assert_equal_results((got[0][b], got[1][b]), (want[0][b], want[1][b]), "set %d" % b)
    np.testing.assert_array_equal(got[2], want[2])
    # a new request list: its records are the call's only allocations, and their failure leaves the old list in place
    other = variable_requests(cs)
    before = live_bytes()
    plan.debug_set("fail_alloc", 2)
    with pytest.raises(MemoryError):
        plan.max_marginals(other)
    assert live_bytes() == before
    plan.debug_set("fail_alloc", 0)
    got = plan.max_marginals(requests, 0, 1)
    assert_equal_results((got[0][0], got[1][0]), (want[0][0], want[1][0]))
    plan.close()


# ---------------------------------------------------------------------------------------------- 12. side effects, the tree's interface

def test_max_propagate_leaves_propagate_and_map_alone():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    before = tree.propagate(README_VALUES)
    states, value = tree.map(README_VALUES, evidence={"wet_grass": 1})
    tables, log_value = tree.max_propagate(README_VALUES, evidence={"wet_grass": 1})
    assert log_value == value
    for a, b in zip(before, tree.propagate(README_VALUES)):
        np.testing.assert_array_equal(a, b)
    again_states, again_value = tree.map(README_VALUES, evidence={"wet_grass": 1})
    assert again_states == states and again_value == value
    free, free_value = tree.max_propagate(README_VALUES)                    # the evidence does not stick to the cached plan
    assert free_value == tree.map(README_VALUES)[1] and np.isfinite(free[3][1, 1, 0])


def test_plan_level_side_effects():
    cs = case("wide7")
    plan = make(cs, "f64")
    requests = factor_requests(probe_of(cs))
    plan.set_evidence({sorted(cs[3])[2]: 1})
    plan.propagate()
    before = [plan.belief(node) for node in range(len(cs[2]))]
    z = plan.log_z()
    states, value = plan.map()
    plan.max_marginals(requests)
    for a, b in zip(before, [plan.belief(node) for node in range(len(cs[2]))]):
        np.testing.assert_array_equal(a, b)
    assert plan.log_z() == z
    plan.propagate()
    for a, b in zip(before, [plan.belief(node) for node in range(len(cs[2]))]):
        np.testing.assert_array_equal(a, b)
    again_states, again_value = plan.map()
    np.testing.assert_array_equal(again_states, states)
    assert again_value[0] == value[0]
    plan.close()


def brute_force_logs(evidence):
    labels = sorted(README_SIZES)
    letters = {lab: chr(ord("a") + i) for i, lab in enumerate(labels)}
    expr = ",".join("".join(letters[v] for v in f) for f in README_FACTORS) + "->" + "".join(letters[v] for v in labels)
    joint = np.einsum(expr, *[np.asarray(v, dtype=np.float64) for v in README_VALUES])
    for lab, st in (evidence or {}).items():
        keep = np.zeros(README_SIZES[lab], dtype=bool)
        keep[st] = True
        joint = np.where(keep.reshape([README_SIZES[u] if u == lab else 1 for u in labels]), joint, 0.0)
    return labels, joint


def test_junction_tree_max_propagate_against_brute_force():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    n = len(tree.clique_tree.maxcliques)
    sets = [{}, {"wet_grass": 1}, {"cloudy": 0, "sprinkler": 1}]
    per_set, values = tree.max_propagate_evidence_sets(README_VALUES, sets)
    assert values.shape == (3,) and len(per_set) == 3
    for b, evidence in enumerate(sets):
        labels, joint = brute_force_logs(evidence)
        tol = log_tol(n, len(README_FACTORS), values[b])
        assert abs(values[b] - np.log(joint.max())) <= tol
        one, one_value = tree.max_propagate(README_VALUES, evidence=evidence)
        assert one_value == values[b]
        for f, (fvars, got) in enumerate(zip(README_FACTORS, per_set[b])):
            np.testing.assert_array_equal(got, one[f])
            drop = tuple(i for i, v in enumerate(labels) if v not in fvars)
            best = joint.max(axis=drop)
            left = [v for v in labels if v in fvars]
            with np.errstate(divide="ignore"):
                want = np.log(np.transpose(best, [left.index(v) for v in fvars]))
            assert got.shape == want.shape and np.all((got == -np.inf) == (want == -np.inf))
            fin = np.isfinite(want)
            assert np.all(np.abs(got[fin] - want[fin]) <= tol)
    with pytest.raises(_capi.JtpError) as err:                                    # wet grass without sprinkler or rain: probability zero
        tree.max_propagate_evidence_sets(README_VALUES, [{}, {"sprinkler": 0, "rain": 0, "wet_grass": 1}])
    assert err.value.log_value[1] == -np.inf and all(np.all(t == -np.inf) for t in err.value.max_marginals[1])
    assert err.value.log_value[0] == values[0]
    for a, b in zip(err.value.max_marginals[0], per_set[0]):
        np.testing.assert_array_equal(a, b)
