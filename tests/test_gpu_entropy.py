"""Posterior entropy and cross-entropy on the device (`jtp_entropy`: kernels `jt_entropy_sums`, `jt_entropy_finish`) on a real MI355X,
against the long-double restatement of the definition (`tests/entropy_reference.py`) applied to the beliefs read back from the same
plan - the numbers the kernel read.  The tolerance is `parity_bound`, derived there from the order the kernels add in: no rtol here.
Where a test compares with something that is NOT formed from the plan's own beliefs (enumeration, another plan) the beliefs' own
rounding comes on top, as `calibration_slack` derives it there from the tree's shape; X - H against ln Z0 - ln Z1 is held to the
summed bound alone.  (Every test prints its figures before it asserts; on an MI355X the worst |h_c - reference|
over this file was 0.053 of its bound.)"""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import junctiontree_amd as jt
from entropy_reference import EPS, brute_force_entropy, calibration_slack, entropy_reference, parity_bound
from junctiontree_amd import _capi, engine, synthetic
from sample_reference import schedule
from test_gpu_sample import README_FACTORS, README_SIZES, README_VALUES, RUNS, beliefs_of, case_of, make, spec_case, variants_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    gc.collect()
    yield
    engine.clear_plan_cache()


def check_parity(plan, case, what, batch=0, ref=None):
    """H, every h_c - and X, with a reference set - of evidence set `batch` within the bound of the restatement; returns (H, X, the
    summed bound, the slack for the rounding of the beliefs themselves)"""
    tree, _, node_vars, sizes, n = case
    sched = schedule(plan)
    a = beliefs_of(plan, n, batch)
    b = beliefs_of(plan, n, ref) if ref is not None else None
    want_h, want_x, per = entropy_reference(a, sched, node_vars, ref_beliefs=b)
    bound = parity_bound(a, sched, node_vars, ref_beliefs=b)
    got = plan.entropy(batch, batch + 1, ref=ref, per_clique=True)
    h, rows = got[0], got[-1]
    assert h.shape == (1,) and rows.shape == (1, n) and h.dtype == rows.dtype == np.float64
    worst = max(abs(rows[0, c] - per[c]) / bound[c] for c in range(n))
    total = sum(bound.values()) + n * EPS * abs(want_h)
    slack = calibration_slack(a, sched, node_vars, ref_beliefs=b)
    print("%s: H %.17g (reference %.17g), |H - reference| / bound %.3g, worst |h_c - reference| / bound %.3g" % (what, h[0], want_h, abs(h[0] - want_h) / total, worst))
    assert worst <= 1.0, what
    assert abs(h[0] - want_h) <= total, what
    assert np.all(rows >= -np.array([bound[c] for c in range(n)])), what
    if ref is None:
        return h[0], None, total, slack
    x = got[1][0]
    if np.isinf(want_x):
        assert x == np.inf, what
    else:
        print("%s: X %.17g (reference %.17g)" % (what, x, want_x))
        assert abs(x - want_x) <= sum(bound.values()) + n * EPS * abs(want_x), what
    return h[0], x, total, slack


# ---------------------------------------------------------------------------------------------- 1. parity with the restatement

@pytest.mark.parametrize("name,dtype,opts", RUNS, ids=["%s-%s%s" % (n, d, "-no_compact" if o else "") for n, d, o in RUNS])
def test_entropies_equal_the_restatement_on_the_plans_own_beliefs(name, dtype, opts):
    case = case_of(name)
    plan = make(case, dtype, **opts)
    d = plan.describe()
    if name == "contained":
        assert sorted(c["R"] for c in d["sample"]["cliques"])[:2] == [1, 1]
    if name == "root64k":
        assert max(c["R"] for c in d["sample"]["cliques"]) == 1 << 16          # (segments, and their merge)
    h = check_parity(plan, case, "%s %s" % (name, dtype))[0]
    assert h > 0.0
    plan.close()


# ---------------------------------------------------------------------------------------------- 2. layouts

@pytest.mark.parametrize("name", ["wide7", "random16_card5"])
def test_every_layout_agrees_within_the_bound_and_a_second_call_bit_for_bit(name):
    case = case_of(name)
    seen = {}
    for key, opts in variants_of({}).items():
        plan = make(case, "f64", **opts)
        h, _, total, slack = check_parity(plan, case, "%s %s" % (name, key))
        first = plan.entropy(per_clique=True)
        again = plan.entropy(per_clique=True)
        assert first[0][0] == h
        np.testing.assert_array_equal(first[0], again[0])
        np.testing.assert_array_equal(first[1], again[1])
        seen[key] = (h, total + slack)
        plan.close()
    # (two layouts add their messages in different orders, so their beliefs differ in the last bits: each plan's entropy lies within
    #  its bound and its beliefs' slack of the exact one)
    h0, t0 = seen["default"]
    for key, (h, total) in seen.items():
        print("%s: |H - H(default)| / (the two bounds and slacks) %.3g" % (key, abs(h - h0) / (t0 + total)))
        assert abs(h - h0) <= t0 + total, key


# ---------------------------------------------------------------------------------------------- 3. evidence

def chain5():
    return spec_case(synthetic.chain_tree(3, card=2, width=3), seed=7)


def readme():
    """the README network as a plan-level case: the clique potentials are the products of the cliques' factors, formed here"""
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    ct = tree.clique_tree
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]
    pots = []
    for c, labels in enumerate(ct.maxcliques):
        table = np.ones([README_SIZES[v] for v in labels])
        for f, mc in enumerate(ct.factor_to_maxclique):
            if mc == c:
                shape = [README_SIZES[v] if v in README_FACTORS[f] else 1 for v in labels]
                order = np.argsort([list(labels).index(v) for v in README_FACTORS[f]]).tolist()
                table = table * np.transpose(np.asarray(README_VALUES[f], dtype=np.float64), order).reshape(shape)
        pots.append(table)
    return (tree.tree, pots, node_vars, README_SIZES, len(ct.maxcliques)), README_FACTORS, README_VALUES


def chain5_model():
    case = chain5()
    tree, pots, node_vars, sizes, n = case
    return case, [list(vs) for vs in node_vars[:n]], pots[:n]


ENUMERATED = [("chain5", None), ("chain5", {2: 1}), ("chain5", {0: 1, 4: 0}), ("readme", None), ("readme", {"wet_grass": 1}), ("readme", {"cloudy": 0, "sprinkler": 1})]


@pytest.mark.parametrize("name,evidence", ENUMERATED, ids=["%s-%s" % (n, "free" if not e else "_".join(map(str, e))) for n, e in ENUMERATED])
def test_small_networks_against_enumeration(name, evidence):
    case, factors, values = chain5_model() if name == "chain5" else readme()
    plan = make(case, "f64", evidence={0: evidence} if evidence else None)
    h, _, total, slack = check_parity(plan, case, "%s %r" % (name, evidence))
    want = brute_force_entropy(factors, case[3], values, evidence)[0]
    print("%s %r: |H - enumeration| %.3g, bound %.3g + slack %.3g" % (name, evidence, abs(h - want), total, slack))
    assert abs(h - want) <= total + slack
    plan.close()


def test_evidence_on_every_variable_leaves_no_entropy_and_clearing_it_restores_the_first_value():
    case = case_of("random16_card3")
    tree, pots, node_vars, sizes, n = case
    plan = make(case, "f64")
    first = plan.entropy(per_clique=True)
    plan.set_evidence({v: (v * 7 + 1) % sizes[v] for v in sizes})
    plan.propagate()
    h, _, total, _ = check_parity(plan, case, "every variable observed")
    assert abs(h) <= total
    plan.set_evidence({})
    plan.propagate()
    again = plan.entropy(per_clique=True)
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. many sets, shared tables

def shared_plan(case, evidence_sets, dtype="f64", **opts):
    tree, pots, node_vars, sizes, n = case
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, n_batch=len(evidence_sets), share_potentials=True, **opts)
    for c in range(n):
        plan.set_potential(c, np.asarray(pots[c], dtype=np.float32 if dtype == "f32" else np.float64))
    for b, obs in enumerate(evidence_sets):
        plan.set_evidence(obs, batch=b)
    plan.propagate()
    return plan


def test_one_call_over_five_sets_equals_five_calls():
    case = case_of("chain6")
    n = case[4]
    sets = [{}, {0: 3}, {7: 15, 2: 0}, {3: 9}, {1: 1, 4: 4, 6: 6}]
    plan = shared_plan(case, sets)
    h, rows = plan.entropy(per_clique=True)
    assert h.shape == (5,) and rows.shape == (5, n) and len(set(h.tolist())) == 5
    for b in range(5):
        one, row = plan.entropy(b, b + 1, per_clique=True)
        assert one[0] == h[b]
        np.testing.assert_array_equal(row[0], rows[b])
        check_parity(plan, case, "set %d of five" % b, batch=b)
    assert np.all(np.abs(rows.sum(axis=1) - h) <= n * EPS * h)
    np.testing.assert_array_equal(plan.entropy(1, 4), h[1:4])
    plan.close()


# ---------------------------------------------------------------------------------------------- 5. cross-entropy

def test_the_posterior_against_the_prior_is_the_log_of_the_evidences_probability():
    case = case_of("chain6")
    n = case[4]
    plan = shared_plan(case, [{}, {2: 5, 6: 11}])
    h, x, total, _ = check_parity(plan, case, "posterior against prior", batch=1, ref=0)
    log_z = [plan.log_z(batch=b)[1] for b in range(2)]
    # (the summed bound: H's and X's)
    print("KL %.17g, ln Z0 - ln Z1 %.17g, difference / summed bound %.3g" % (x - h, log_z[0] - log_z[1], abs((x - h) - (log_z[0] - log_z[1])) / (2 * total)))
    assert abs((x - h) - (log_z[0] - log_z[1])) <= 2 * total
    # the other way round the reference lacks support: +inf, and no error
    ref = (C.c_int32 * 1)(1)
    out_h, out_x = np.zeros(1), np.zeros(1)
    rc = plan._lib.jtp_entropy(plan._handle, 0, 1, C.cast(ref, C.c_void_p), out_h.ctypes.data_as(C.c_void_p), out_x.ctypes.data_as(C.c_void_p), None)
    assert rc == _capi.JTP_OK and out_x[0] == np.inf and out_h[0] == plan.entropy(0, 1)[0]
    check_parity(plan, case, "prior against posterior", batch=0, ref=1)
    # a reference per set, inside the range or not; a set against itself: X = H up to the two sums' rounding
    h2, x2 = plan.entropy(0, 2, ref=[0, 0])
    assert x2[1] == x and abs(x2[0] - h2[0]) <= total
    plan.close()


def test_kl_between_two_potential_sets():
    case = case_of("random16_card3")
    tree, pots, node_vars, sizes, n = case
    rng = np.random.default_rng(31)
    other = [rng.uniform(0.5, 1.5, np.shape(p)) if c < n else p for c, p in enumerate(pots)]
    plan = engine.Plan(tree, node_vars, sizes, n_batch=2)
    for c in range(n):
        plan.set_potential(c, np.asarray(pots[c], dtype=np.float64), batch=0)
        plan.set_potential(c, other[c], batch=1)
    plan.propagate()
    kl = []
    for a, b in ((0, 1), (1, 0)):
        h, x, total, _ = check_parity(plan, case, "KL(%d || %d)" % (a, b), batch=a, ref=b)
        assert x - h >= -2 * total
        kl.append(x - h)
    assert kl[0] > 0 and kl[1] > 0 and kl[0] != kl[1]
    plan.close()


# ---------------------------------------------------------------------------------------------- 6. scaled plans

def test_scaled_plans_give_the_entropy_where_z_is_beyond_float64():
    """the model of `test_scaled_plans_sample_where_z_is_beyond_float64`: every table x 2^90, Z moved by 2^1350"""
    case = spec_case(synthetic.wide_binary_tree(15, 10, 5), seed=2)
    tree, pots, node_vars, sizes, n = case
    moved = [np.ldexp(p, 90) if c < n else p for c, p in enumerate(pots)]
    base = make(case, "f64", scaled=True)
    want, _, t0, s0 = check_parity(base, case, "scaled, unmoved")
    base.close()
    scaled = make(case, "f64", pots=moved, scaled=True)
    h, _, total, slack = check_parity(scaled, case, "scaled, every table x 2^90")
    print("moved against unmoved: |difference| %.3g, bounds %.3g + slacks %.3g" % (abs(h - want), t0 + total, s0 + slack))
    assert abs(h - want) <= t0 + total + s0 + slack              # (the same distribution, each plan's beliefs rounded on their own)
    scaled.close()
    plain = make(case, "f64", pots=moved)
    with pytest.raises(_capi.JtpError) as err:
        plain.entropy()
    assert re.search(r"1 of 1 evidence sets failed, the first set 0 at clique \d+", str(err.value)), str(err.value)
    assert np.isnan(err.value.entropy).all()
    plain.close()


def test_junction_tree_entropy_normalize():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    big = [np.ldexp(np.asarray(v, dtype=np.float64), 300) for v in README_VALUES]          # Z = 2^1200
    want = brute_force_entropy(README_FACTORS, README_SIZES, README_VALUES)[0]
    assert abs(tree.entropy(big, normalize=True) - want) <= 1e-12
    with pytest.raises(_capi.JtpError):
        tree.entropy(big)


# ---------------------------------------------------------------------------------------------- 7. failures and refusals

def zero_case():
    case = spec_case(synthetic.chain_tree(4, card=3, width=3), seed=3)
    pots = [np.array(p) for p in case[1]]
    pots[0][2, :, :] = 0.0                                   # variable 0 is never in state 2
    return case, pots


def test_a_failed_set_is_nan_and_the_other_sets_are_written():
    case, pots = zero_case()
    tree, _, node_vars, sizes, n = case
    # evidence of probability zero in set 1 of three
    plan = shared_plan((tree, pots, node_vars, sizes, n), [{}, {0: 2}, {1: 1}])
    good = [plan.entropy(b, b + 1, per_clique=True) for b in (0, 2)]
    with pytest.raises(_capi.JtpError) as err:
        plan.entropy(per_clique=True)
    assert re.search(r"1 of 3 evidence sets failed, the first set 1 at clique \d+", str(err.value)), str(err.value)
    h, rows = err.value.entropy, err.value.clique_entropy
    assert np.isnan(h[1]) and np.isnan(rows[1]).all() and h[0] == good[0][0][0] and h[2] == good[1][0][0]
    np.testing.assert_array_equal(rows[[0, 2]], np.concatenate([good[0][1], good[1][1]]))
    with pytest.raises(_capi.JtpError) as err:             # (as a reference it lacks all support: +inf for the set that names it, no failure of that set)
        plan.entropy(ref=[0, 0, 1])
    assert np.isnan(err.value.cross[1]) and err.value.cross[2] == np.inf and err.value.entropy[2] == good[1][0][0]
    assert plan.entropy(2, 3, ref=1)[1][0] == np.inf
    plan.close()
    # a signed table: one negative factor entry in set 1 of two
    signed = [np.array(p) for p in case[1]]
    signed[1][0, 1, 2] = -signed[1][0, 1, 2]
    plan = engine.Plan(tree, node_vars, sizes, n_batch=2)
    for c in range(n):
        plan.set_potential(c, case[1][c], batch=0)
        plan.set_potential(c, signed[c], batch=1)
    plan.propagate()
    assert min(plan.belief(c, batch=1).min() for c in range(n)) < 0
    with pytest.raises(_capi.JtpError) as err:
        plan.entropy()
    assert re.search(r"1 of 2 evidence sets failed, the first set 1", str(err.value))
    assert np.isnan(err.value.entropy[1]) and err.value.entropy[0] == plan.entropy(0, 1)[0] > 0
    with pytest.raises(_capi.JtpError) as err:             # ... and as a reference it fails the set that names it
        plan.entropy(0, 1, ref=1)
    assert np.isnan(err.value.entropy[0]) and np.isnan(err.value.cross[0])
    plan.close()


def test_refusals_say_why():
    case = spec_case(synthetic.wide_binary_tree(7, 8, 4))
    tree, pots, node_vars, sizes, n = case
    multi = engine.Plan(tree, node_vars, sizes, multiset=True, n_batch=8)
    for c in range(n):
        multi.set_potential(c, pots[c])
    multi.propagate()
    with pytest.raises(_capi.UnsupportedStructure, match="multi-set"):
        multi.entropy()
    multi.close()
    lean = engine.Plan(tree, node_vars, sizes, cover=[[] for _ in range(n)])
    lean.propagate()
    with pytest.raises(_capi.UnsupportedStructure, match="without `cover`"):
        lean.entropy()
    lean.close()
    plan = engine.Plan(tree, node_vars, sizes, n_batch=2)
    for c in range(n):
        plan.set_potential(c, pots[c], batch=0)
        plan.set_potential(c, pots[c], batch=1)
    lib, h = plan._lib, plan._handle
    out, x = np.full(2, -1.0), np.full(2, -1.0)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)
    ref = np.zeros(2, dtype=np.int32)
    assert lib.jtp_entropy(h, 0, 1, None, ptr(out), None, None) == _capi.JTP_EINVAL               # never propagated
    assert b"not been propagated" in lib.jtp_last_error()
    plan.propagate(0, 1)
    assert lib.jtp_entropy(h, 0, 1, None, ptr(out), None, None) == _capi.JTP_OK and out[0] > 0
    assert lib.jtp_entropy(h, 0, 2, None, ptr(out), None, None) == _capi.JTP_EINVAL               # set 1 never propagated
    ref[0] = 1
    assert lib.jtp_entropy(h, 0, 1, ptr(ref), ptr(out), ptr(x), None) == _capi.JTP_EINVAL         # ... nor as a reference
    plan.propagate()
    assert lib.jtp_entropy(h, 0, 2, ptr(ref), ptr(out), ptr(x), None) == _capi.JTP_OK
    assert lib.jtp_entropy(h, 0, 2, ptr(ref), ptr(out), None, None) == _capi.JTP_EINVAL           # one of ref_set and cross
    assert lib.jtp_entropy(h, 0, 2, None, ptr(out), ptr(x), None) == _capi.JTP_EINVAL
    assert lib.jtp_entropy(h, 0, 2, None, None, None, None) == _capi.JTP_EINVAL                   # no entropy
    ref[1] = 2
    assert lib.jtp_entropy(h, 0, 2, ptr(ref), ptr(out), ptr(x), None) == _capi.JTP_EINVAL         # a reference out of range
    ref[1] = -1
    assert lib.jtp_entropy(h, 0, 2, ptr(ref), ptr(out), ptr(x), None) == _capi.JTP_EINVAL
    for begin, end in ((0, 3), (1, 1), (2, 1), (-1, 1)):
        assert lib.jtp_entropy(h, begin, end, None, ptr(out), None, None) == _capi.JTP_EINVAL, (begin, end)
    plan.close()


# ---------------------------------------------------------------------------------------------- 8. no side effects

def read_messages(plan):
    """the whole message arena half of evidence set 0 (`jtp_debug_read_msg`)"""
    n = int(plan.describe()["msg_doubles"])
    out = np.zeros(n)
    _capi.check(plan._lib.jtp_debug_read_msg(plan._handle, 0, 0, n, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


@pytest.mark.parametrize("opts", [{}, dict(level_launches=True), dict(scaled=True)], ids=["flow", "level", "scaled"])
def test_entropy_leaves_beliefs_and_messages_alone(opts):
    case = case_of("wide7")
    plan = make(case, "f64", evidence={0: {sorted(case[3])[2]: 1}}, **opts)
    n_nodes = len(case[2])
    before = [plan.belief(node) for node in range(n_nodes)]
    msgs = read_messages(plan)
    z = plan.log_z()
    first = plan.entropy(ref=0, per_clique=True)
    for a, b in zip(before, [plan.belief(node) for node in range(n_nodes)]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(read_messages(plan), msgs)
    assert plan.log_z() == z
    plan.propagate()                                         # ... and the next propagate finds its messages as it left them
    for a, b in zip(before, [plan.belief(node) for node in range(n_nodes)]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(first, plan.entropy(ref=0, per_clique=True)):
        np.testing.assert_array_equal(a, b)
    plan.close()


# ---------------------------------------------------------------------------------------------- 9. allocation failures

def live_bytes():
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().jtp_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def test_the_call_survives_the_failure_of_each_of_its_allocations():
    case = case_of("root64k")
    sets = [{}, {sorted(case[3])[0]: 1}, {sorted(case[3])[5]: 0}]
    fresh = shared_plan(case, sets)
    want = fresh.entropy(0, 1, per_clique=True)
    want_all = fresh.entropy(ref=[1, 2, 0])
    fresh.close()
    plan = shared_plan(case, sets)
    failed = 0
    for n in range(1, 16):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            got = plan.entropy(0, 1, per_clique=True)
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    assert failed == n - 1 and failed >= 2, (failed, n)          # the records, the work area
    plan.debug_set("fail_alloc", 0)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    # three sets with references need a larger work area: the allocation failing leaves the smaller one in place, and it still serves
    before = live_bytes()
    plan.debug_set("fail_alloc", 1)
    with pytest.raises(MemoryError):
        plan.entropy(ref=[1, 2, 0])
    assert live_bytes() == before
    plan.debug_set("fail_alloc", 0)
    np.testing.assert_array_equal(plan.entropy(0, 1), want[0])
    for a, b in zip(plan.entropy(ref=[1, 2, 0]), want_all):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(plan.entropy(0, 1), want[0])
    plan.close()


# ---------------------------------------------------------------------------------------------- 10. JunctionTree

def test_junction_tree_entropy_and_kl_against_enumeration():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    before = tree.propagate(README_VALUES)
    sets = [None, {"wet_grass": 1}, {"cloudy": 0, "sprinkler": 1}]
    want = [brute_force_entropy(README_FACTORS, README_SIZES, README_VALUES, ev)[0] for ev in sets]
    for ev, w in zip(sets, want):
        got = tree.entropy(README_VALUES, evidence=ev)
        assert isinstance(got, float) and abs(got - w) <= 1e-12, ev
    many = tree.entropy_evidence_sets(README_VALUES, sets)
    assert many.shape == (3,) and np.max(np.abs(many - np.array(want))) <= 1e-12
    assert tree.entropy_evidence_sets(README_VALUES, []).shape == (0,)
    assert abs(tree.entropy(README_VALUES) - want[0]) <= 1e-12             # the evidence does not stick to the cached plan
    rng = np.random.default_rng(5)
    other = [np.asarray(v, dtype=np.float64) * rng.uniform(0.5, 1.5, np.shape(v)) for v in README_VALUES]
    for ev in (None, {"rain": 1}):
        for p, q in ((README_VALUES, other), (other, README_VALUES)):
            w = brute_force_entropy(README_FACTORS, README_SIZES, p, ev, values_q=q)[2]
            got = tree.kl_divergence(p, q, evidence=ev)
            assert w > 0 and abs(got - w) <= 1e-12
    # against itself: 0 within the bound of H and of X on the plan the call ran on (the cached plan of two sets, its beliefs still there)
    same = tree.kl_divergence(README_VALUES, README_VALUES)
    plan = tree._table_plan("plan_kl", "f64", False, n_batch=2)
    n = len(tree.clique_tree.maxcliques)
    node_vars = [list(c) for c in tree.clique_tree.maxcliques] + [list(s) for s in tree.separators]
    bound = parity_bound(beliefs_of(plan, n, 0), schedule(plan), node_vars, ref_beliefs=beliefs_of(plan, n, 1))
    print("KL(v || v) = %.3g, bound %.3g" % (same, 2 * sum(bound.values())))
    assert 0.0 <= same <= 2 * sum(bound.values())
    # Q rules out rain under a clear sky where P does not: no support
    holed = [np.array(v, dtype=np.float64) for v in README_VALUES]
    holed[2][:, 1] = [0.0, 1e-3]
    holed[2][0, 0] = 1.0
    assert tree.kl_divergence(README_VALUES, holed) == float("inf")
    assert np.isfinite(tree.kl_divergence(holed, README_VALUES))
    with pytest.raises(_capi.JtpError):                     # evidence of probability zero
        tree.entropy(README_VALUES, evidence={"sprinkler": 0, "rain": 0, "wet_grass": 1})
    for a, b in zip(before, tree.propagate(README_VALUES)):
        np.testing.assert_array_equal(a, b)
