"""Joint posterior samples drawn on the device (`jtp_sample`, kernel `jt_sample_level`) on a real MI355X.

What is checked is the definition, not a distribution fit: for every clique and every sample, the entry the returned states name
is the inverse CDF of the slice of the clique's belief that the sample's earlier digits select, at the uniform
`synthetic.sample_uniform(seed, clique, i)` - with the beliefs read back from the same plan (`tests/sample_reference.py`).  The
tolerance is the float64 summation bound of a slice of R entries, 4 R 2^-53 total, on both sides; a drawn entry is never zero."""
import itertools
import re

import numpy as np
import pytest

import junctiontree_amd as jt
from junctiontree_amd import _capi, engine, synthetic
from sample_reference import clique_draws, schedule
from test_planner_emulated import star

pytestmark = pytest.mark.gpu

N = 61          # not a multiple of the four samples of a workgroup


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


def spec_case(spec, seed=5):
    return spec["tree"], synthetic.potentials_for(spec, seed=seed), spec["node_vars"], spec["sizes"], spec["n_cliques"]


def star_case(n_children):
    tree, pots, node_vars, sizes = star(n_children, card=2, seed=n_children)
    return tree, pots, node_vars, sizes, n_children + 1


def contained_case():
    """clique 1 lies inside its parent (nothing to draw there, R = 1), clique 3 inside clique 2"""
    rng = np.random.default_rng(8)
    node_vars = [[0, 1, 2, 3], [1, 2], [2, 3, 4], [4, 2], [1, 2], [2, 3], [2, 4]]
    sizes = {0: 3, 1: 2, 2: 3, 3: 2, 4: 5}
    tree = [0, (4, [1]), (5, [2, (6, [3])])]
    pots = [rng.uniform(0.5, 1.5, [sizes[v] for v in vs]) for vs in node_vars[:4]] + [np.ones([sizes[v] for v in vs]) for vs in node_vars[4:]]
    return tree, pots, node_vars, sizes, 4


CASES = {
    "wide7": lambda: spec_case(synthetic.wide_binary_tree(7, 12, 6)),
    "chain6": lambda: spec_case(synthetic.chain_tree(6, 16, 3)),
    "random16_card3": lambda: spec_case(synthetic.random_tree(16, 6, 3, card=3)),
    "random16_card5": lambda: spec_case(synthetic.random_tree(16, 6, 3, card=5)),
    "random16_card6": lambda: spec_case(synthetic.random_tree(16, 6, 3, card=6)),
    "random16_card7": lambda: spec_case(synthetic.random_tree(16, 6, 3, card=7)),
    "star5": lambda: star_case(5),
    "contained": contained_case,
    "root64k": lambda: spec_case(synthetic.wide_binary_tree(3, 16, 4)),
}
_built = {}


def case_of(name):
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


def make(case, dtype="f64", pots=None, evidence=None, n_batch=1, **opts):
    tree, base, node_vars, sizes, n = case
    pots = base if pots is None else pots
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, n_batch=n_batch, **opts)
    np_t = np.float32 if dtype == "f32" else np.float64
    for b in range(n_batch):
        for c in range(n):
            plan.set_potential(c, np.asarray(pots[c], dtype=np_t), batch=b)
    if evidence:
        for b, obs in evidence.items():
            plan.set_evidence(obs, batch=b)
    plan.propagate()
    return plan


def beliefs_of(plan, n, batch=0):
    """the numbers the kernel read: every clique belief in the storage type, widened"""
    np_t = np.float32 if plan.dtype == _capi.JTP_F32 else np.float64
    return [plan.belief(c, batch=batch, dtype=np_t).astype(np.float64) for c in range(n)]


def check_inverse_cdf(plan, case, states, seed, batch=0, beliefs=None, first=0):
    """`states`: samples first .. first + len(states) - 1 of a call with `seed`"""
    tree, _, node_vars, sizes, n = case
    count = states.shape[0]
    columns = {lab: j for j, lab in enumerate(plan.var_labels)}
    assert states.dtype == np.int32 and states.shape == (count, len(columns))
    for lab, j in columns.items():
        assert states[:, j].min() >= 0 and states[:, j].max() < sizes[lab], "variable %r out of range" % (lab,)
    beliefs = beliefs_of(plan, n, batch) if beliefs is None else beliefs
    sched = schedule(plan)
    assert sorted(s[0] for s in sched) == list(range(n))
    for clique, parent, depth, K, F, R in sched:
        got = clique_draws(beliefs[clique], list(node_vars[clique]), K, F, states, columns)
        assert got["slice"].shape == (count, R)
        u = synthetic.sample_uniform(seed, plan.abi_of[clique], first + count)[first:]
        total = got["total"]
        tol = 4.0 * R * 2.0 ** -53 * total
        target = u * total
        what = "clique %d (R = %d)" % (clique, R)
        print(what, "worst (lo - target) / tol %.3g, (target - hi) / tol %.3g, min w / total %.3g"
              % (np.max((got["lo"] - target) / tol), np.max((target - got["hi"]) / tol), np.min(got["w"] / total)))
        assert np.all(total > 0) and np.all(np.isfinite(total)), what
        assert np.all(got["w"] > 0), what + ": an entry without mass was drawn"
        assert np.all(got["lo"] - tol <= target), what + ": the drawn entry begins beyond u * total"
        assert np.all(target <= got["hi"] + tol), what + ": the drawn entry ends before u * total"
    return beliefs


# ---------------------------------------------------------------------------------------------- 1. inverse CDF

RUNS = [("wide7", "f64", {}), ("wide7", "f32", {}), ("chain6", "f64", {}), ("chain6", "f32", {}),
        ("random16_card3", "f64", {}), ("random16_card5", "f64", {}), ("random16_card6", "f64", {}), ("random16_card7", "f64", {}),
        ("random16_card3", "f32", {}), ("random16_card5", "f32", {}), ("random16_card6", "f32", {}), ("random16_card7", "f32", {}),
        ("random16_card3", "f64", dict(no_compact=True)), ("random16_card5", "f32", dict(no_compact=True)),
        ("random16_card6", "f64", dict(no_compact=True)), ("random16_card7", "f32", dict(no_compact=True)),
        ("star5", "f64", {}), ("star5", "f32", {}), ("contained", "f64", {}), ("contained", "f32", {}),
        ("root64k", "f64", {}), ("root64k", "f32", {})]


@pytest.mark.parametrize("name,dtype,opts", RUNS, ids=["%s-%s%s" % (n, d, "-no_compact" if o else "") for n, d, o in RUNS])
def test_every_draw_is_the_inverse_cdf_of_its_slice(name, dtype, opts):
    case = case_of(name)
    plan = make(case, dtype, **opts)
    d = plan.describe()
    if name == "star5":
        assert any(p["real"] < 0 for p in d["pnodes"])
    if name == "contained":
        assert sorted(c["R"] for c in d["sample"]["cliques"])[:2] == [1, 1]
    if name == "root64k":
        assert max(c["R"] for c in d["sample"]["cliques"]) == 1 << 16
    if name.startswith("random16") and not opts:
        assert d["compact"] == 1
    states = plan.sample(N, seed=11)
    check_inverse_cdf(plan, case, states, 11)
    plan.close()


def test_the_cardinality_cases_cover_split_variables_and_mixed_radix_rows():
    """what the cardinality cases are there for: some plan among them stores rows at true cardinalities with a variable across the
    thread part's top bit, some plan keeps plain bit fields"""
    split, mixed, plain = False, False, False
    for name, dtype in itertools.product(("random16_card3", "random16_card5", "random16_card6", "random16_card7"), ("f64", "f32")):
        tree, _, node_vars, sizes, n = case_of(name)
        d = engine.Plan(tree, node_vars, sizes, dtype=dtype, plan_only=True).describe()
        split = split or any(p["split_var"] >= 0 for p in d["pack"])
        mixed = mixed or d["tmix"] == 1
        plain = plain or d["tmix"] == 0
    assert split and mixed and plain


# ---------------------------------------------------------------------------------------------- 2. layout independence

LAYOUTS = {"default": {}, "policy1": dict(layout_policy=1), "policy2": dict(layout_policy=2), "policy3": dict(layout_policy=3),
           "keep_root": dict(keep_root=True)}


def variants_of(extra):
    """every layout with dataflow launches (the default) and with one launch per level"""
    layouts = dict(LAYOUTS)
    layouts.update(extra)
    out = {}
    for key, opts in layouts.items():
        out[key] = dict(opts)
        out[key + "+level"] = dict(opts, level_launches=True)
    return out


def beliefs_and_samples(case, variants, pots=None):
    n = case[4]
    got = {}
    for key, opts in variants.items():
        plan = make(case, "f64", pots=pots, **opts)
        order = [plan.var_labels.index(lab) for lab in sorted(plan.var_labels)]      # (columns by label: the same for every plan anyway)
        got[key] = (beliefs_of(plan, n), plan.sample(N, seed=3)[:, order])
        plan.close()
    return got


def test_exactly_equal_beliefs_give_equal_samples_in_every_layout():
    """The order a slice is summed in is a function of its length alone, so plans that hold the same beliefs draw the same samples,
    whatever their bit order, root, launch mode or row format.  To have the SAME beliefs in every layout - plans sum their messages in
    an order that follows the layout, so rounded beliefs differ in the last bit - the potentials of the (7, 12, 6) tree are small
    integers here: every product is at most 3^7, every sum runs over at most 2^36 assignments, so every message and belief is an
    integer below 2^53 and exact in whatever order it is formed."""
    case = case_of("wide7")
    tree, _, node_vars, sizes, n = case
    rng = np.random.default_rng(12)
    pots = [rng.integers(1, 4, size=[sizes[v] for v in vs]).astype(np.float64) for vs in node_vars[:n]] + [np.ones([sizes[v] for v in vs]) for vs in node_vars[n:]]
    got = beliefs_and_samples(case, variants_of({"no_compact": dict(no_compact=True)}), pots=pots)
    ref_bel, ref_samples = got["default"]
    assert all(np.all(b == np.rint(b)) and b.max() < 2.0 ** 53 for b in ref_bel)
    for key, (bel, samples) in got.items():
        for c in range(n):
            np.testing.assert_array_equal(bel[c], ref_bel[c], err_msg="%s: belief of clique %d" % (key, c))
        np.testing.assert_array_equal(samples, ref_samples, err_msg="%s: equal beliefs, different samples" % key)


@pytest.mark.parametrize("name,extra", [("wide7", {}), ("random16_card3", {"no_compact": dict(no_compact=True)})], ids=["wide7", "card3"])
def test_equal_beliefs_give_equal_samples_whatever_the_layout(name, extra):
    """The same on rounded beliefs (synthetic potentials).  Messages are summed in the same order only where the layout of the
    messages is the same, so the beliefs of two plans may differ in the last bit: samples are compared between the plans whose beliefs
    are `array_equal`.  Those always include every layout - `layout_policy` 1, 2, 3 and the default, `keep_root`, `no_compact` -
    launched as a dataflow plan against the same layout launched per level (the propagate is bit-identical across launch modes,
    tests/test_gpu_scaled.py); every other pair that happens to hold equal beliefs is compared as well and printed.  On an MI355X
    these are, on both trees, the default plan and `keep_root` (the given root already is the centre) in either launch mode; plans of
    different `layout_policy`, and `no_compact` against the compact rows, differ in the last bit of some belief - those layouts are
    compared by the test above, on beliefs that are exact."""
    case = case_of(name)
    variants = variants_of(extra)
    got = beliefs_and_samples(case, variants)
    for a, b in itertools.combinations(sorted(got), 2):
        same = all(np.array_equal(x, y) for x, y in zip(got[a][0], got[b][0]))
        if same or a + "+level" == b:
            print("%s / %s: beliefs %s, samples %s" % (a, b, "equal" if same else "DIFFER", "equal" if np.array_equal(got[a][1], got[b][1]) else "differ"))
        if a + "+level" == b:
            assert same, "%s: per-level and dataflow launches give different beliefs" % a
        if same:
            np.testing.assert_array_equal(got[a][1], got[b][1], err_msg="%s vs %s: equal beliefs, different samples" % (a, b))


# ---------------------------------------------------------------------------------------------- 3. counter based

def test_samples_are_counter_based():
    case = case_of("wide7")
    plan = make(case, "f32")
    a = plan.sample(2 * N, seed=9)
    np.testing.assert_array_equal(plan.sample(2 * N, seed=9), a)
    np.testing.assert_array_equal(plan.sample(N, seed=9), a[:N])
    one = plan.sample(1, seed=9)
    assert one.shape == (1, a.shape[1])
    np.testing.assert_array_equal(one, a[:1])
    assert not np.array_equal(plan.sample(2 * N, seed=10), a)
    # a call that needs several chunks of the state buffer (more than 65536 rows) continues the same stream
    big = plan.sample(65536 + 7, seed=9)
    np.testing.assert_array_equal(big[:2 * N], a)
    assert big.shape[0] == 65536 + 7
    check_inverse_cdf(plan, case, big[-N:], 9, first=65536 + 7 - N)        # (rows of the second chunk)
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. evidence

def test_observed_variables_come_out_observed_and_clearing_restores_the_samples():
    case = case_of("wide7")
    tree, pots, node_vars, sizes, n = case
    probe = engine.Plan(tree, node_vars, sizes, plan_only=True)
    sched = schedule(probe)
    in_k = sorted({v for s in sched for v in s[3]})
    only_f = sorted(set(probe.var_labels) - set(in_k))
    obs = {in_k[0]: 1, only_f[-1]: 0}
    plan = make(case, "f64", n_batch=2)
    before = [plan.sample(N, seed=4, batch=b) for b in range(2)]
    np.testing.assert_array_equal(before[0], before[1])                      # (two sets holding the same potentials)
    plan.set_evidence(obs, batch=1)
    plan.propagate()
    col = {lab: j for j, lab in enumerate(plan.var_labels)}
    with_ev = plan.sample(N, seed=4, batch=1)
    for lab, st in obs.items():
        assert np.all(with_ev[:, col[lab]] == st)
    assert not np.array_equal(with_ev, before[1])
    check_inverse_cdf(plan, case, with_ev, 4, batch=1)
    np.testing.assert_array_equal(plan.sample(N, seed=4, batch=0), before[0])      # set 0 never saw the evidence
    plan.set_evidence({}, batch=1)
    plan.propagate()
    np.testing.assert_array_equal(plan.sample(N, seed=4, batch=1), before[1])
    plan.close()


# ---------------------------------------------------------------------------------------------- 5. scaled plans

def test_scaled_plans_sample_where_z_is_beyond_float64():
    spec = synthetic.wide_binary_tree(15, 10, 5)
    case = spec_case(spec, seed=2)
    tree, pots, node_vars, sizes, n = case
    level = make(case, "f64", level_launches=True)
    want = level.sample(N, seed=6)
    check_inverse_cdf(level, case, want, 6)
    level.close()
    scaled = make(case, "f64", scaled=True)
    np.testing.assert_array_equal(scaled.sample(N, seed=6), want)
    scaled.close()
    for shift in (90, -90):                                                  # Z moves by 2^(+-1350)
        moved = [np.ldexp(p, shift) if c < n else p for c, p in enumerate(pots)]
        scaled = make(case, "f64", pots=moved, scaled=True)
        got = scaled.sample(N, seed=6)
        np.testing.assert_array_equal(got, want, err_msg="every table x 2^%d" % shift)
        check_inverse_cdf(scaled, case, got, 6)
        scaled.close()
        plain = make(case, "f64", pots=moved)
        with pytest.raises(_capi.JtpError) as err:
            plain.sample(N, seed=6)
        assert np.all(err.value.states == -1)
        plain.close()


# ---------------------------------------------------------------------------------------------- 6. distribution

README_FACTORS = [["cloudy"], ["cloudy", "sprinkler"], ["cloudy", "rain"], ["rain", "sprinkler", "wet_grass"]]
README_SIZES = {"cloudy": 2, "sprinkler": 2, "rain": 2, "wet_grass": 2}
README_VALUES = [np.array([0.5, 0.5]), np.array([[0.5, 0.5], [0.9, 0.1]]), np.array([[0.8, 0.2], [0.2, 0.8]]),
                 np.array([[[1, 0], [0.1, 0.9]], [[0.1, 0.9], [0.01, 0.99]]])]


def brute_force(factors, sizes, values, evidence):
    labels = sorted(sizes, key=str)
    letters = {lab: chr(ord("a") + i) for i, lab in enumerate(labels)}
    expr = ",".join("".join(letters[v] for v in f) for f in factors) + "->" + "".join(letters[v] for v in labels)
    joint = np.einsum(expr, *[np.asarray(v, dtype=np.float64) for v in values])
    for lab, st in (evidence or {}).items():
        mask = np.zeros(sizes[lab])
        mask[st] = 1.0
        shape = [1] * len(labels)
        shape[labels.index(lab)] = sizes[lab]
        joint = joint * mask.reshape(shape)
    return labels, joint / joint.sum()


def check_frequencies(labels, joint, columns, count):
    flat = np.ravel_multi_index([columns[lab] for lab in labels], joint.shape)
    freq = np.bincount(flat, minlength=joint.size).reshape(joint.shape) / count
    bound = 5.0 * np.sqrt(joint * (1.0 - joint) / count) + 1.0 / count
    print("worst |freq - p| / bound: %.3f" % np.max(np.abs(freq - joint) / bound))
    assert np.all(np.abs(freq - joint) <= bound)


@pytest.mark.parametrize("evidence", [None, {"wet_grass": 1}, {"cloudy": 0, "sprinkler": 1}], ids=["free", "wet", "cloudy_sprinkler"])
def test_frequencies_of_the_readme_network_match_the_posterior(evidence):
    count = 20000
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    out = tree.sample(README_VALUES, count, seed=2024, evidence=evidence)
    labels, joint = brute_force(README_FACTORS, README_SIZES, README_VALUES, evidence)
    check_frequencies(labels, joint, out, count)


@pytest.mark.parametrize("evidence", [None, {2: 1}], ids=["free", "middle_observed"])
def test_frequencies_of_a_chain_of_five_binary_variables_match_the_posterior(evidence):
    count = 20000
    spec = synthetic.chain_tree(3, card=2, width=3)
    case = spec_case(spec, seed=7)
    tree, pots, node_vars, sizes, n = case
    plan = make(case, "f64", evidence={0: evidence} if evidence else None)
    states = plan.sample(count, seed=2024)
    labels, joint = brute_force(node_vars[:n], sizes, pots[:n], evidence)
    check_frequencies(labels, joint, {lab: states[:, j] for j, lab in enumerate(plan.var_labels)}, count)
    plan.close()


# ---------------------------------------------------------------------------------------------- 7. failure

def test_evidence_of_probability_zero_is_reported_with_the_states():
    spec = synthetic.chain_tree(4, card=3, width=3)
    case = spec_case(spec, seed=3)
    tree, pots, node_vars, sizes, n = case
    pots = [np.array(p) for p in pots]
    pots[0][2, :, :] = 0.0                                   # variable 0 is never in state 2
    plan = make(case, "f64", pots=pots, evidence={0: {0: 2}})
    assert plan.z() == 0.0
    with pytest.raises(_capi.JtpError) as err:
        plan.sample(N, seed=1)
    msg = str(err.value)
    m = re.search(r"(\d+) \(clique, sample\) pairs.*clique (\d+)", msg)
    assert m, msg
    assert int(m.group(1)) == N * n and int(m.group(2)) == 0              # every clique of every sample; the root met it first
    states = err.value.states
    assert states.shape == (N, len(plan.var_labels)) and np.all(states == -1)
    # the evidence gone, the same plan samples again, and every state is in range
    plan.set_evidence({})
    plan.propagate()
    good = plan.sample(N, seed=1)
    assert good.min() >= 0 and good.max() < 3 and np.all(good[:, plan.var_labels.index(0)] < 2)
    plan.close()


# ---------------------------------------------------------------------------------------------- 8. refusals and API

def test_plans_without_belief_tables_refuse():
    spec = synthetic.wide_binary_tree(7, 8, 4)
    case = spec_case(spec)
    tree, pots, node_vars, sizes, n = case
    multi = engine.Plan(tree, node_vars, sizes, multiset=True, n_batch=8)
    for c in range(n):
        multi.set_potential(c, pots[c])
    multi.propagate()
    with pytest.raises(_capi.UnsupportedStructure, match="multi-set"):
        multi.sample(4)
    multi.close()
    lean = engine.Plan(tree, node_vars, sizes, cover=[[] for _ in range(n)])
    assert lean.describe()["has_unit"] == 1
    lean.propagate()
    with pytest.raises(_capi.UnsupportedStructure, match="without `cover`"):
        lean.sample(4)
    lean.close()
    plan = make(case)
    with pytest.raises(ValueError):
        plan.sample(0)
    with pytest.raises(ValueError):
        plan.sample(-3)
    plan.close()
    fresh = engine.Plan(tree, node_vars, sizes)
    with pytest.raises(ValueError, match="not been propagated"):
        fresh.sample(4)
    fresh.close()


def test_junction_tree_sample():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    before = tree.propagate(README_VALUES)
    out = tree.sample(README_VALUES, 50, seed=1)
    assert sorted(out) == sorted(README_SIZES)
    for lab, col in out.items():
        assert col.dtype == np.int32 and col.shape == (50,) and col.min() >= 0 and col.max() < 2
    # wet grass is impossible with the sprinkler off and no rain
    assert not np.any((out["sprinkler"] == 0) & (out["rain"] == 0) & (out["wet_grass"] == 1))
    again = tree.sample(README_VALUES, 50, seed=1)
    for lab in out:
        np.testing.assert_array_equal(out[lab], again[lab])
    obs = tree.sample(README_VALUES, 50, seed=1, evidence={"rain": 1, "cloudy": 0})
    assert np.all(obs["rain"] == 1) and np.all(obs["cloudy"] == 0)
    free = tree.sample(README_VALUES, 50, seed=1)                         # the evidence does not stick to the cached plan
    for lab in out:
        np.testing.assert_array_equal(out[lab], free[lab])
    # every factor x 2^90 on the overflow-safe plan: the same distribution, the same draws
    big = [np.ldexp(np.asarray(v, dtype=np.float64), 90) for v in README_VALUES]
    scaled = tree.sample(big, 50, seed=1, normalize=True)
    base = tree.sample(README_VALUES, 50, seed=1, normalize=True)
    for lab in out:
        np.testing.assert_array_equal(scaled[lab], base[lab])
    after = tree.propagate(README_VALUES)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    # arbitrary hashable labels
    factors = [[("x", 0), "y"], ["y", 3], [3, frozenset({1, 2})]]
    sizes = {("x", 0): 3, "y": 2, 3: 4, frozenset({1, 2}): 2}
    rng = np.random.default_rng(0)
    values = [rng.uniform(0.5, 1.5, [sizes[v] for v in f]) for f in factors]
    other = jt.create_junction_tree(factors, sizes)
    got = other.sample(values, 33, seed=5)
    assert set(got) == set(sizes)
    for lab, col in got.items():
        assert col.shape == (33,) and col.min() >= 0 and col.max() < sizes[lab]
