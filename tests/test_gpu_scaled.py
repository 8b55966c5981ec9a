"""The overflow-safe propagate (JTP_SCALED: every message divided by a power of two as it is produced, `jt_rescale_level`) on a
real MI355X.

Powers of two commute exactly with every multiply and add downstream, so on in-range inputs a scaled plan returns the unscaled
plan's tables bit for bit, up to one known exponent per node (`Plan.log2_scale`): those checks use `array_equal`.  Against the
oracle the project's tolerances hold (float64 storage 1e-11, float32 storage 1e-6).  A logarithm is compared to
rtol * max(1, |log|): two roundings of a number of that size are ~5e-13 of it."""
import math

import numpy as np
import pytest

import jt_oracle as oracle
import junctiontree_amd as jt
from junctiontree_amd import engine, synthetic
from test_planner_emulated import star

pytestmark = pytest.mark.gpu

RTOL = {"f64": 1e-11, "f32": 1e-6}
LN2 = math.log(2.0)


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


def close(got, want, rtol, what=""):
    got = np.asarray(got, dtype=np.float64)
    want = np.broadcast_to(np.asarray(want, dtype=np.float64), got.shape)
    scale = np.max(np.abs(want)) if want.size else 0.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-30 * scale + 1e-300, err_msg=what)


def log_close(got, want, rtol):
    return abs(got - want) <= rtol * max(1.0, abs(want))


def spec_case(spec, seed=5):
    return spec["tree"], synthetic.potentials_for(spec, seed=seed), spec["node_vars"], spec["sizes"], spec["n_cliques"]


def star_case(n_children):
    tree, pots, node_vars, sizes = star(n_children, card=2, seed=n_children)
    return tree, pots, node_vars, sizes, n_children + 1


REDUCE_OPTS = dict(block_log2=10, layout_policy=3)
PARITY = {
    "wide31": (lambda: spec_case(synthetic.wide_binary_tree(n_cliques=31, width=15, sep=7), seed=2), dict(block_log2=11), None),
    "reduce_wide": (lambda: spec_case(synthetic.wide_binary_tree(n_cliques=15, width=14, sep=7, card=2, seed=2)), REDUCE_OPTS, "2"),
    "reduce_random": (lambda: spec_case(synthetic.random_tree(n_cliques=9, width=13, sep=5, card=2, seed=3)), REDUCE_OPTS, "2"),
    "reduce_chain": (lambda: spec_case(synthetic.chain_tree(n_cliques=6, card=16, width=3)), REDUCE_OPTS, "2"),
    "card3": (lambda: spec_case(synthetic.wide_binary_tree(n_cliques=7, width=8, sep=4, card=3, seed=3), seed=11), {}, None),
    "card5": (lambda: spec_case(synthetic.wide_binary_tree(n_cliques=7, width=6, sep=3, card=5, seed=5), seed=11), {}, None),
    "card6": (lambda: spec_case(synthetic.wide_binary_tree(n_cliques=7, width=5, sep=2, card=6, seed=6), seed=11), {}, None),
    "star4": (lambda: star_case(4), {}, None),
    "star7": (lambda: star_case(7), {}, None),
}


def run(case, dtype, pots=None, **opts):
    """every belief, every exponent, z and (sign, log|Z|) of one plan after one propagate"""
    tree, base, node_vars, sizes, n = case
    pots = base if pots is None else pots
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, **opts)
    for c in range(n):
        plan.set_potential(c, np.asarray(pots[c], dtype=np.float32 if dtype == "f32" else np.float64))
    plan.propagate()
    out = {"bel": [plan.belief(node) for node in range(len(node_vars))],
           "e": [plan.log2_scale(node) for node in range(len(node_vars))],
           "log_z": plan.log_z(), "desc": plan.describe(), "stats": plan.stats()}
    with np.errstate(over="ignore"):
        out["z"] = plan.z()
    out["marg"] = plan.marginals([(c, node_vars[c][:2]) for c in range(n)])
    plan.close()
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(PARITY))
def test_in_range_a_scaled_plan_returns_the_unscaled_tables_bit_for_bit(name, dtype, monkeypatch):
    make, opts, reduce_min = PARITY[name]
    if reduce_min:
        monkeypatch.setenv("JTP_REDUCE_MIN", reduce_min)
    case = make()
    scaled = run(case, dtype, scaled=True, **opts)
    level = run(case, dtype, level_launches=True, **opts)
    flow = run(case, dtype, **opts)
    d = scaled["desc"]
    assert d["scaled"] == 1 and scaled["stats"]["launch_mode"] == "level" and flow["stats"]["launch_mode"] == "flow"
    n_rescale = sum(1 for kind, _, _ in d["steps"] if kind == 2)
    assert n_rescale > 0 and scaled["stats"]["n_launches"] == level["stats"]["n_launches"] + n_rescale
    if reduce_min and (name, dtype) != ("reduce_chain", "f32"):       # reduce tasks behind producers of several copies (the chain's
        # float32 rows are wide enough for one copy per message)
        assert any(t["kind"] == 1 for t in d["tasks"]) and any(s["up_npart"] > 1 or s["dn_npart"] > 1 for s in d["pseps"])
    if name == "wide31":  # messages whose consumers sum several copies themselves
        assert any(s["up_rnpart"] > 1 or s["dn_rnpart"] > 1 for s in d["pseps"])
    if name.startswith("star"):
        assert any(p["real"] < 0 for p in d["pnodes"])
    assert any(scaled["e"]) and not any(level["e"]) and not any(flow["e"])
    for node, (b, e) in enumerate(zip(scaled["bel"], scaled["e"])):
        np.testing.assert_array_equal(np.ldexp(b, e), level["bel"][node], err_msg="node %d vs per-level launches" % node)
        np.testing.assert_array_equal(np.ldexp(b, e), flow["bel"][node], err_msg="node %d vs dataflow launches" % node)
    for c, m in enumerate(scaled["marg"]):
        np.testing.assert_array_equal(np.ldexp(m, scaled["e"][c]), level["marg"][c], err_msg="marginal of clique %d" % c)
    sign, log_z = scaled["log_z"]
    assert sign == 1 and scaled["z"] == level["z"] and log_close(log_z, math.log(level["z"]), 1e-11)
    assert level["log_z"][0] == 1 and log_close(level["log_z"][1], math.log(level["z"]), 1e-11)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_out_of_range_inputs_keep_the_normalised_tables_and_shift_log_z(dtype):
    """Every clique table of the 31-clique tree x 2^+40 (x 2^-40): Z moves by 2^+-1240, out of float64's range."""
    k, opts = 40, dict(block_log2=11)
    case = spec_case(synthetic.wide_binary_tree(n_cliques=31, width=15, sep=7), seed=2)
    tree, pots, node_vars, sizes, n = case
    np_t = np.float32 if dtype == "f32" else np.float64
    held = [np.asarray(p, dtype=np_t).astype(np.float64) for p in pots]        # the values the device holds
    want, z = oracle.beliefs_exact(tree, held, node_vars, return_z=True)
    base = run(case, dtype, scaled=True, **opts)
    assert log_close(base["log_z"][1], math.log(z), RTOL[dtype])
    for shift in (k, -k):
        moved = [np.ldexp(np.asarray(p, dtype=np_t), shift) if c < n else p for c, p in enumerate(pots)]
        for c in range(n):       # still normal numbers of the storage type, and exactly the base values x 2^shift
            assert moved[c].dtype == np_t and np.all(np.abs(moved[c]) >= np.finfo(np_t).tiny) and np.all(np.isfinite(moved[c]))
            np.testing.assert_array_equal(np.ldexp(moved[c].astype(np.float64), -shift), held[c])
        got = run(case, dtype, pots=moved, scaled=True, **opts)
        for node, b in enumerate(got["bel"]):
            assert np.all(np.isfinite(b)) and b.sum() > 0
            np.testing.assert_array_equal(b / b.sum(), base["bel"][node] / base["bel"][node].sum(), err_msg="node %d" % node)
            close(b / b.sum(), want[node] / want[node].sum(), RTOL[dtype], "node %d vs the oracle" % node)
        for c, m in enumerate(got["marg"]):
            np.testing.assert_array_equal(m / m.sum(), base["marg"][c] / base["marg"][c].sum(), err_msg="marginal of clique %d" % c)
        sign, log_z = got["log_z"]
        assert sign == 1 and log_close(log_z, base["log_z"][1] + n * shift * LN2, 1e-11)
        assert got["z"] in (0.0, float("inf"))                                   # jtp_get_z: ldexp of the scaled sum
        for c in range(n):
            assert log_close(math.log(got["bel"][c].sum()) + got["e"][c] * LN2, log_z, RTOL[dtype]), c
        unscaled = run(case, dtype, pots=moved, level_launches=True, **opts)
        assert not (np.isfinite(unscaled["z"]) and unscaled["z"] > 0)           # what the plan without the flag makes of it


SPRINKLER = ([["cloudy"], ["cloudy", "sprinkler"], ["cloudy", "rain"], ["rain", "sprinkler", "wet_grass"]],
             {"cloudy": 2, "sprinkler": 2, "rain": 2, "wet_grass": 2},
             [np.array([0.5, 0.5]), np.array([[0.5, 0.5], [0.9, 0.1]]), np.array([[0.8, 0.2], [0.2, 0.8]]),
              np.array([[[1, 0], [0.1, 0.9]], [[0.1, 0.9], [0.01, 0.99]]])])


def oracle_propagate(tree, factors, sizes, values):
    ct = tree.clique_tree
    return oracle.propagate(tree.tree, tree.separators, ct.maxcliques, ct.factor_to_maxclique, factors, sizes,
                            [np.asarray(v, dtype=np.float64) for v in values])


def test_normalize_on_the_readme_network():
    factors, sizes, values = SPRINKLER
    tree = jt.create_junction_tree(factors, sizes)
    plain = tree.propagate(values)
    got = tree.propagate(values, normalize=True)
    for f, (g, p) in enumerate(zip(got, plain)):
        np.testing.assert_array_equal(g, p / p.sum(), err_msg="factor %d" % f)
    assert tree.z_sign == 1 and log_close(tree.log_z, math.log(plain[0].sum()), 1e-11)
    assert tree.plan("f64", scaled=True).scaled and not tree.plan("f64").scaled


@pytest.mark.parametrize("sweep", [False, True])
def test_normalize_on_a_lattice_with_unit_cliques_lean_tasks_and_folded_marginals(sweep, monkeypatch):
    # (a lattice this small plans as a chain of latency-bound levels and folds nothing by itself: planned here as the large ones
    #  are, as tests/test_gpu_parity.py test_factor_marginals_folded_into_the_propagate does)
    monkeypatch.setenv("JTP_TINY_LEVEL_ELEMS", "0")
    monkeypatch.setenv("JTP_FOLD", "1")
    h, w, card = 3, 6, 8
    factors, sizes, values = synthetic.lattice_mrf(h, w, card, dtype=np.float64)
    tree = jt.create_junction_tree(factors, sizes, order=synthetic.lattice_column_order(h, w) if sweep else None)
    plain = tree.propagate(values)
    got = tree.propagate(values, normalize=True)
    d = tree.plan("f64", scaled=True).describe()
    assert d["scaled"] == 1 and any(p["unit"] and p["real"] >= 0 for p in d["pnodes"])
    assert any(t["lean_off"] > 0 for t in d["tasks"]) and any(t["fold"] for t in d["tasks"])
    want = oracle_propagate(tree, factors, sizes, values)
    for f, (g, p) in enumerate(zip(got, plain)):
        np.testing.assert_array_equal(g, p / p.sum(), err_msg="factor %d" % f)
        close(g, want[f] / want[f].sum(), 1e-11, "factor %d vs the oracle" % f)
    log_z = tree.log_z
    assert tree.z_sign == 1 and log_close(log_z, math.log(want[0].sum()), 1e-11)
    # every factor x 2^30: the marginals stay, log Z moves by n_factors * 30 * ln 2
    moved = tree.propagate([np.ldexp(v, 30) for v in values], normalize=True)
    for f, (g, m) in enumerate(zip(got, moved)):
        np.testing.assert_array_equal(m, g, err_msg="factor %d x 2^30" % f)
    assert tree.z_sign == 1 and log_close(tree.log_z, log_z + len(factors) * 30 * LN2, 1e-11)


def test_a_normalised_call_leaves_the_plain_plans_staged_tables_alone():
    factors, sizes, values = synthetic.lattice_mrf(3, 6, 4, dtype=np.float64)
    tree = jt.create_junction_tree(factors, sizes)
    first = [m.copy() for m in tree.propagate(values)]
    other = list(values)
    other[5] = values[5] * 3.0
    got = tree.propagate(other, changed=[5], normalize=True)          # (the scaled plan has seen nothing yet: it stages every table)
    want = oracle_propagate(tree, factors, sizes, other)
    for f, (g, w_) in enumerate(zip(got, want)):
        close(g, w_ / w_.sum(), 1e-11, "factor %d" % f)
    again = tree.propagate(values, changed=[])                        # the plain plan still holds `values`
    for f, (a, b) in enumerate(zip(again, first)):
        np.testing.assert_array_equal(a, b, err_msg="factor %d" % f)
    got = tree.propagate(values, changed=[5], normalize=True)         # ... and the scaled plan `other`: factor 5 is named
    for f, (g, b) in enumerate(zip(got, first)):
        np.testing.assert_array_equal(g, b / b.sum(), err_msg="factor %d, second scaled call" % f)


@pytest.mark.parametrize("shift", [90, -90])
def test_evidence_sets_normalised_with_factors_far_out_of_range(shift):
    """A chain of 12 cliques of 16^3 entries, every factor x 2^+-90 (Z moves by 2^+-1080): normalised marginals per evidence set
    and log P(evidence) as a difference of log Z against the oracle on the base values with the contradicting entries removed."""
    n, card = 12, 16
    factors = [[i, i + 1, i + 2] for i in range(n)]
    sizes = {v: card for v in range(n + 2)}
    rng = np.random.default_rng(7)
    base = [rng.uniform(0.5, 1.5, (card,) * 3) / card for _ in factors]
    tree = jt.create_junction_tree(factors, sizes)
    v, w = 3, 9
    sets = [{}, {v: 1}, {v: 0, w: 3}]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = tree.propagate_evidence_sets([np.ldexp(b, shift) for b in base], sets, normalize=True)
    assert "one pass per evidence set" in tree._memo["evidence_plan"].evidence_mode and tree._memo["evidence_plan"].scaled
    zs = []
    for e, observed in enumerate(sets):
        sliced = []
        for fvars, b in zip(factors, base):
            b = b.copy()
            for var, state in observed.items():
                if var in fvars:
                    keep = np.zeros(card)
                    keep[state] = 1.0
                    b *= keep.reshape([card if x == var else 1 for x in fvars])
            sliced.append(b)
        want = oracle_propagate(tree, factors, sizes, sliced)
        zs.append(want[0].sum())
        for f, (g, w_) in enumerate(zip(got[e], want)):
            close(g, w_ / w_.sum(), 1e-11, "set %d factor %d" % (e, f))
    log_z = tree.log_z_sets
    assert log_z.shape == (3,) and log_close(log_z[0], math.log(zs[0]) + n * shift * LN2, 1e-11)
    for e in (1, 2):
        assert log_close(log_z[e] - log_z[0], math.log(zs[e] / zs[0]), 1e-11), e


def test_evidence_set_then_cleared_on_a_single_set_scaled_plan():
    case = spec_case(synthetic.wide_binary_tree(n_cliques=7, width=12, sep=6), seed=3)
    tree, pots, node_vars, sizes, n = case
    plan = engine.Plan(tree, node_vars, sizes, dtype="f64", scaled=True)
    for c in range(n):
        plan.set_potential(c, pots[c])
    plan.propagate()
    free = (plan.log_z(), [plan.belief(c) for c in range(n)], [plan.log2_scale(c) for c in range(n)])
    var = node_vars[3][0]
    plan.set_evidence({var: 1})
    plan.propagate()
    held = list(pots)
    for c in range(n):
        if var in node_vars[c]:
            keep = np.zeros(sizes[var])
            keep[1] = 1.0
            held[c] = pots[c] * keep.reshape([sizes[var] if x == var else 1 for x in node_vars[c]])
    want, z = oracle.beliefs_exact(tree, held, node_vars, return_z=True)
    sign, log_z = plan.log_z()
    assert sign == 1 and log_close(log_z, math.log(z), 1e-11) and log_z < free[0][1]
    for c in range(n):
        close(np.ldexp(plan.belief(c), plan.log2_scale(c)), want[c], 1e-11, "clique %d under evidence" % c)
    plan.set_evidence({})
    plan.propagate()
    assert plan.log_z() == free[0] and [plan.log2_scale(c) for c in range(n)] == free[2]
    for c in range(n):
        np.testing.assert_array_equal(plan.belief(c), free[1][c])
    plan.close()


def test_a_message_of_zeros_and_a_nan_potential():
    # b is 0 wherever a deterministic table (clique 0, the root) allows it, and it is observed as 1: the downward message of clique 0
    # is all zero - e = 0, zeros out - while the upward message of clique 1 (15 at b = 1) is scaled as any other
    tree, node_vars, sizes = [0, (2, [1])], [["a", "b"], ["b", "c"], ["b"]], {"a": 2, "b": 2, "c": 3}
    table = np.array([[1.0, 0.0], [2.0, 0.0]])
    other = np.arange(1.0, 7.0).reshape(2, 3)
    plan = engine.Plan(tree, node_vars, sizes, dtype="f64", scaled=True)
    plan.set_potential(0, table)
    plan.set_potential(1, other)
    plan.propagate()
    sign, log_z = plan.log_z()
    assert sign == 1 and log_close(log_z, math.log((table.sum(axis=0) * other.sum(axis=1)).sum()), 1e-11)
    plan.set_evidence({"b": 1})
    plan.propagate()
    assert plan.log_z() == (0, -math.inf) and plan.z() == 0.0
    assert plan.describe()["root"] == 0
    e_root, e_child, e_sep = (plan.log2_scale(node) for node in range(3))
    assert e_sep - e_root == 0                     # e_dn of the all-zero message (a separator: E_parent + e_dn)
    assert e_sep - e_child == e_root == 3          # e_up: the largest entry 15 = 1.875 x 2^3, and E_root = the sum of every e_up
    for node in range(3):
        assert not np.any(plan.belief(node))
    plan.close()
    # the same through the public API: contradictory factors
    ftree = jt.create_junction_tree([["b"], ["a", "b"]], {"a": 2, "b": 2})
    out = ftree.propagate([np.array([0.0, 1.0]), table], normalize=True)
    assert ftree.z_sign == 0 and ftree.log_z == -math.inf and all(not np.any(o) for o in out)
    # a NaN in a potential comes out as NaN (the message that carries it is left unscaled), and nothing hangs
    plan = engine.Plan(tree, node_vars, sizes, dtype="f64", scaled=True)
    bad = other.copy()
    bad[1, 2] = np.nan
    plan.set_potential(0, np.array([[1.0, 3.0], [2.0, 4.0]]))
    plan.set_potential(1, bad)
    plan.propagate()
    sign, log_z = plan.log_z()
    assert sign == 0 and math.isnan(log_z) and np.isnan(plan.belief(1)[1, 2]) and np.any(np.isnan(plan.belief(0)))
    plan.close()
