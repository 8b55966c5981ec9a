"""Tables with negative entries through every kernel family on a real MI355X, against the oracle under the cancellation bound of
tests/signed_reference.py: |got - want| <= rtol * B_abs + 1e-300 on EVERY entry, B_abs the oracle on the absolute tables, rtol the
project's constants (1e-11 float64 storage, 1e-6 float32 storage, `want` and `B_abs` from the float32-cast tables).  On non-negative
tables that is the elementwise tolerance of tests/test_gpu_parity.py.

Every case first asserts on the oracle alone that the bound is sharp (kappa = B_abs / |want|: median <= 100, max <= 1e4) and that at
least 5 % of the belief entries are negative; the numbers are printed (`pytest -s`).  Every family runs three inputs: the generated
tables (signs flipped at rate 1/8), the same with one leaf clique negated (Z < 0, the message above the leaf negative) and with an
inner clique negated as well (Z > 0 again).  Every case asserts from `describe()` / `stats()` that the family it is named for ran.
tests/test_signed_emulated.py runs the same inputs through the planner's task tables on the CPU."""
import functools
import math
import re

import numpy as np
import pytest

import jt_oracle as oracle
import junctiontree_amd as jt
import signed_reference as sr
from counts_reference import indicator_potentials
from joint_reference import joint_reference, parity_bound
from junctiontree_amd import _capi, engine, synthetic
from sample_reference import schedule
from test_gpu_parity import expected_mode

pytestmark = pytest.mark.gpu

RTOL = sr.RTOL
NP = {"f64": np.float64, "f32": np.float32}
LN2 = math.log(2.0)

SPECS = {
    "wide15": lambda: synthetic.wide_binary_tree(n_cliques=15, width=14, sep=7, card=2, seed=2),
    "random9": lambda: synthetic.random_tree(n_cliques=9, width=13, sep=5, card=2, seed=3),
    "chain6": lambda: synthetic.chain_tree(n_cliques=6, card=16, width=3),
    "card3": lambda: synthetic.wide_binary_tree(n_cliques=7, width=8, sep=4, card=3, seed=3),
    "card5": lambda: synthetic.wide_binary_tree(n_cliques=7, width=6, sep=3, card=5, seed=5),
    "card6": lambda: synthetic.wide_binary_tree(n_cliques=7, width=5, sep=2, card=6, seed=6),
}


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """(spec, {"plain" | "leaf" | "leaf+inner": (tables in the storage type, Bound)}, leaf, inner): made once per spec and storage type;
    the conditions on the oracle and the facts about the negations are asserted here, before any device result is looked at"""
    spec = SPECS[name]()
    runs, leaf, inner = sr.negation_facts(spec, sr.signed_potentials(spec, seed=21, dtype=NP[dtype]), "%s %s" % (name, dtype))
    return spec, runs, leaf, inner


def make_plan(spec, pots, dtype, propagates=1, **opts):
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, **opts)
    load(plan, spec, pots, propagates)
    return plan


def load(plan, spec, pots, propagates=1):
    for c in range(spec["n_cliques"]):
        plan.set_potential(c, pots[c])
    for _ in range(propagates):
        plan.propagate()


def check_plan(plan, spec, bound, dtype, what, batch=0):
    """every clique belief, every separator belief and z of the plan under the bound; returns the tables"""
    out = [plan.belief(node, batch=batch) for node in range(len(spec["node_vars"]))]
    for node, b in enumerate(out):
        bound.check(node, b, RTOL[dtype], what)
    z = plan.z(batch=batch)
    bound.check_z(z, RTOL[dtype], what)
    assert (z < 0) == (bound.z < 0), (what, z, bound.z)
    assert plan.stats()["flow_fallbacks"] == 0
    print("%s %s %s: worst |got - want| / (rtol * B_abs) so far %.3g" % (bound.what, dtype, what, bound.worst))
    return out


def rows_per_clique(d):
    return max(p["phys_elems"] // p["trow"] for p in d["pnodes"] if not p.get("unit"))


# ---------------------------------------------------------------------------------------------- 1. power-of-two tables

POW2_OPTS = [{}, {"level_launches": True}, {"flow_tickets": True}, {"block_log2": 10}, {"split_variants": True}]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["wide15", "random9"])
def test_power_of_two_tables_in_every_launch_mode(name, dtype):
    """multi-row bit-field tables through `jt_collect_flow` / `jt_distribute_flow` / `jt_propagate_flow` and the per-level kernels; the
    three launch modes run the same workgroups on the same tables: bit-identical beliefs"""
    spec, runs, _, _ = inputs(name, dtype)
    for key, (pots, bound) in runs.items():
        modes = []
        for opts in POW2_OPTS if key != "leaf+inner" else POW2_OPTS[:1]:
            plan = make_plan(spec, pots, dtype, **opts)
            d, st = plan.describe(), plan.stats()
            assert d["tmix"] == 0 and rows_per_clique(d) > 1 and not d.get("multiset")
            assert st["launch_mode"] == expected_mode(opts), (st["launch_mode"], opts)
            assert st["tickets_used"] == (1 if expected_mode(opts) == "flow_tickets" else 0)
            out = check_plan(plan, spec, bound, dtype, "%s %r" % (key, opts))
            if opts in POW2_OPTS[:3]:
                modes.append((st["launch_mode"], out))
            plan.close()
        if key != "leaf+inner":
            assert [m for m, _ in modes] == ["flow", "level", "flow_tickets"]
            for _, other in modes[1:]:
                for a, b in zip(modes[0][1], other):
                    np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 2. reduce tasks

@pytest.mark.parametrize("level_launches", [False, True])
@pytest.mark.parametrize("name", ["wide15", "random9", "chain6"])
def test_reduce_tasks_sum_signed_partial_copies(monkeypatch, name, level_launches):
    """the specs and options of `test_reduce_tasks_on_device`: partial copies of either sign summed by reduce tasks, three propagates on
    one plan (both arena halves), then the negated inputs on the same plan"""
    monkeypatch.setenv("JTP_REDUCE_MIN", "2")
    for dtype in ("f64", "f32"):
        spec, runs, _, _ = inputs(name, dtype)
        plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, block_log2=10, level_launches=level_launches, layout_policy=3)
        d = plan.describe()
        if (name, dtype) != ("chain6", "f32"):          # (the chain's float32 rows are wide enough for one copy per message)
            assert sum(t["kind"] for t in d["tasks"]) > 0 and any(s["up_npart"] > 1 or s["dn_npart"] > 1 for s in d["pseps"])
        for key, (pots, bound) in runs.items():
            load(plan, spec, pots, propagates=3 if key == "plain" else 1)
            assert plan.stats()["launch_mode"] == ("level" if level_launches else "flow")
            check_plan(plan, spec, bound, dtype, "%s %s" % (key, "levels" if level_launches else "flow"))
        plan.close()


# ---------------------------------------------------------------------------------------------- 3. mixed-radix rows

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["card3", "card5", "card6"])
def test_mixed_radix_rows_and_their_marginals(name, dtype):
    """cardinalities 3, 5 and 6 of `test_wide_cliques_of_odd_cardinalities`: rows at true cardinalities reached through the thread map
    (`tmix`) and the padded layout (`no_compact`); a two-variable marginal and a request list with permuted axes (`jt_marginals`)"""
    spec, runs, _, _ = inputs(name, dtype)
    rng = np.random.default_rng(0)
    requests = []
    for c in range(spec["n_cliques"]):
        labels = list(spec["node_vars"][c])
        for k in (0, 1, 2, 3, len(labels)):
            requests.append((c, [labels[i] for i in rng.permutation(len(labels))[:k]]))
    for no_compact in (False, True):
        for key, (pots, bound) in runs.items():
            if key == "leaf+inner" and no_compact:
                continue
            plan = make_plan(spec, pots, dtype, no_compact=no_compact)
            d = plan.describe()
            assert d["tmix"] == (0 if no_compact else 1) and d["compact"] == (0 if no_compact else 1) and rows_per_clique(d) > 1
            assert plan.stats()["launch_mode"] == "flow"
            what = "%s%s" % (key, " no_compact" if no_compact else "")
            check_plan(plan, spec, bound, dtype, what)
            pair = list(spec["node_vars"][3])[1:3]
            bound.check_marginal(3, pair, plan.marginal(3, pair), RTOL[dtype], what)
            got = plan.marginals(requests)
            assert len(got) == len(requests)
            for (c, labels), g in zip(requests, got):
                assert g.shape == tuple(spec["sizes"][v] for v in labels)
                bound.check_marginal(c, labels, g, RTOL[dtype], what)
            plan.close()


# ---------------------------------------------------------------------------------------------- 4. the public API with unit cliques

def _clique_bound(tree, factors, sizes, values, what):
    """`Bound` over the cliques and separators of a JunctionTree, from the oracle's `evaluate`"""
    ct = tree.clique_tree
    psi = oracle.evaluate(factors, ct.factor_to_maxclique, ct.maxcliques, [np.asarray(v, dtype=np.float64) for v in values])
    psi = [np.broadcast_to(p, tuple(sizes[v] for v in clique)).copy() for p, clique in zip(psi, ct.maxcliques)]
    seps = [np.ones(tuple(sizes[v] for v in sep)) for sep in tree.separators]
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]
    return sr.Bound(tree.tree, psi + seps, node_vars, what)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("sweep", [False, True])
def test_signed_factors_through_unit_cliques_the_lean_pass_and_folded_marginals(sweep, dtype, monkeypatch):
    """`tree.propagate` on the 3 x 6 lattice of cardinality 8, planned as the large ones are (tests/test_gpu_scaled.py): cliques that
    keep no table, the lean unit pass, factor marginals folded into the propagate; beliefs of unit cliques formed on demand
    (`jt_lean_single`); one factor negated whole: Z < 0, and `normalize=True` reports `z_sign == -1`"""
    monkeypatch.setenv("JTP_TINY_LEVEL_ELEMS", "0")
    monkeypatch.setenv("JTP_FOLD", "1")
    h, w, card = 3, 6, 8
    factors, sizes, values = synthetic.lattice_mrf(h, w, card, dtype=NP[dtype])
    tree = jt.create_junction_tree(factors, sizes, order=synthetic.lattice_column_order(h, w) if sweep else None)
    signed = sr.signed_factors(values)
    flipped = list(signed)
    flipped[-1] = -signed[-1]
    bounds = {}
    for key, vals in (("plain", signed), ("negated", flipped)):
        bounds[key] = sr.FactorBound(tree, factors, sizes, vals, "lattice %s %s%s" % (dtype, key, " sweep" if sweep else ""))
        bounds[key].conditions()
    assert bounds["plain"].z > 0 > bounds["negated"].z
    plain = {}
    for key, vals in (("plain", signed), ("negated", flipped)):
        got = tree.propagate(vals)
        assert all(g.shape == np.shape(v) and g.dtype == np.float64 for g, v in zip(got, vals))
        bounds[key].check(got, RTOL[dtype], "propagate")
        plain[key] = [g.copy() for g in got]
        plan = tree.plan(dtype)
        d, st = plan.describe(), plan.stats()
        assert any(p["unit"] and p["real"] >= 0 for p in d["pnodes"]) and st["n_unit_cliques"] > 0
        assert any(t["lean_off"] > 0 for t in d["tasks"]) and any(t["fold"] for t in d["tasks"])
        assert st["launch_mode"] == "flow" and st["flow_fallbacks"] == 0
        z = plan.z()
        assert abs(z - bounds[key].z) <= RTOL[dtype] * bounds[key].z_abs and (z < 0) == (key == "negated")
        cb = _clique_bound(tree, factors, sizes, vals, "lattice cliques " + key)
        unit = [p["real"] for p in d["pnodes"] if p["unit"] and p["real"] >= 0 and p["stat"] >= 0][:3]
        assert unit
        for c in unit:                                       # formed on demand from the static table and the final messages
            cb.check(c, plan.belief(c), RTOL[dtype], "unit clique on demand")
    got = tree.propagate(flipped, normalize=True)
    d = tree.plan(dtype, scaled=True).describe()
    assert d["scaled"] == 1 and any(t["lean_off"] > 0 for t in d["tasks"]) and any(t["fold"] for t in d["tasks"])
    for f, (g, p) in enumerate(zip(got, plain["negated"])):
        np.testing.assert_array_equal(g, p / p.sum(), err_msg="factor %d" % f)
    assert tree.z_sign == -1 and abs(tree.log_z - math.log(-bounds["negated"].z)) <= 1e-11 * max(1.0, abs(tree.log_z)) + RTOL[dtype] * bounds["negated"].z_abs / -bounds["negated"].z


@pytest.mark.parametrize("nv,card,dt", [(7, 3, np.float64), (6, 5, np.float32), (6, 6, np.float32), (5, 5, np.float64)])
def test_factor_products_with_negative_entries_in_mixed_radix_tables(nv, card, dt):
    """`jtp_set_potential_product` (through `tree.propagate`) with factors of either sign, in one mixed-radix clique of several rows
    (the shapes of `test_factor_products_formed_on_the_device_in_mixed_radix_tables`), against the brute-force joint"""
    rng = np.random.default_rng(0)
    names = list("abcdefghi")[:nv]
    sizes = {v: card for v in names}
    factors = [names, names[:2], names[-3:]]
    values = sr.flip_signs([rng.uniform(0.2, 1.0, [sizes[v] for v in f]).astype(dt) for f in factors], 21)
    values[1] = -np.abs(values[1])                           # one factor negative throughout
    ax = {v: i for i, v in enumerate(names)}

    def marginals(vals):
        ops = []
        for f, val in zip(factors, vals):
            ops += [np.asarray(val, dtype=np.float64), [ax[v] for v in f]]
        joint = np.einsum(*ops, list(range(nv)))
        return [np.einsum(joint, list(range(nv)), [ax[v] for v in f]) for f in factors]

    want, b_abs = marginals(values), marginals([np.abs(v) for v in values])
    kappa = np.concatenate([np.ravel(b / np.abs(w)) for w, b in zip(want, b_abs)])
    neg = np.mean(np.concatenate([np.ravel(w) for w in want]) < 0)
    print("card %d nv %d: kappa median %.3g max %.3g, negative share %.3f" % (card, nv, np.median(kappa), kappa.max(), neg))
    assert np.median(kappa) <= sr.KAPPA_MEDIAN and kappa.max() <= sr.KAPPA_MAX and neg >= sr.NEGATIVE_SHARE
    tree = jt.create_junction_tree(factors, sizes)
    got = tree.propagate(values)
    dtype = "f32" if dt == np.float32 else "f64"
    d = tree.plan(dtype).describe()
    assert rows_per_clique(d) > 1 and d["tmix"] == 1
    for f, (g, w, b) in enumerate(zip(got, want, b_abs)):
        sr.check(g, w, b, RTOL[dtype], "factor %d" % f)


# ---------------------------------------------------------------------------------------------- 5. evidence sets

def evidence_sets(spec, nb=6):
    """set 0 observes nothing, the others one to four variables"""
    labels = sorted(spec["sizes"])
    out = [{}]
    for b in range(1, nb):
        rng = np.random.default_rng(700 + b)
        out.append({labels[i]: int(rng.integers(0, spec["sizes"][labels[i]])) for i in rng.choice(len(labels), size=1 + b % 4, replace=False)})
    return out


@functools.lru_cache(maxsize=None)
def evidence_bounds(name, dtype, key):
    """per evidence set the oracle on the indicator-multiplied tables (signed, and absolute for the bound), conditions asserted"""
    spec, runs, _, _ = inputs(name, dtype)
    out = []
    for b, obs in enumerate(evidence_sets(spec)):
        bound = sr.Bound(spec["tree"], indicator_potentials(spec, runs[key][0], obs), spec["node_vars"], "%s %s %s set %d" % (name, dtype, key, b))
        bound.conditions()
        out.append(bound)
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("multiset", [False, True], ids=["share_potentials", "multiset"])
@pytest.mark.parametrize("name", ["wide15", "card3"])
def test_evidence_sets_over_signed_shared_tables(name, multiset, dtype):
    """six evidence sets over one copy of signed tables: one pass per set (`share_potentials`) and eight sets per pass
    (`jt_multi_flow`); with the leaf negated every set's z is negative"""
    spec, runs, _, _ = inputs(name, dtype)
    sets = evidence_sets(spec)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, n_batch=len(sets), share_potentials=True, multiset=multiset)
    d = plan.describe()
    assert bool(d.get("multiset")) == multiset and rows_per_clique(d) > 1
    if name == "card3":      # rows at true cardinalities; through the thread map where every set has its own pass (multi-set passes keep bit-field rows)
        assert any(p["group_mask"] for p in d["pnodes"]) and d["tmix"] == (0 if multiset else 1)
    else:
        assert d["tmix"] == 0
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    for key in ("plain", "leaf"):
        bounds = evidence_bounds(name, dtype, key)
        assert all((bd.z < 0) == (key == "leaf") for bd in bounds)
        for c in range(spec["n_cliques"]):
            plan.set_potential(c, runs[key][0][c])
        plan.propagate(0, len(sets))
        assert plan.stats()["launch_mode"] == ("flow" if multiset else "flow_tickets")      # (a pass per set: the sets' streams run side by side)
        for b, bound in enumerate(bounds):
            check_plan(plan, spec, bound, dtype, "%s set %d" % (key, b), batch=b)
            pair = list(spec["node_vars"][2])[:2]
            bound.check_marginal(2, pair, plan.marginal(2, pair, batch=b), RTOL[dtype], "%s set %d" % (key, b))
    plan.close()


def test_evidence_sets_through_the_public_api_say_how_they_ran():
    """`tree.propagate_evidence_sets` with signed factors, one of them negative throughout: a multi-set plan (`evidence_mode`), every
    set against the oracle's `propagate` on indicator-multiplied factors"""
    names = list("abcdefg")
    sizes = {v: 3 for v in names}
    factors = [names[:5], names[3:], names[:2], names[-2:]]
    rng = np.random.default_rng(4)
    values = sr.flip_signs([rng.uniform(0.2, 1.0, [3] * len(f)) for f in factors], 21)
    values[2] = -np.abs(values[2])
    tree = jt.create_junction_tree(factors, sizes)
    sets = [{}, {"a": 1}, {"g": 2, "c": 0}, {"d": 1, "b": 2, "f": 0}]
    got = tree.propagate_evidence_sets(values, sets)
    assert tree._memo["evidence_plan"].evidence_mode.startswith("multiset")
    signs = []
    for e, (obs, out) in enumerate(zip(sets, got)):
        vals = [v.copy() for v in values]
        for var, state in obs.items():
            f = next(i for i, fv in enumerate(factors) if var in fv)
            ind = np.zeros(3)
            ind[state] = 1.0
            vals[f] = vals[f] * ind.reshape([3 if lab == var else 1 for lab in factors[f]])
        fb = sr.FactorBound(tree, factors, sizes, vals, "public API set %d" % e)
        live = np.concatenate([np.ravel(b) for b in fb.b_abs]) > 0
        w = np.concatenate([np.ravel(a) for a in fb.want])[live]
        k = np.concatenate([np.ravel(b) for b in fb.b_abs])[live] / np.abs(w)
        print("set %d: kappa median %.3g max %.3g, negative share %.3f" % (e, np.median(k), k.max(), np.mean(w < 0)))
        assert np.median(k) <= sr.KAPPA_MEDIAN and k.max() <= sr.KAPPA_MAX and np.mean(w < 0) >= sr.NEGATIVE_SHARE
        signs.append(fb.z < 0)
        fb.check(out, 1e-11, "evidence set %d" % e)
        assert all(abs(o.sum() - fb.z) <= 1e-11 * fb.z_abs for o in out)
    assert any(signs) and not all(signs)                     # (sets of either sign of Z)


# ---------------------------------------------------------------------------------------------- 6. scaled plans

def log_close(got, want, rtol):
    return abs(got - want) <= rtol * max(1.0, abs(want))


def run_scaled(spec, pots, dtype, **opts):
    plan = make_plan(spec, pots, dtype, **opts)
    nodes = range(len(spec["node_vars"]))
    out = {"bel": [plan.belief(node) for node in nodes], "e": [plan.log2_scale(node) for node in nodes], "log_z": plan.log_z(),
           "desc": plan.describe(), "stats": plan.stats()}
    with np.errstate(over="ignore"):
        out["z"] = plan.z()
    plan.close()
    return out


SCALED = {"wide15": ({}, None), "card3": ({}, None), "random9": (dict(block_log2=10, layout_policy=3), "2")}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCALED))
def test_scaled_plans_take_their_exponents_from_signed_entries_and_report_the_sign(name, dtype, monkeypatch):
    """`jt_rescale_level` on messages of either sign: in range, ldexp(belief, e) is the unscaled per-level and dataflow table bit for
    bit; one clique negated: `jtp_get_log_z` gives sign -1 and log|Z| = log(-z); every table x 2^+-40: the normalised tables stay
    bit-equal and the sign stays -1"""
    opts, reduce_min = SCALED[name]
    if reduce_min:
        monkeypatch.setenv("JTP_REDUCE_MIN", reduce_min)
    spec, runs, _, _ = inputs(name, dtype)
    n = spec["n_cliques"]
    for key in ("plain", "leaf"):
        pots, bound = runs[key]
        scaled = run_scaled(spec, pots, dtype, scaled=True, **opts)
        level = run_scaled(spec, pots, dtype, level_launches=True, **opts)
        flow = run_scaled(spec, pots, dtype, **opts)
        d = scaled["desc"]
        assert d["scaled"] == 1 and scaled["stats"]["launch_mode"] == "level" and flow["stats"]["launch_mode"] == "flow"
        assert sum(1 for kind, _, _ in d["steps"] if kind == 2) > 0
        if reduce_min:
            assert any(t["kind"] == 1 for t in d["tasks"])
        assert any(scaled["e"]) and not any(level["e"]) and not any(flow["e"])
        for node, (b, e) in enumerate(zip(scaled["bel"], scaled["e"])):
            np.testing.assert_array_equal(np.ldexp(b, e), level["bel"][node], err_msg="%s node %d vs per-level launches" % (key, node))
            np.testing.assert_array_equal(np.ldexp(b, e), flow["bel"][node], err_msg="%s node %d vs dataflow launches" % (key, node))
            bound.check(node, level["bel"][node], RTOL[dtype], key)
        want_sign = -1 if key == "leaf" else 1
        sign, log_z = scaled["log_z"]
        assert sign == want_sign == level["log_z"][0] and scaled["z"] == level["z"] and (level["z"] < 0) == (key == "leaf")
        bound.check_z(level["z"], RTOL[dtype], key)
        assert log_close(log_z, math.log(abs(level["z"])), 1e-11) and log_close(level["log_z"][1], math.log(abs(level["z"])), 1e-11)
        if key != "leaf":
            continue
        for shift in (40, -40):
            moved = [np.ldexp(p, shift) if c < n else p for c, p in enumerate(pots)]
            for c in range(n):       # still normal numbers of the storage type, and exactly the base values x 2^shift
                assert moved[c].dtype == NP[dtype] and np.all(np.abs(moved[c]) >= np.finfo(NP[dtype]).tiny) and np.all(np.isfinite(moved[c]))
            got = run_scaled(spec, moved, dtype, scaled=True, **opts)
            for node, b in enumerate(got["bel"]):
                assert np.all(np.isfinite(b)) and b.sum() < 0
                np.testing.assert_array_equal(b / b.sum(), scaled["bel"][node] / scaled["bel"][node].sum(), err_msg="node %d x 2^%d" % (node, shift))
            assert got["log_z"][0] == -1 and log_close(got["log_z"][1], log_z + n * shift * LN2, 1e-11)


# ---------------------------------------------------------------------------------------------- 7. expected counts

def counts_case(name, dtype):
    """Signed shared tables whose Z changes sign with the evidence: the slice of the last leaf where its first private variable v is in
    state 1 is negated, so a set that observes v = 1 has Z < 0, one that observes another state Z > 0 (on the binary tree every set
    observes v: unobserved, the two halves would cancel; with three states the unobserved sum keeps a third)."""
    spec = SPECS[name]()
    n = spec["n_cliques"]
    leaf = n - 1
    pots = sr.signed_potentials(spec, seed=21, dtype=NP[dtype])
    v = [x for x in spec["node_vars"][leaf] if x not in spec["node_vars"][n + leaf - 1]][0]
    table = pots[leaf].copy()
    table[tuple(1 if x == v else slice(None) for x in spec["node_vars"][leaf])] *= -1
    pots = pots[:leaf] + [table] + pots[leaf + 1:]
    others = [lab for lab in sorted(spec["sizes"]) if lab != v]
    card = spec["sizes"][v]
    sets = [{v: 0}, {v: 1}, {v: 1, others[3]: 0}, {v: 0, others[10]: 1, others[20]: 0}, {v: 1, others[15]: 1}, {v: card - 1, others[7]: 0}]
    if card > 2:
        sets += [{}, {others[5]: 2}]
    rng = np.random.default_rng(9)
    requests = []
    for c in range(n):
        labels = list(spec["node_vars"][c])
        requests.append((c, [labels[int(rng.integers(0, len(labels)))]]))
        requests.append((c, labels[1:3][::-1]))
    requests += [(0, []), (leaf, list(spec["node_vars"][leaf]))]
    weights = np.random.default_rng(3).uniform(0.5, 2.0, len(sets))
    weights[2] = 0.0                                         # (a set of weight 0 contributes nothing; its log Z and sign are still reported)
    bounds = []
    for b, obs in enumerate(sets):
        bound = sr.Bound(spec["tree"], indicator_potentials(spec, pots, obs), spec["node_vars"], "counts %s %s set %d" % (name, dtype, b))
        bound.conditions()
        bounds.append(bound)
    assert any(bd.z < 0 for bd in bounds) and any(bd.z > 0 for bd in bounds)
    want = [np.zeros([spec["sizes"][x] for x in labels]) for _, labels in requests]
    limit = [np.zeros_like(w) for w in want]
    for bd, wt in zip(bounds, weights):                      # (tests/counts_reference.py's sum, with the bound accumulated beside it)
        for i, (c, labels) in enumerate(requests):
            m, m_abs = bd.marginal(c, labels)
            want[i] = want[i] + wt * (m / m.sum())
            limit[i] = limit[i] + wt * (m_abs / abs(m.sum()))
    return spec, pots, sets, requests, weights, bounds, want, limit


@pytest.mark.parametrize("name,dtype,opts", [("card3", "f64", {"multiset": True}), ("wide15", "f32", {"share_potentials": True}),
                                             ("wide15", "f64", {"multiset": True, "level_launches": True}), ("card3", "f32", {"share_potentials": True})],
                         ids=["card3-multiset-f64", "wide15-share-f32", "wide15-multiset-levels-f64", "card3-share-f32"])
def test_expected_counts_over_sets_of_either_sign(name, dtype, opts):
    """`jtp_accumulate_marginals` (`jt_marg_sums`, `jt_marg_accumulate`) where S is negative for some sets: m / S is the same probability
    table whatever the sign; the bound is the accumulation of w * marginal(B_abs) / |S|; the per-set sign is that of the oracle's Z"""
    from counts_reference import expected_counts_reference
    spec, pots, sets, requests, weights, bounds, want, limit = counts_case(name, dtype)
    ref, ref_log_z = expected_counts_reference(spec, pots[:spec["n_cliques"]], requests, sets, weights)
    for w, r in zip(want, ref):
        np.testing.assert_allclose(w, r, rtol=1e-12, atol=1e-15)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, n_batch=len(sets), **opts)
    assert bool(plan.describe().get("multiset")) == bool(opts.get("multiset"))
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    load(plan, spec, pots, propagates=2)
    got, log_z, sign = plan.accumulate_marginals(requests, weights=weights)
    assert len(got) == len(requests) and plan.stats()["flow_fallbacks"] == 0
    for (c, labels), g, w, lim in zip(requests, got, ref, limit):
        assert g.shape == w.shape and g.dtype == np.float64
        sr.check(g, w, lim, RTOL[dtype], "clique %d labels %r" % (c, labels))
    for b, bd in enumerate(bounds):
        s, lz = plan.log_z(batch=b)
        assert sign[b] == s == (-1 if bd.z < 0 else 1), (b, sign[b], s, bd.z)
        tol = RTOL[dtype] * (bd.z_abs / abs(bd.z) + max(1.0, abs(ref_log_z[b])))       # (d log|Z| = dZ / |Z|, dZ <= rtol * Z_abs)
        assert abs(log_z[b] - ref_log_z[b]) <= tol and abs(lz - ref_log_z[b]) <= tol, (b, log_z[b], lz, ref_log_z[b])
    plan.close()


def test_expected_counts_through_the_public_api_with_a_negative_factor():
    names = ["v%d" % i for i in range(8)]
    factors = [[names[0]]] + [[names[i], names[i + 1]] for i in range(7)]
    sizes = {v: 3 for v in names}
    rng = np.random.default_rng(0)
    values = [rng.uniform(0.5, 1.5, [3] * len(f)) for f in factors]
    sets = [{}, {names[1]: 2}, {names[0]: 0, names[6]: 1}, {names[4]: 1}]
    weights = [1.0, 0.5, 2.0, 1.5]
    tree = jt.create_junction_tree(factors, sizes)
    want = tree.expected_counts(values, sets, weights=weights)
    log_z = np.array(tree.log_z_sets)
    flipped = list(values)
    flipped[3] = -values[3]                                  # the same distribution: every Z negated
    got = tree.expected_counts(flipped, sets, weights=weights)
    for f, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_allclose(g, w, rtol=1e-11, atol=0.0, err_msg="factor %d" % f)
    np.testing.assert_allclose(np.array(tree.log_z_sets), log_z, rtol=0.0, atol=1e-11)


# ---------------------------------------------------------------------------------------------- 8. sample and joint refuse a negative entry

def _refusal_plan(evidence=None):
    """the chain of four cliques of 3 x 3 x 3 entries (clique i holds variables i, i + 1, i + 2) with ONE entry of clique 2 negated:
    (x2, x3, x4) = (1, 0, 2)"""
    spec = synthetic.chain_tree(4, card=3, width=3)
    pots = [np.array(p) for p in synthetic.potentials_for(spec, seed=3)]
    pots[2][1, 0, 2] = -pots[2][1, 0, 2]
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f64")
    if evidence:
        plan.set_evidence(evidence)
    load(plan, spec, pots)
    return spec, pots, plan


def test_sample_reports_a_negative_entry_and_draws_where_none_is_read():
    spec, pots, plan = _refusal_plan()
    n, count = spec["n_cliques"], 61
    beliefs = [plan.belief(c) for c in range(n)]
    assert [int((b < 0).sum()) for b in beliefs] == [0, 0, 1, 0] and beliefs[2][1, 0, 2] < 0      # the entry is the only negative one anywhere
    with pytest.raises(_capi.JtpError, match="negative or NaN entry") as err:
        plan.sample(count, seed=1)
    states = err.value.states
    assert states.shape == (count, len(plan.var_labels)) and int(re.search(r"(\d+) \(clique, sample\) pairs", str(err.value)).group(1)) >= 1
    col = {lab: j for j, lab in enumerate(plan.var_labels)}
    sched = {s[0]: s for s in schedule(plan)}
    _, parent, _, K, F, _ = sched[2]
    # a sample fails at clique 2 exactly where its conditioning digits select the slice that holds the entry (or are themselves -1);
    # what clique 2 and the cliques below it would have drawn is then -1, nothing else is
    hit = np.ones(count, dtype=bool)
    for lab in K:
        hit &= (states[:, col[lab]] == {2: 1, 3: 0, 4: 2}[lab]) | (states[:, col[lab]] < 0)
    assert hit.any() and not hit.all()
    below = {2}
    for c in sorted(sched, key=lambda c: sched[c][2]):
        if sched[c][1] in below:
            below.add(c)
    failed_vars = {lab for c in below for lab in sched[c][4]}
    for lab, j in col.items():
        if lab in failed_vars:
            assert np.all((states[:, j] == -1) == hit), lab
        else:
            assert np.all(states[:, j] >= 0), lab
    # evidence that keeps the sweep off the entry (x3 = 1: the entry lies at x3 = 0 and is zero in the beliefs): every draw succeeds
    plan.set_evidence({3: 1})
    plan.propagate()
    good = plan.sample(count, seed=1)
    assert good.min() >= 0 and good.max() < 3 and np.all(good[:, col[3]] == 1)
    plan.close()
    # the public API: the same report, nothing returned silently
    factors = [list(vs) for vs in spec["node_vars"][:n]]
    tree = jt.create_junction_tree(factors, spec["sizes"])
    with pytest.raises(_capi.JtpError, match="negative or NaN entry") as err:
        tree.sample(pots[:n], count, seed=1)
    assert (err.value.states == -1).any()
    out = tree.sample(pots[:n], count, seed=1, evidence={3: 1})
    assert all(colv.min() >= 0 for colv in out.values()) and np.all(out[3] == 1)


def test_joint_reports_a_negative_entry_and_answers_where_none_is_read():
    spec, pots, plan = _refusal_plan()
    n = spec["n_cliques"]
    sched = schedule(plan)
    by = {s[0]: s for s in sched}
    beliefs = {c: plan.belief(c) for c in range(n)}

    def active(query):
        return {c for c, _, _, _ in joint_reference(beliefs, sched, query, spec["node_vars"])[1]}

    # a query whose sweep reads clique 2 fails and says why; the table comes back with the error
    reads = [q for q in ([5, 0], [4, 1], [5, 2]) if 2 in active(q)]
    assert reads
    for query in reads:
        with pytest.raises(_capi.JtpError, match="negative or NaN belief entry") as err:
            plan.joint(query)
        assert err.value.joint.shape == (3, 3) and re.search(r"\d+ \(clique, k\) pairs.*clique %d" % plan.abi_of[2], str(err.value))
    # a query whose active cliques leave clique 2 out never reads the entry: it succeeds and matches the restatement
    away = [q for q in ([0, 1], [0, 3], [1, 2], [5, 4], [0]) if 2 not in active(q)]
    assert away
    for query in away:
        want, report = joint_reference(beliefs, sched, query, spec["node_vars"])
        got, e = plan.joint(query)
        assert e == 0 and got.shape == want.shape and np.all(got > 0)
        assert np.max(np.abs(got - want) / want) <= 4.0 * parity_bound(report), query
    # evidence that zeroes the entry (x3 = 1) lets every query through
    plan.set_evidence({3: 1})
    plan.propagate()
    beliefs = {c: plan.belief(c) for c in range(n)}
    for query in reads:
        want, report = joint_reference(beliefs, sched, query, spec["node_vars"])
        got, _ = plan.joint(query)
        assert np.all((got == 0) == (want == 0)) and np.all(got >= 0)
        nz = want != 0
        assert np.max(np.abs(got[nz] - want[nz]) / want[nz]) <= 4.0 * parity_bound(report), query
    plan.close()
    factors = [list(vs) for vs in spec["node_vars"][:n]]
    tree = jt.create_junction_tree(factors, spec["sizes"])
    with pytest.raises(_capi.JtpError, match="negative or NaN belief entry"):
        tree.joint(pots[:n], [5, 0])
    assert np.all(tree.joint(pots[:n], [5, 0], evidence={3: 1}) >= 0)
