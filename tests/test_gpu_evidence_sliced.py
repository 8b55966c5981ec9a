"""Hard evidence is slicing: an entry that contradicts the evidence never reaches a sum, whatever it holds.

Every case makes two assertions (tests/evidence_reference.py has the reference and the poison, tests/test_evidence_host.py the
conditions both rest on):
  (a) beliefs, separator beliefs, Z and marginals on clean tables match the SLICED reference - 1e-11 (float64 storage) / 1e-6
      (float32), elementwise;
  (b) the same plan with the same evidence on tables whose contradicted entries hold +inf, -inf, NaN or 1e200 returns the bit
      patterns of its own clean run: a contradicted entry is replaced before it is used, so the arithmetic does not change and
      no tolerance applies.
No propagate may fall back from its dataflow launch (`flow_fallbacks == 0`): np.nan and the NaNs arithmetic forms are not the
arena's "unwritten" marker."""
import functools

import numpy as np
import pytest

import evidence_reference as er
import junctiontree_amd as jt
from junctiontree_amd import engine, synthetic
from junctiontree_amd._capi import JtpError
from test_gpu_parity import RTOL32, RTOL64, close

pytestmark = pytest.mark.gpu

CASES = er.tree_cases()


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


@functools.lru_cache(maxsize=None)
def _reference(name, obs_items):
    spec, dtype, _ = CASES[name]
    return er.sliced_beliefs(spec, er.clean_tables(spec, dtype), dict(obs_items))


def reference(name, obs):
    return _reference(name, tuple(sorted(obs.items())))


def upload(plan, spec, tables, batch=0):
    for c in range(spec["n_cliques"]):
        plan.set_potential(c, tables[c], batch=batch)


def propagate(plan, *span):
    plan.propagate(*span)
    assert plan.stats()["flow_fallbacks"] == 0


def read_set(plan, spec, b):
    """everything a propagate leaves for evidence set b: every node's belief, Z, a two-variable marginal of every clique"""
    out = [plan.belief(node, batch=b) for node in range(len(spec["node_vars"]))]
    out.append(np.array([plan.z(batch=b)]))
    out += plan.marginals([(c, list(spec["node_vars"][c])[:2]) for c in range(spec["n_cliques"])], batch=b)
    return out


def check_a(name, obs, got, what):
    spec, dtype, _ = CASES[name]
    want, z = reference(name, obs)
    rtol = RTOL32 if dtype == "f32" else RTOL64
    n_nodes, n = len(spec["node_vars"]), spec["n_cliques"]
    for node in range(n_nodes):
        close(got[node], want[node], rtol=rtol, what="%s node %d" % (what, node))
    assert abs(got[n_nodes][0] - z) <= rtol * abs(z), what
    for c in range(n):
        axes = tuple(range(2, len(spec["node_vars"][c])))
        close(got[n_nodes + 1 + c], want[c].sum(axis=axes), rtol=rtol, what="%s marginal of clique %d" % (what, c))


def check_b(got, clean, what):
    assert len(got) == len(clean)
    for i, (g, c) in enumerate(zip(got, clean)):
        assert g.shape == c.shape
        assert np.array_equal(er.bits(g), er.bits(c)), "%s: array %d differs from the clean run's in %d of %d entries (%d not finite)" % (
            what, i, int(np.sum(er.bits(g) != er.bits(c))), g.size, int(np.sum(~np.isfinite(g))))


def run_own_tables(name, one_at_a_time=False, **opts):
    """Every evidence set on tables of its own, poisoned against its own evidence: one plan of one set that takes the sets in turn
    (the default dataflow launch in blockIdx order), or one of a set per batch."""
    spec, dtype, sets = CASES[name]
    nb = len(sets)
    tables = er.clean_tables(spec, dtype)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, n_batch=1 if one_at_a_time else nb, **opts)
    results = {}
    for kind in [None] + er.kinds_for(dtype):
        results[kind] = []
        for b, obs in enumerate(sets):
            slot = 0 if one_at_a_time else b
            upload(plan, spec, tables if kind is None else er.poison(spec, tables, obs, kind), batch=slot)
            plan.set_evidence(obs, batch=slot)
            if one_at_a_time:
                propagate(plan)
                results[kind].append(read_set(plan, spec, 0))
        if not one_at_a_time:
            propagate(plan, 0, nb)
            results[kind] = [read_set(plan, spec, b) for b in range(nb)]
    desc = plan.describe()
    plan.close()
    for b, obs in enumerate(sets):
        check_a(name, obs, results[None][b], "%s %r set %d" % (name, opts, b))
        for kind in er.kinds_for(dtype):
            check_b(results[kind][b], results[None][b], "%s %r set %d %r poisoned with %s" % (name, opts, b, obs, kind))
    return desc


def run_shared_tables(name, rounds=1, **opts):
    """All evidence sets over ONE copy of the tables (share_potentials / multiset).  The tables are poisoned against one set's
    evidence at a time; that set, and every set that observes at least what it observes, must not notice - the others, which
    are allowed to read those entries, may return what they like."""
    spec, dtype, sets = CASES[name]
    sets = [dict(s) for s in sets]
    nb = len(sets)
    tables = er.clean_tables(spec, dtype)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, n_batch=nb, **opts)
    desc = plan.describe()
    for rnd in range(rounds):
        for b, obs in enumerate(sets):
            plan.set_evidence(obs, batch=b)
        upload(plan, spec, tables)
        propagate(plan)
        clean = [read_set(plan, spec, b) for b in range(nb)]
        for b, obs in enumerate(sets):
            check_a(name, obs, clean[b], "%s %r round %d set %d" % (name, opts, rnd, b))
        for t, target in enumerate(sets):
            if not target:
                continue
            safe = [b for b, obs in enumerate(sets) if all(obs.get(v) == s for v, s in target.items())]
            assert t in safe
            for kind in er.kinds_for(dtype):
                upload(plan, spec, er.poison(spec, tables, target, kind))
                propagate(plan)
                for b in safe:
                    check_b(read_set(plan, spec, b), clean[b], "%s %r round %d set %d %r, tables poisoned with %s against set %d" % (
                        name, opts, rnd, b, sets[b], kind, t))
        # evidence can be replaced: the next round swaps two sets (the other half of the message arenas, new active lists)
        sets[1], sets[nb - 1] = sets[nb - 1], sets[1]
    plan.close()
    return desc


# ------------------------------------------------------------------------------------------ jt_pass, power-of-two rows

@pytest.mark.parametrize("mode", ["flow", "flow_tickets", "level_launches"])
@pytest.mark.parametrize("name", ["pow2_f64", "pow2_f32"])
def test_pass_over_power_of_two_rows(name, mode):
    """14 sets that observe nothing, then each variable of the widest clique in turn - a mask on element bits, lane bits, loop bits
    and chunk bits - and two sets of three variables, in the three launch modes."""
    if mode == "flow":
        desc = run_own_tables(name, one_at_a_time=True)
    else:
        desc = run_own_tables(name, **{mode: True})
    # every index bit of the widest clique's table carries some set's mask
    spec, _, sets = CASES[name]
    wide = er.widest_clique(spec)
    assert {v for obs in sets for v in obs} >= set(spec["node_vars"][wide])


@pytest.mark.parametrize("name", ["pow2_f64", "pow2_f32"])
def test_reduce_tasks(monkeypatch, name):
    monkeypatch.setenv("JTP_REDUCE_MIN", "2")
    desc = run_own_tables(name, block_log2=11, layout_policy=3)       # (the layout with the most partial copies)
    assert sum(t["kind"] for t in desc["tasks"]) > 0


# ------------------------------------------------------------------------------------------ mixed-radix rows

@pytest.mark.parametrize("no_compact", [False, True])
@pytest.mark.parametrize("name", ["card3_f64", "card3_f32", "card5_f64", "card5_f32"])
def test_mixed_radix_rows(name, no_compact):
    desc = run_own_tables(name, no_compact=no_compact)
    assert desc["tmix"] == (0 if no_compact else 1)                   # (a mixed-radix thread part, or rows of padded bit fields)


# ------------------------------------------------------------------------------------------ shared tables, one pass per set

@pytest.mark.parametrize("name", ["pow2_f64", "card3_f64"])
def test_shared_tables_one_pass_per_set(name):
    run_shared_tables(name, share_potentials=True)


# ------------------------------------------------------------------------------------------ jt_multi_flow

def multi_paths(desc, plan_var_id, sets):
    """Per group of eight sets, which forms of the multi-set pass its distribute tasks (whose groups are the caller's sets 8 g ..
    8 g + 7) run: row evidence with / without element-dependent messages, thread-part evidence only, and a set with none."""
    TB = desc["TB"]
    out = []
    for g in range(0, len(sets), 8):
        group, seen = sets[g:g + 8], set()
        ids = [{plan_var_id[v] for v in obs} for obs in group]
        if any(not obs for obs in group) or len(group) < 8:       # (a short last group is padded with evidence-free sets)
            seen.add("free")
        for tk in desc["tasks"]:
            if tk["kind"] != 0:
                continue
            pn = desc["pnodes"][tk["pnode"]]
            top = {v: pos + nb for v, pos, nb in zip(pn["vars"], pn["pos"], pn["nb"])}
            here = [{v for v in obs if v in top} for obs in ids]
            if not any(here):
                continue
            row = any(top[v] > TB for obs in here for v in obs)
            edep = any(m["e_dep"] for m in tk["in"])
            seen.add(("row+edep" if edep else "row") if row else "thread")
        out.append(seen)
    return out


@pytest.mark.parametrize("name,opts", [("multi_pow2_f64", {}), ("multi_pow2_f32", {"block_log2": 11}), ("multi_card3_f64", {"level_launches": True})])
def test_multi_set_pass(name, opts):
    """11 sets (a padded last group) eight to a pass over one copy of the tables, two rounds with the evidence of two sets swapped."""
    spec, dtype, sets = CASES[name]
    probe = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, n_batch=len(sets), multiset=True, plan_only=True, **opts)
    desc0 = probe.describe()
    paths = multi_paths(desc0, probe.var_id, sets)
    probe.close()
    # one group runs every form of the pass: rows skipped for some of its sets, thread-part evidence only, a set that observes nothing -
    # and, in the one tree whose layout has messages that depend on the element bits, skipped rows with such messages
    edep = any(m["e_dep"] for tk in desc0["tasks"] if tk["kind"] == 0 for m in tk["in"])
    assert edep == (name == "multi_card3_f64")
    assert any(p >= {"row", "thread", "free"} | ({"row+edep"} if edep else set()) for p in paths), paths
    desc = run_shared_tables(name, rounds=2, multiset=True, **opts)
    assert desc["multiset"] == 1


def test_multi_set_pass_with_active_lists(monkeypatch):
    """the same with an evidence-free set of the engine's own (JTP_EF_SHARE): a set takes the upward messages of the subtrees it
    observes nothing in from that set - which reads every entry, the poisoned ones too - and the lists follow the swapped evidence"""
    monkeypatch.setenv("JTP_EF_SHARE", "1")
    desc = run_shared_tables("multi_pow2_f64", rounds=2, multiset=True)
    assert desc["multiset"] == 1


# ------------------------------------------------------------------------------------------ the public API: factor lists

def lattice_case(h, w, card, order=False):
    factors, sizes, values = synthetic.lattice_mrf(h, w, card, dtype=np.float64)
    tree = jt.create_junction_tree(factors, sizes, order=synthetic.lattice_column_order(h, w) if order else None)
    names = sorted(sizes)
    # every set observes at least the core, so a table poisoned against the core is poisoned for every set
    core = {names[3]: 2 % card, names[7]: 0}
    sets = [dict(core), {**core, names[11]: 3 % card}, {**core, names[0]: 1, names[14]: 2 % card},
            {**core, **{v: 0 for v in names[:6] if v not in core}}]
    return factors, sizes, values, tree, core, sets


def poisoned_values(factors, values, tree, core, kind):
    """factor tables poisoned against the core - one factor is 0 where another of its clique is inf: the clique table formed on the
    device then holds NaN there"""
    zeros = er.zero_partners(factors, tree.clique_tree.factor_to_maxclique, core)
    assert zeros
    return er.poison_factors(factors, values, core, kind, zeros=zeros)


def check_factor_marginals(got, factors, values, tree, sizes, sets, what, normalized=False):
    for b, obs in enumerate(sets):
        want = er.sliced_factor_marginals(tree, factors, sizes, values, obs)
        for f, (g, w_) in enumerate(zip(got[b], want)):
            close(g, w_ / w_.sum() if normalized else w_, rtol=RTOL64, what="%s set %d factor %d" % (what, b, f))
            assert not np.any(g[er._contradicted(factors[f], g.shape, obs)]), "%s set %d factor %d: mass at a contradicted entry" % (what, b, f)


@pytest.mark.parametrize("order", [False, True])
def test_evidence_sets_through_the_public_api_with_poisoned_factors(order):
    """`propagate_evidence_sets` (multi-set plan; `normalize`: scaled plan over shared tables, unit cliques, the lean pass) on the
    lattice of test_evidence_and_unit_cliques, min-fill and column-sweep trees, and the same sets on a plan with `cover` directly."""
    factors, sizes, values, tree, core, sets = lattice_case(3, 6, 4, order)
    ct = tree.clique_tree
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]

    def direct(vals):
        plan = engine.Plan(tree.tree, node_vars, sizes, dtype="f64", cover=tree.cover(), n_batch=len(sets), share_potentials=True)
        assert plan.stats()["n_unit_cliques"] > 0
        plan.stage_factors(factors, ct.factor_to_maxclique, vals)
        for b, obs in enumerate(sets):
            plan.set_evidence(obs, batch=b)
        propagate(plan, 0, len(sets))
        out = [[np.array(m) for m in plan.factor_marginals(factors, ct.factor_to_maxclique, batch=b)] for b in range(len(sets))]
        plan.close()
        return out, None

    def api(vals, normalize=False):
        out = [[np.array(m) for m in per_set] for per_set in tree.propagate_evidence_sets(vals, sets, normalize=normalize)]
        assert tree._memo["evidence_plan"].stats()["flow_fallbacks"] == 0
        return out, (np.array(tree.log_z_sets) if normalize else None)

    for what, run, normalized in (("multiset", api, False), ("scaled", lambda v: api(v, normalize=True), True), ("cover", direct, False)):
        clean, log_z = run(values)
        check_factor_marginals(clean, factors, values, tree, sizes, sets, what, normalized)
        if normalized:
            z = [er.sliced_factor_marginals(tree, factors, sizes, values, obs)[0].sum() for obs in sets]
            np.testing.assert_allclose(log_z, np.log(z), rtol=0, atol=1e-11)
        for kind in er.kinds_for("f64"):
            got, log_z_bad = run(poisoned_values(factors, values, tree, core, kind))
            for b in range(len(sets)):
                check_b(got[b], clean[b], "%s set %d, factors poisoned with %s" % (what, b, kind))
                assert all(np.isfinite(m).all() for m in got[b])
            if normalized:
                assert np.array_equal(er.bits(log_z_bad), er.bits(log_z))


# ------------------------------------------------------------------------------------------ queries built on the beliefs

@pytest.mark.parametrize("card", [2, 3])
def test_queries_read_sliced_beliefs(card):
    """expected_counts, sample, joint and map under evidence on poisoned factors: what the clean factors give, bit for bit"""
    from joint_reference import brute_force_joint
    factors, sizes, values, tree, core, sets = lattice_case(3, 5, card)
    names = sorted(sizes)
    weights = np.array([0.5, 2.0, 1.0, 0.25])
    query = [names[1], names[13], names[6]]
    obs = sets[2]

    def run(vals):
        counts = tree.expected_counts(vals, sets, weights=weights)
        out = {"counts": [np.array(c) for c in counts], "log_z": np.array(tree.log_z_sets)}
        states = tree.sample(vals, 64, seed=5, evidence=obs)
        out["sample"] = np.stack([states[v] for v in names])
        out["joint"] = tree.joint(vals, query, evidence=obs)
        st, val = tree.map_evidence_sets(vals, sets)
        out["map"] = np.stack([st[v] for v in names])
        out["map_value"] = np.array(val)
        return out

    clean = run(values)
    # (a) against slicing
    per_set = [er.sliced_factor_marginals(tree, factors, sizes, values, o) for o in sets]
    for f in range(len(factors)):
        close(clean["counts"][f], sum(w * m[f] / m[f].sum() for w, m in zip(weights, per_set)), rtol=RTOL64, what="counts of factor %d" % f)
    np.testing.assert_allclose(clean["log_z"], [np.log(m[0].sum()) for m in per_set], rtol=0, atol=1e-11)
    for i, v in enumerate(names):
        if v in obs:
            assert np.all(clean["sample"][i] == obs[v])
    cut_sizes = {v: (1 if v in obs else n) for v, n in sizes.items()}
    cut = [er._slice(np.asarray(x, dtype=np.float64), f, obs) for f, x in zip(factors, values)]
    want = er._embed(brute_force_joint(factors, cut_sizes, cut, None, query), query, [sizes[v] for v in query], obs)
    close(clean["joint"], want, rtol=RTOL64, what="joint")
    for b, o in enumerate(sets):
        for i, v in enumerate(names):
            if v in o:
                assert clean["map"][i, b] == o[v]
    # (b) the poison is not seen
    for kind in er.kinds_for("f64"):
        got = run(poisoned_values(factors, values, tree, core, kind))
        for key in clean:
            if key == "counts":
                check_b(got[key], clean[key], "counts, factors poisoned with %s" % kind)
            else:
                check_b([np.asarray(got[key])], [np.asarray(clean[key])], "%s, factors poisoned with %s" % (key, kind))


def test_an_entry_that_agrees_with_the_evidence_is_not_sanitised():
    """Slicing removes what contradicts the evidence and nothing else: a NaN at an ALLOWED entry still reaches the marginals, and
    sample, joint and map still refuse it."""
    factors, sizes, values, tree, core, sets = lattice_case(3, 5, 3)
    names = sorted(sizes)
    obs = sets[0]
    f = next(i for i, fv in enumerate(factors) if any(v in obs for v in fv))
    bad = [np.array(v) for v in values]
    allowed = np.argwhere(~er._contradicted(factors[f], bad[f].shape, obs))[0]
    bad[f][tuple(allowed)] = np.nan
    out = tree.propagate_evidence_sets(bad, [obs])[0]
    assert np.isnan(out[f]).any() and np.isnan(out[f][tuple(allowed)])
    with pytest.raises(JtpError):
        tree.sample(bad, 8, seed=1, evidence=obs)
    with pytest.raises(JtpError):
        tree.joint(bad, list(factors[f]), evidence=obs)
    with pytest.raises(JtpError):
        tree.map(bad, evidence=obs)
    bad[f][tuple(allowed)] = np.inf
    out = tree.propagate_evidence_sets(bad, [obs])[0]
    assert np.isinf(out[f][tuple(allowed)])
