"""Signed tables through the planner's task tables on the CPU: the emulator (tests/emulator.py, tests/scaled_emulator.py) executes
what `jtp_plan_create` emits on tables with negative entries, against the oracle under the cancellation bound of
tests/signed_reference.py - |got - want| <= 1e-11 * B_abs, B_abs the oracle on the absolute tables.  The emulator adds in the order
the kernels add (partial copies, reduce tasks, sub-box staging), in float64 whatever the storage type of the layout, so this also
shows that the bound holds for the summation orders the planner emits before any device run (tests/test_gpu_signed.py)."""
import math

import numpy as np
import pytest

import junctiontree_amd as jt
import signed_reference as sr
from emulator import Emulator
from junctiontree_amd import engine, synthetic
from test_planner_emulated import emulate
from test_scaled_emulated import run as run_scaled

RTOL = 1e-11

SPECS = {
    "wide15": lambda: synthetic.wide_binary_tree(n_cliques=15, width=14, sep=7, card=2, seed=2),
    "random9": lambda: synthetic.random_tree(n_cliques=9, width=13, sep=5, card=2, seed=3),
    "chain6_card16": lambda: synthetic.chain_tree(n_cliques=6, card=16, width=3),
    "chain5_card4": lambda: synthetic.chain_tree(n_cliques=5, card=4, width=3),
    "card3": lambda: synthetic.wide_binary_tree(n_cliques=7, width=8, sep=4, card=3, seed=3),
    "card5": lambda: synthetic.wide_binary_tree(n_cliques=7, width=6, sep=3, card=5, seed=5),
    "card6": lambda: synthetic.wide_binary_tree(n_cliques=7, width=5, sep=2, card=6, seed=6),
    "random8_card5": lambda: synthetic.random_tree(n_cliques=8, width=4, sep=2, card=5, seed=6),
}
_inputs = {}


def inputs_of(name):
    """(spec, {"plain" | "leaf" | "leaf+inner": (tables, Bound)}) of a spec, made once: the conditions and the facts about the negations
    are asserted on the oracle here, before any emulated result is looked at"""
    if name not in _inputs:
        spec = SPECS[name]()
        runs, _, _ = sr.negation_facts(spec, sr.signed_potentials(spec, seed=21), name)
        _inputs[name] = (spec, runs)
    return _inputs[name]


def check_emulated(name, dtypes=("f64", "f32"), which=("plain", "leaf", "leaf+inner"), **opts):
    """every belief, every separator belief and z of the emulated plan (per-level order, then dataflow order: `emulate` asserts
    the two bit-equal) under the bound; returns the last description"""
    spec, runs = inputs_of(name)
    desc = None
    for key in which:
        pots, bound = runs[key]
        for dtype in dtypes:
            got, desc = emulate(spec["tree"], pots, spec["node_vars"], spec["sizes"], dtype=dtype, **opts)
            assert sorted(got) == list(range(len(spec["node_vars"])))
            for node, arr in got.items():
                bound.check(node, arr, RTOL, "%s %s %r" % (key, dtype, opts))
            for c in range(spec["n_cliques"]):              # every clique belief sums to Z
                bound.check_z(float(got[c].sum()), RTOL, "%s %s clique %d" % (key, dtype, c))
            assert (got[0].sum() < 0) == (key == "leaf")
    return desc


@pytest.mark.parametrize("name", sorted(SPECS))
def test_signed_tables_per_level_and_in_dataflow_order(name):
    desc = check_emulated(name)
    assert desc["n_messages"] == 2 * (inputs_of(name)[0]["n_cliques"] - 1)
    check_emulated(name, dtypes=("f64",), which=("leaf",), block_log2=10)


@pytest.mark.parametrize("name", ["wide15", "random9", "chain6_card16"])
def test_signed_partial_copies_summed_by_reduce_tasks(monkeypatch, name):
    monkeypatch.setenv("JTP_REDUCE_MIN", "2")
    desc = check_emulated(name, dtypes=("f64",), block_log2=10, layout_policy=3)
    assert sum(t["kind"] for t in desc["tasks"]) > 0
    assert any(s["up_red_task"] >= 0 or s["dn_red_task"] >= 0 for s in desc["pseps"])


def test_signed_mixed_radix_rows():
    desc = check_emulated("card3", which=("plain", "leaf"))
    assert desc["tmix"] == 1 and any(p["group_mask"] for p in desc["pnodes"])


@pytest.mark.parametrize("sweep", [False, True])
def test_signed_factors_through_unit_cliques_lean_records_and_folded_marginals(monkeypatch, sweep):
    """the 3 x 6 lattice of cardinality 8 planned as the large ones are: cliques that keep no table, lean records, factor marginals
    folded into the propagate - signed factor tables (`signed_reference.signed_factors`), one factor negated whole for Z < 0"""
    monkeypatch.setenv("JTP_TINY_LEVEL_ELEMS", "0")
    monkeypatch.setenv("JTP_FOLD", "1")
    h, w, card = 3, 6, 8
    factors, sizes, values = synthetic.lattice_mrf(h, w, card, dtype=np.float64)
    tree = jt.create_junction_tree(factors, dict(sizes), order=synthetic.lattice_column_order(h, w) if sweep else None)
    ct = tree.clique_tree
    f2c = ct.factor_to_maxclique
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]
    signed = sr.signed_factors(values)
    flipped = list(signed)
    flipped[-1] = -signed[-1]
    bounds = {}
    for key, vals in (("plain", signed), ("negated", flipped)):
        bounds[key] = sr.FactorBound(tree, factors, sizes, vals, "lattice %s%s" % (key, " sweep" if sweep else ""))
        bounds[key].conditions()
    assert bounds["plain"].z > 0 > bounds["negated"].z
    plan = engine.Plan(tree.tree, node_vars, sizes, dtype="f64", plan_only=True, cover=tree.cover(), fold=(tuple(f2c), tuple(map(tuple, factors))))
    d = plan.describe()
    fold_tasks = [i for i, t in enumerate(d["tasks"]) if t["fold"]]
    assert fold_tasks and any(t["lean_off"] > 0 for t in d["tasks"]) and any(p["unit"] and p["real"] >= 0 for p in d["pnodes"])
    groups, open_ = [], {}                                  # (requests on cliques without a table, by clique in request order, three to a task)
    for i, c in enumerate(f2c):
        if not d["pnodes"][plan.abi_of[c]]["unit"]:
            continue
        if c not in open_ or len(groups[open_[c]]) >= 3:
            open_[c] = len(groups)
            groups.append([])
        groups[open_[c]].append(i)
    assert len(groups) == len(fold_tasks)
    for key, vals in (("plain", signed), ("negated", flipped)):
        b = bounds[key]
        emu = Emulator(d)
        pots = ct.evaluate(vals)
        for c in plan.cliques:
            emu.set_potential(plan.abi_of[c], [plan.var_id[lab] for lab in node_vars[c]], [sizes[lab] for lab in node_vars[c]], pots[c])
        emu.propagate()
        level = emu.msg.copy()
        emu.propagate_flow()
        np.testing.assert_array_equal(level, emu.msg)
        bel = [emu.belief(plan.abi_of[c], [plan.var_id[lab] for lab in node_vars[c]], [sizes[lab] for lab in node_vars[c]]) for c in plan.cliques]
        b.check(ct.marginalize(bel), RTOL, "from the beliefs")
        for t, grp in zip(fold_tasks, groups):
            for j, i in enumerate(grp):
                got = emu.folded_marginal(t, j, [plan.var_id[lab] for lab in factors[i]], [sizes[lab] for lab in factors[i]])
                sr.check(got, b.want[i], b.b_abs[i], RTOL, "%s folded factor %d" % (key, i))
    plan.close()


SCALED_SPECS = {          # (the recipes behind tests/test_scaled_emulated.py's cases of these names, whose plans `run` describes once)
    "wide": lambda: synthetic.wide_binary_tree(n_cliques=7, width=12, sep=6),
    "card3": lambda: synthetic.wide_binary_tree(n_cliques=7, width=5, sep=2, card=3, seed=4),
}


@pytest.mark.parametrize("name", sorted(SCALED_SPECS))
def test_a_scaled_plan_reports_a_negative_z(name):
    """JTP_SCALED on signed tables: the exponent of a message comes from the magnitudes of signed entries.  In range the scaled run is
    the unscaled run bit for bit up to one exponent per node; with one clique negated the sign is -1 and log|Z| = log(-z); every table
    x 2^200 moves log|Z| and leaves sign and normalised tables alone."""
    from test_scaled_emulated import CASES, LN2
    spec = SCALED_SPECS[name]()
    n = spec["n_cliques"]
    assert CASES[name][2] == spec["node_vars"] and CASES[name][0] == spec["tree"]
    runs, _, _ = sr.negation_facts(spec, sr.signed_potentials(spec, seed=21), "scaled " + name)
    for key, (tables, bound) in runs.items():
        scaled, exps, (sign, log_z) = run_scaled(name, tables)
        plain, zeros, (sign_plain, _) = run_scaled(name, tables, rescale=False)
        assert any(exps.values()) and not any(zeros.values())
        for node in scaled:
            np.testing.assert_array_equal(np.ldexp(scaled[node], exps[node]), plain[node], err_msg="%s node %r" % (key, node))
            bound.check(node, plain[node], RTOL, "scaled " + key)
        want_sign = -1.0 if key == "leaf" else 1.0
        assert sign == sign_plain == want_sign == math.copysign(1.0, bound.z)
        assert abs(log_z - math.log(abs(bound.z))) <= 1e-11 * max(1.0, abs(math.log(abs(bound.z))))
        moved = [np.ldexp(np.asarray(p, dtype=np.float64), 200) if c < n else p for c, p in enumerate(tables)]
        far, _, (sign_far, log_z_far) = run_scaled(name, moved)
        for node in far:
            np.testing.assert_array_equal(far[node] / abs(far[node].sum()), scaled[node] / abs(scaled[node].sum()), err_msg="%s node %r x 2^200" % (key, node))
        assert sign_far == want_sign and abs(log_z_far - (log_z + n * 200 * LN2)) <= 1e-11 * abs(log_z_far)
