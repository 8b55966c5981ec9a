"""The conditions the device tests of hard evidence rest on (tests/test_gpu_evidence_sliced.py), checked on the host for every
case before any device result exists: the slicing reference agrees with the older indicator reference on finite tables, it does
not read a contradicted entry, and the poison reaches enough of the tables - cliques other than the one the engine used to
mask included."""
import numpy as np
import pytest

import evidence_reference as er
from junctiontree_amd import computation as comp

CASES = er.tree_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_sliced_reference_ignores_contradicted_entries(name):
    spec, dtype, sets = CASES[name]
    pots = er.clean_tables(spec, dtype)
    assert sets[0] == {} and len(sets) >= 9
    multi_holder = off_host = False
    for obs in sets[1:]:
        clean, z = er.sliced_beliefs(spec, pots, obs)
        ind, z_ind = er.indicator_beliefs(spec, pots, obs)
        # finite tables: slicing and the one-hot indicator in one clique are the same computation up to rounding
        assert abs(z - z_ind) <= 1e-14 * abs(z)
        for a, b in zip(clean, ind):
            assert a.shape == b.shape
            assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(b))
        # the poison is no token: a tenth of some clique at least, and cliques beside the first that holds the variable
        frac = er.poisoned_fraction(spec, obs)
        assert max(frac) >= 0.1
        for var in obs:
            held = er.holders(spec, var)
            assert held
            multi_holder = multi_holder or len(held) >= 2
            off_host = off_host or any(frac[c] > 0 for c in held[1:])
        for kind in er.kinds_for(dtype):
            bad = er.poison(spec, pots, obs, kind)
            assert sum(int(np.sum(~np.isfinite(t.astype(np.float64)) | (np.abs(t.astype(np.float64)) >= 1e200))) for t in bad[:spec["n_cliques"]]) > 0
            got, z_bad = er.sliced_beliefs(spec, bad, obs)
            assert z_bad == z
            for a, b in zip(got, clean):
                assert np.array_equal(a, b), (name, obs, kind)
            # ... where the indicator reference, which every older evidence test uses, is lost
            if kind != "big":
                with np.errstate(invalid="ignore"):
                    assert np.isnan(er.indicator_beliefs(spec, bad, obs)[1])
    assert multi_holder and off_host


def test_every_axis_of_the_widest_clique_is_observed_by_some_set():
    for name in ("pow2_f64", "pow2_f32", "card3_f64", "card5_f32"):
        spec, _, sets = CASES[name]
        seen = {v for obs in sets for v in obs}
        assert set(spec["node_vars"][er.widest_clique(spec)]) <= seen
    for name in ("multi_pow2_f64", "multi_pow2_f32", "multi_card3_f64"):
        spec, _, sets = CASES[name]
        wide = spec["node_vars"][er.widest_clique(spec)]
        seen = {v for obs in sets for v in obs}
        assert len(sets) == 11 and {wide[0], wide[len(wide) // 2], wide[-1]} & seen >= {wide[0], wide[-1]}


def test_factor_list_reference_on_the_lattice():
    """the public API's pair: slicing every factor that holds the variable, and a poison that includes a 0 x inf product"""
    import junctiontree_amd as jt
    from junctiontree_amd import synthetic
    import jt_oracle as oracle
    factors, sizes, values = synthetic.lattice_mrf(3, 6, 4, dtype=np.float64)
    names = sorted(sizes)
    obs = {names[3]: 2, names[7]: 0, names[11]: 3}
    for order in (None, synthetic.lattice_column_order(3, 6)):
        tree = jt.create_junction_tree(factors, sizes, order=order)
        ct = tree.clique_tree
        clean = er.sliced_factor_marginals(tree, factors, sizes, values, obs)
        # against the indicator in one factor, on finite tables
        vals, done = [np.array(v, dtype=np.float64) for v in values], set()
        for i, f in enumerate(factors):
            for ax, v in enumerate(f):
                if v in obs and v not in done:
                    done.add(v)
                    ind = np.zeros(sizes[v])
                    ind[obs[v]] = 1.0
                    vals[i] = vals[i] * ind.reshape([-1 if a == ax else 1 for a in range(len(f))])
        want = oracle.propagate(tree.tree, tree.separators, ct.maxcliques, ct.factor_to_maxclique, factors, sizes, vals)
        for a, b in zip(clean, want):
            assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(b))
        zeros = er.zero_partners(factors, ct.factor_to_maxclique, obs)
        assert zeros                                           # (a clique whose product holds 0 x inf)
        for kind in ("+inf", "-inf", "nan", "big"):
            bad = er.poison_factors(factors, values, obs, kind, zeros=zeros)
            for a, b in zip(er.sliced_factor_marginals(tree, factors, sizes, bad, obs), clean):
                assert np.array_equal(a, b)
        # a poisoned factor sits in a clique that is not the first to hold its observed variable
        first = {v: next(c for c, cl in enumerate(ct.maxcliques) if v in cl) for v in obs}
        assert any(v in f and ct.factor_to_maxclique[i] != first[v] for i, f in enumerate(factors) for v in obs)


def test_apply_evidence_fixture_agrees_with_slicing(golden):
    """the reference's own `apply_evidence` outputs (tests/golden/apply_evidence.npz) are what `_slice` cuts"""
    g = golden("apply_evidence.npz")
    n_checked = 0
    for case in g.meta["cases"]:
        pots = g.arrs(case["potentials"])
        evidence = {k: v for k, v in case["evidence"]}
        for p, labels, ref in zip(pots, case["variables"], g.arrs(case["ref"])):
            if np.ndim(p) == 0:
                continue
            cut = er._slice(np.asarray(p), list(labels), evidence)
            assert cut.shape == ref.shape
            np.testing.assert_array_equal(cut, ref)
            n_checked += 1
        out = comp.apply_evidence(pots, case["variables"], evidence)
        for o, p, labels in zip(out, pots, case["variables"]):
            if np.ndim(p):
                np.testing.assert_array_equal(np.asarray(o[0]), er._slice(np.asarray(p), list(labels), evidence))
    assert n_checked >= 5
