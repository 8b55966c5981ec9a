"""Joints over variables of different cliques on the device (`jtp_joint`: kernels `jt_joint_sigma`, `jt_joint_level`) on a real MI355X,
against the numpy restatement of the definition (`tests/joint_reference.py`) applied to the beliefs read back from the same plan.

Both sides add the same non-negative terms in different orders, so the tolerance is derived, not measured: relative difference at most
4 B, B = 2^-53 x sum over the active cliques of (R_c + m_c + 2) - per clique the R_c terms of sigma, the at most R_c terms of U, one
multiplication per active child and the division; a factor 2 for the two sides and 2 for the second-order terms.  Entries that are
exactly zero on one side are zero on the other (potentials lie in [0.5, 1.5): nothing underflows)."""
import ctypes as C
import re

import numpy as np
import pytest

import junctiontree_amd as jt
from joint_reference import brute_force_joint, joint_reference, parity_bound
from junctiontree_amd import _capi, engine, synthetic
from sample_reference import schedule
from test_gpu_parity import RTOL32, RTOL64, close
from test_gpu_sample import README_FACTORS, README_SIZES, README_VALUES, case_of, spec_case, star_case, variants_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


def mixed_case():
    """the random tree of 16 cliques with cardinalities 2, 3, 5, 3, 4 in turn"""
    spec = synthetic.random_tree(16, 6, 3, card=3)
    spec["sizes"] = {v: (2, 3, 5, 3, 4)[v % 5] for v in spec["sizes"]}
    return spec_case(spec)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = mixed_case() if name == "random16_mixed" else star_case(int(name[4:])) if name.startswith("star") else case_of(name)
    return _cases[name]


def tables(cs, dtype, seed=21):
    """clique tables in [0.5, 1.5) in the numbers a plan of `dtype` holds (float32: drawn as float32), separators all ones"""
    tree, pots, node_vars, sizes, n = cs
    rng = np.random.default_rng(seed)
    np_t = np.float32 if dtype == "f32" else np.float64
    return [(rng.uniform(0.5, 1.5, np.shape(p)) if c < n else np.asarray(p)).astype(np_t) for c, p in enumerate(pots)]


def make(cs, dtype="f64", pots=None, evidence=None, **opts):
    tree, _, node_vars, sizes, n = cs
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, **opts)
    pots = tables(cs, dtype) if pots is None else pots
    for c in range(n):
        plan.set_potential(c, pots[c])
    if evidence:
        plan.set_evidence(evidence)
    plan.propagate()
    return plan


def probe(cs):
    return engine.Plan(cs[0], cs[2], cs[3], plan_only=True)


def free_of(sched):
    return {s[0]: s[4] for s in sched}


def queries(name):
    """{key: labels}: the queries of a case, named after what they are there for; picked from the schedule, so that they say what
    they ask for whatever labels the recipe gave the variables"""
    sched = schedule(probe(case(name)))
    F = free_of(sched)
    parent = {s[0]: s[1] for s in sched}
    depth = {s[0]: s[2] for s in sched}
    if name == "wide7":                                   # clique 0 the root, 1 and 2 below it, 3, 4 below 1 and 5, 6 below 2
        return {"two_leaves_under_the_root": [F[3][0], F[6][1]],
                "siblings_below_clique_1": [F[4][2], F[3][0], F[3][5]],
                "root_and_leaf": [F[5][0], F[0][3]],
                "one_clique": [F[4][5], F[4][0]]}
    if name == "chain6":                                  # clique i holds variables i, i + 1, i + 2
        return {"carried_up_four_cliques": [7, 3], "ends": [0, 7], "three": [2, 7, 0]}
    if name == "star5":
        kids = sorted(c for c in parent if parent[c] == sched[0][0])
        return {"three_children_and_the_root": [F[kids[3]][0], F[kids[0]][0], F[sched[0][0]][0], F[kids[4]][0]]}
    if name == "star12":                                  # the hub is the top; eight of its active children are staged, two read in place
        kids = sorted(c for c in parent if parent[c] == sched[0][0])
        return {"ten_children": [F[kids[i]][0] for i in (9, 0, 11, 3, 7, 1, 10, 4, 6, 2)]}
    # the random trees: the two deepest cliques that draw something and do not lie on one path, and the root
    def path(c):
        out = [c]
        while parent[out[-1]] >= 0:
            out.append(parent[out[-1]])
        return out
    deep = sorted((c for c in F if F[c]), key=lambda c: (-depth[c], c))
    a = deep[0]
    b = next(c for c in deep[1:] if c not in path(a) and a not in path(c))
    root = sched[0][0]
    return {"two_deep_cliques": [F[b][0], F[a][-1]],
            "two_of_one_clique_and_the_root": [F[a][0], F[root][1], F[a][-1], F[b][-1]],
            "below_the_root_only": [F[a][-1], F[path(a)[1]][0]] if len(path(a)) > 2 and F[path(a)[1]] else [F[a][0], F[a][-1]]}


def check_parity(plan, cs, query, what):
    tree, _, node_vars, sizes, n = cs
    beliefs = {c: plan.belief(c, dtype=np.float64) for c in range(n)}
    want, report = joint_reference(beliefs, schedule(plan), query, node_vars)
    got, e = plan.joint(query)
    bound = 4.0 * parity_bound(report)
    assert got.dtype == np.float64 and got.shape == want.shape == tuple(sizes[v] for v in query) and e == 0
    assert np.all((got == 0.0) == (want == 0.0)), what
    nz = want != 0.0
    worst = float(np.max(np.abs(got[nz] - want[nz]) / want[nz])) if nz.any() else 0.0
    print("%s: %d active cliques, worst relative difference %.3g, bound %.3g" % (what, len(report), worst, bound))
    assert worst <= bound, what
    return got, want, report


# ---------------------------------------------------------------------------------------------- 1. parity with the restatement

NAMES = ["wide7", "chain6", "star5", "star12", "random16_card3", "random16_mixed"]
RUNS = [(n, d, {}) for n in NAMES for d in ("f64", "f32")] + [("random16_card3", "f64", dict(no_compact=True)), ("random16_mixed", "f32", dict(no_compact=True)),
                                                              ("wide7", "f32", dict(no_compact=True)), ("chain6", "f64", dict(no_compact=True))]


@pytest.mark.parametrize("name,dtype,opts", RUNS, ids=["%s-%s%s" % (n, d, "-no_compact" if o else "") for n, d, o in RUNS])
def test_joints_equal_the_restatement_on_the_plans_own_beliefs(name, dtype, opts):
    cs = case(name)
    plan = make(cs, dtype, **opts)
    if name.startswith("random16") and not opts:
        assert plan.describe()["compact"] == 1
    for key, query in queries(name).items():
        got, want, report = check_parity(plan, cs, query, "%s %s %s" % (name, dtype, key))
        z = plan.z()                                          # it sums to Z, as every belief does: to the storage type's rounding
        assert abs(got.sum() - z) <= (4.0 * parity_bound(report) + (RTOL32 if dtype == "f32" else RTOL64)) * z
    plan.close()


def test_the_queries_cover_what_they_are_there_for():
    """from the restatement's report and the pack records: every situation the kernels treat differently occurs in some query above"""
    seen = set()
    for name in NAMES:
        cs = case(name)
        tree, _, node_vars, sizes, n = cs
        plan = probe(cs)
        sched = schedule(plan)
        F = free_of(sched)
        root = sched[0][0]
        ones = {c: np.ones([sizes[v] for v in node_vars[c]]) for c in range(n)}
        visit = [s[0] for s in sched]
        for key, query in queries(name).items():
            _, report = joint_reference(ones, sched, query, node_vars)
            home = {q: next(c for c in visit if q in F[c]) for q in query}
            seen.add("top is the root" if report[0][0] == root else "top is not the root")
            seen.update("R' > 64" for _, r, rp, m in report if rp > 64)
            seen.update("R' = 1" for _, r, rp, m in report if rp == 1)
            seen.update("R' cut into segments" for _, r, rp, m in report if rp >= 2048)
            seen.update("two active children" for _, r, rp, m in report if m >= 2)
            seen.update("three active children" for _, r, rp, m in report if m >= 3)
            seen.update("more active children than are staged" for _, r, rp, m in report if m >= 9)
            if len(set(home.values())) < len(query):
                seen.add("a clique home to two query variables")
            if len(report) == 1:
                seen.add("one clique")
            # a variable carried across at least three cliques: the path from its home to the top
            parent = {s[0]: s[1] for s in sched}
            for q in query:
                steps, c = 0, home[q]
                while c != report[0][0]:
                    c, steps = parent[c], steps + 1
                if steps >= 3:
                    seen.add("carried across three cliques")
            tree_order = sorted(query, key=lambda q: (visit.index(home[q]), node_vars[home[q]].index(q)))
            if list(query) != tree_order:
                seen.add("an order that is not the tree's")
    assert seen >= {"top is the root", "top is not the root", "R' > 64", "R' = 1", "R' cut into segments", "two active children", "three active children",
                    "more active children than are staged",
                    "a clique home to two query variables", "one clique", "carried across three cliques", "an order that is not the tree's"}, seen
    # ... and among the active cliques of the cardinality cases are tables stored as mixed-radix rows, one with a variable across
    # the thread part's top bit
    split, mixed = False, False
    for name in ("random16_card3", "random16_mixed"):
        cs = case(name)
        ones = {c: np.ones([cs[3][v] for v in cs[2][c]]) for c in range(cs[4])}
        for dtype in ("f64", "f32"):
            plan = engine.Plan(cs[0], cs[2], cs[3], dtype=dtype, plan_only=True)
            d = plan.describe()
            for query in queries(name).values():
                for clique, _, _, _ in joint_reference(ones, schedule(plan), query, cs[2])[1]:
                    split = split or d["pack"][plan.abi_of[clique]]["split_var"] >= 0
                    mixed = mixed or d["pnodes"][plan.abi_of[clique]]["tmix"] == 1
    assert split and mixed
    assert len(set(case("random16_mixed")[3].values())) > 2


# ---------------------------------------------------------------------------------------------- 2. single-clique queries

@pytest.mark.parametrize("name,dtype", [("wide7", "f32"), ("random16_mixed", "f64")])
def test_queries_inside_one_clique_are_the_cliques_marginals(name, dtype):
    cs = case(name)
    tree, _, node_vars, sizes, n = cs
    plan = make(cs, dtype)
    sched = schedule(plan)
    requests, across = [], []
    for clique, parent, depth, K, F, R in sched[:6]:
        if len(F) >= 2:
            requests.append((clique, [F[-1], F[0]]))             # one home: the clique is the top and the only clique read
        if K and F:
            across.append((clique, [F[0], K[0]]))                # K[0] has its home further up: the same table, formed from several cliques
    bound = 4.0 * 2.0 ** -53 * max(s[5] + 2 for s in sched)      # (one active clique without children)
    for (clique, labels), w in zip(requests, plan.marginals(requests)):
        got, e = plan.joint(labels)
        assert e == 0 and np.max(np.abs(got - w) / w) <= bound, (clique, labels)
    # (beliefs of different cliques agree to the rounding of the storage type, not to the summation bound)
    for (clique, labels), w in zip(across, plan.marginals(across)):
        close(plan.joint(labels)[0], w, rtol=RTOL32 if dtype == "f32" else RTOL64, what=str((clique, labels)))
    plan.close()


# ---------------------------------------------------------------------------------------------- 3. brute force

def chain5():
    spec = synthetic.chain_tree(3, card=2, width=3)
    return spec_case(spec, seed=7)


@pytest.mark.parametrize("evidence", [None, {"wet_grass": 1}], ids=["free", "wet"])
def test_the_readme_network_against_brute_force(evidence):
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    for query in (["cloudy", "wet_grass"], ["wet_grass", "cloudy"], ["sprinkler", "rain"], ["wet_grass", "rain", "cloudy", "sprinkler"], ["wet_grass"]):
        want = brute_force_joint(README_FACTORS, README_SIZES, README_VALUES, evidence, query)
        got = tree.joint(README_VALUES, query, evidence=evidence, normalize=True)
        close(got, want / want.sum(), rtol=RTOL64, what=str(query))
        raw = tree.joint(README_VALUES, query, evidence=evidence)
        close(raw, want, rtol=RTOL64, what=str(query))
        if evidence and "wet_grass" in query:                     # zero off the observed state
            assert np.all(np.take(got, 0, axis=query.index("wet_grass")) == 0.0) and got.sum() > 0.0
    before = tree.propagate(README_VALUES)                        # the evidence does not stick to the cached plan
    close(tree.joint(README_VALUES, ["cloudy", "wet_grass"]), brute_force_joint(README_FACTORS, README_SIZES, README_VALUES, None, ["cloudy", "wet_grass"]))
    for a, b in zip(before, tree.propagate(README_VALUES)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("evidence", [None, {2: 1}], ids=["free", "middle_observed"])
def test_a_chain_of_five_binary_variables_against_brute_force(evidence):
    cs = chain5()
    tree, pots, node_vars, sizes, n = cs
    plan = make(cs, "f64", pots=pots, evidence=evidence)
    for query in ([0, 4], [4, 0], [4, 2, 0], [1, 2], [3]):
        want = brute_force_joint(node_vars[:n], sizes, pots[:n], evidence, query)
        got, e = plan.joint(query)
        close(got / got.sum(), want / want.sum(), rtol=RTOL64, what=str(query))
        close(got, want, rtol=RTOL64, what=str(query))
        if evidence and 2 in query:
            assert np.all(np.take(got, 0, axis=query.index(2)) == 0.0) and got.sum() > 0.0
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. layout independence

def test_exactly_equal_beliefs_give_bit_equal_joints_in_every_layout():
    """The plans of `test_exactly_equal_beliefs_give_equal_samples_in_every_layout`: potentials that are small integers, so that every
    belief is an integer below 2^53 and the same in every layout; the order a joint's sums are added in depends on their lengths alone."""
    cs = case("wide7")
    tree, _, node_vars, sizes, n = cs
    rng = np.random.default_rng(12)
    pots = [rng.integers(1, 4, size=[sizes[v] for v in vs]).astype(np.float64) for vs in node_vars[:n]] + [np.ones([sizes[v] for v in vs]) for vs in node_vars[n:]]
    ref_bel, ref = None, None
    for key, opts in variants_of({"no_compact": dict(no_compact=True)}).items():
        plan = make(cs, "f64", pots=pots, **opts)
        bel = [plan.belief(c) for c in range(n)]
        got = {name: plan.joint(q)[0] for name, q in queries("wide7").items()}
        plan.close()
        if ref is None:
            ref_bel, ref = bel, got
            assert all(np.all(b == np.rint(b)) and b.max() < 2.0 ** 53 for b in bel)
        for c in range(n):
            np.testing.assert_array_equal(bel[c], ref_bel[c], err_msg="%s: belief of clique %d" % (key, c))
        for name in ref:
            np.testing.assert_array_equal(got[name], ref[name], err_msg="%s: equal beliefs, different joints (%s)" % (key, name))


# ---------------------------------------------------------------------------------------------- 5. scaled plans

def test_scaled_plans_give_joints_where_z_is_beyond_float64():
    """the model of `test_scaled_plans_sample_where_z_is_beyond_float64`: every table x 2^+-90, Z moved by 2^+-1350"""
    spec = synthetic.wide_binary_tree(15, 10, 5)
    cs = spec_case(spec, seed=2)
    tree, pots, node_vars, sizes, n = cs
    sched = schedule(probe(cs))
    F = free_of(sched)
    query = [F[14][0], F[7][1], F[3][0]]
    base = make(cs, "f64", pots=pots, scaled=True)
    want, _ = base.joint(query)
    want = want / want.sum()
    base.close()
    for shift in (90, -90):
        moved = [np.ldexp(p, shift) if c < n else p for c, p in enumerate(pots)]
        plan = make(cs, "f64", pots=moved, scaled=True)
        got, report = check_parity_scaled(plan, cs, query)
        table, e = plan.joint(query)
        assert np.all(np.isfinite(table)) and table.sum() > 0
        prob = table / table.sum()
        assert abs(prob.sum() - 1.0) <= 1e-15 * prob.size
        bound = 4.0 * parity_bound(report)
        assert np.max(np.abs(prob - want) / want) <= 2 * bound + 1e-11          # (the same distribution as the unmoved model's)
        sign, log_z = plan.log_z()
        assert sign == 1 and abs(np.log(table.sum()) + e * np.log(2.0) - log_z) <= (bound + 4 * 2.0 ** -53) * max(1.0, abs(log_z))
        assert e == plan.log2_scale(report[0][0]) and abs(e) > 1000
        plan.close()
        plain = make(cs, "f64", pots=moved)                       # without the flag the beliefs overflow (or vanish)
        if shift > 0:
            with pytest.raises(_capi.JtpError) as err:
                plain.joint(query)
            assert err.value.joint.shape == table.shape and re.search(r"\d+ \(clique, k\) pairs.*clique \d+", str(err.value))
        plain.close()


def check_parity_scaled(plan, cs, query):
    tree, _, node_vars, sizes, n = cs
    beliefs = {c: plan.belief(c, dtype=np.float64) for c in range(n)}
    want, report = joint_reference(beliefs, schedule(plan), query, node_vars)
    got, e = plan.joint(query)
    assert np.max(np.abs(got - want) / want) <= 4.0 * parity_bound(report)
    return got, report


def test_junction_tree_joint_normalises_where_z_is_beyond_float64():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    big = [np.ldexp(np.asarray(v, dtype=np.float64), 300) for v in README_VALUES]          # Z = 2^1200
    got = tree.joint(big, ["cloudy", "wet_grass"], normalize=True)
    want = brute_force_joint(README_FACTORS, README_SIZES, README_VALUES, None, ["cloudy", "wet_grass"])
    assert np.all(np.isfinite(got)) and abs(got.sum() - 1.0) <= 1e-15
    close(got, want / want.sum(), rtol=RTOL64)


# ---------------------------------------------------------------------------------------------- 6. evidence of probability zero

def zero_case():
    spec = synthetic.chain_tree(4, card=3, width=3)
    cs = spec_case(spec, seed=3)
    pots = [np.array(p) for p in cs[1]]
    pots[0][2, :, :] = 0.0                                   # variable 0 is never in state 2
    return cs, pots


def test_evidence_of_probability_zero_gives_zeros_and_no_error():
    cs, pots = zero_case()
    plan = make(cs, "f64", pots=pots, evidence={0: 2})
    assert plan.z() == 0.0
    for query in ([5, 1], [0, 5], [4]):
        ids = (C.c_int32 * len(query))(*[plan.var_id[v] for v in query])
        out = np.full((3,) * len(query), -1.0)
        rc = plan._lib.jtp_joint(plan._handle, 0, len(query), C.cast(ids, C.c_void_p), out.ctypes.data_as(C.c_void_p), None)
        assert rc == _capi.JTP_OK and np.all(out == 0.0)
    plan.set_evidence({})
    plan.propagate()
    assert plan.joint([5, 1])[0].min() > 0.0
    plan.close()
    factors = [list(vs) for vs in cs[2][:cs[4]]]
    tree = jt.create_junction_tree(factors, cs[3])
    assert np.all(tree.joint(pots[:cs[4]], [5, 1], evidence={0: 2}) == 0.0)
    with pytest.raises(_capi.JtpError, match="probability zero"):
        tree.joint(pots[:cs[4]], [5, 1], evidence={0: 2}, normalize=True)
    assert abs(tree.joint(pots[:cs[4]], [5, 1], normalize=True).sum() - 1.0) < 1e-14


# ---------------------------------------------------------------------------------------------- 7. non-finite beliefs

def test_beliefs_that_overflowed_are_reported_with_the_joint():
    cs = case("chain6")
    tree, _, node_vars, sizes, n = cs
    pots = [p * 1e80 if c < n else p for c, p in enumerate(tables(cs, "f64"))]      # the beliefs: 1e480
    plan = make(cs, "f64", pots=pots)
    assert np.isinf(plan.belief(3)).all()
    with pytest.raises(_capi.JtpError) as err:
        plan.joint([7, 3])
    m = re.search(r"(\d+) \(clique, k\) pairs.*first at clique (\d+)", str(err.value))
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) == plan.abi_of[1], str(err.value)      # clique 1 is the top
    assert err.value.joint.shape == (16, 16)
    with pytest.raises(_capi.JtpError):                      # one clique: its sums are not finite either
        plan.joint([0, 1])
    plan.close()


# ---------------------------------------------------------------------------------------------- 8. refusals

def test_refusals_say_why():
    spec = synthetic.wide_binary_tree(7, 8, 4)
    cs = spec_case(spec)
    tree, pots, node_vars, sizes, n = cs
    multi = engine.Plan(tree, node_vars, sizes, multiset=True, n_batch=8)
    for c in range(n):
        multi.set_potential(c, pots[c])
    multi.propagate()
    with pytest.raises(_capi.UnsupportedStructure, match="multi-set"):
        multi.joint([0, 1])
    multi.close()
    lean = engine.Plan(tree, node_vars, sizes, cover=[[] for _ in range(n)])
    assert lean.describe()["has_unit"] == 1
    lean.propagate()
    with pytest.raises(_capi.UnsupportedStructure, match="without `cover`"):
        lean.joint([0, 1])
    lean.close()
    plan = make(cs)
    labels = sorted(sizes)
    assert len(labels) >= 17
    with pytest.raises(_capi.UnsupportedStructure, match="at most 16"):
        plan.joint(labels[:17])
    assert plan.joint(labels[:16])[0].shape == (2,) * 16
    with pytest.raises(ValueError, match="twice"):
        plan.joint([labels[0], labels[1], labels[0]])
    with pytest.raises(ValueError, match="no clique"):
        plan.joint([labels[0], "nobody"])
    ids = (C.c_int32 * 2)(0, 0)
    out = np.zeros(4)
    lib, h = plan._lib, plan._handle
    assert lib.jtp_joint(h, 0, 2, C.cast(ids, C.c_void_p), out.ctypes.data_as(C.c_void_p), None) == _capi.JTP_EINVAL        # a duplicate
    ids[1] = len(plan.var_labels)
    assert lib.jtp_joint(h, 0, 2, C.cast(ids, C.c_void_p), out.ctypes.data_as(C.c_void_p), None) == _capi.JTP_EINVAL        # out of range
    assert lib.jtp_joint(h, 0, 0, C.cast(ids, C.c_void_p), out.ctypes.data_as(C.c_void_p), None) == _capi.JTP_EINVAL        # n_query < 1
    plan.close()
    fresh = engine.Plan(tree, node_vars, sizes)
    with pytest.raises(ValueError, match="not been propagated"):
        fresh.joint([0, 1])
    fresh.close()


def test_a_query_whose_messages_pass_the_cap_is_refused():
    """chain of 14 cliques of 16^3 entries: four variables of the last two cliques carried up eleven cliques, 256 x 16^4 doubles each"""
    spec = synthetic.chain_tree(14, card=16, width=3)
    cs = spec_case(spec)
    plan = make(cs, "f64")
    with pytest.raises(_capi.UnsupportedStructure) as err:
        plan.joint([0, 15, 14, 13, 12])
    m = re.search(r"64 MiB at clique (\d+).*has (\d+) entries", str(err.value))
    assert m and int(m.group(2)) == 256 * 16 ** 4, str(err.value)
    with pytest.raises(_capi.UnsupportedStructure, match="result beyond 64 MiB"):
        plan.joint([0, 3, 6, 9, 12, 15, 14])               # 16^7 entries
    got, _ = plan.joint([0, 15])                            # ... and the plan answers what fits
    assert got.shape == (16, 16) and got.min() > 0
    plan.close()


# ---------------------------------------------------------------------------------------------- 9. no side effects

@pytest.mark.parametrize("opts", [{}, dict(level_launches=True), dict(scaled=True)], ids=["flow", "level", "scaled"])
def test_joint_leaves_beliefs_and_messages_alone(opts):
    cs = case("wide7")
    plan = make(cs, "f64", evidence={sorted(cs[3])[2]: 1}, **opts)
    n_nodes = len(cs[2])
    before = [plan.belief(node) for node in range(n_nodes)]
    msgs = read_messages(plan)
    z = plan.log_z()
    first = [plan.joint(q)[0] for q in queries("wide7").values()]
    after = [plan.belief(node) for node in range(n_nodes)]
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(read_messages(plan), msgs)
    assert plan.log_z() == z
    plan.propagate()                                         # ... and the next propagate finds its messages as it left them
    for a, b in zip(before, [plan.belief(node) for node in range(n_nodes)]):
        np.testing.assert_array_equal(a, b)
    for a, q in zip(first, queries("wide7").values()):
        np.testing.assert_array_equal(plan.joint(q)[0], a)
    plan.close()


def read_messages(plan):
    """the whole message arena half of evidence set 0 (`jtp_debug_read_msg`)"""
    n = int(plan.describe()["msg_doubles"])
    out = np.zeros(n)
    _capi.check(plan._lib.jtp_debug_read_msg(plan._handle, 0, 0, n, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out
