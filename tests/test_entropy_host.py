"""The restatement of `jtp_entropy` (`tests/entropy_reference.py`) against enumeration and against the identities an entropy obeys,
without a GPU: the beliefs it is given here are the marginals of the enumerated joint.  Plans are made `plan_only`, for their schedule."""
import math

import numpy as np
import pytest

import junctiontree_amd as jt
from entropy_reference import EPS, brute_force_entropy, chain, entropy_reference, parity_bound
from junctiontree_amd import _capi, engine, synthetic
from sample_reference import schedule
from test_gpu_sample import CASES, README_FACTORS, README_SIZES, README_VALUES, case_of, contained_case, spec_case

TOL = 1e-13           # enumeration and the restatement both add a handful of terms in long double


def enumerated_beliefs(node_vars, n, factors, sizes, values, evidence):
    """the clique beliefs a propagate would leave, up to rounding: the joint, times the evidence, summed onto each clique"""
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
    full = "".join(letters[v] for v in labels)
    return [np.einsum(full + "->" + "".join(letters[v] for v in node_vars[c]), joint) for c in range(n)], joint


def readme_model():
    tree = jt.create_junction_tree(README_FACTORS, README_SIZES)
    node_vars = [list(c) for c in tree.clique_tree.maxcliques] + [list(s) for s in tree.separators]
    return tree.tree, node_vars, len(tree.clique_tree.maxcliques), README_FACTORS, README_SIZES, README_VALUES


def chain5_model():
    tree, pots, node_vars, sizes, n = spec_case(synthetic.chain_tree(3, card=2, width=3), seed=7)
    return tree, node_vars, n, [list(vs) for vs in node_vars[:n]], sizes, pots[:n]


MODELS = {"readme": (readme_model, [None, {"wet_grass": 1}, {"cloudy": 0, "sprinkler": 1}]), "chain5": (chain5_model, [None, {2: 1}, {0: 1, 4: 0}])}
MODEL_RUNS = [(name, ev) for name, (_, evs) in MODELS.items() for ev in evs]


@pytest.mark.parametrize("name,evidence", MODEL_RUNS, ids=["%s-%s" % (n, "free" if not e else "_".join(map(str, e))) for n, e in MODEL_RUNS])
def test_the_restatement_equals_enumeration_and_the_free_energy_identity(name, evidence):
    tree, node_vars, n, factors, sizes, values = MODELS[name][0]()
    sched = schedule(engine.Plan(tree, node_vars, sizes, plan_only=True))
    beliefs, joint = enumerated_beliefs(node_vars, n, factors, sizes, values, evidence)
    H, X, per = entropy_reference(beliefs, sched, node_vars)
    want, log_z, _ = brute_force_entropy(factors, sizes, values, evidence)
    assert X is None and sorted(per) == list(range(n))
    assert abs(H - want) <= TOL * max(1.0, want)
    assert all(h >= -TOL for h in per.values())
    # H = ln Z - sum over the factors of E[ln psi]
    p = joint / joint.sum()
    labels = sorted(sizes, key=str)
    e_log = 0.0
    for f, v in zip(factors, values):
        v = np.asarray(v, dtype=np.float64)
        shape = [sizes[lab] if lab in f else 1 for lab in labels]
        lifted = np.transpose(v, np.argsort([labels.index(lab) for lab in f]).tolist()).reshape(shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(p > 0, p * np.log(np.broadcast_to(lifted, p.shape)), 0.0)
        e_log += term.sum()
    assert abs(H - (log_z - e_log)) <= 1e-12 * max(1.0, abs(log_z), abs(e_log))
    # the posterior against the prior: KL(P(.|e) || P(.)) = ln Z(no evidence) - ln Z(e); against itself: 0
    prior, _ = enumerated_beliefs(node_vars, n, factors, sizes, values, None)
    H2, X, _ = entropy_reference(beliefs, sched, node_vars, ref_beliefs=prior)
    _, log_z0, _ = brute_force_entropy(factors, sizes, values, None)
    assert H2 == H and abs((X - H) - (log_z0 - log_z)) <= 1e-12
    assert abs(entropy_reference(beliefs, sched, node_vars, ref_beliefs=beliefs)[1] - H) <= TOL
    if evidence:          # ... and the prior lacks nothing the posterior has, but not the other way round
        assert entropy_reference(prior, sched, node_vars, ref_beliefs=beliefs)[1] == float("inf")


def test_evidence_on_every_variable_leaves_no_entropy():
    tree, node_vars, n, factors, sizes, values = chain5_model()
    sched = schedule(engine.Plan(tree, node_vars, sizes, plan_only=True))
    beliefs, _ = enumerated_beliefs(node_vars, n, factors, sizes, values, {v: 1 for v in sizes})
    H, _, per = entropy_reference(beliefs, sched, node_vars)
    assert H == 0.0 and all(h == 0.0 for h in per.values())


def test_kl_between_two_models_equals_enumeration():
    tree, node_vars, n, factors, sizes, values = chain5_model()
    rng = np.random.default_rng(3)
    other = [rng.uniform(0.5, 1.5, np.shape(v)) for v in values]
    sched = schedule(engine.Plan(tree, node_vars, sizes, plan_only=True))
    for ev in (None, {1: 0}):
        p, _ = enumerated_beliefs(node_vars, n, factors, sizes, values, ev)
        q, _ = enumerated_beliefs(node_vars, n, factors, sizes, other, ev)
        H, X, _ = entropy_reference(p, sched, node_vars, ref_beliefs=q)
        want = brute_force_entropy(factors, sizes, values, ev, values_q=other)[2]
        assert want > 0.0 and abs((X - H) - want) <= 1e-12
        H, X, _ = entropy_reference(q, sched, node_vars, ref_beliefs=p)
        assert abs((X - H) - brute_force_entropy(factors, sizes, other, ev, values_q=values)[2]) <= 1e-12


def test_the_entropy_does_not_depend_on_the_root_and_the_single_terms_do():
    tree, pots, node_vars, sizes, n = contained_case()
    factors = [list(vs) for vs in node_vars[:n]]
    beliefs, _ = enumerated_beliefs(node_vars, n, factors, sizes, pots[:n], {4: 2})
    want = brute_force_entropy(factors, sizes, pots[:n], {4: 2})[0]
    seen = {}
    for root in range(n):
        plan = engine.Plan(tree, node_vars, sizes, plan_only=True, root=root)
        sched = schedule(plan)
        assert sched[0][0] == root and sched[0][3] == []
        H, _, per = entropy_reference(beliefs, sched, node_vars)
        assert abs(H - want) <= TOL, root
        seen[root] = tuple(round(per[c], 9) for c in range(n))
    assert seen[0] != seen[2]             # (clique 2 gives H(4 | 2, 3) below clique 0 and H(2, 3, 4) on top)


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_in_another_order_stays_inside_the_bound(name):
    """what the bound is for, on the shapes of the GPU cases: the same definition in float64 - numpy's pairwise order, another
    order than the device's - lies within `parity_bound` of long double, on tables of entries e^N(0, 10) with half the entries zero,
    as float64 and as float32 widened; so does a cross-entropy"""
    tree, _, node_vars, sizes, n = case_of(name)
    sched = schedule(engine.Plan(tree, node_vars, sizes, plan_only=True))
    rng = np.random.default_rng(17)
    for np_t in (np.float64, np.float32):
        a, b = ([(np.exp(rng.normal(0.0, 10.0, [sizes[v] for v in node_vars[c]])) * (rng.random([sizes[v] for v in node_vars[c]]) < 0.5)).astype(np_t).astype(np.float64)
                 for c in range(n)] for _ in range(2))
        b = [np.where(x > 0, y + 1e-3, y) for x, y in zip(a, b)]          # (the reference has support wherever the set has)
        bound = parity_bound(a, sched, node_vars, ref_beliefs=b)
        H, X, per = entropy_reference(a, sched, node_vars, ref_beliefs=b)
        H64, X64, per64 = entropy_reference(a, sched, node_vars, ref_beliefs=b, dtype=np.float64)
        worst = max(abs(per64[c] - per[c]) / bound[c] for c in range(n))
        print("%s %s: worst |h_c - reference| / bound %.3g, H %.6g, X %.6g" % (name, np_t.__name__, worst, H, X))
        assert worst <= 1.0 and np.isfinite(X)
        total = sum(bound.values())
        assert abs(H64 - H) <= total + n * EPS * abs(H) and abs(X64 - X) <= total + n * EPS * abs(X)


def test_the_chain_counts_what_the_kernels_add():
    assert chain(1, 1) == 1 + 0 + 1 + 6 + 3                       # one entry, one k
    assert chain(64, 4096) == 1 + 6 + 16 + 6 + 3                  # a wave per k, sixteen k a thread
    assert chain(2047, 1) == 32 + 6 + 1 + 6 + 3                   # the longest row that is not cut
    assert chain(1 << 16, 3) == 16 + 6 + (1 + 6 + 1) + 3          # 64 segments of 1024: one segment sum a lane, a k a wave
    assert chain(1 << 23, 1) == 32 + 6 + (64 + 6 + 1) + 3         # 4096 segments of 2048


def test_the_binding_lists_the_symbol():
    assert "jtp_entropy" in _capi.SYMBOLS
    assert math.isclose(EPS, np.finfo(np.float64).eps / 2)
