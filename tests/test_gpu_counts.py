"""Expected counts accumulated on the device (`jtp_accumulate_marginals`: kernels `jt_marg_sums`, `jt_marg_accumulate`) on a real MI355X,
against `tests/counts_reference.py` (the oracle on indicator-multiplied potentials, pinned by `tests/test_counts_host.py`).

Tolerances are those of `tests/test_gpu_parity.py`: elementwise 1e-11 for float64 tables, 1e-6 for float32 ones; a sum of at most 64
non-negative terms adds 64 ulp to either, far inside both."""
import ctypes as C
import functools
import gc
import math

import numpy as np
import pytest

import junctiontree_amd as jt
from counts_reference import expected_counts_reference
from junctiontree_amd import _capi, engine, synthetic
from junctiontree_amd.junctiontree import _normalised

pytestmark = pytest.mark.gpu

RTOL64, RTOL32 = 1e-11, 1e-6
LN2 = math.log(2.0)


def close(got, want, rtol=RTOL64, what=""):
    """(`tests/test_gpu_parity.py`) non-negative tables: elementwise relative error above 1e-30 * max, absolute below."""
    got = np.asarray(got, dtype=np.float64)
    want = np.broadcast_to(np.asarray(want, dtype=np.float64), got.shape)
    scale = np.max(np.abs(want)) if want.size else 0.0
    assert want.size == 0 or np.all(want >= 0)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-30 * scale + 1e-300, err_msg=what)


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    gc.collect()
    yield
    engine.clear_plan_cache()


def live_bytes():
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().jtp_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


# name: (tree, storage type, plan options, evidence sets)
CASES = {
    "multiset": (lambda: synthetic.wide_binary_tree(n_cliques=15, width=13, sep=6, card=2, seed=2), "f64", {"multiset": True}, 11),
    "multiset level launches": (lambda: synthetic.random_tree(n_cliques=9, width=6, sep=3, card=3, seed=4), "f64",
                                {"multiset": True, "level_launches": True}, 11),
    "multiset f32": (lambda: synthetic.wide_binary_tree(n_cliques=7, width=14, sep=7, card=2, seed=6), "f32", {"multiset": True, "block_log2": 11}, 11),
    "share_potentials": (lambda: synthetic.wide_binary_tree(n_cliques=15, width=13, sep=6, card=2, seed=2), "f64", {"share_potentials": True}, 5),
    "n_batch": (lambda: synthetic.wide_binary_tree(n_cliques=15, width=13, sep=6, card=2, seed=2), "f64", {}, 5),
    # (all variables of a clique of 15: 2^15 entries - past one sweep of a 64 x 256 grid)
    "multiset width 15": (lambda: synthetic.wide_binary_tree(n_cliques=3, width=15, sep=6, card=2, seed=8), "f64", {"multiset": True}, 11),
}


def _requests(spec):
    """Per clique one single variable and one pair in reversed axis order; the empty list (a scalar) on clique 0; ALL variables of
    clique 1."""
    rng = np.random.default_rng(9)
    out = []
    for c in range(spec["n_cliques"]):
        labels = list(spec["node_vars"][c])
        out.append((c, [labels[int(rng.integers(0, len(labels)))]]))
        out.append((c, labels[1:3][::-1]))
    out.append((0, []))
    out.append((1, list(spec["node_vars"][1])))
    return out


def _evidence_sets(spec, nb):
    """(`test_multiset_plans_many_evidence_sets`) b % 5 observed variables: some sets observe nothing"""
    labels = sorted(spec["sizes"])
    observed = []
    for b in range(nb):
        rng = np.random.default_rng(500 + b)
        k = min(len(labels), b % 5)
        observed.append({labels[i]: int(rng.integers(0, spec["sizes"][labels[i]])) for i in rng.choice(len(labels), size=k, replace=False)})
    return observed


@functools.lru_cache(maxsize=None)
def _case(name):
    """The model of a case and its expected counts, computed once."""
    make, dtype, opts, nb = CASES[name]
    spec = make()
    np_dt = np.float32 if dtype == "f32" else np.float64
    rng0 = np.random.default_rng(len(name))
    base = [(rng0.uniform(0.5, 1.5, [spec["sizes"][v] for v in spec["node_vars"][c]]) * spec["scales"][c]).astype(np_dt)
            for c in range(spec["n_cliques"])]
    requests, sets = _requests(spec), _evidence_sets(spec, nb)
    weights = np.random.default_rng(3).uniform(0.5, 2.0, nb)
    want, want_log_z = expected_counts_reference(spec, base, requests, sets, weights)
    for w in want:
        w.setflags(write=False)
    return dict(spec=spec, dtype=dtype, opts=opts, nb=nb, base=base, requests=requests, sets=sets, weights=weights, want=want, log_z=want_log_z)


def _plan(case, propagates=2, nb=None):
    spec, nb = case["spec"], nb or case["nb"]
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=case["dtype"], n_batch=nb, **case["opts"])
    shared = case["opts"].get("multiset") or case["opts"].get("share_potentials")
    for b in range(1 if shared else nb):
        for c in range(spec["n_cliques"]):
            plan.set_potential(c, case["base"][c], batch=b)
    for b in range(nb):
        plan.set_evidence(case["sets"][b], batch=b)
    for _ in range(propagates):                         # (two: the other half of the message arenas is in use)
        plan.propagate()
    return plan


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_match_the_reference_on_every_kind_of_plan(name):
    case = _case(name)
    rtol = RTOL32 if case["dtype"] == "f32" else RTOL64
    plan = _plan(case)
    assert bool(plan.describe().get("multiset")) == bool(case["opts"].get("multiset"))
    got, log_z, sign = plan.accumulate_marginals(case["requests"], weights=case["weights"])
    assert len(got) == len(case["requests"])
    for (c, labels), g, w in zip(case["requests"], got, case["want"]):
        assert g.shape == w.shape and g.dtype == np.float64
        close(g, w, rtol, "%s: clique %d labels %r" % (name, c, labels))
    for b in range(case["nb"]):
        s, lz = plan.log_z(batch=b)
        assert sign[b] == s == 1
        assert abs(log_z[b] - lz) <= rtol * max(1.0, abs(lz)), (b, log_z[b], lz)
        assert abs(log_z[b] - case["log_z"][b]) <= rtol * max(1.0, abs(case["log_z"][b])), (b, log_z[b], case["log_z"][b])
    plan.close()


def test_the_chunk_size_does_not_change_a_bit():
    case = _case("multiset")
    plan = _plan(case)
    results = []
    for chunk in (1, 3, 0, 0):                          # (0: by size - all eleven sets at once; the second time from the cached list)
        plan.debug_set("acc_chunk", chunk)
        results.append(plan.accumulate_marginals(case["requests"], weights=case["weights"]))
    for got, log_z, sign in results[1:]:
        for g, w in zip(got, results[0][0]):
            assert np.array_equal(g, w)
        assert np.array_equal(log_z, results[0][1]) and np.array_equal(sign, results[0][2])
    for g, w in zip(results[0][0], case["want"]):
        close(g, w)
    # a sub-range with its own weights: the sets before and after it stay out
    got, log_z, _ = plan.accumulate_marginals(case["requests"], weights=case["weights"][2:7], batch_begin=2, batch_end=7)
    want, _ = expected_counts_reference(case["spec"], case["base"], case["requests"], case["sets"][2:7], case["weights"][2:7])
    for g, w in zip(got, want):
        close(g, w)
    assert np.array_equal(log_z, results[0][1][2:7])
    plan.close()


def test_counts_agree_with_the_marginals_read_out_set_by_set():
    case = _case("multiset level launches")
    nb = 5
    plan = _plan(case, nb=nb)
    before = [plan.marginals(case["requests"], batch=b) for b in range(nb)]
    want = [sum(_normalised(before[b])[i] for b in range(nb)) for i in range(len(case["requests"]))]
    got, _, _ = plan.accumulate_marginals(case["requests"])
    for g, w in zip(got, want):
        # (two device paths to one quantity, the partial copies added in different orders: `test_gpu_parity.py`'s bound for that)
        assert g.shape == w.shape and np.allclose(g, w, rtol=1e-13, atol=0.0)
    # the task records and the arenas are as they were: the read-out of every set returns what it returned
    for b in reversed(range(nb)):
        for g, w in zip(plan.marginals(case["requests"], batch=b), before[b]):
            assert np.array_equal(g, w)
    plan.close()


def _lattice(h=3, w=4, card=3):
    factors, sizes, values = synthetic.lattice_mrf(h, w, card, dtype=np.float64)
    tree = jt.create_junction_tree(factors, sizes)
    ct = tree.clique_tree
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]
    spec = {"tree": tree.tree, "node_vars": node_vars, "sizes": sizes, "n_cliques": len(ct.maxcliques)}
    return tree, factors, sizes, values, spec


def test_cliques_that_keep_no_table(monkeypatch):
    """plans made with `cover`: set 0 observes nothing (the lean pass), the others one or two variables (jt_single)"""
    monkeypatch.setenv("JTP_UNIT_RATIO", "1")
    tree, factors, sizes, values, spec = _lattice()
    ct = tree.clique_tree
    names = sorted(sizes)
    sets = [{}, {names[0]: 1}, {names[3]: 2, names[7]: 0}, {names[5]: 1}, {names[2]: 0, names[11]: 2}]
    weights = np.random.default_rng(4).uniform(0.5, 2.0, len(sets))
    plan = engine.Plan(tree.tree, spec["node_vars"], sizes, dtype="f64", share_potentials=True, n_batch=len(sets), cover=tree.cover())
    assert plan.stats()["n_unit_cliques"] > 0
    plan.stage_factors(factors, ct.factor_to_maxclique, values)
    for b, obs in enumerate(sets):
        plan.set_evidence(obs, batch=b)
    plan.propagate()
    requests = [(mc, list(f)) for f, mc in zip(factors, ct.factor_to_maxclique)]
    want, want_log_z = expected_counts_reference(spec, ct.evaluate(values), requests, sets, weights)
    got, log_z, _ = plan.accumulate_marginals(requests, weights=weights)
    for i, (g, w) in enumerate(zip(got, want)):
        close(g, w, what="factor %d" % i)
    np.testing.assert_allclose(log_z, want_log_z, rtol=0.0, atol=1e-11 * np.max(np.abs(want_log_z)))
    again, _, _ = plan.factor_counts(factors, ct.factor_to_maxclique, weights=weights)
    for g, w in zip(again, got):
        assert np.array_equal(g, w)
    plan.close()


def _chain(n_vars=8, card=3, seed=0):
    """pairwise factors along a chain and one unary factor: every clique holds at most two factors"""
    rng = np.random.default_rng(seed)
    names = ["v%d" % i for i in range(n_vars)]
    factors = [[names[0]]] + [[names[i], names[i + 1]] for i in range(n_vars - 1)]
    sizes = {v: card for v in names}
    values = [rng.uniform(0.5, 1.5, [card] * len(f)) for f in factors]
    return names, factors, sizes, values


def test_scaled_plans_through_the_public_api():
    names, factors, sizes, values = _chain()
    sets = [{}, {names[1]: 2}, {names[0]: 0, names[6]: 1}, {names[4]: 1}]
    weights = [1.0, 0.5, 2.0, 1.5]
    tree = jt.create_junction_tree(factors, sizes)
    want = tree.expected_counts(values, sets, weights=weights)
    want_log_z = np.array(tree.log_z_sets)
    for f, (w, v) in enumerate(zip(want, values)):
        assert w.shape == v.shape and w.dtype == np.float64
        np.testing.assert_allclose(w.sum(), sum(weights), rtol=1e-12)
    for shift in (200, -200):
        moved = [v * 2.0 ** shift for v in values]
        got = tree.expected_counts(moved, sets, weights=weights, normalize=True)
        for f, (g, w) in enumerate(zip(got, want)):
            close(g, w, what="shift %d factor %d" % (shift, f))
        assert np.all(np.abs(np.array(tree.log_z_sets) - (want_log_z + len(factors) * shift * LN2)) <= 1e-9)
    # without the overflow-safe plan Z = 2^1600 x ... is inf: every pair is without mass
    with pytest.raises(_capi.JtpError, match="without mass") as exc:
        tree.expected_counts([v * 2.0 ** 200 for v in values], sets, weights=weights)
    assert len(exc.value.counts) == len(factors)


def test_evidence_of_probability_zero():
    names, factors, sizes, values = _chain(seed=1)
    values[2] = values[2].copy()
    values[2][0, 1] = 0.0                               # factor (v1, v2): v1 = 0 and v2 = 1 never occur together
    sets = [{names[0]: 1}, {}, {names[1]: 0, names[2]: 1}, {names[5]: 2}]
    tree = jt.create_junction_tree(factors, sizes)
    others = tree.expected_counts(values, sets, weights=[1, 1, 0, 1])       # (weight 0: nothing is raised)
    assert tree.log_z_sets[2] == -np.inf and np.isfinite(np.delete(tree.log_z_sets, 2)).all()
    with pytest.raises(_capi.JtpError, match=r"the first: evidence set 2, request 0\b") as exc:
        tree.expected_counts(values, sets, weights=[1, 1, 1, 1])
    assert "%d (evidence set, request) pairs" % len(factors) in str(exc.value)
    for g, w in zip(exc.value.counts, others):
        assert np.array_equal(g, w)
    assert exc.value.log_z[2] == -np.inf and tree.log_z_sets[2] == -np.inf
    assert np.array_equal(np.delete(exc.value.log_z, 2), np.delete(np.array(tree.log_z_sets), 2))


def test_one_em_loop_through_the_public_api():
    """A naive-Bayes network with a hidden class: the E-step is `expected_counts`, the M-step normalises the counts over the child axis
    (every factor is a CPT whose last axis is the child).  EM never lowers the data log-likelihood, and every case is counted once."""
    rng = np.random.default_rng(11)
    children = ["x0", "x1", "x2", "x3"]
    factors = [["h"]] + [["h", x] for x in children]
    sizes = dict({"h": 2}, **{x: 3 for x in children})

    def cpts(r):
        out = [r.uniform(0.2, 1.0, [sizes[v] for v in f]) for f in factors]
        return [t / t.sum(axis=-1, keepdims=True) for t in out]

    truth = cpts(rng)
    cases = []
    for _ in range(40):
        h = int(rng.choice(2, p=truth[0]))
        cases.append({x: int(rng.choice(3, p=truth[1 + i][h])) for i, x in enumerate(children)})
    tree = jt.create_junction_tree(factors, sizes)
    values = cpts(np.random.default_rng(12))
    log_lik = []
    for _ in range(3):
        counts = tree.expected_counts(values, cases + [{}], weights=[1] * 40 + [0])
        lz = np.array(tree.log_z_sets)
        log_lik.append(float(np.sum(lz[:40] - lz[40])))
        for c, v in zip(counts, values):
            assert c.shape == v.shape and abs(c.sum() - 40.0) <= 1e-9
        values = [c / c.sum(axis=-1, keepdims=True) for c in counts]
    assert all(b >= a - 1e-9 for a, b in zip(log_lik, log_lik[1:])), log_lik
    assert log_lik[-1] > log_lik[0]                    # (the start is random: the first steps do move)


def test_the_first_call_survives_the_failure_of_each_of_its_allocations():
    case = _case("multiset level launches")
    fresh = _plan(case)
    want = fresh.accumulate_marginals(case["requests"], weights=case["weights"])
    fresh.close()
    plan = _plan(case)
    failed = 0
    for n in range(1, 32):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            got = plan.accumulate_marginals(case["requests"], weights=case["weights"])
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    plan.debug_set("fail_alloc", 0)
    # (the list's six tables; the slots' scratch, entries and S, the weights and the buffer that goes back - and the slots' records where the
    #  plan has an evidence-free group)
    assert failed == n - 1 and failed >= 11, (failed, n)
    for g, w in zip(got[0], want[0]):
        assert np.array_equal(g, w)
    assert np.array_equal(got[1], want[1])
    for g, w in zip(plan.accumulate_marginals(case["requests"], weights=case["weights"])[0], case["want"]):
        close(g, w)
    plan.close()
