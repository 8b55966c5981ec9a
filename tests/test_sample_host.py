"""Joint sampling (`jtp_sample`), the part that needs no GPU: the entry point, the sampling schedule the planner reports under
describe()["sample"] (a root-to-leaves sweep over the tree as the caller gave it), the refusals, and the uniform stream."""
import numpy as np
import pytest

from junctiontree_amd import _capi, engine, synthetic
from test_planner_emulated import star


def plan_only(spec_or_case, **opts):
    if isinstance(spec_or_case, dict):
        tree, node_vars, sizes = spec_or_case["tree"], spec_or_case["node_vars"], spec_or_case["sizes"]
    else:
        tree, node_vars, sizes = spec_or_case
    return engine.Plan(tree, node_vars, sizes, plan_only=True, **opts)


def star5():
    tree, _, node_vars, sizes = star(5, card=2, seed=5)
    return tree, node_vars, sizes


def renumbered():
    spec = synthetic.random_tree(n_cliques=9, width=6, sep=3, card=2, seed=4)
    return synthetic.renumber(spec, [4, 0, 7, 2, 8, 1, 3, 6, 5])        # the root is clique 4


TREES = {
    "wide7": lambda: synthetic.wide_binary_tree(7, 12, 6),
    "random16_card3": lambda: synthetic.random_tree(16, 6, 3, card=3),
    "chain6": lambda: synthetic.chain_tree(6, 16, 3),
    "star5": star5,
    "renumbered": renumbered,
}


def test_jtp_sample_is_exported_and_bound():
    assert "jtp_sample" in _capi.SYMBOLS
    fn = _capi.lib().jtp_sample
    assert fn.argtypes is not None and len(fn.argtypes) == 5
    assert _capi.lib().jtp_version().decode().split()[1] == "0.8.1"


def test_a_plan_only_plan_raises_and_does_not_crash():
    plan = plan_only(synthetic.wide_binary_tree(3, 6, 3))
    with pytest.raises(_capi.JtpError):
        plan.sample(4)
    with pytest.raises(ValueError):
        plan.sample(0)


def lists(plan):
    d = plan.describe()["sample"]
    return d["depths"], [(c["clique"], c["parent"], c["depth"], c["K"], c["F"], c["R"]) for c in d["cliques"]]


@pytest.mark.parametrize("name", sorted(TREES))
def test_the_sampling_schedule_is_a_sweep_over_the_callers_tree(name):
    case = TREES[name]()
    plan = plan_only(case)
    d = plan.describe()
    s = d["sample"]
    assert s["refused"] == ""
    n = plan.n_cliques
    node_vars = {plan.abi_of[c]: [plan.var_id[lab] for lab in plan.node_vars[c]] for c in plan.cliques}
    parent = {plan.abi_of[c]: (plan.abi_of[plan.parent[c]] if plan.parent[c] != -1 else -1) for c in plan.cliques}
    by_clique = {c["clique"]: c for c in s["cliques"]}
    assert sorted(by_clique) == list(range(n)) and len(s["cliques"]) == n          # every real clique once, no virtual one
    if name == "star5":
        assert any(p["real"] < 0 for p in d["pnodes"])                             # (the propagate's tree does have virtual cliques)
    if name == "renumbered":
        assert parent[0] != -1 and parent[plan.abi_of[4]] == -1
    free_in = {}
    for c, rec in by_clique.items():
        assert rec["parent"] == parent[c]
        pvars = set(node_vars[parent[c]]) if parent[c] >= 0 else set()
        assert set(rec["K"]) <= pvars                                               # K_c lies in the parent clique
        assert rec["K"] == [v for v in node_vars[c] if v in pvars]                  # ... and is ALL the clique shares with it
        assert rec["F"] == [v for v in node_vars[c] if v not in pvars]              # F_c in host axis order, K u F = vars(c)
        assert rec["R"] == int(np.prod([plan.card[v] for v in rec["F"]], dtype=np.int64))
        if parent[c] >= 0:
            assert rec["depth"] > by_clique[parent[c]]["depth"]
        else:
            assert rec["depth"] == 0 and rec["K"] == []
        for v in rec["F"]:
            assert v not in free_in, "variable %d is drawn by cliques %d and %d" % (v, free_in.get(v), c)
            free_in[v] = c
    assert sorted(free_in) == list(range(len(plan.card)))                           # every variable is drawn exactly once
    # the depth lists are the visit order: by depth, then by clique number
    assert [c for level in s["depths"] for c in level] == [c["clique"] for c in s["cliques"]]
    for depth, level in enumerate(s["depths"]):
        assert level == sorted(level) and all(by_clique[c]["depth"] == depth for c in level)
    # nothing in it depends on the root the planner picks or on the layout
    base = lists(plan)
    for opts in (dict(keep_root=True), dict(layout_policy=1), dict(layout_policy=2), dict(layout_policy=3), dict(no_compact=True),
                 dict(level_launches=True), dict(dtype="f32")):
        assert lists(plan_only(case, **opts)) == base, opts


def test_plans_that_cannot_be_sampled_say_so_in_their_description():
    spec = synthetic.wide_binary_tree(7, 8, 4)
    multi = plan_only(spec, multiset=True, n_batch=8)
    assert "multi-set" in multi.describe()["sample"]["refused"]
    ranks = plan_only(spec, n_ranks=2, rank=0, owner=[0, 0, 1, 0, 0, 1, 1])
    assert "ranks" in ranks.describe()["sample"]["refused"]
    lean = plan_only(spec, cover=[[] for _ in range(7)])
    d = lean.describe()
    assert d["has_unit"] == 1 and "without `cover`" in d["sample"]["refused"]
    for plan in (multi, ranks, lean):
        with pytest.raises(_capi.UnsupportedStructure):
            plan.sample(1)
    # ... and the schedule itself is still described
    assert len(lean.describe()["sample"]["cliques"]) == 7


def test_sample_uniform_is_a_counter_based_stream_of_its_own():
    for seed, clique in ((0, 0), (7, 3), (2**63 + 5, 250)):
        u = synthetic.sample_uniform(seed, clique, 1000)
        assert u.dtype == np.float64 and u.shape == (1000,) and np.all(u >= 0.0) and np.all(u < 1.0)
        np.testing.assert_array_equal(synthetic.sample_uniform(seed, clique, 2000)[:1000], u)        # prefix stable
        other = synthetic.synth_values(seed, clique, (1000,)) - 0.5                                   # the fill's u of the same seed and node
        assert not np.any(u == other)
        assert 0.45 < u.mean() < 0.55
    assert not np.array_equal(synthetic.sample_uniform(1, 0, 16), synthetic.sample_uniform(1, 1, 16))
    assert not np.array_equal(synthetic.sample_uniform(1, 0, 16), synthetic.sample_uniform(2, 0, 16))


def digit_of(pd, i, x, low_bits, row_elems):
    """`jt_digit` of the pack / unpack kernels: the digit of variable i at stored element x of a clique table"""
    ds, dmod = pd["dstride"][i], pd["dmod"][i]
    if row_elems > 0 and i == pd["split_var"]:
        return ((x % row_elems) // ds) % dmod + (((x // pd["split_ds2"]) % pd["split_mod2"]) << pd["split_lb"])
    if row_elems > 0 and pd["pos"][i] < low_bits:
        return ((x % row_elems) // ds) % dmod if ds else 0
    return (x // ds) % dmod if ds else 0


@pytest.mark.parametrize("opts", [dict(dtype="f64"), dict(dtype="f32"), dict(dtype="f64", no_compact=True), dict(dtype="f32", layout_policy=1)],
                         ids=["f64", "f32", "f64-no_compact", "f32-policy1"])
@pytest.mark.parametrize("card", [2, 3, 5, 6, 7])
def test_a_digits_place_in_a_stored_table_is_linear_in_the_digit(card, opts):
    """What `jt_sample_level` addresses the belief tables by: the offset of an entry is the sum over its variables of
    (digit mod 2^lb) * stride + (digit >> lb) * stride2 (lb = 31, stride2 = 0 but for the variable across the thread part's top bit
    of a compact row) - the `back` sum of `jt_dev_to_host`.  Checked against the digit extraction the unpack kernel uses, for every
    entry of every clique: the offsets are distinct, inside the stored table, and give back the digits."""
    spec = synthetic.random_tree(16, 6, 3, card=card) if card > 2 else synthetic.wide_binary_tree(7, 12, 6)
    plan = plan_only(spec, **opts)
    d = plan.describe()
    low_bits = d["TB"]
    for c, pd in enumerate(d["pack"]):
        p = d["pnodes"][c]
        row_elems = p["trow"] if p["tmix"] else 0
        cards = pd["card"]
        grids = np.indices(cards).reshape(len(cards), -1)
        off = np.zeros(grids.shape[1], dtype=np.int64)
        for i in range(len(cards)):
            lb, s2 = (pd["split_lb"], pd["split_ds2"]) if (row_elems > 0 and i == pd["split_var"]) else (31, 0)
            off += (grids[i] & ((1 << lb) - 1)) * pd["dstride"][i] + (grids[i] >> lb) * s2
        assert off.min() >= 0 and off.max() < pd["phys_elems"] and len(np.unique(off)) == len(off)
        for i in range(len(cards)):
            back = np.array([digit_of(pd, i, int(x), low_bits, row_elems) for x in off[:: max(1, len(off) // 997)]])
            np.testing.assert_array_equal(back, grids[i][:: max(1, len(off) // 997)])
