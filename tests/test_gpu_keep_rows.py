"""Table rows kept in the Infinity Cache (`JtTask::keep_rows`) on a real MI355X: the cache policy of a load changes no result.  At the
smallest shapes whose workgroups have more than four rows - the refills inside the row loop carry the policy, not only the four
first loads - every budget (nothing kept, the default, everything, part of the tree) in every launch mode (dataflow, ticket
order, one launch per level - whose kernels do not look at the flag, so nothing is kept there) agrees with the oracle at the suite's
tolerances and with every other variant bit for bit; twenty propagates queued back to back give the same bits; a two-rank plan over
the mock transport gives the same beliefs with and without kept rows.  tests/test_keep_rows_emulated.py checks WHAT is kept."""
import functools

import numpy as np
import pytest

import jt_oracle as oracle
from junctiontree_amd import engine, synthetic
from test_gpu_parity import RTOL32, RTOL64, close, expected_mode

pytestmark = pytest.mark.gpu

# environment of a variant (the planner reads its knobs at every plan creation)
VARIANTS = {
    "nothing": {"JTP_KEEP_ROWS_MB": "0"},
    "default": {},
    "everything": {"JTP_KEEP_ROWS_MB": "4096"},
    "part": {"JTP_KEEP_ROWS_MB": "PART", "JTP_KEEP_BW": "1"},        # (every level counts as bandwidth-bound; the budget: 0.45 of the tables - levels 0 and 1)
}
# (trees this small are latency-bound plans: the planner's search gives them workgroups of two and four rows - the greedy split of
#  layout policy 3 at 2^14 elements per workgroup gives 16 rows in float32 and 32 in float64, so the row loop refills its ring)
BASE = {"layout_policy": 3, "block_log2": 14}
MODES = [dict(BASE), dict(BASE, flow_tickets=True), dict(BASE, level_launches=True)]
KNOBS = ("JTP_KEEP_ROWS_MB", "JTP_KEEP_BW", "JTP_KEEP_TOP")

CASES = {
    "wide15 f32": (lambda: synthetic.wide_binary_tree(n_cliques=15, width=16, sep=8, card=2, seed=1), "f32"),
    "wide15 f64": (lambda: synthetic.wide_binary_tree(n_cliques=15, width=15, sep=8, card=2, seed=2), "f64"),
    "card7 f32": (lambda: synthetic.wide_binary_tree(n_cliques=7, width=5, sep=3, card=7, seed=7), "f32"),
}


@pytest.fixture(autouse=True)
def _no_cached_plans(monkeypatch):
    # (trees of tiny levels are planned as chains, whose kernels have no choice of policy and keep nothing: plan these as the large
    #  trees they stand for - one launch of jt_propagate_flow, the kernel that looks at the flag)
    monkeypatch.setenv("JTP_TINY_LEVEL_ELEMS", "0")
    engine.clear_plan_cache()
    yield
    engine.clear_plan_cache()


@functools.lru_cache(maxsize=None)
def inputs(name):
    make, dtype = CASES[name]
    spec = make()
    pots = synthetic.potentials_for(spec, seed=31)
    if dtype == "f32":
        pots = [p.astype(np.float32) for p in pots]
    want, z = oracle.beliefs_exact(spec["tree"], pots, spec["node_vars"], return_z=True)
    for w in want:
        w.setflags(write=False)
    return spec, pots, want, z


def set_variant(monkeypatch, variant, table_bytes):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, repr(0.45 * table_bytes / 1048576.0) if v == "PART" else v)


@pytest.mark.parametrize("name", list(CASES))
def test_every_budget_in_every_launch_mode_gives_the_same_bits(monkeypatch, name):
    spec, pots, want, z = inputs(name)
    dtype = CASES[name][1]
    rtol = RTOL32 if dtype == "f32" else RTOL64
    first = None
    probe = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, plan_only=True, **BASE)
    table_bytes = sum(p["phys_elems"] for p in probe.describe()["pnodes"] if not p["unit"]) * (4 if dtype == "f32" else 8)
    probe.close()
    for variant in VARIANTS:
        set_variant(monkeypatch, variant, table_bytes)
        for opts in MODES:
            plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, **opts)
            d = plan.describe()
            tables = [t for t in d["tasks"] if t["kind"] == 0 and not t["unit"]]
            kept = [t for t in tables if t["keep_rows"]]
            assert d["tmix"] == 0 and not d["multiset"]
            assert [s["phase"] for s in d["segments"]] == [2]      # both phases in one launch: jt_propagate_flow
            # the row loop refills: workgroups of more than four rows, kept ones among them
            assert max(t["total"] for t in tables) > 4
            if variant == "nothing" or opts.get("level_launches"):        # (the per-level kernels do not look at the flag: nothing is kept)
                assert not kept and d["keep"]["distribute_bytes"] == 0 and not any(b[-1] & 2 for b in d["blocks"])
            elif variant == "part":
                assert 0 < len(kept) < len(tables) and d["keep"]["distribute_bytes"] <= d["keep"]["budget_bytes"]
                assert max(t["total"] for t in kept) > 4
            else:
                assert len(kept) == len(tables) and d["keep"]["distribute_bytes"] == table_bytes       # (the default budget holds these trees)
                assert max(t["total"] for t in kept) > 4
            if name.startswith("card7"):                  # rows that do not exist (a digit of 7): the refill can be the zero row
                assert any(row[0] in (-1, 0xFFFFFFFF) for t in tables for row in t["itab"][4:])
            for c in range(spec["n_cliques"]):
                plan.set_potential(c, pots[c])
            plan.propagate()
            st = plan.stats()
            assert st["launch_mode"] == expected_mode(opts) and st["flow_fallbacks"] == 0
            got = [plan.belief(n) for n in range(len(spec["node_vars"]))]
            gz = plan.z()
            plan.close()
            for n, (g, w) in enumerate(zip(got, want)):
                close(g, w, rtol=rtol, what="%s %s %r node %d" % (name, variant, opts, n))
            assert abs(gz - z) <= rtol * abs(z)
            if first is None:
                first = (got, gz)
            else:
                assert gz == first[1]
                for g, f in zip(got, first[0]):
                    np.testing.assert_array_equal(g, f)


@pytest.mark.parametrize("name", list(CASES))
def test_twenty_queued_propagates_give_the_same_bits(monkeypatch, name):
    spec, pots, want, z = inputs(name)
    dtype = CASES[name][1]
    results = []
    for variant in ("nothing", "default", "everything"):
        set_variant(monkeypatch, variant, 0)
        plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, **BASE)
        d = plan.describe()
        assert max(t["total"] for t in d["tasks"] if t["kind"] == 0) > 4
        assert (d["keep"]["distribute_bytes"] > 0) == (variant != "nothing")
        for c in range(spec["n_cliques"]):
            plan.set_potential(c, pots[c])
        plan.propagate()
        once = [plan.belief(n) for n in range(len(spec["node_vars"]))]
        for _ in range(20):
            plan.propagate(sync=False)
        plan.sync()
        assert plan.stats()["flow_fallbacks"] == 0
        again = [plan.belief(n) for n in range(len(spec["node_vars"]))]
        results.append((once, plan.z()))
        plan.close()
        for a, b in zip(once, again):
            np.testing.assert_array_equal(a, b)
        for n, (g, w) in enumerate(zip(once, want)):
            close(g, w, rtol=RTOL32 if dtype == "f32" else RTOL64, what="%s %s node %d" % (name, variant, n))
    for other in results[1:]:
        assert results[0][1] == other[1]
        for a, b in zip(results[0][0], other[0]):
            np.testing.assert_array_equal(a, b)


def test_two_ranks_over_the_mock_transport_with_and_without_kept_rows(monkeypatch, tmp_path):
    """the first shape of tests/test_gpu_multirank_mock.py: a rank's collect launch (`jt_collect_flow_keep`) leaves in the cache what
    its distribute launch reads - same beliefs as with nothing kept, bit for bit, and the oracle's"""
    import multiprocessing as mp
    import test_gpu_multirank_mock as mock

    world, recipe = 2, "wide_binary_tree"
    kwargs = {"n_cliques": 15, "width": 13, "sep": 6, "card": 2, "seed": 1}
    runs = {}
    from junctiontree_amd import partition
    spec = mock._spec(synthetic, recipe, kwargs)
    weights = [float(np.prod([spec["sizes"][v] for v in spec["node_vars"][c]])) for c in range(spec["n_cliques"])]
    owner = partition.subtree_owners(spec["parent"], weights, world, replicate_top=False)
    for variant in ("nothing", "everything"):
        # what the workers' plans keep (the planner is the same code with and without a device): a rank that keeps rows launches its
        # collect phase through jt_collect_flow_keep, and both of its passes carry the flag
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in VARIANTS[variant].items():
            monkeypatch.setenv(k, v)
        for rank in range(world):
            probe = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f64", n_ranks=world, rank=rank, owner=owner,
                                plan_only=True, **BASE)
            keep = probe.describe()["keep"]
            probe.close()
            assert (keep["collect_bytes"] > 0 and keep["distribute_bytes"] > 0) == (variant == "everything"), (variant, rank, keep)
        env = dict(VARIANTS[variant], JTP_RCCL_LIB=mock._build_mock(), JTP_FLOW_TICKETS="1", JTP_TINY_LEVEL_ELEMS="0")
        ctx = mp.get_context("spawn")
        queue = ctx.Queue()
        port_file = str(tmp_path / ("rdzv_port_" + variant))
        procs = [ctx.Process(target=mock._worker, args=(r, world, port_file, recipe, kwargs, dict(BASE), env, queue)) for r in range(world)]
        for p in procs:
            p.start()
        got = {}
        try:
            for _ in range(world):
                rank, status, results, owner, n_comm, fallbacks = queue.get(timeout=300)
                assert status == "ok", results
                assert fallbacks == 0
                got[rank] = results
        finally:
            for p in procs:
                p.join(timeout=60)
                if p.is_alive():
                    p.kill()
        assert all(p.exitcode == 0 for p in procs)
        runs[variant] = got
    for rep in range(3):
        pots = synthetic.potentials_for(spec, seed=40 + rep)
        want = oracle.beliefs_exact(spec["tree"], pots, spec["node_vars"])
        seen = {}
        for rank in range(world):
            mine, _ = runs["everything"][rank][rep]
            base, _ = runs["nothing"][rank][rep]
            assert sorted(mine) == sorted(base)
            for c in mine:
                np.testing.assert_array_equal(mine[c], base[c])
            seen.update(mine)
        assert sorted(seen) == list(range(spec["n_cliques"]))
        for c, g in seen.items():
            np.testing.assert_allclose(g, want[c], rtol=1e-11, atol=1e-13 * np.max(np.abs(want[c])))
