"""Which table rows a plan keeps in the Infinity Cache (`JtTask::keep_rows`, PlanBuilder::schedule), checked on the CPU from
`describe()` of JTP_PLAN_ONLY plans: the budget holds, bandwidth-bound levels come before the narrow top, nearest the root first, whole
levels only, both passes of a kept clique are flagged, multi-set plans keep nothing - and the emulator, which runs the planner's task
tables, computes the oracle's beliefs whatever is kept (the flag is a cache-policy hint: no table entry moves).

The scaled tree is BASELINE config 4's shape at 1/256 of its bytes: 255 cliques of 2^12 float32 (16 KiB), levels 0..7 of 16 KiB x 2^d.
Trees this small count as latency-bound ("chain") plans, whose kernels have no choice of policy and which therefore keep nothing:
JTP_TINY_LEVEL_ELEMS=0 plans them as the large trees they stand for.  The workgroups then have four rows, so a workgroup's life is
1.5 + 8 + 1 + 4 x 0.55 = 12.7 us in the cost model (`jtp_keep_cost`); at JTP_KEEP_BW = 30000 bytes/us level 3 (128 KiB read + 128 KiB written: 8.7 us) is narrow and level 4 (17.5 us) is the first
bandwidth-bound one - where config 4's own levels divide at the model's 5 TB/s with their 8 and 16 rows."""
import numpy as np
import pytest

import jt_oracle as oracle
from emulator import Emulator
from junctiontree_amd import engine, synthetic

KIB = 1024
BW = "30000"
NOTHING = {"budget_bytes": 0, "collect_bytes": 0, "distribute_bytes": 0, "levels": []}


@pytest.fixture(autouse=True)
def _not_a_chain(monkeypatch):
    monkeypatch.setenv("JTP_TINY_LEVEL_ELEMS", "0")


def plan_desc(spec, dtype="f32", **opts):
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, plan_only=True, **opts)
    d = plan.describe()
    plan.close()
    return d


def kept(d):
    """{level: [bytes kept, bytes of the level]} over table-keeping cliques; asserts that both passes of a clique agree"""
    esize = 4 if d["dtype"] == 0 else 8
    out = {}
    for p in d["pnodes"]:
        if p["unit"]:
            continue
        flags = {d["tasks"][t]["keep_rows"] for t in (p["collect_task"], p["distribute_task"]) if t >= 0}
        assert len(flags) == 1, p                          # both passes of a clique, or neither
        lvl = out.setdefault(p["depth"], [0, 0])
        lvl[1] += p["phys_elems"] * esize
        lvl[0] += p["phys_elems"] * esize * flags.pop()
    return out


def block_flags(d):
    """JtBlock::flags per task, from the workgroup records (the last field of a record)"""
    per_task = {}
    for b in d["blocks"]:
        per_task.setdefault(b[0], set()).add(b[-1])
    return per_task


@pytest.fixture(scope="module")
def scaled_c4():
    return synthetic.wide_binary_tree(n_cliques=255, width=12, sep=6, card=2, seed=1)


def scaled(monkeypatch, spec, budget_kib, **env):
    monkeypatch.setenv("JTP_KEEP_BW", BW)
    monkeypatch.setenv("JTP_KEEP_ROWS_MB", repr(budget_kib / 1024.0))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = plan_desc(spec)
    levels = kept(d)
    assert sorted(levels) == list(range(8)) and [levels[l][1] for l in range(8)] == [16 * KIB << l for l in range(8)]
    assert all(t["total"] == 4 for t in d["tasks"] if t["kind"] == 0 and t["mode"] == 1)      # (what the docstring's 12.7 us stands on)
    whole = sorted(l for l, (k, n) in levels.items() if k == n)
    assert all(k in (0, n) for k, n in levels.values())                           # whole levels only
    assert d["keep"]["levels"] == whole and d["keep"]["budget_bytes"] == budget_kib * KIB
    assert d["keep"]["distribute_bytes"] == sum(k for k, _ in levels.values()) <= budget_kib * KIB
    # (the root has no collect pass)
    assert d["keep"]["collect_bytes"] == d["keep"]["distribute_bytes"] - (16 * KIB if 0 in whole else 0)
    return whole, d


@pytest.mark.parametrize("budget_kib,want", [
    (0, []),
    (200, [0, 1, 2]),                     # no bandwidth-bound level fits: the narrow top alone, levels 0-2 (112 KiB; level 3 would make 240)
    (256, [4]),                           # the first bandwidth-bound level, nothing left above it
    (512, [0, 1, 2, 3, 4]),               # config 4 at 128 MiB: level 4, then the narrow top (240 KiB)
    (640, [0, 1, 2, 3, 4]),               # ... at 160 MiB: level 5 (512 KiB) does not fit behind level 4
    (768, [4, 5]),                        # a budget that fits two levels: the two bandwidth-bound levels nearest the root
    (896, [0, 1, 2, 4, 5]),               # ... at 224 MiB: 112 KiB of the 128 left
    (1024, [0, 1, 2, 3, 4, 5]),
    (4080, list(range(8))),               # the plan's tables fit altogether (255 x 16 KiB): everything
])
def test_levels_kept_by_what_they_save(monkeypatch, scaled_c4, budget_kib, want):
    whole, _ = scaled(monkeypatch, scaled_c4, budget_kib)
    assert whole == want


def test_budget_holds_at_every_size(monkeypatch, scaled_c4):
    for budget_kib in range(0, 4200, 150):
        scaled(monkeypatch, scaled_c4, budget_kib)                                # (asserts kept <= budget)


def test_narrow_top_can_be_left_out(monkeypatch, scaled_c4):
    assert scaled(monkeypatch, scaled_c4, 512, JTP_KEEP_TOP="0")[0] == [4]


def test_workgroup_records_carry_the_flags(monkeypatch, scaled_c4):
    _, d = scaled(monkeypatch, scaled_c4, 768)
    flags = block_flags(d)
    for t, tk in enumerate(d["tasks"]):
        if tk["kind"] == 0:
            assert {f & 2 for f in flags[t]} == {2 if tk["keep_rows"] else 0}, (t, tk["mode"], flags[t])      # JT_BLOCK_KEEP_ROWS


def test_config_4_itself(monkeypatch):
    """the headline plan at the cost model's own constants: levels 0-3 are narrow, level 4 (64 MiB) is the first bandwidth-bound one"""
    spec = synthetic.wide_binary_tree(n_cliques=256, width=20, sep=10, card=2, seed=1)
    for mb, want in ((128, [0, 1, 2, 3, 4]), (192, [4, 5]), (256, [0, 1, 2, 3, 4, 5]), (0, [])):
        monkeypatch.setenv("JTP_KEEP_ROWS_MB", str(mb))
        d = plan_desc(spec)
        assert d["keep"]["levels"] == want and d["keep"]["distribute_bytes"] <= mb << 20
        assert d["keep"]["distribute_bytes"] == sum(4 << 20 << l for l in want)


def test_multiset_plans_keep_nothing(monkeypatch):
    monkeypatch.setenv("JTP_KEEP_ROWS_MB", "4096")
    spec = synthetic.wide_binary_tree(n_cliques=15, width=12, sep=6, card=2, seed=2)
    d = plan_desc(spec, n_batch=8, multiset=True)
    assert d["multiset"] == 1 and d["keep"] == NOTHING
    assert not any(t["keep_rows"] for t in d["tasks"]) and not any(b[-1] & 2 for b in d["blocks"])


def test_plans_whose_kernels_do_not_look_at_the_flag_keep_nothing(monkeypatch):
    """per-level launches, per-shape launches, chains and mixed-radix rows run kernels without the choice of policy: what `describe()`
    reports as kept is what some load keeps"""
    monkeypatch.setenv("JTP_KEEP_ROWS_MB", "4096")
    wide = synthetic.wide_binary_tree(n_cliques=15, width=12, sep=6, card=2, seed=2)
    assert plan_desc(wide)["keep"]["distribute_bytes"] == 15 * 16 * KIB
    cases = [(wide, {"level_launches": True}), (wide, {"split_variants": True}),
             (synthetic.wide_binary_tree(n_cliques=7, width=8, sep=4, card=3, seed=3), {}),
             (None, None), (wide, {}), (synthetic.chain_tree(n_cliques=9, card=8, width=3), {})]
    for spec, opts in cases:
        if spec is None:                  # from here on the planner's own rule: trees of tiny levels are chains
            monkeypatch.delenv("JTP_TINY_LEVEL_ELEMS")
            continue
        d = plan_desc(spec, **opts)
        assert d["keep"] == NOTHING, (opts, d["keep"])
        assert not any(t["keep_rows"] for t in d["tasks"]) and not any(b[-1] & 2 for b in d["blocks"])
    monkeypatch.setenv("JTP_FORCE_LEVEL_LAUNCHES", "1")
    assert plan_desc(wide)["keep"] == NOTHING


def test_a_rank_keeps_within_its_own_budget(monkeypatch, scaled_c4):
    """several ranks: every rank chooses among ITS tables (its subtrees and the replicated top)"""
    from junctiontree_amd import partition
    monkeypatch.setenv("JTP_KEEP_BW", BW)
    spec = scaled_c4
    weights = [float(2 ** 12)] * spec["n_cliques"]
    owner = partition.subtree_owners(spec["parent"], weights, 4, replicate_top=True)
    for budget_kib in (0, 128, 300, 4096):
        monkeypatch.setenv("JTP_KEEP_ROWS_MB", repr(budget_kib / 1024.0))
        for rank in range(4):
            d = plan_desc(spec, n_ranks=4, rank=rank, owner=owner)
            mine = [p for p in d["pnodes"] if p["owner"] in (rank, 4) and not p["unit"]]
            got = sum(p["phys_elems"] * 4 for p in mine if d["tasks"][p["distribute_task"]]["keep_rows"])
            assert got == d["keep"]["distribute_bytes"] <= budget_kib * KIB
            if budget_kib == 4096:
                assert got == sum(p["phys_elems"] * 4 for p in mine) > 0                  # fits: all of it
            if budget_kib == 0:
                assert got == 0


@pytest.mark.parametrize("budget_mb", ["0", "0.1", "4096"])
def test_emulated_beliefs_do_not_depend_on_what_is_kept(monkeypatch, budget_mb):
    monkeypatch.setenv("JTP_KEEP_BW", "1")              # every level counts as bandwidth-bound
    monkeypatch.setenv("JTP_KEEP_ROWS_MB", budget_mb)
    spec = synthetic.wide_binary_tree(n_cliques=15, width=12, sep=6, card=2, seed=3)
    pots = synthetic.potentials_for(spec, seed=9)
    want = oracle.beliefs_exact(spec["tree"], pots, spec["node_vars"])
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f64", plan_only=True)
    d = plan.describe()
    n_kept = sum(1 for t in d["tasks"] if t["keep_rows"])
    assert (n_kept == 0) == (budget_mb == "0") and (budget_mb != "0.1" or 0 < n_kept < sum(1 for t in d["tasks"] if t["kind"] == 0))
    emu = Emulator(d)
    for c in plan.cliques:
        ids = [plan.var_id[lab] for lab in spec["node_vars"][c]]
        emu.set_potential(plan.abi_of[c], ids, [spec["sizes"][lab] for lab in spec["node_vars"][c]], pots[c])
    emu.propagate_flow()
    for c in plan.cliques:
        ids = [plan.var_id[lab] for lab in spec["node_vars"][c]]
        got = emu.belief(plan.abi_of[c], ids, [spec["sizes"][lab] for lab in spec["node_vars"][c]])
        np.testing.assert_allclose(got, want[c], rtol=1e-11, atol=1e-13)
    plan.close()
