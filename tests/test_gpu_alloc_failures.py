"""Every allocation the engine makes can fail, one at a time, and nothing is left behind.

The buffers of `csrc/jtp_device.h` carry a test hook: the N-th allocation from now on reports out of memory on the host, without calling
HIP (`JTP_FAIL_ALLOC=N` for the allocations of `jtp_plan_create`, `jtp_debug_set(plan, "fail_alloc", N)` for a live plan), and
`jtp_debug_live_bytes` says what the library holds.  For N = 1, 2, ... until the call goes through: the call raises `MemoryError`
(`JTP_ENOMEM` from EVERY entry point), the bytes held are what they were before the call, and the call that finally succeeds returns exactly
what a plan that never saw a failure returns.

Two of these are defects of the hand-kept pointers this replaced: a `jtp_get_belief` of a unit clique whose second or third allocation
failed left `d_task` set, so the next call skipped the build and launched with a null block list and a grid of zero; `jtp_sample` took
its schedule records for built as soon as they were allocated, before the copy that fills them."""
import ctypes as C
import gc

import numpy as np
import pytest

from junctiontree_amd import _capi, engine, synthetic
from test_lean_emulated import _with_cover
from test_planner_emulated import star

pytestmark = pytest.mark.gpu

N_SETS = 64              # eight groups of evidence sets: the plan gets an evidence-free group (set0 != 0), active lists and d_fanout


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


class Case:
    """One kind of plan: how it is created, what it is loaded with, and every belief it gives after a propagate."""

    def __init__(self, kind):
        self.kind = kind
        self.opts = {}
        if kind == "star":
            self.tree, self.pots, self.node_vars, self.sizes = star(3, card=2)
            self.n = 4
        else:
            spec = synthetic.wide_binary_tree(n_cliques=7, width=12, sep=6, card=2, seed=1)
            self.tree, self.node_vars, self.sizes, self.n = spec["tree"], spec["node_vars"], spec["sizes"], 7
            self.pots = synthetic.potentials_for(spec, seed=3)
            if kind == "unit":           # (tests/test_gpu_lean.py: wide unit cliques; JTP_UNIT_RATIO=1 is set by the test)
                cover, self.pots = _with_cover(spec, self.pots, np.random.default_rng(2), p_none=0.2)
                cover[3], self.pots[3] = list(self.node_vars[3]), synthetic.potentials_for(spec, seed=3)[3]
                self.opts = {"cover": cover}
            elif kind == "scaled":
                self.opts = {"scaled": True}
            elif kind == "multi":
                self.opts = {"n_batch": N_SETS, "multiset": True}
        self.labels = sorted(self.sizes)

    def create(self):
        return engine.Plan(self.tree, self.node_vars, self.sizes, dtype="f64", **self.opts)

    def load(self, plan):
        plan.fill_synthetic(3)           # (on the device: the upload buffers of set_potential stay unallocated)
        if self.kind == "multi":
            for b in range(N_SETS):
                rng = np.random.default_rng(70 + b)
                plan.set_evidence({self.labels[i]: int(rng.integers(0, 2)) for i in rng.choice(len(self.labels), size=b % 3, replace=False)}, batch=b)
        return plan

    def beliefs(self, plan):
        plan.propagate()
        sets = (0, 9, N_SETS - 1) if self.kind == "multi" else (0,)
        return [plan.belief(node, batch=b) for b in sets for node in range(len(self.node_vars))]


def same(got, want):
    got, want = (x if isinstance(x, list) else [x] for x in (got, want))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("kind", ["wide", "scaled", "multi"])
def test_plan_creation_survives_the_failure_of_each_of_its_allocations(kind, monkeypatch):
    case = Case(kind)
    ref = case.load(case.create())
    want = case.beliefs(ref)
    ref.close()
    before = live_bytes()
    plan, failed = None, 0
    for n in range(1, 64):
        monkeypatch.setenv("JTP_FAIL_ALLOC", str(n))
        try:
            plan = case.create()
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of jtp_plan_create failed and something stayed behind" % n
            continue
        break
    monkeypatch.delenv("JTP_FAIL_ALLOC")
    assert plan is not None and failed == n - 1 and failed >= 5       # (arenas, sync area, abort flag, task tables: more than five)
    now = live_bytes()                                                 # jtp_stats.device_bytes is counted, not derived: what the plan holds
    assert (now[0] - before[0]) + (now[1] - before[1]) == int(plan.stats()["device_bytes"])
    same(case.beliefs(case.load(plan)), want)
    plan.close()
    assert live_bytes() == before


def _unit_clique(plan):
    return next(p["real"] for p in plan.describe()["pnodes"] if p["unit"] and p["real"] >= 0 and p["stat"] >= 0)


def _products(case):
    vs, p0 = case.node_vars[0], np.random.default_rng(5).uniform(0.5, 1.5, (2,) * 6)
    return lambda plan: plan.set_potential_product(0, [p0, 2.0 * p0], [vs[:6], vs[6:]])


# name: (kind of plan, the call under test, fewest allocations its first call must make);  a call that returns nothing is judged by
# the beliefs of the propagate that follows it
LAZY = {
    "belief of a unit clique": ("unit", lambda case: lambda plan: plan.belief(_unit_clique(plan)), 4),        # scratch arena, task, blocks, rows (+ stage)
    "belief on a multi-set plan": ("multi", lambda case: lambda plan: plan.belief(2, batch=9), 3),
    "marginals": ("wide", lambda case: lambda plan: plan.marginals([(0, case.node_vars[0][:2]), (3, case.node_vars[3][-1:])]), 4),
    "sample": ("wide", lambda case: lambda plan: plan.sample(5, seed=11), 3),                                  # records, failure report, state rows
    "set_potential": ("wide", lambda case: lambda plan: plan.set_potential(0, 1.5 * case.pots[0]), 1),        # 32 KiB: above the 256-byte minimum stage
    "set_potential_products": ("wide", _products, 2),                                                          # device buffer and its pinned mirror
    "set_evidence": ("wide", lambda case: lambda plan: plan.set_evidence({case.labels[0]: 1, case.labels[5]: 0}), 1),
}


@pytest.mark.parametrize("name", sorted(LAZY))
def test_first_calls_survive_the_failure_of_each_of_their_allocations(name, monkeypatch):
    monkeypatch.setenv("JTP_UNIT_RATIO", "1")
    kind, make_call, fewest = LAZY[name]
    case = Case(kind)
    call = make_call(case)

    def outcome(plan):
        out = call(plan)
        return case.beliefs(plan) if out is None else out

    fresh = case.load(case.create())
    fresh.propagate()
    want = outcome(fresh)
    fresh.close()

    plan = case.load(case.create())
    plan.propagate()
    failed = 0
    for n in range(1, 16):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            call(plan)
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    assert failed == n - 1 and failed >= fewest, (failed, n)
    plan.debug_set("fail_alloc", 0)
    same(outcome(plan), want)
    plan.close()


def test_closed_plans_leave_no_bytes_behind(monkeypatch):
    monkeypatch.setenv("JTP_UNIT_RATIO", "1")
    plans = []
    for kind in ("wide", "star", "scaled", "unit", "multi"):
        case = Case(kind)
        plan = case.load(case.create())
        plans.append(plan)
        case.beliefs(plan)
        plan.marginals([(0, case.node_vars[0][:2]), (1, case.node_vars[1][-1:])])
        plan.z()
        if kind in ("wide", "star", "scaled"):                # (plans that keep every belief table)
            plan.sample(5, seed=3)
            plan.set_potential_product(1, [case.pots[1]], [case.node_vars[1]])
        plan.set_evidence({case.labels[0]: 1})
        plan.propagate()
    assert live_bytes()[0] > 0 and live_bytes()[1] > 0
    for plan in plans:
        plan.close()
    engine.clear_plan_cache()
    assert live_bytes() == (0, 0)
