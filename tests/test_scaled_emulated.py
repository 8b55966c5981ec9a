"""JTP_SCALED plans on the CPU: the step list `jtp_plan_create` emits for an overflow-safe propagate (JTP_PLAN_ONLY, no GPU
needed) - the usual launches with one rescale step behind every level - is executed by tests/scaled_emulator.py.

The scale of every message is a power of two, which commutes exactly with every multiply and add downstream: absent underflow,
overflow and subnormals a scaled run IS the unscaled run, bit for bit, up to one known exponent per node.  The checks hang on
that (`array_equal`, no tolerance); the kernel that runs the same records on the device is checked in tests/test_gpu_scaled.py."""
import math

import numpy as np
import pytest

import jt_oracle as oracle
from junctiontree_amd import _capi, engine, synthetic
from scaled_emulator import ScaledEmulator
from test_planner_emulated import star

LN2 = math.log(2.0)


def cases():
    out = {}
    for name, spec in (("wide", synthetic.wide_binary_tree(n_cliques=7, width=12, sep=6)),
                       ("chain", synthetic.chain_tree(n_cliques=6, card=16, width=3)),
                       ("card3", synthetic.wide_binary_tree(n_cliques=7, width=5, sep=2, card=3, seed=4))):
        out[name] = (spec["tree"], synthetic.potentials_for(spec, seed=21), spec["node_vars"], spec["sizes"], spec["n_cliques"])
    tree, pots, node_vars, sizes = star(4, card=2, seed=4)
    out["star4"] = (tree, pots, node_vars, sizes, 5)
    return out


CASES = cases()
_memo = {}


def described(name, dtype="f64"):
    """(plan description, {caller's node: (ABI node, variable ids, cardinalities)}) of the scaled plan of a case, made once"""
    if (name, dtype) not in _memo:
        tree, _, node_vars, sizes, _ = CASES[name]
        plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, plan_only=True, scaled=True)
        desc = plan.describe()
        nodes = {n: (plan.abi_of[n], [plan.var_id[lab] for lab in node_vars[n]], [sizes[lab] for lab in node_vars[n]])
                 for n in plan.node_ids}
        _memo[name, dtype] = (desc, nodes, list(plan.cliques), list(plan.seps))
        plan.close()
    return _memo[name, dtype]


def run(name, pots, rescale=True, dtype="f64", check_written=True):
    """beliefs {node: array} as the emulated arenas hold them, {node: E}, and (sign, log|Z|)"""
    desc, nodes, cliques, seps = described(name, dtype)
    emu = ScaledEmulator(desc, rescale=rescale)
    emu.check_written = check_written
    for c in cliques:
        abi, ids, cards = nodes[c]
        emu.set_potential(abi, ids, cards, pots[c])
    emu.propagate()
    node_e, sep_e = emu.node_exponents()
    psep_of = {s["node"]: i for i, s in enumerate(desc["pseps"]) if s["node"] >= 0}
    bel, exps = {}, {}
    for c in cliques:
        abi, ids, cards = nodes[c]
        bel[c], exps[c] = emu.belief(abi, ids, cards), node_e[abi]
    for s in seps:
        abi, ids, cards = nodes[s]
        bel[s], exps[s] = emu.sep_belief(psep_of[abi], ids, cards), sep_e[psep_of[abi]]
    root = desc["root"]
    total = float(bel[cliques[root]].sum())
    log_abs = math.log(abs(total)) + node_e[root] * LN2 if total != 0 and np.isfinite(total) else float("nan")
    return bel, exps, (float(np.sign(total)), log_abs)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_message_has_one_rescale_record_between_producer_and_consumers(name):
    desc, _, _, _ = described(name)
    if name == "star4":
        assert any(p["real"] < 0 for p in desc["pnodes"])            # a binarised virtual clique
    if name == "card3":
        assert desc["tmix"] == 1                                     # mixed-radix rows
    step_of_launch = {first: i for i, (kind, first, _) in enumerate(desc["steps"]) if kind == 0}
    step_of_record = {}
    for i, (kind, first, count) in enumerate(desc["steps"]):
        assert kind in (0, 2)
        if kind == 2:
            assert count > 0
            for r in range(first, first + count):
                assert r not in step_of_record
                step_of_record[r] = i
    assert sorted(step_of_record) == list(range(len(desc["rescale"])))
    # who writes / reads which doubles of the message arena, by step
    writes, reads = [], []
    for li, L in enumerate(desc["launches"]):
        for t in L["tasks"]:
            tk = desc["tasks"][t]
            for m in tk["out"]:
                writes.append((m["off"], m["off"] + m["npart"] * m["pstride"], step_of_launch[li], tk["kind"], tk["in"][0] if tk["kind"] == 1 else None))
            if tk["kind"] == 0:
                for m in tk["in"]:
                    if not m["fixed"]:
                        reads.append((m["off"], m["off"] + m["npart"] * m["pstride"], step_of_launch[li]))

    def writers(lo, hi):
        steps = []
        for a, b, step, kind, src in writes:
            if a < hi and lo < b:
                steps.append(step)
                if kind == 1:                                        # a reduce task: behind the producer of the copies it sums
                    steps += writers(src["off"], src["off"] + src["npart"] * src["pstride"])
        return steps

    by_slot = {}
    for r, rec in enumerate(desc["rescale"]):
        assert rec["slot"] not in by_slot
        by_slot[rec["slot"]] = r
    n_msg = 0
    for i, s in enumerate(desc["pseps"]):
        for up in (1, 0):
            d = "up" if up else "dn"
            if s[d + "_off"] < 0:
                continue
            n_msg += 1
            rec = desc["rescale"][by_slot[2 * i + (0 if up else 1)]]
            # the buffer consumers and the read-out read: the sum where a reduce task exists, else the copies themselves
            assert rec["off"] == s[d + "_roff"] and rec["count"] == s[d + "_rnpart"] << s["nbits"]
            assert (s[d + "_red_task"] >= 0) == (s[d + "_roff"] != s[d + "_off"])
            at = step_of_record[by_slot[2 * i + (0 if up else 1)]]
            w = writers(rec["off"], rec["off"] + rec["count"])
            rd = [step for a, b, step in reads if a < rec["off"] + rec["count"] and rec["off"] < b]
            assert w and max(w) < at
            assert (rd or not up) and all(at < step for step in rd)
    assert n_msg == len(desc["rescale"]) == 2 * len(desc["pseps"])
    # no other buffer is scaled: the records do not overlap each other
    spans = sorted((r["off"], r["off"] + r["count"]) for r in desc["rescale"])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_in_range_the_scaled_run_is_the_unscaled_run_up_to_an_exponent(name, dtype):
    pots = CASES[name][1]
    scaled, exps, (sign, log_z) = run(name, pots, dtype=dtype)
    plain, zeros, (_, log_z_plain) = run(name, pots, rescale=False, dtype=dtype)
    assert any(exps.values()) and not any(zeros.values())
    for n in scaled:
        np.testing.assert_array_equal(np.ldexp(scaled[n], exps[n]), plain[n], err_msg="node %r" % (n,))
    want, z = oracle.beliefs_exact(CASES[name][0], pots, CASES[name][2], return_z=True)
    for n in scaled:
        np.testing.assert_allclose(plain[n], np.broadcast_to(want[n], plain[n].shape), rtol=1e-11, atol=1e-13)
    assert sign == 1.0 and abs(log_z - math.log(z)) <= 1e-11 * max(abs(math.log(z)), 1.0) and abs(log_z - log_z_plain) <= 1e-11


@pytest.mark.parametrize("name", sorted(CASES))
def test_out_of_range_inputs_give_the_same_normalised_beliefs_and_a_shifted_log_z(name):
    """Every clique table x 2^+200 (and x 2^-200): Z moves by 2^(+-200 n_cliques), beyond float64 even on the 6-clique chain.
    Fails without the feature: the unscaled run of the same plan overflows."""
    tree, pots, node_vars, sizes, n_cliques = CASES[name]
    _, z = oracle.beliefs_exact(tree, pots, node_vars, return_z=True)
    assert 2.0 ** -100 < z < 2.0 ** 100
    base, _, (_, log_z_base) = run(name, pots)
    assert abs(log_z_base - math.log(z)) <= 1e-11 * max(abs(math.log(z)), 1.0)
    for k in (200, -200):
        moved = [np.ldexp(np.asarray(p, dtype=np.float64), k) if c < n_cliques else p for c, p in enumerate(pots)]
        got, _, (sign, log_z) = run(name, moved)
        for n in got:
            assert np.all(np.isfinite(got[n]))
            np.testing.assert_array_equal(got[n] / got[n].sum(), base[n] / base[n].sum(), err_msg="node %r, 2^%d" % (n, k))
        want = math.log(z) + n_cliques * k * LN2
        assert sign == 1.0 and abs(log_z - want) <= 1e-11 * abs(want)
    big = [np.ldexp(np.asarray(p, dtype=np.float64), 200) if c < n_cliques else p for c, p in enumerate(pots)]
    with np.errstate(over="ignore", invalid="ignore"):
        plain, _, _ = run(name, big, rescale=False, check_written=False)
    root_clique = described(name)[2][described(name)[0]["root"]]
    # (Z x 2^(200 n_cliques) is beyond float64 from six cliques on; the 5-clique star stays just inside)
    assert np.all(np.isfinite(plain[root_clique])) == (math.log2(z) + 200 * n_cliques < 1023)
    assert name == "star4" or not np.all(np.isfinite(plain[root_clique]))


def test_scaled_multiset_and_multirank_plans_are_refused():
    spec = synthetic.wide_binary_tree(n_cliques=7, width=12, sep=6)
    args = (spec["tree"], spec["node_vars"], spec["sizes"])
    with pytest.raises(_capi.UnsupportedStructure, match="JTP_SCALED with JTP_MULTISET"):
        engine.Plan(*args, plan_only=True, scaled=True, multiset=True, n_batch=8)
    with pytest.raises(_capi.UnsupportedStructure, match="JTP_SCALED with n_ranks"):
        engine.Plan(*args, plan_only=True, scaled=True, n_ranks=2, rank=0, owner=[0, 0, 1, 0, 0, 1, 1])
    # ... and a plan without the flag describes as before: no trace of the feature
    plan = engine.Plan(*args, plan_only=True)
    d = plan.describe()
    assert "scaled" not in d and "rescale" not in d and all(kind != 2 for kind, _, _ in d["steps"]) and d["segments"]
    assert plan.log2_scale(0) == 0
    plan.close()
