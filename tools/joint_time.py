"""What the joint of two variables of different cliques costs on the device (`jtp_joint`, `engine.Plan.joint`): the time of the whole
call - records up, the sigma launch, one launch per active depth, the table back - after a propagate, on a chain of small cliques
(float64: the joint of a variable of the first clique and one of the last, carried across every level) and on the shape of BASELINE
config 4 cut to 63 cliques (float32: two variables homed in two different leaves).

Beside each the route users have had for the same table: one evidence set per state of the first variable (the plan
`propagate_evidence_sets` makes: eight sets per pass over shared tables), every set propagated, the second variable's marginal read
from each set and the rows stacked on the host - a row of set s is P(a = s, z) x Z already.  Both routes are timed from the tables
resident on the device to the table on the host, the propagate(s) included; the joint call is also timed alone.

    python tools/joint_time.py [repeats]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, engine, synthetic

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7


def best(fn):
    out, wall = None, float("inf")
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        out = fn()
        wall = min(wall, (time.perf_counter() - t0) * 1e3)
    return out, wall


def timed(spec, dtype, a, z, clique_of_z, label):
    n_states = spec["sizes"][a]
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype)
    plan.fill_synthetic(1, spec["scales"])
    plan.propagate()
    plan.joint([a, z])                                       # (buffers allocated)

    def joint_route():
        plan.propagate(sync=False)
        return plan.joint([a, z])[0]

    def joint_alone():
        plan.region_begin()
        plan.joint([a, z])
        return plan.region_end()

    table, route_ms = best(joint_route)
    dev_ms = min(joint_alone() for _ in range(REPEATS))
    _, call_ms = best(lambda: plan.joint([a, z]))
    sched = plan.describe()["sample"]
    plan.close()

    try:
        sets = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, n_batch=n_states, multiset=True)
        mode = "multi-set plan"
    except _capi.UnsupportedStructure:
        sets = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, n_batch=n_states, share_potentials=True)
        mode = "one pass per set over shared tables"
    sets.fill_synthetic(1, spec["scales"])

    def clamp_route():
        for s in range(n_states):
            sets.set_evidence({a: s}, batch=s)
        sets.propagate(0, n_states)
        return np.stack([sets.marginal(clique_of_z, [z], batch=s) for s in range(n_states)])

    clamp_route()
    rows, clamp_ms = best(clamp_route)
    sets.close()
    worst = float(np.max(np.abs(rows - table) / table))
    print("%s: %d cliques on %d depths;  P(%r, %r), %d x %d entries" % (label, len(sched["cliques"]), len(sched["depths"]), a, z, table.shape[0], table.shape[1]))
    print("%s: jtp_joint alone: device %.3f ms, whole call %.3f ms;  propagate + jtp_joint %.3f ms;  %d clamped sets (%s) + marginals + stacking %.3f ms;  "
          "ratio %.2f;  the two tables differ by %.2g relative" % (label, dev_ms, call_ms, route_ms, n_states, mode, clamp_ms, clamp_ms / route_ms, worst))


print("# library build:", _capi.lib().jtp_version().decode())
chain = synthetic.chain_tree(200, card=16, width=3)
timed(chain, "f64", 0, 201, 199, "chain_tree(200, card=16, width=3) f64")
wide = synthetic.wide_binary_tree(63, width=20, sep=10)
leaf_a, leaf_z = 31, 62                                      # the first and the last leaf of the balanced tree: the root is the top
fresh = lambda c: [v for v in wide["node_vars"][c] if v not in wide["node_vars"][(c - 1) // 2]]
timed(wide, "f32", fresh(leaf_a)[0], fresh(leaf_z)[0], leaf_z, "wide_binary_tree(63, width=20, sep=10) f32")
