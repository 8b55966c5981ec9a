"""What max-propagation costs on the device (`jtp_max_marginals`, `engine.Plan.max_marginals`), by the method of tools/map_time.py:
a device-time region around the whole call, the best of K repeats after a warm-up call - on the shape of BASELINE config 4 cut to
63 cliques (float32) and on a chain of small cliques (float64), for 1 and for 64 evidence sets.

Three figures per shape and set count:
  jtp_map            the upward max-product sweep and the decode: the yardstick (one pass over the tables)
  jtp_max_marginals  upward, downward and the read-out of a request list: every variable's max-marginal (one request per variable, on
                     the first clique that holds it) and every clique's onto its first two variables
  clamping           what the call replaces: jtp_map under evidence {v: s} for every variable v and state s, sum(card) sets, run
                     through the same plan 64 sets a call (measured once for one evidence set; for 64 evidence sets it is 64 times that)

    python tools/max_time.py [repeats]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, engine, synthetic

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def best_of(plan, call, repeats):
    call()                                                   # (records uploaded, work area allocated)
    wall, dev = float("inf"), float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        plan.region_begin()
        out = call()
        dev = min(dev, plan.region_end())
        wall = min(wall, (time.perf_counter() - t0) * 1e3)
    return dev, wall, out


def timed(spec, dtype, label):
    n = spec["n_cliques"]
    node_vars, sizes = spec["node_vars"], spec["sizes"]
    variables = sorted(sizes)
    requests = [(next(c for c in range(n) if v in node_vars[c]), [v]) for v in variables] + [(c, node_vars[c][:2]) for c in range(n)]
    clamps = [(v, s) for v in variables for s in range(sizes[v])]
    plan = engine.Plan(spec["tree"], node_vars, sizes, dtype=dtype, n_batch=64, share_potentials=True)
    plan.fill_synthetic(1, spec["scales"])
    sched = plan.describe()["sample"]["cliques"]
    kids = max(sum(1 for c in sched if c["parent"] == p["clique"]) for p in sched)
    print("%s: %d cliques on %d depths, at most %d children a clique, %d variables, sum of cardinalities %d; %d requests"
          % (label, n, 1 + max(c["depth"] for c in sched), kids, len(variables), len(clamps), len(requests)))
    one = {}
    for n_sets in (1, 64):
        map_dev, map_wall, (_, value) = best_of(plan, lambda: plan.map(0, n_sets), REPEATS)
        max_dev, max_wall, (tables, scale, max_value) = best_of(plan, lambda: plan.max_marginals(requests, 0, n_sets), REPEATS)
        assert np.array_equal(value, max_value)              # (the same computation)
        one[n_sets] = (map_dev, max_dev)
        print("%s: %2d sets:  jtp_map device %.3f ms (whole call %.3f);  jtp_max_marginals device %.3f ms (whole call %.3f) = %.2f x jtp_map"
              % (label, n_sets, map_dev, map_wall, max_dev, max_wall, max_dev / map_dev))
    # the clamping route for ONE evidence set: sum(card) sets of jtp_map, 64 a call; the clamp of the last state of the first variable
    # is checked against the max-marginal
    logs = np.log(tables[0][0]) + scale[0][0] * np.log(2.0)
    t0 = time.perf_counter()
    plan.region_begin()
    clamped = []
    for at in range(0, len(clamps), 64):
        part = clamps[at:at + 64]
        for b, (v, s) in enumerate(part):
            plan.set_evidence({v: s}, batch=b)
        clamped.append(plan.map(0, len(part))[1])
    dev = plan.region_end()
    wall = (time.perf_counter() - t0) * 1e3
    clamped = np.concatenate(clamped)
    assert abs(clamped[sizes[variables[0]] - 1] - logs[-1]) <= 1e-9 * max(1.0, abs(logs[-1]))
    map_dev, max_dev = one[1]
    print("%s: clamping route, one evidence set: %d sets of jtp_map in %d calls, device %.3f ms (wall %.3f) = %.0f x jtp_max_marginals;  "
          "for 64 evidence sets 64 times that, %.0f ms, against %.3f ms"
          % (label, len(clamps), (len(clamps) + 63) // 64, dev, wall, dev / max_dev, 64 * dev, one[64][1]))
    plan.close()


print("# library build:", _capi.lib().jtp_version().decode())
timed(synthetic.wide_binary_tree(63, width=20, sep=10), "f32", "wide_binary_tree(63, width=20, sep=10) f32")
timed(synthetic.chain_tree(200, card=16, width=3), "f64", "chain_tree(200, card=16, width=3) f64")
