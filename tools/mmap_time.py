"""What marginal MAP costs on the device (`jtp_marginal_map`, `engine.Plan.marginal_map`) beside `jtp_map`, on the plan
tools/map_time.py times `jtp_map` on: BASELINE config 4 cut to 63 cliques (float32), 64 evidence sets.

  (a) the query of all variables: every clique sums nothing, the call launches jtp_map's kernels over records equal to jtp_map's;
  (b) the 320 variables of the 31 cliques of the top five levels (half of the 640): the given tree is strong for them
      (`construction.is_strong`), the 32 leaves sum 1024 entries behind each of their 1024 separator assignments, the rest is (a)'s.

Per call the device time (`region_begin` / `region_end`) and the wall time of the whole call; of REPEATS timed calls after two
warm-up calls the smallest, the median and the largest are printed: the spread to read a difference against.  With JTPROP_LIB naming
a library that lacks `jtp_marginal_map` (the build of an earlier commit) only `jtp_map` is timed: the baseline of (a).

    python tools/mmap_time.py [repeats]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, construction, engine, synthetic

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
N_SETS = 64


def timed(plan, label, call):
    for _ in range(2):
        call()
    dev, wall = [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        plan.region_begin()
        states, value = call()
        dev.append(plan.region_end())
        wall.append((time.perf_counter() - t0) * 1e3)
    assert states.min() >= 0 and np.all(np.isfinite(value))
    dev.sort()
    wall.sort()
    print("%-34s device ms: min %.3f  median %.3f  max %.3f   whole call ms: min %.3f  median %.3f  max %.3f"
          % (label, dev[0], dev[len(dev) // 2], dev[-1], wall[0], wall[len(wall) // 2], wall[-1]))
    return states, value


print("# library build:", _capi.lib().jtp_version().decode())
spec = synthetic.wide_binary_tree(63, width=20, sep=10)
plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f32", n_batch=N_SETS, share_potentials=True)
plan.fill_synthetic(1, spec["scales"])
for b in range(N_SETS):                                      # distinct evidence per set, on a leaf's own variable
    plan.set_evidence({plan.var_labels[-1 - b]: b & 1}, batch=b)
print("wide_binary_tree(63, width=20, sep=10) f32, %d evidence sets, %d variables, %d timed calls each" % (N_SETS, len(plan.var_labels), REPEATS))
map_states, map_value = timed(plan, "jtp_map", plan.map)
if hasattr(_capi.lib(), "jtp_marginal_map"):
    full = list(plan.var_labels)
    states, value = timed(plan, "(a) jtp_marginal_map, all variables", lambda: plan.marginal_map(full))
    assert np.array_equal(states, map_states) and np.array_equal(value, map_value)       # bit for bit
    order, parent, _, _ = engine.flatten_tree(spec["tree"])
    depth = {}
    for c in order:
        depth[c] = depth[parent[c]] + 1 if parent[c] >= 0 else 0
    n = spec["n_cliques"]
    top = sorted({v for c in range(n) if depth[c] < 5 for v in spec["node_vars"][c]}, key=plan.var_labels.index)
    assert construction.is_strong([parent[c] for c in range(n)], spec["node_vars"][:n], top)
    print("(b): %d of %d variables, those of the %d cliques above the leaves" % (len(top), len(plan.var_labels), sum(1 for c in range(n) if depth[c] < 5)))
    timed(plan, "(b) jtp_marginal_map, top half", lambda: plan.marginal_map(top))
    timed(plan, "jtp_map again", plan.map)
plan.close()
