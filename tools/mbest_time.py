"""What the M most probable assignments cost on the device (`jtp_map_best`, `engine.Plan.map_best`) beside the single most probable
one (`jtp_map`): device time of the whole call over a region (`jtp_region_begin` / `jtp_region_end`) on the shape of BASELINE config
4 cut to 63 cliques (float32, the width-20 tree of DESIGN.md section 6) and on the three-clique tree whose root has 2^16 entries per k
(float64, cut into segments: the merge kernel runs), one evidence set, for m = 1, 4 and 16 - the three list lengths the kernels
are built for.

The calls are interleaved round by round in one process, so that whatever the clock does it does to all of them; per call the
smallest, the median and the largest time of the rounds are printed.  `jtp_map`'s line is the yardstick, and the one to compare
between two builds of the library (JTPROP_LIB=... python tools/mbest_time.py on the older one prints that line alone).

    python tools/mbest_time.py [rounds]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, engine, synthetic

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
HAS_MBEST = hasattr(_capi.lib(), "jtp_map_best")


def timed(spec, dtype, label):
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype)
    plan.fill_synthetic(1, spec["scales"])
    sched = plan.describe()["sample"]
    print("%s: %d cliques on %d depths, largest slice %d entries" % (label, len(sched["cliques"]), len(sched["depths"]), max(c["R"] for c in sched["cliques"])))
    calls = [("jtp_map", lambda: plan.map())]
    if HAS_MBEST:
        calls += [("jtp_map_best m = %d" % m, lambda m=m: plan.map_best(m)) for m in (1, 4, 16)]
    for _, call in calls:                                    # (records uploaded, work areas allocated)
        call()
    ms = {name: [] for name, _ in calls}
    for _ in range(ROUNDS):
        for name, call in calls:
            plan.region_begin()
            states, value = call()
            ms[name].append(plan.region_end())
            assert states.min() >= 0 and len(value) == len(states)
    base = float(np.median(ms["jtp_map"]))
    for name, _ in calls:
        t = np.array(ms[name])
        print("%s: %-22s device ms  min %.3f  median %.3f  max %.3f  (%d rounds);  median / jtp_map's %.2f" % (label, name, t.min(), np.median(t), t.max(), ROUNDS, np.median(t) / base))
    if HAS_MBEST:
        assert np.array_equal(plan.map_best(1)[0], plan.map()[0]) and np.array_equal(plan.map_best(16)[0][:4], plan.map_best(4)[0])
    plan.close()


print("# library build:", _capi.lib().jtp_version().decode())
timed(synthetic.wide_binary_tree(63, width=20, sep=10), "f32", "wide_binary_tree(63, width=20, sep=10) f32")
timed(synthetic.wide_binary_tree(3, 16, 4), "f64", "wide_binary_tree(3, 16, 4) f64 (root64k)")
