"""What the most probable assignment costs on the device (`jtp_map`, `engine.Plan.map`): the time of the whole call - evidence
rows and table pointers up, one launch per depth of the tree, the decode launch, states and maxima back - on the shape of BASELINE
config 4 cut to 63 cliques (float32) for 1 and for 64 evidence sets, and on a chain of small cliques (float64).

Beside each figure the yardstick: the COLLECT phase of the sum-product propagate on the same plan (`collect_ms` of `jtp_get_stats`
with profiling on, one evidence set) - it reads the same tables once.  The ratio is per evidence set.

    python tools/map_time.py [repeats] [segment lengths to compare, e.g. 0,1024,256: jtp_debug_set "map_seg"]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, engine, synthetic

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SEGS = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [0]


def collect_ms(spec, dtype):
    """the yardstick: with one launch per level the propagate's phases are timed apart (a dataflow plan may run both in one launch)"""
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, level_launches=True)
    plan.fill_synthetic(1, spec["scales"])
    for _ in range(3):
        plan.propagate()
    plan.set_profiling(5)
    for _ in range(5):
        plan.propagate()
    ms = plan.stats()["collect_ms"]
    plan.close()
    return ms


def timed(spec, dtype, n_sets, label, collect):
    opts = dict(n_batch=n_sets, share_potentials=True) if n_sets > 1 else {}
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype, **opts)
    plan.fill_synthetic(1, spec["scales"])
    sched = plan.describe()["sample"]
    itemsize = 4 if plan.dtype == _capi.JTP_F32 else 8
    entries = sum(c["R"] * int(np.prod([plan.card[v] for v in c["K"]], dtype=np.int64)) for c in sched["cliques"])
    table_bytes = float(entries) * itemsize
    print("%s: %d cliques on %d depths, largest slice %d entries, %.1f MB of tables;  collect of the propagate (one launch per level) %.3f ms"
          % (label, len(sched["cliques"]), len(sched["depths"]), max(c["R"] for c in sched["cliques"]), table_bytes * 1e-6, collect))
    first = None
    for seg in SEGS:
        plan.debug_set("map_seg", seg)                       # (0: the library's segment length; the records are built again)
        plan.map()                                           # (records uploaded, work area allocated)
        wall, dev = float("inf"), float("inf")
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            plan.region_begin()
            states, value = plan.map()
            dev = min(dev, plan.region_end())
            wall = min(wall, (time.perf_counter() - t0) * 1e3)
        assert states.min() >= 0
        first = states if first is None else first
        assert np.array_equal(states, first)                 # (the cut of r changes nothing)
        print("%s: %d sets, segments of %s entries:  jtp_map device %.3f ms (%.3f ms per set, %.1f GB/s of tables), whole call %.3f ms;  map / collect per set %.2f"
              % (label, n_sets, seg or "default", dev, dev / n_sets, table_bytes * n_sets / dev * 1e-6, wall, dev / n_sets / collect))
    plan.close()


print("# library build:", _capi.lib().jtp_version().decode())
wide = synthetic.wide_binary_tree(63, width=20, sep=10)
c = collect_ms(wide, "f32")
timed(wide, "f32", 1, "wide_binary_tree(63, width=20, sep=10) f32", c)
timed(wide, "f32", 64, "wide_binary_tree(63, width=20, sep=10) f32", c)
chain = synthetic.chain_tree(200, card=16, width=3)
timed(chain, "f64", 1, "chain_tree(200, card=16, width=3) f64", collect_ms(chain, "f64"))
