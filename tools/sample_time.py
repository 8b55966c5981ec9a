"""What joint sampling on the device costs (`jtp_sample`, `engine.Plan.sample`): samples per second and the bytes of belief
tables the draws gather per second - N * sum over the cliques of R_c * sizeof(T), R_c the entries of one conditional slice - on
the shape of BASELINE config 4 cut to 63 cliques (float32) and on a chain of small cliques (float64), N = 4096 samples.  The time
is that of the whole call: state rows cleared, one launch per depth of the tree, the states copied to the host.

    python tools/sample_time.py [n_samples] [repeats]
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, engine, synthetic

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def timed(spec, dtype, label):
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype=dtype)
    plan.fill_synthetic(1, spec["scales"])
    plan.propagate()
    sched = plan.describe()["sample"]
    entries = sum(c["R"] for c in sched["cliques"])
    gathered = float(N) * entries * (4 if plan.dtype == _capi.JTP_F32 else 8)
    plan.sample(N, seed=1)                                   # (records uploaded, state buffer allocated)
    wall, dev = float("inf"), float("inf")
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        plan.region_begin()
        states = plan.sample(N, seed=1)
        dev = min(dev, plan.region_end())
        wall = min(wall, (time.perf_counter() - t0) * 1e3)
    assert states.min() >= 0
    print("%s: %d cliques on %d depths, largest slice %d entries, %d entries per sample in all"
          % (label, len(sched["cliques"]), len(sched["depths"]), max(c["R"] for c in sched["cliques"]), entries))
    print("%s: N = %d  device %.3f ms = %.3g samples/s, %.1f GB/s gathered;  whole call %.3f ms = %.3g samples/s"
          % (label, N, dev, N / dev * 1e3, gathered / dev * 1e-6, wall, N / wall * 1e3))
    plan.close()


print("# library build:", _capi.lib().jtp_version().decode())
timed(synthetic.wide_binary_tree(63, width=20, sep=10), "f32", "wide_binary_tree(63, width=20, sep=10) f32")
timed(synthetic.chain_tree(200, card=16, width=3), "f64", "chain_tree(200, card=16, width=3) f64")
