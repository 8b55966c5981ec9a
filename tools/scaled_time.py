"""What the overflow-safe propagate (JTP_SCALED: `engine.Plan(scaled=True)`) costs: device time per propagate of a scaled plan, of
the same plan launched per level without the flag (its yardstick) and of the default dataflow plan, on the shape of BASELINE
config 4 and on the config-3 lattice, with in-range inputs; the number of rescale launches and the overhead per launch.

    python tools/scaled_time.py [c4_cliques] [c3_width] [propagates]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
import junctiontree_amd as jt
from junctiontree_amd import _capi, engine, synthetic

N4 = int(sys.argv[1]) if len(sys.argv) > 1 else 256
W3 = int(sys.argv[2]) if len(sys.argv) > 2 else 167
K = int(sys.argv[3]) if len(sys.argv) > 3 else 50


def timed(make, fill, label):
    rows = {}
    for name, opts in (("default", {}), ("level", {"level_launches": True}), ("scaled", {"scaled": True})):
        plan = make(**opts)
        fill(plan)
        for _ in range(5):
            plan.propagate()
        best = float("inf")
        for _ in range(3):
            plan.region_begin()
            for _ in range(K):
                plan.propagate(sync=False)
            best = min(best, plan.region_end() / K)
        d = plan.describe()
        rows[name] = (best, plan.stats()["n_launches"], sum(1 for kind, _, _ in d["steps"] if kind == 2), plan.log_z()[1])
        plan.close()
    n_rescale = rows["scaled"][2]
    over = rows["scaled"][0] - rows["level"][0]
    print("%s: default %.4f ms (%d launches)  per level %.4f ms (%d launches)  scaled %.4f ms (%d launches, %d of them rescale)"
          % (label, rows["default"][0], rows["default"][1], rows["level"][0], rows["level"][1], rows["scaled"][0], rows["scaled"][1], n_rescale))
    print("%s: scaled - per level = %+.4f ms = %+.2f %%, %.2f us per rescale launch; log Z %.6f (scaled) %.6f (per level)"
          % (label, over, 100.0 * over / rows["level"][0], 1e3 * over / max(n_rescale, 1), rows["scaled"][3], rows["level"][3]))


print("# library build:", _capi.lib().jtp_version().decode())
spec = synthetic.wide_binary_tree(n_cliques=N4, width=20, sep=10, card=2, seed=0)
timed(lambda **o: engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f32", **o),
      lambda plan: plan.fill_synthetic(1, spec["scales"]), "config-4 shape (%d cliques, f32)" % N4)
factors, sizes, _ = synthetic.lattice_mrf(6, W3, 8)
tree = jt.create_junction_tree(factors, sizes)
cliques = tree.clique_tree.maxcliques
node_vars = [list(c) for c in cliques] + [list(s) for s in tree.separators]
timed(lambda **o: engine.Plan(tree.tree, node_vars, sizes, dtype="f32", **o),
      lambda plan: plan.fill_synthetic(1, [8.0 ** -(len(c) - 1) for c in cliques]), "config-3 lattice (6 x %d, f32, every table stored)" % W3)
