"""What expected counts cost beside the propagate (`jtp_accumulate_marginals`, `engine.Plan.factor_counts`), on the tree of
`bench.py --batch 64 --multiset`: wide_binary_tree(256, width=20, sep=10), float32 tables, S evidence sets of 16 observed variables
each (the benchmark's seeds).  The request list is that of a pairwise model laid over the tree, three "factors" per clique:
(v0, v1), (v2, v3) and (v4) of the clique's variables - 768 requests, 2560 entries in all.  Three figures, wall clock of the whole
step, best and median of the repeats:

    (a) the propagate alone, waited for;
    (b) the route without this entry point: the propagate, then `factor_marginals(batch=b)` for every set, every table divided by
        its own sum and added on the host (`_normalised`, numpy);
    (c) the propagate, then one `factor_counts` call.

    python tools/counts_time.py [sets] [repeats]          (-> profiles/counts_time.txt)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, engine, synthetic      # noqa: E402
from junctiontree_amd.junctiontree import _normalised      # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 7

print("# library build:", _capi.lib().jtp_version().decode())
spec = synthetic.wide_binary_tree(n_cliques=256, width=20, sep=10, card=2, seed=0)
plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f32", n_batch=S, multiset=True)
plan.fill_synthetic(1, spec["scales"])
names = sorted(spec["sizes"])
for b in range(S):
    rng = np.random.default_rng(1000 + b)
    plan.set_evidence({names[i]: int(rng.integers(0, spec["sizes"][names[i]])) for i in rng.choice(len(names), size=16, replace=False)}, batch=b)
labels, cliques = [], []
for c in range(spec["n_cliques"]):
    v = list(spec["node_vars"][c])
    labels += [v[0:2], v[2:4], v[4:5]]
    cliques += [c, c, c]
print("# wide_binary_tree(256, width=20, sep=10) f32, multi-set plan, %d evidence sets x 16 observed variables; %d requests "
      "((v0, v1), (v2, v3), (v4) of every clique), %d entries" % (S, len(labels), sum(2 ** len(l) for l in labels)))


def propagate_only():
    plan.propagate(sync=True)


def host_route():
    plan.propagate(sync=False)
    total = None
    for b in range(S):
        tables = _normalised(plan.factor_marginals(labels, cliques, batch=b))
        total = tables if total is None else [t + u for t, u in zip(total, tables)]
    return total


def device_route():
    plan.propagate(sync=False)
    return plan.factor_counts(labels, cliques)[0]


def timed(fn):
    fn()
    fn()                                                     # (tables built, buffers allocated)
    ms = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), float(np.median(ms)), out


a = timed(propagate_only)
b = timed(host_route)
c = timed(device_route)
worst = max(float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-30))) for x, y in zip(c[2], b[2]))
print("(a) propagate alone:                                   best %8.3f ms   median %8.3f ms" % a[:2])
print("(b) propagate + %3d x factor_marginals + host sums:     best %8.3f ms   median %8.3f ms   (read-out: %.3f ms)" % (S, b[0], b[1], b[1] - a[1]))
print("(c) propagate + factor_counts (on the device):         best %8.3f ms   median %8.3f ms   (read-out: %.3f ms)" % (c[0], c[1], c[1] - a[1]))
print("(c) / (b), medians: %.3f;  largest relative difference between the two routes' counts: %.2e" % (c[1] / b[1], worst))
plan.close()
