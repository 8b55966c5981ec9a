"""sha256 of what the queries on the sampling schedule return (`Plan.sample`, `Plan.map`, `Plan.max_marginals`, `Plan.map_best`,
`Plan.joint`) on the shapes their GPU tests use, float32 and float64, the default plan and `no_compact=True`: two builds of the library that print the same lines answer
these queries bit for bit alike (`JTPROP_LIB=<other build> python tools/query_digest.py` for the second column).  Needs a GPU.  The
beliefs the samples and the joints are formed from are hashed first, so that a difference in the propagate is told from one in a query.

    python tools/query_digest.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("junction-tree_amd", "oracle", "tests"):             # (as tests/conftest.py sets the path: the test modules import each other)
    sys.path.insert(0, os.path.join(ROOT, p))

from junctiontree_amd import _capi, engine                    # noqa: E402
from max_reference import factor_requests                     # noqa: E402   (the requests of the max-propagation tests)
from test_gpu_joint import case, queries                      # noqa: E402   (the cases and the queries of the tests, "star12" among them)

N_SETS = 5
# (root64k: a root whose slice has 2^16 entries - jt_map_merge runs on it, and jt_joint_merge for a query that leaves 2^14 of them to sum)
CASES = ["wide7", "chain6", "star12", "random16_card3", "random16_mixed", "root64k"]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode() + a.tobytes())
    return h.hexdigest()


def digests(name, dtype, opts):
    tree, pots, node_vars, sizes, n = case(name)
    tag = "%s %s%s" % (name, dtype, " no_compact" if opts else "")
    np_t = np.float32 if dtype == "f32" else np.float64
    plan = engine.Plan(tree, node_vars, sizes, dtype=dtype, n_batch=N_SETS, **opts)
    labels = sorted(sizes)
    for b in range(N_SETS):
        for c in range(n):
            plan.set_potential(c, np.asarray(pots[c], dtype=np_t), batch=b)
        # set 0 observes nothing (the samples and the joints are its); set b observes b variables
        plan.set_evidence({labels[(5 * i + 3 * b) % len(labels)]: (i + b) % sizes[labels[(5 * i + 3 * b) % len(labels)]] for i in range(b)}, batch=b)
    plan.propagate()
    print("%-44s %s" % (tag + " beliefs", sha(*[plan.belief(c, dtype=np_t) for c in range(n)])), flush=True)
    print("%-44s %s" % (tag + " sample", sha(plan.sample(4096, seed=7))), flush=True)
    plan.debug_set("map_chunk", 2)
    states, log_value = plan.map()
    print("%-44s %s" % (tag + " map", sha(states, log_value)), flush=True)
    tables, log2_scale, log_value = plan.max_marginals(factor_requests(plan))      # (every clique; the five sets in chunks of two)
    print("%-44s %s" % (tag + " max_marginals", sha(*[t for per_set in tables for t in per_set], log2_scale, log_value)), flush=True)
    for m in (1, 5, 16):
        for b in (0, N_SETS - 1):                              # (the set that observes nothing, the set that observes the most)
            print("%-44s %s" % (tag + " map_best %d set %d" % (m, b), sha(*plan.map_best(m, batch=b))), flush=True)
    if name == "root64k":
        root_vars = plan.describe()["sample"]["cliques"][0]["F"]
        asked = {"two_of_the_root": [plan.var_labels[v] for v in root_vars[:2]]}
    else:
        asked = queries(name)
    for key, query in asked.items():
        table, e = plan.joint(query)
        print("%-44s %s" % (tag + " joint " + key, sha(table, np.int64(e))), flush=True)
    plan.close()


def main():
    print("# library build:", _capi.lib().jtp_version().decode())
    for name in CASES:
        for dtype in ("f32", "f64"):
            for opts in ({}, dict(no_compact=True)):
                digests(name, dtype, opts)


if __name__ == "__main__":
    main()
