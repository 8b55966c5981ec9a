"""sha256 of what the planner makes of the benchmark's shapes (`Plan(..., plan_only=True).describe()`, no GPU needed): two builds
of the library that print the same lines plan these trees alike.  The planner's fuzz harness (tests/fuzz/fuzz_plan.cpp, third
argument `digest`) does the same for thousands of small random trees; these are the shapes it is too small for.

    python tools/plan_digest.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "junction-tree_amd"))

import junctiontree_amd as jt                                  # noqa: E402
from junctiontree_amd import engine, partition, synthetic     # noqa: E402


def digest(name, *args, **kwargs):
    plan = engine.Plan(*args, plan_only=True, **kwargs)
    text = json.dumps(plan.describe(), sort_keys=True)
    plan.close()
    print("%-24s %s" % (name, hashlib.sha256(text.encode()).hexdigest()), flush=True)


def main():
    c4 = synthetic.wide_binary_tree(n_cliques=256, width=20, sep=10, card=2, seed=0)       # bench.py's default
    shape = (c4["tree"], c4["node_vars"], c4["sizes"])
    digest("c4 f32", *shape, dtype="f32")
    digest("c4 f64", *shape, dtype="f64")
    c2 = synthetic.chain_tree(n_cliques=1000, card=64, width=3)                             # --config c2
    digest("c2 f64", c2["tree"], c2["node_vars"], c2["sizes"], dtype="f64")
    # --config c3 as bench.py's sub_c3 plans it: the API's plan, with the cover and the factor marginals named ahead
    factors, sizes, _ = synthetic.lattice_mrf(6, 167, 8)
    tree = jt.create_junction_tree(factors, sizes)
    ct = tree.clique_tree
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]
    fold = (tuple(ct.factor_to_maxclique), tuple(map(tuple, ct.factor_graph.factors)))
    digest("c3 f32 cover fold", tree.tree, node_vars, sizes, dtype="f32", cover=tree.cover(), fold=fold)
    digest("c3 f32 cover", tree.tree, node_vars, sizes, dtype="f32", cover=tree.cover())
    # (the column-sweep tree of the same lattice: its narrow levels are where the planner does fold the marginals)
    tree = jt.create_junction_tree(factors, sizes, order=synthetic.lattice_column_order(6, 167))
    ct = tree.clique_tree
    node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in tree.separators]
    fold = (tuple(ct.factor_to_maxclique), tuple(map(tuple, ct.factor_graph.factors)))
    digest("c3 sweep f32 cover fold", tree.tree, node_vars, sizes, dtype="f32", cover=tree.cover(), fold=fold)
    digest("c3 sweep f32 cover", tree.tree, node_vars, sizes, dtype="f32", cover=tree.cover())
    digest("c4 multiset 64", *shape, dtype="f32", n_batch=64, multiset=True)                # --batch 64 --multiset
    root, _, owner = partition.partition_tree(c4["parent"], [1.0] * c4["n_cliques"], 8, replicate_top=True)
    for rank in (0, 7):
        digest("c4 rank %d of 8" % rank, *shape, dtype="f32", n_ranks=8, rank=rank, owner=owner, root=root)
    digest("c4 scaled", *shape, dtype="f32", scaled=True)


if __name__ == "__main__":
    main()
