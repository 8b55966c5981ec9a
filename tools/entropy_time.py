"""What the entropy of a posterior costs on the device (`jtp_entropy`, `engine.Plan.entropy`): repeated calls bracketed with
`jtp_region_begin` / `jtp_region_end`, after a propagate, beside the same plan's propagate timed the same way in the same process.

  config4   the shape of BASELINE config 4 (256 cliques x 2^20 float32, synthetic fill), in the default layout and with
            `layout_policy=3`; the implied bytes/s of belief traffic (one read of every clique table); with a reference set (two
            tables read); and the route a caller had before: `Plan.belief` of every clique into pinned memory and the one-pass
            formula in numpy, same plan, same process
  sets      64 evidence sets over shared tables on a chain of 64^3 cliques (config 2 cut to a length that fits beside other work):
            ms per set in one call against 64 calls of one set

    python tools/entropy_time.py [config4|config4_dev|config4_p3|sets|all] [repeats]      (config4_dev: without the host route, for runs under a profiler)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "junction-tree_amd"))
from junctiontree_amd import _capi, engine, synthetic

WHAT = sys.argv[1] if len(sys.argv) > 1 else "all"
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 7


def region(plan, fn, inner=1):
    """best device time of `inner` calls of fn between the two events, per call, in ms"""
    out = float("inf")
    for _ in range(REPEATS):
        plan.region_begin()
        for _ in range(inner):
            fn()
        out = min(out, plan.region_end() / inner)
    return out


def host_route(plan, spec, bufs):
    """every belief into pinned memory, then per clique sum b ln b - sum sigma ln sigma over S, in float64"""
    sched = plan.describe()["sample"]["cliques"]
    total = 0.0
    for c in sched:
        node = plan.node_ids[c["clique"]]
        b = plan.belief(node, out=bufs[node])
        axes = [plan.var_id[lab] for lab in plan.node_vars[node]]
        order = [axes.index(v) for v in c["K"]] + [axes.index(v) for v in c["F"]]
        rows = np.transpose(b, order).reshape(-1, int(c["R"])).astype(np.float64)
        sig = rows.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(rows > 0, rows * np.log(rows), 0.0).sum() - np.where(sig > 0, sig * np.log(sig), 0.0).sum()
        total += -t / sig.sum()
    return total


def config4(label, host=True, **opts):
    spec = synthetic.wide_binary_tree(n_cliques=256, width=20, sep=10, card=2, seed=0)
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f32", n_batch=2, share_potentials=True, **opts)
    plan.fill_synthetic(1, spec["scales"])
    some = sorted(spec["sizes"])
    plan.set_evidence({some[3]: 1, some[40]: 0}, batch=1)
    plan.propagate()
    n = spec["n_cliques"]
    bel_bytes = sum(int(np.prod(plan.node_shape[c])) for c in range(n)) * 4
    h = plan.entropy(0, 1)[0]                                # (records and work area allocated)
    plan.entropy(1, 2, ref=0)
    prop_ms = region(plan, lambda: plan.propagate(0, 1, sync=False))
    plan.sync()
    ent_ms = region(plan, lambda: plan.entropy(0, 1))
    ent4_ms = region(plan, lambda: plan.entropy(0, 1), inner=4)
    ref_ms = region(plan, lambda: plan.entropy(1, 2, ref=0))
    t0 = time.perf_counter()
    plan.entropy(0, 1)
    call_ms = (time.perf_counter() - t0) * 1e3
    print("%s: %d cliques, %.1f MiB of beliefs;  propagate %.3f ms;  jtp_entropy %.3f ms device (%.3f per call over 4 calls, whole call %.3f ms wall), "
          "ratio to the propagate %.2f, %.0f GB/s of belief traffic;  with a reference set %.3f ms, %.0f GB/s over both tables;  H = %.6f nats"
          % (label, n, bel_bytes / 2 ** 20, prop_ms, ent_ms, ent4_ms, call_ms, ent_ms / prop_ms, bel_bytes / ent_ms / 1e6, ref_ms, 2 * bel_bytes / ref_ms / 1e6, h))
    if host:
        bufs = {c: engine.pinned_empty(plan.node_shape[c], dtype=np.float32) for c in range(n)}
        t0 = time.perf_counter()
        for c in range(n):
            plan.belief(c, out=bufs[c])
        copy_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        h_host = host_route(plan, spec, bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
        print("%s: the host route: %d beliefs into pinned memory %.1f ms (%.1f GB/s), with the numpy formula %.0f ms;  %.0f x the device call;  "
              "the two entropies differ by %.2g nats" % (label, n, copy_ms, bel_bytes / copy_ms / 1e6, host_ms, host_ms / call_ms, abs(h_host - h)))
    plan.close()


def sets():
    spec = synthetic.chain_tree(n_cliques=100, card=64, width=3)
    n_sets = 64
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f64", n_batch=n_sets, share_potentials=True)
    plan.fill_synthetic(1, spec["scales"])
    for b in range(n_sets):
        plan.set_evidence({(b * 7) % 102: b % 64} if b else {}, batch=b)
    plan.propagate()
    h = plan.entropy()
    one = region(plan, lambda: plan.entropy())
    each = region(plan, lambda: [plan.entropy(b, b + 1) for b in range(n_sets)])
    single = np.array([plan.entropy(b, b + 1)[0] for b in range(n_sets)])
    print("chain_tree(100, card=64, width=3) f64, %d evidence sets over shared tables (%.0f MiB of beliefs a set): one call %.3f ms = %.4f ms a set;  "
          "%d calls of one set %.3f ms = %.4f ms a set;  ratio %.2f;  bit-equal: %s;  H from %.4f to %.4f nats"
          % (n_sets, 100 * 64 ** 3 * 8 / 2 ** 20, one, one / n_sets, n_sets, each, each / n_sets, each / one, bool(np.array_equal(single, h)), h.min(), h.max()))
    plan.close()


print("# library build: %s;  %s, best of %d" % (_capi.lib().jtp_version().decode(), WHAT, REPEATS))
if WHAT in ("config4", "config4_dev", "all"):
    config4("wide_binary_tree(256, width=20, sep=10) f32, default layout", host=WHAT != "config4_dev")
if WHAT in ("config4_p3", "all"):
    config4("wide_binary_tree(256, width=20, sep=10) f32, layout_policy=3", host=False, layout_policy=3)
if WHAT in ("sets", "all"):
    sets()
