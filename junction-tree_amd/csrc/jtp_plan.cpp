// Host planner: junction tree description -> bit layouts, kernel task tables, level
// schedule, message buffers, separator exchange schedule.  Pure C++ (no HIP calls), so it
// also runs in JTP_PLAN_ONLY mode on machines without a GPU.
//
// Replaces, for the whole tree at once, what the reference does per einsum call:
//   label -> axis-number remapping          junctiontree/sum_product.py:22-43
//   recursion order of collect / distribute junctiontree/computation.py:47-96, 140-224
// and removes `remove_message` (computation.py:99-136): every downward message is planned
// as an all-but-one product, never as a division.
#include "jtp_plan_build.h"

PlanKnobs jtp_read_knobs() {
    PlanKnobs k;
    auto geti = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
    auto getd = [](const char *name, double dflt) { const char *v = getenv(name); return v ? atof(v) : dflt; };
    k.debug = geti("JTP_DEBUG", 0);
    k.layout_policy = geti("JTP_LAYOUT_POLICY", -1);
    k.reduce_min = geti("JTP_REDUCE_MIN", -1);
    k.target_blocks_c = getd("JTP_TARGET_BLOCKS", 1024.0);
    k.target_set = getenv("JTP_TARGET_BLOCKS") != nullptr;
    k.target_blocks_d = getd("JTP_TARGET_BLOCKS_D", k.target_blocks_c);
    k.min_block_log2 = geti("JTP_MIN_BLOCK_LOG2", 13);
    k.multi_min_block_log2 = geti("JTP_MULTI_MIN_BLOCK_LOG2", 16);
    k.max_block_log2 = geti("JTP_MAX_BLOCK_LOG2", 16);
    k.max_block_log2_d = geti("JTP_MAX_BLOCK_LOG2_D", std::min(k.max_block_log2, 15));
    k.tiny_level_elems = getd("JTP_TINY_LEVEL_ELEMS", 2097152.0);
    k.force_level_launches = geti("JTP_FORCE_LEVEL_LAUNCHES", 0);
    k.force_flow = geti("JTP_FORCE_FLOW", 0);
    k.fake_comm = geti("JTP_FAKE_COMM", 0);
    k.flow_debug = (unsigned)geti("JTP_FLOW_DEBUG", 0);
    k.flow_tickets = geti("JTP_FLOW_TICKETS", 0);
    k.no_compact = geti("JTP_NO_COMPACT", 0);
    k.no_search = geti("JTP_NO_SEARCH", 0);
    k.search_all = geti("JTP_SEARCH_ALL", 1);
    k.roctx = geti("JTP_ROCTX", 0);
    k.merge_phases = geti("JTP_MERGE_PHASES", -1);
    k.no_tmix = geti("JTP_NO_TMIX", 0);
    k.tmix_fill = getd("JTP_TMIX_FILL", 0.6);
    k.no_tsplit = geti("JTP_NO_TSPLIT", 0);
    k.settle_level_elems = getd("JTP_SETTLE_LEVEL_ELEMS", 8388608.0);
    k.top_min_loop = geti("JTP_TOP_MIN_LOOP", 3);
    k.lane_low = geti("JTP_LANE_LOW", 2);
    k.longest_first = geti("JTP_LONGEST_FIRST", 1);
    k.top_share = getd("JTP_TOP_SHARE", 0.12);
    k.top_rows2 = getd("JTP_TOP_ROWS2", 2048.0);
    k.top_loop2 = geti("JTP_TOP_LOOP2", 2);
    k.keep_rows_mb = getd("JTP_KEEP_ROWS_MB", k.keep_rows_mb);
    k.keep_top = geti("JTP_KEEP_TOP", k.keep_top);
    k.keep_bw = getd("JTP_KEEP_BW", k.keep_bw);
    k.esum_always = geti("JTP_EXPERIMENT_ESUM_ALWAYS", 0);
    k.marg_group = std::max(1, std::min(geti("JTP_MARG_GROUP", JT_MAX_OUT), JT_MAX_OUT));
    k.marg_block_log2 = geti("JTP_MARG_BLOCK_LOG2", 0);
    k.no_unit = geti("JTP_NO_UNIT", 0);
    k.keep_invalid = geti("JTP_KEEP_INVALID", 0);
    k.no_vgroups = geti("JTP_NO_VGROUPS", 0);
    k.unit_joint_down = geti("JTP_UNIT_JOINT_DOWN", 0);
    k.no_ef_share = geti("JTP_EF_SHARE", 0) ? -1 : geti("JTP_NO_EF_SHARE", 0);      // (-1: the evidence-free group whatever the number of sets)
    k.unit_ratio = getd("JTP_UNIT_RATIO", 4.0);
    k.no_lean = geti("JTP_NO_LEAN", 0);
    k.no_fold = geti("JTP_NO_FOLD", 0);
    k.fold = geti("JTP_FOLD", -1);
    if (k.fold == 0) k.no_fold = 1;
    k.fold_slots = geti("JTP_FOLD_SLOTS", 1024);
    k.fail_alloc = std::max(0, geti("JTP_FAIL_ALLOC", 0));
    return k;
}

int PlanBuilder::block_log2_for(int phase, int level, int owner, bool tiny_rule) const {
        if (hp.block_log2 > 0) return std::max(hp.block_log2, hp.TB);
        // aim at ~1024 workgroups per tree level (one round of resident workgroups; in a dataflow launch
        // the next level fills the tail), each streaming 16 KiB .. 256 KiB.  Measured on C4: 1024 is
        // 2-3 % faster than 2048 (which was best with one launch per level), 512 and 4096 slower.
        // (plans whose elements are mostly those of unit cliques - no rows to stream, a workgroup is sub-boxes and arithmetic - do
        //  better with twice the workgroups per level: config 3 8.98 -> 8.63 ms, A/B on one box; 4096: 10.9)
        const double target = (phase == 0 ? hp.knobs.target_blocks_c : hp.knobs.target_blocks_d) * (hp.unit_dominated && !hp.knobs.target_set ? 2.0 : 1.0);
        // (the distribute pass - read + write - streams best in workgroups of at most 32 rows: config 4 0.4345 -> 0.4300 ms,
        //  the collect pass in up to 64: 0.2055 against 0.2084 ms; multi-set plans - whose second phase is marginalisations,
        //  not a read + write pass - keep 64: 1.058 against 1.074 ms)
        // (multi-set plans: always the 64 rows a workgroup can hold - a step serves eight evidence sets, so a workgroup's fixed
        //  cost, eight sets' sub-boxes staged through 8-byte loads, weighs more against its loop than in single-set plans:
        //  64 evidence sets 6.73 -> 6.11 ms, env sweep on one box; 512 / 256 / 128 workgroups per level as the target:
        //  6.33 / 6.16 / 6.11;
        //  one group of eight sets alone is too few workgroups for that: 1.03 -> 1.13 ms; 16 sets 1.82 -> 1.80)
        const int lgmin = hp.multiset && hp.n_batch > JT_MSETS ? hp.knobs.multi_min_block_log2 : hp.knobs.min_block_log2;
        const int lgmax = phase == 1 && !hp.multiset ? hp.knobs.max_block_log2_d : hp.knobs.max_block_log2;
        // levels of a clique or two are latency bound: 4 iterations per workgroup, so that every element
        // load is already in flight while the workgroup waits for its messages
        const double tiny = hp.knobs.tiny_level_elems;
        // (searched layouts price a lone workgroup's latency themselves: config 2 6.87 -> 6.49 ms without the rule)
        if (tiny_rule && lvl_elems[phase][owner][level] <= tiny) return hp.TB + JT_MIN_ITER_LOG2;
        double want = lvl_elems[phase][owner][level] / target;
        int lg = lgmin;
        while (lg < lgmax && (double)(1 << (lg + 1)) <= want) ++lg;
        return std::max(lg, hp.TB);
    }

int PlanBuilder::read_description() {
    if (!d) FAIL(JTP_EINVAL, "null description");
    hp.knobs = jtp_read_knobs();
    if (d->struct_size != (int32_t)sizeof(jtp_tree_desc))
        FAIL(JTP_EINVAL, "jtp_tree_desc size mismatch (%d vs %zu)", d->struct_size, sizeof(jtp_tree_desc));
    if (d->n_cliques < 1 || d->n_vars < 0) FAIL(JTP_EINVAL, "empty tree");
    if (d->n_nodes != 2 * d->n_cliques - 1)
        FAIL(JTP_EINVAL, "n_nodes must be 2*n_cliques-1 (got %d for %d cliques)", d->n_nodes, d->n_cliques);
    if (d->dtype != JTP_F32 && d->dtype != JTP_F64) FAIL(JTP_EINVAL, "bad dtype %d", d->dtype);
    if (d->n_batch < 1) FAIL(JTP_EINVAL, "n_batch must be >= 1");
    if (d->n_ranks < 1 || d->rank < 0 || d->rank >= d->n_ranks) FAIL(JTP_EINVAL, "bad rank %d/%d", d->rank, d->n_ranks);

    hp.n_vars = d->n_vars;
    hp.n_cliques = d->n_cliques;
    hp.n_nodes = d->n_nodes;
    hp.dtype = d->dtype;
    hp.n_ranks = d->n_ranks;
    hp.rank = d->rank;
    hp.n_batch = d->n_batch;
    hp.device = d->device;
    hp.flags = d->flags;
    hp.lds_budget = d->lds_budget;
    hp.block_log2 = d->block_log2;
    hp.layout_policy = d->layout_policy;
    if (hp.knobs.layout_policy >= 0) hp.layout_policy = hp.knobs.layout_policy;               // experiments
    hp.compact = !hp.knobs.no_compact && !(d->flags & JTP_NO_COMPACT);
    hp.multiset = (d->flags & JTP_MULTISET) != 0;
    hp.scaled = (d->flags & JTP_SCALED) != 0;
    if (hp.scaled) {
        if (hp.multiset) FAIL(JTP_EUNSUPPORTED, "JTP_SCALED with JTP_MULTISET: scaled multi-set plans are not built (share the potentials without JTP_MULTISET)");
        if (d->n_ranks != 1) FAIL(JTP_EUNSUPPORTED, "JTP_SCALED with n_ranks = %d: scaled multi-rank plans are not built", d->n_ranks);
        hp.flags |= JTP_LEVEL_LAUNCHES;            // the rescale steps sit between the levels: no dataflow launches
    }
    if (hp.multiset) {
        if (d->n_ranks != 1) FAIL(JTP_EUNSUPPORTED, "multi-set plans run on one rank (evidence sets are independent: give every rank its own sets)");
        // Bit order: "epilogue first" (3) measured 2x faster than "traffic first" (2) on the width-20 tree (fewer
        // epilogues per row; its sub-boxes still fit the 4 KiB regions).  jtp_plan_create falls back to 2 - the
        // smallest sub-boxes - when a clique's sub-boxes do not fit one evidence set's LDS region under 3.
        if (hp.layout_policy == 0) hp.layout_policy = 3;
    }
    hp.VEC = d->dtype == JTP_F32 ? 4 : 2;
    hp.EB = d->dtype == JTP_F32 ? 2 : 1;
    hp.TB = hp.EB + 8;
    N = d->n_cliques;
    esize = d->dtype == JTP_F32 ? 4 : 8;

    if ((d->n_vars > 0 && !d->var_card) || !d->node_var_off || !d->parent_clique || !d->parent_sep)
        FAIL(JTP_EINVAL, "null array in the description");
    hp.card.assign(d->var_card, d->var_card + d->n_vars);
    hp.vbits.resize(d->n_vars);
    for (int v = 0; v < d->n_vars; ++v) {
        if (hp.card[v] < 1) FAIL(JTP_EINVAL, "variable %d has cardinality %d", v, hp.card[v]);
        if (hp.card[v] > (1 << 28)) FAIL(JTP_EUNSUPPORTED, "variable %d has cardinality %d (max 2^28)", v, hp.card[v]);
        hp.vbits[v] = ceil_log2(hp.card[v]);
    }
    hp.node_vars.resize(d->n_nodes);
    // (the CSR offsets are the only bound on node_var_ids this ABI has: they must start at 0 and never decrease)
    if (d->node_var_off[0] != 0) FAIL(JTP_EINVAL, "node_var_off[0] must be 0 (got %d)", d->node_var_off[0]);
    if (d->node_var_off[d->n_nodes] > 0 && !d->node_var_ids) FAIL(JTP_EINVAL, "null array in the description");
    for (int n = 0; n < d->n_nodes; ++n) {
        int a = d->node_var_off[n], b = d->node_var_off[n + 1];
        if (a < 0 || b < a) FAIL(JTP_EINVAL, "node_var_off decreases at node %d (%d, %d)", n, a, b);
        if (b - a > JT_MAX_VARS) FAIL(JTP_EUNSUPPORTED, "node %d has %d variables (max %d)", n, b - a, JT_MAX_VARS);
        for (int i = a; i < b; ++i) {
            int v = d->node_var_ids[i];
            if (v < 0 || v >= d->n_vars) FAIL(JTP_EINVAL, "node %d: unknown variable %d", n, v);
            if (find_var(hp.node_vars[n], v) >= 0) FAIL(JTP_EINVAL, "node %d: variable %d listed twice", n, v);
            hp.node_vars[n].push_back(v);
        }
    }
    if (d->fold_n < 0 || (d->fold_n > 0 && (!d->fold_cliques || !d->fold_var_off))) FAIL(JTP_EINVAL, "null array in the description (fold_*)");
    if (d->fold_n > 0) {
        if (d->fold_var_off[0] != 0) FAIL(JTP_EINVAL, "fold_var_off[0] must be 0");
        for (int i = 0; i < d->fold_n; ++i) {
            const int c = d->fold_cliques[i], a = d->fold_var_off[i], b = d->fold_var_off[i + 1];
            if (c < 0 || c >= N) FAIL(JTP_EINVAL, "fold request %d: node %d is not a clique", i, c);
            if (b < a || b - a > JT_MAX_VARS || (b > a && !d->fold_var_ids)) FAIL(JTP_EINVAL, "fold request %d: bad variable list", i);
            for (int k = a; k < b; ++k)
                if (d->fold_var_ids[k] < 0 || d->fold_var_ids[k] >= hp.n_vars) FAIL(JTP_EINVAL, "fold request %d: variable %d out of range", i, d->fold_var_ids[k]);
        }
        hp.fold_cliques.assign(d->fold_cliques, d->fold_cliques + d->fold_n);
        hp.fold_var_off.assign(d->fold_var_off, d->fold_var_off + d->fold_n + 1);
        hp.fold_var_ids.assign(d->fold_var_ids, d->fold_var_ids + d->fold_var_off[d->fold_n]);
        // (the key jtp_get_marginals makes of a request list: n, cliques, offsets, variables)
        hp.fold_key.push_back(d->fold_n);
        hp.fold_key.insert(hp.fold_key.end(), hp.fold_cliques.begin(), hp.fold_cliques.end());
        hp.fold_key.insert(hp.fold_key.end(), hp.fold_var_off.begin(), hp.fold_var_off.end());
        hp.fold_key.insert(hp.fold_key.end(), hp.fold_var_ids.begin(), hp.fold_var_ids.end());
        hp.folded.assign((size_t)d->fold_n, HostPlan::FoldReq());
    }
    hp.lean = d->cover_off != nullptr && !hp.multiset;
    if (d->cover_off) {
        // (validated for every plan that passes them, used by single-set plans)
        if (d->cover_off[0] != 0) FAIL(JTP_EINVAL, "cover_off[0] must be 0 (got %d)", d->cover_off[0]);
        if (d->cover_off[N] > 0 && !d->cover_ids) FAIL(JTP_EINVAL, "null array in the description");
        hp.cover.assign(N, std::vector<int>());
        for (int c = 0; c < N; ++c) {
            const int a = d->cover_off[c], b = d->cover_off[c + 1];
            if (a < 0 || b < a || b - a > JT_MAX_VARS) FAIL(JTP_EINVAL, "cover_off decreases at clique %d (%d, %d)", c, a, b);
            for (int i = a; i < b; ++i) {
                const int v = d->cover_ids[i];
                if (v < 0 || v >= d->n_vars || find_var(hp.node_vars[c], v) < 0) FAIL(JTP_EINVAL, "clique %d: covered variable %d is not one of its variables", c, v);
                if (find_var(hp.cover[c], v) >= 0) FAIL(JTP_EINVAL, "clique %d: covered variable %d listed twice", c, v);
                hp.cover[c].push_back(v);
            }
        }
    }
    hp.parent_clique.assign(d->parent_clique, d->parent_clique + N);
    hp.parent_sep.assign(d->parent_sep, d->parent_sep + N);
    hp.owner.assign(N, 0);
    if (d->clique_owner)
        for (int c = 0; c < N; ++c) {
            hp.owner[c] = d->clique_owner[c];
            // owner == n_ranks: the clique is REPLICATED - every rank holds its table and runs its tasks (the small
            // top of a partitioned tree: its children's upward messages go to every rank, its downward messages are
            // formed where they are consumed, so a propagate needs one exchange instead of two)
            if (hp.owner[c] < 0 || hp.owner[c] > d->n_ranks || (hp.owner[c] == d->n_ranks && d->n_ranks == 1))
                FAIL(JTP_EINVAL, "clique %d: bad owner %d", c, hp.owner[c]);
        }

    return JTP_OK;
}

int PlanBuilder::link_nodes() {
    // ---- nodes and separators -------------------------------------------------------------
    hp.pn.assign(N, PNode());
    hp.sep_of_node.assign(d->n_nodes, -1);
    hp.root = -1;
    for (int c = 0; c < N; ++c) {
        PNode &p = hp.pn[c];
        p.real = c;
        p.owner = hp.owner[c];
        p.parent = hp.parent_clique[c];
        if (p.parent < 0) {
            if (hp.root >= 0) FAIL(JTP_EINVAL, "two roots (%d and %d)", hp.root, c);
            hp.root = c;
        } else if (p.parent >= N || p.parent == c) FAIL(JTP_EINVAL, "clique %d: bad parent %d", c, p.parent);
    }
    if (hp.root < 0) FAIL(JTP_EINVAL, "no root clique");
    for (int c = 0; c < N; ++c) {
        if (c == hp.root) continue;
        int sn = hp.parent_sep[c];
        if (sn < N || sn >= d->n_nodes) FAIL(JTP_EINVAL, "clique %d: separator node %d out of range", c, sn);
        if (hp.sep_of_node[sn] >= 0) FAIL(JTP_EINVAL, "separator node %d used twice", sn);
        for (int v : hp.node_vars[sn]) {
            if (find_var(hp.node_vars[c], v) < 0 || find_var(hp.node_vars[hp.pn[c].parent], v) < 0)
                FAIL(JTP_EINVAL, "separator node %d: variable %d is not in both adjacent cliques", sn, v);
        }
        PSep s;
        s.node = sn;
        s.child = c;
        s.parent = hp.pn[c].parent;
        s.vars = hp.node_vars[sn];
        hp.sep_of_node[sn] = (int)hp.ps.size();
        hp.pn[c].psep = (int)hp.ps.size();
        hp.ps.push_back(s);
        hp.pn[hp.pn[c].parent].children.push_back(c);
    }
    {   // reachability (rejects cycles)
        std::vector<int> q{hp.root};
        std::vector<char> seen(N, 0);
        seen[hp.root] = 1;
        for (size_t i = 0; i < q.size(); ++i)
            for (int k : hp.pn[q[i]].children)
                if (!seen[k]) seen[k] = 1, q.push_back(k);
        if ((int)q.size() != N) FAIL(JTP_EINVAL, "parent pointers do not form a tree");
    }
    ALL = hp.n_ranks;                                              // owner value of replicated cliques
    for (int c = 0; c < N; ++c)
        if (hp.pn[c].owner == ALL && hp.pn[c].parent >= 0 && hp.pn[hp.pn[c].parent].owner != ALL)
            FAIL(JTP_EINVAL, "clique %d is replicated but its parent %d is not (the replicated part must contain the root)", c, hp.pn[c].parent);

    return JTP_OK;
}

int PlanBuilder::reroot() {
    // ---- re-root at the tree's centre (single rank): results do not depend on the root (every
    //      belief is psi times ALL incoming messages), but the number of levels = dependent launches
    //      does: a chain of N cliques needs N/2 levels per phase instead of N.
    if (hp.n_ranks == 1 && !(hp.flags & JTP_KEEP_ROOT) && N > 2) {
        std::vector<std::vector<std::pair<int, int>>> adj(N);      // (neighbour, psep)
        for (int c = 0; c < N; ++c)
            if (c != hp.root) {
                adj[c].push_back({hp.pn[c].parent, hp.pn[c].psep});
                adj[hp.pn[c].parent].push_back({c, hp.pn[c].psep});
            }
        auto bfs = [&](int src, std::vector<int> &dist, std::vector<int> &prev) {
            dist.assign(N, -1);
            prev.assign(N, -1);
            std::vector<int> q{src};
            dist[src] = 0;
            for (size_t i = 0; i < q.size(); ++i)
                for (auto &e : adj[q[i]])
                    if (dist[e.first] < 0) dist[e.first] = dist[q[i]] + 1, prev[e.first] = q[i], q.push_back(e.first);
            return q.back();                                       // a farthest clique
        };
        std::vector<int> d1, d2, p1, p2;
        const int a = bfs(hp.root, d1, p1);
        const int b = bfs(a, d2, p2);                              // a..b is a diameter
        int centre = b;
        for (int steps = d2[b] / 2; steps > 0; --steps) centre = p2[centre];
        if (d2[b] > 0 && centre != hp.root) {
            std::vector<int> order{centre};
            std::vector<int> np(N, -2), nsep(N, -1);
            np[centre] = -1;
            for (size_t i = 0; i < order.size(); ++i)
                for (auto &e : adj[order[i]])
                    if (np[e.first] == -2) np[e.first] = order[i], nsep[e.first] = e.second, order.push_back(e.first);
            for (int c = 0; c < N; ++c) {
                hp.pn[c].parent = np[c];
                hp.pn[c].psep = nsep[c];
                hp.pn[c].children.clear();
            }
            for (int c : order)
                if (np[c] >= 0) {
                    hp.pn[np[c]].children.push_back(c);
                    hp.ps[nsep[c]].child = c;
                    hp.ps[nsep[c]].parent = np[c];
                }
            hp.root = centre;
        }
    }
    return JTP_OK;
}

int PlanBuilder::decide_units() {
    // ---- unit cliques (JtTask::unit): no table, no belief table.  A clique becomes one when the description says its
    //      potential depends on few of its variables: on none (no factor assigned: 365 of the 878 cliques of the config-3
    //      lattice, 98 % of its table bytes), or on a part at most 1 / unit_ratio of the table - the product of its factors
    //      then travels as a static table over the covered variables.  The reference leaves such axes at length 1
    //      (junctiontree.py:52-61); rounds 1-4 of this engine materialised them, and streamed 9 GiB of ones three times per
    //      propagate on that lattice.  A clique covered (nearly) whole keeps its table: streaming it costs less than staging it.
    if (!hp.lean || hp.knobs.no_unit) return JTP_OK;
    double all = 0, unit = 0;
    for (int c = 0; c < N; ++c) {
        PNode &p = hp.pn[c];
        p.cover = hp.cover[c];
        double full = 1, part = 1;
        for (int v : hp.node_vars[c]) full *= hp.card[v];
        for (int v : p.cover) part *= hp.card[v];
        p.unit = p.cover.size() < hp.node_vars[c].size() && part * hp.knobs.unit_ratio <= full;
        all += full;
        unit += p.unit ? full : 0.0;
    }
    hp.unit_dominated = unit > 0.5 * all;
    return JTP_OK;
}

int PlanBuilder::binarise() {
    // ---- binarise: at most 3 children per node, via virtual all-ones cliques ---------------
    // (a unit clique with a static table stages it like one more incoming message: JT_MAX_IN = 4 then leaves room for the
    //  parent's message and TWO children)
    for (int c = 0; c < (int)hp.pn.size(); ++c) {
        const size_t lim = (wants_static(hp.pn[c]) && hp.pn[c].parent >= 0) ? 2 : 3;
        while (hp.pn[c].children.size() > lim) {
            std::vector<int> old = hp.pn[c].children, fresh;
            for (size_t g = 0; g < old.size(); g += 3) {
                size_t ge = std::min(old.size(), g + 3);
                if (ge - g == 1) {
                    fresh.push_back(old[g]);
                    continue;
                }
                PNode v;
                v.real = -1;
                v.unit = !hp.multiset && !hp.knobs.no_unit;     // (all ones: nothing to store)
                v.owner = hp.pn[c].owner;
                v.parent = c;
                for (size_t i = g; i < ge; ++i) {
                    for (int var : hp.ps[hp.pn[old[i]].psep].vars)
                        if (find_var(v.vars, var) < 0) v.vars.push_back(var);
                    v.children.push_back(old[i]);
                }
                if (v.vars.size() > JT_MAX_VARS) FAIL(JTP_EUNSUPPORTED, "virtual clique too wide");
                int vi = (int)hp.pn.size();
                PSep s;
                s.node = -1;
                s.child = vi;
                s.parent = c;
                s.vars = v.vars;
                v.psep = (int)hp.ps.size();
                hp.ps.push_back(s);
                for (size_t i = g; i < ge; ++i) {
                    hp.pn[old[i]].parent = vi;
                    hp.ps[hp.pn[old[i]].psep].parent = vi;
                }
                hp.pn.push_back(v);
                fresh.push_back(vi);
            }
            hp.pn[c].children = fresh;
        }
    }
    NP = (int)hp.pn.size();

    return JTP_OK;
}

int PlanBuilder::depths() {
    // ---- depth ------------------------------------------------------------------------------
    maxdepth = 0;
    {
        std::vector<int> q{hp.root};
        hp.pn[hp.root].depth = 0;
        for (size_t i = 0; i < q.size(); ++i)
            for (int k : hp.pn[q[i]].children) {
                hp.pn[k].depth = hp.pn[q[i]].depth + 1;
                maxdepth = std::max(maxdepth, hp.pn[k].depth);
                q.push_back(k);
            }
    }

    return JTP_OK;
}

int PlanBuilder::arenas() {
    // ---- arena offsets (this rank's real cliques) --------------------------------------------
    // rows 0 and 1 of the arenas are shared: row 0 stays all zero (what rows that do not exist read), row 1 takes
    // the belief stores of such rows (a belief arena is read again by the marginal tasks: its row 0 must stay zero)
    hp.arena_elems = (int64_t)2 << hp.TB;
    hp.host_table_elems = 0;
    auto pack_of = [&](const PNode &p, const std::vector<int> &host_vars) {
        JtPackDesc pd;
        memset(&pd, 0, sizeof pd);
        pd.dev_off = p.arena_off;
        pd.nbits = p.nbits;
        pd.nvars = (int)host_vars.size();
        pd.phys_elems = p.phys_elems;
        pd.low_bits = hp.TB;
        int64_t stride = 1;
        for (int i = pd.nvars - 1; i >= 0; --i) {
            const int v = host_vars[i];
            const int j = find_var(p.vars, v);
            bool whole = false;
            for (size_t g = 0; g < p.group_pos.size(); ++g) whole = whole || p.group_pos[g] == p.pos[j];
            pd.pos[i] = (uint8_t)p.pos[j];
            pd.nb[i] = (uint8_t)p.nb[j];
            pd.card[i] = hp.card[v];
            pd.hstride[i] = stride;
            pd.dstride[i] = p.nb[j] > 0 ? (uint32_t)p.bitw[p.pos[j]] : 0u;
            pd.dmod[i] = whole ? hp.card[v] : 1 << p.nb[j];
            if (p.tmix && p.pos[j] + p.nb[j] <= hp.TB) {          // a mixed-radix digit of the row
                int64_t ts = 1;
                for (int jj = 0; jj < j; ++jj)
                    if (p.pos[jj] + p.nb[jj] <= hp.TB) ts *= hp.card[p.vars[jj]];
                pd.dstride[i] = p.nb[j] > 0 ? (uint32_t)ts : 0u;
                pd.dmod[i] = hp.card[v];
            }
            stride *= hp.card[v];
        }
        pd.row_elems = p.tmix ? p.trow : 0;
        pd.host_elems = stride;
        pd.split_var = -1;
        if (p.tmix && p.tsplit >= 0) {
            const int j = p.tsplit, card = hp.card[p.vars[j]];
            for (int i = 0; i < pd.nvars; ++i)
                if (host_vars[i] == p.vars[j]) pd.split_var = i;
            if (pd.split_var >= 0) {
                int64_t ts = 1;
                for (int jj = 0; jj < j; ++jj)
                    if (p.pos[jj] + p.nb[jj] <= hp.TB) ts *= hp.card[p.vars[jj]];
                pd.split_lb = p.tsplit_lb;
                pd.dstride[pd.split_var] = (uint32_t)ts;
                pd.dmod[pd.split_var] = 1 << p.tsplit_lb;
                pd.split_ds2 = (uint32_t)p.bitw[hp.TB];
                pd.split_mod2 = (card + (1 << p.tsplit_lb) - 1) >> p.tsplit_lb;
            }
        }
        return pd;
    };
    std::map<std::vector<int32_t>, int64_t> map_at;          // thread maps already in the table buffer (unit cliques: mostly one)
    hp.fix_doubles = 0;
    // compact mixed-radix rows are kernels of their own (*_mix<T, true>): all of the plan's mixed-radix cliques, or none
    {
        bool all = hp.tmix, any = false;
        // (EVERY table-keeping clique of such a plan runs in the *_mix kernels - also those whose thread part stayed a bit field,
        //  and they have no list: one of them and the plan keeps one row per step)
        for (int c = 0; c < NP; ++c)
            if (!hp.pn[c].unit) {
                any = true;
                all = all && !hp.pn[c].vmap.empty();
            }
        hp.tmix_compact = all && any;
        if (!hp.tmix_compact)
            for (int c = 0; c < NP; ++c) hp.pn[c].vmap.clear();
    }
    hp.scratch_elems = 0;
    for (int c = 0; c < NP; ++c) {
        PNode &p = hp.pn[c];
        if (!mine(c)) continue;
        if (p.unit) {
            // no table: the passes make up the ones (jt_pass<..., UNIT>); beliefs on demand, into a scratch arena laid out like
            // the table would be (rows 0 and 1 shared, as in the arenas)
            p.arena_off = (int64_t)2 << hp.TB;
            hp.scratch_elems = std::max(hp.scratch_elems, p.arena_off + p.phys_elems);
            hp.has_unit = true;
            double he = 1;
            for (int v : p.cover) he *= hp.card[v];
            if (p.stat >= 0) hp.host_table_elems += he;
        } else {
            p.arena_off = hp.arena_elems;
            hp.arena_elems += p.phys_elems;
            hp.arena_elems = (hp.arena_elems + 255) & ~(int64_t)255;
            double he = 1;
            for (int v : p.vars) he *= hp.card[v];
            hp.host_table_elems += he;
            if (p.real < 0) hp.virtual_fills.push_back({pack_of(p, p.vars)});     // virtual clique: a resident 0/1 table
        }
        if (hp.tmix || p.unit) {
            auto it = p.unit ? map_at.find(p.tmap) : map_at.end();
            if (it != map_at.end()) p.tmap_off = it->second;
            else {
                p.tmap_off = (int64_t)hp.itab.size();
                hp.itab.insert(hp.itab.end(), p.tmap.begin(), p.tmap.end());
                hp.itab.insert(hp.itab.end(), p.vmap.begin(), p.vmap.end());          // (compact mixed-radix rows: PNode::vmap)
                if (p.unit) map_at[p.tmap] = p.tmap_off;
            }
        }
        if (p.stat >= 0) {
            // (16-byte aligned and at least two doubles: the kernels that fill it store 16-byte vectors)
            PStatic &st = hp.statics[p.stat];
            st.off = hp.fix_doubles;
            hp.fix_doubles += std::max<int64_t>((int64_t)1 << st.nbits, 2);
            hp.fix_doubles = (hp.fix_doubles + 1) & ~(int64_t)1;
        }
    }
    hp.pack.assign(N, JtPackDesc());
    hp.stat_pack.assign(N, JtPackDesc());
    for (int c = 0; c < N; ++c) {
        hp.pack[c] = pack_of(hp.pn[c], hp.node_vars[c]);
        memset(&hp.stat_pack[c], 0, sizeof(JtPackDesc));
        const PNode &p = hp.pn[c];
        if (p.stat < 0) continue;
        // host array of the clique (its uncovered axes have length 1) <-> the static table
        const PStatic &st = hp.statics[p.stat];
        JtPackDesc &pd = hp.stat_pack[c];
        pd.dev_off = st.off;
        pd.nbits = st.nbits;
        pd.nvars = (int)hp.node_vars[c].size();
        int64_t stride = 1;
        for (int i = pd.nvars - 1; i >= 0; --i) {
            const int v = hp.node_vars[c][i];
            const int j = find_var(st.vars, v);
            pd.pos[i] = j >= 0 ? (uint8_t)st.pos[j] : 0;
            pd.nb[i] = j >= 0 ? (uint8_t)st.nb[j] : 0;
            pd.card[i] = j >= 0 ? hp.card[v] : 1;
            pd.hstride[i] = j >= 0 ? stride : 0;
            pd.dstride[i] = j >= 0 && st.nb[j] > 0 ? 1u << st.pos[j] : 0u;
            pd.dmod[i] = j >= 0 ? 1 << st.nb[j] : 1;
            if (j >= 0) stride *= hp.card[v];
        }
        pd.host_elems = stride;
        pd.phys_elems = (int64_t)1 << st.nbits;
        pd.low_bits = st.nbits;
        pd.row_elems = 0;
        pd.split_var = -1;
    }
    return JTP_OK;
}

int PlanBuilder::level_work() {
    // ---- per (phase, level, rank) work, to size workgroups ----------------------------------------
    // (per owning rank: a rank's launches hold only its own cliques, and every rank must size every
    // task the same way because the partial-copy counts of the cut messages follow from it)
    for (int ph = 0; ph < 2; ++ph) lvl_elems[ph].assign(hp.n_ranks + 1, std::vector<double>(maxdepth + 1, 0.0));
    for (int c = 0; c < NP; ++c) {
        double e = (double)hp.pn[c].phys_elems;
        // (a mixed-radix row holds trow of the 2^TB entries a workgroup step covers: workgroups are sized by steps,
        //  as if the rows were full - sized by elements they came out at 8 rows of 500 bytes each, 6 x slower)
        if (hp.pn[c].tmix && hp.pn[c].trow > 0) e *= (double)(1 << hp.TB) / (double)hp.pn[c].trow;
        if (c != hp.root) lvl_elems[0][hp.pn[c].owner][hp.pn[c].depth] += e;
        lvl_elems[1][hp.pn[c].owner][hp.pn[c].depth] += e;
    }

    return JTP_OK;
}

int jtp_build_plan(const jtp_tree_desc *d, HostPlan &hp, std::string &err) {
    return PlanBuilder(d, hp, err).run();
}
