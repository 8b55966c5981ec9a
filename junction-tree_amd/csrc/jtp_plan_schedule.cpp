// Planner, unit 5 of 6 (jtp_plan_build.h has the map): launches, workgroup records and the exchange schedule; dataflow segments;
// the sampling schedule.
#include "jtp_plan_build.h"

int PlanBuilder::schedule() {
    // Which passes load their table rows with the default cache policy (JtTask::keep_rows; everything else non-temporal).
    // The levels nearest the root are read LAST by collect and FIRST by distribute: both passes over the levels chosen below (this
    // rank's tables, knobs.keep_rows_mb in all) keep their rows in the 256 MiB Infinity Cache and the second finds them there
    // instead of in HBM.  A plan whose tables fit the budget altogether keeps every row.  HostPlan::keep_* say what was chosen.
    // Only where the kernels that look at the flag run - the dataflow launches of single-set plans of bit-field rows that are no
    // chains (jt_propagate_flow, jt_propagate_flow_marg, jt_collect_flow_keep): multi-set plans, mixed-radix rows, chains and plans
    // launched per level keep nothing, and say so (budget 0).
    const bool keep_kernels = !hp.multiset && !hp.tmix && !hp.chain_plan && !(hp.flags & (JTP_LEVEL_LAUNCHES | JTP_SPLIT_VARIANTS)) &&
                              !(hp.knobs.debug & 1) && !hp.knobs.force_level_launches;
    hp.keep_budget = keep_kernels ? std::max(0.0, hp.knobs.keep_rows_mb) * 1048576.0 : 0.0;
    hp.keep_bytes[0] = hp.keep_bytes[1] = 0;
    hp.keep_levels.clear();
    if (hp.keep_budget > 0) {
        std::vector<double> level_bytes(maxdepth + 1, 0.0);
        double all_bytes = 0;
        for (int c = 0; c < NP; ++c)
            if (mine(c) && !hp.pn[c].unit) level_bytes[hp.pn[c].depth] += (double)hp.pn[c].phys_elems * esize, all_bytes += (double)hp.pn[c].phys_elems * esize;
        std::vector<char> keep(maxdepth + 1, 0);
        if (all_bytes <= hp.keep_budget) {
            for (int d = 0; d <= maxdepth; ++d) keep[d] = level_bytes[d] > 0;
        } else {
            // By what a kept level saves.  A kept row is an HBM read the distribute pass does not make, and that is time only where the
            // level's distribute pass is bandwidth-bound: its bytes (read + written) at the streaming rate take longer than the life
            // of ONE of its workgroups - start, staging, its rows, flush: the level's hand-over, which no bandwidth shortens (the
            // cost model's constants, task_cost_us).  Such levels come first, nearest the root first (the shortest time between the
            // two passes); the narrow levels above them - a hand-over each whatever their bytes cost - take what is left.  Whole
            // levels only: part of a level, visited by both passes in the same order, is pushed out before it is used again.
            double fix_us, iter_us, bytes_per_us;
            jtp_keep_cost(fix_us, iter_us, bytes_per_us);
            if (hp.knobs.keep_bw > 0) bytes_per_us = hp.knobs.keep_bw;
            std::vector<int> rows(maxdepth + 1, 0);              // rows per distribute workgroup, the longest of the level
            for (const JtTask &tk : hp.tasks)
                if (tk.kind == 0 && !tk.unit && tk.mode == 1 && mine(tk.pnode)) rows[hp.pn[tk.pnode].depth] = std::max(rows[hp.pn[tk.pnode].depth], tk.total);
            auto bw_bound = [&](int d) { return 2.0 * level_bytes[d] / bytes_per_us > fix_us + iter_us * rows[d]; };
            double left = hp.keep_budget;
            int top_end = maxdepth + 1;                          // the narrow top: the levels above the first bandwidth-bound one
            for (int d = maxdepth; d >= 0; --d)
                if (level_bytes[d] > 0 && bw_bound(d)) top_end = d;
            for (int pass = 0; pass < (hp.knobs.keep_top ? 2 : 1); ++pass)
                for (int d = 0; d < (pass == 0 ? maxdepth + 1 : top_end); ++d) {
                    if (level_bytes[d] <= 0 || keep[d] || bw_bound(d) != (pass == 0) || level_bytes[d] > left) continue;
                    keep[d] = 1;
                    left -= level_bytes[d];
                }
        }
        for (JtTask &tk : hp.tasks)
            if (tk.kind == 0 && !tk.unit && mine(tk.pnode) && keep[hp.pn[tk.pnode].depth]) {
                tk.keep_rows = 1;
                if (!tk.fold) hp.keep_bytes[tk.mode ? 1 : 0] += (double)hp.pn[tk.pnode].phys_elems * esize;
            }
        for (int d = 0; d <= maxdepth; ++d)
            if (keep[d]) hp.keep_levels.push_back(d);
    }
    // ---- launches, blocks, exchange schedule -----------------------------------------------------
    hp.alg_bytes = 0;
    hp.max_lds = 0;
    std::vector<CommOp> pending;            // comm ops waiting to be grouped before the next launch
    auto flush_comm = [&]() {
        if (pending.empty()) return;
        Step st;
        st.kind = 1;
        st.first = (int)hp.comm.size();
        st.count = (int)pending.size();
        for (auto &op : pending) hp.comm.push_back(op);
        hp.steps.push_back(st);
        pending.clear();
    };
    auto comm_op = [&](int send, int psep, int up, int peer) {
        const PSep &s = hp.ps[psep];
        CommOp op;
        op.send = send;
        op.psep = psep;
        op.up = up;
        op.peer = peer;
        op.off = up ? s.up_roff : s.dn_roff;                 // (the sum, when the producer's rank reduces)
        op.count = ((int64_t)1 << s.nbits) * (up ? s.up_rnpart : s.dn_rnpart);
        pending.push_back(op);
    };
    // Multi-set plans: a launch's block list is padded to a multiple of eight records with records that start no work
    // (JT_BLOCK_NULL).  jt_multi_flow hands runs of eight records to the groups of evidence sets in turn; with active lists (round 6) a
    // workgroup of one group waits for entries another group's workgroup writes, and with every launch - every tree level -
    // starting on a multiple of eight, that producer has the lower blockIdx whatever its group.
    auto pad_launch = [&](const Launch &L) {
        if (!hp.multiset) return;
        while ((hp.blocks.size() - (size_t)L.blk_off) % 8) {
            JtBlock nb;
            memset(&nb, 0, sizeof nb);
            nb.task = L.tasks.empty() ? 0u : (uint32_t)L.tasks[0];
            nb.flags = JT_BLOCK_NULL;
            hp.blocks.push_back(nb);
            hp.block_chunk.push_back(0xffffffffu);
        }
    };
    auto by_level = [&](int level) {
        std::vector<int> v;
        for (int c = 0; c < NP; ++c) if (hp.pn[c].depth == level) v.push_back(c);
        return v;
    };
    auto emit_launches = [&](int phase, int level) {
        std::map<int, std::vector<int>> groups;
        for (int c : by_level(level)) {
            const PNode &p = hp.pn[c];
            if (!mine(c)) continue;
            if (hp.multiset) {
                if (phase == 0 && p.collect_task >= 0) groups[JT_K_MULTI_COLLECT].push_back(p.collect_task);
                if (phase == 1) for (int t : p.down_tasks) groups[JT_K_MULTI_DISTRIBUTE].push_back(t);
                continue;
            }
            if (phase == 1)
                for (int t : p.fold_tasks) groups[JT_K_DISTRIBUTE_LEVEL].push_back(t);      // (marginals folded into the propagate)
            if (phase == 1 && !p.down_tasks.empty()) {       // (a unit clique: a task per downward message)
                for (int t : p.down_tasks) groups[JT_K_DISTRIBUTE_LEVEL].push_back(t);
                continue;
            }
            int t = phase == 0 ? p.collect_task : p.distribute_task;
            if (t < 0) continue;
            int key = hp.task_variant[t];
            // (per-shape launches are a profiling aid of plans whose cliques all keep tables: unit tasks have shapes of their own)
            if (!(hp.flags & JTP_SPLIT_VARIANTS) || hp.has_unit) key = phase == 0 ? JT_K_COLLECT_LEVEL : JT_K_DISTRIBUTE_LEVEL;
            groups[key].push_back(t);
        }
        if (!groups.empty()) flush_comm();
        for (auto &g : groups) {
            Launch L;
            L.phase = phase;
            L.level = level;
            L.variant = g.first;
            L.tasks = g.second;
            if (hp.knobs.longest_first) {
                // Longest workgroups first: a level is over when its LAST workgroup is, and the workgroups of one task all
                // take about as long as each other.  Multi-set plans: the tasks that cannot sum a vector's four elements
                // before the message product (JtTask::esum == 0, 8 % of them on the width-20 tree) run 4-5 x longer per
                // row - sixteen such workgroups, started two thirds into their level, ended 140 us after everybody else.
                auto weight = [&](int t) { return (long)hp.tasks[t].total * (hp.multiset && !hp.tasks[t].esum ? 4 : 1); };
                std::stable_sort(L.tasks.begin(), L.tasks.end(), [&](int a, int b) { return weight(a) > weight(b); });
            }
            L.blk_off = (int64_t)hp.blocks.size();
            for (int t : L.tasks) {
                const JtTask &tk = hp.tasks[t];
                for (uint32_t f = 0; f < (1u << tk.nF); ++f) {
                    const JtBlock b = jtp_make_block(hp, tk, (uint32_t)t, f);
                    if ((b.flags & JT_BLOCK_INVALID) && !hp.knobs.keep_invalid) {
                        // (a chunk that does not exist: zeros, written once per arena - HostPlan::init_blocks)
                        hp.init_blocks[tk.mode ? 1 : 0].push_back(b);
                        hp.init_chunk[tk.mode ? 1 : 0].push_back(f);
                        continue;
                    }
                    hp.blocks.push_back(b);
                    hp.block_chunk.push_back(f);
                }
                L.lds_bytes = std::max(L.lds_bytes, tk.lds_bytes);
                L.alg_bytes += task_bytes[t];
                for (int k = 0; k < tk.n_in; ++k) hp.staging_bytes += (double)(1u << tk.nF) * (8.0 * (1 << tk.msg[k].nfree)) * tk.msg[k].npart;
                if (!tk.unit) hp.table_bytes += (double)hp.pn[tk.pnode].phys_elems * esize * (phase == 1 && !hp.multiset ? 2 : 1);
            }
            pad_launch(L);
            L.nblocks = (int)(hp.blocks.size() - L.blk_off);
            hp.max_lds = std::max(hp.max_lds, L.lds_bytes);
            hp.alg_bytes += L.alg_bytes;
            Step st;
            st.kind = 0;
            st.first = (int)hp.launches.size();
            st.count = 1;
            hp.launches.push_back(L);
            hp.steps.push_back(st);
        }
    };
    // reduce tasks of the messages one level has just produced (its own launch when launching per level)
    auto emit_reduce = [&](int phase, int level) {
        std::vector<int> tasks;
        for (int c : by_level(level)) {
            const PNode &p = hp.pn[c];
            if (!mine(c)) continue;
            if (phase == 0) {
                if (p.psep >= 0 && hp.ps[p.psep].up_red_task >= 0) tasks.push_back(hp.ps[p.psep].up_red_task);
            } else {
                for (int k : p.children)
                    if (hp.ps[hp.pn[k].psep].dn_red_task >= 0) tasks.push_back(hp.ps[hp.pn[k].psep].dn_red_task);
            }
        }
        if (tasks.empty()) return;
        Launch L;
        L.phase = phase;
        L.level = level;
        L.variant = JT_K_REDUCE_LEVEL;
        L.tasks = tasks;
        L.blk_off = (int64_t)hp.blocks.size();
        for (int t : tasks)
            for (uint32_t f = 0; f < (1u << hp.tasks[t].nF); ++f) {
                hp.blocks.push_back(jtp_make_block(hp, hp.tasks[t], (uint32_t)t, f));
                hp.block_chunk.push_back(f);
            }
        pad_launch(L);
        L.nblocks = (int)(hp.blocks.size() - L.blk_off);
        Step st;
        st.kind = 0;
        st.first = (int)hp.launches.size();
        st.count = 1;
        hp.launches.push_back(L);
        hp.steps.push_back(st);
    };
    // JTP_SCALED: the messages one level has just produced (behind their reduce tasks) are divided by a power of two each
    auto emit_rescale = [&](int phase, int level) {
        if (!hp.scaled) return;
        Step st;
        st.kind = 2;
        st.first = (int)hp.rescale.size();
        auto add = [&](int psep, bool up) {
            const PSep &s = hp.ps[psep];
            JtRescale r;
            r.off = up ? s.up_roff : s.dn_roff;
            r.count = ((int64_t)1 << s.nbits) * (up ? s.up_rnpart : s.dn_rnpart);
            r.slot = 2 * psep + (up ? 0 : 1);
            r.pad = 0;
            if (r.off >= 0) hp.rescale.push_back(r);
        };
        for (int c : by_level(level)) {
            const PNode &p = hp.pn[c];
            if (!mine(c)) continue;
            if (phase == 0) {
                if (p.psep >= 0) add(p.psep, true);
            } else {
                for (int k : p.children) add(hp.pn[k].psep, false);
            }
        }
        st.count = (int)hp.rescale.size() - st.first;
        if (st.count > 0) hp.steps.push_back(st);
    };
    // Exchange order: ncclSend/ncclRecv (and every transport standing in for them) pair the operations
    // between two ranks in ISSUE order, so both sides of a cut must enumerate the cut edges of one level
    // in the same order whatever the numbering of the cliques: always by the CHILD clique of the edge
    // (ascending), never by the parent's position.
    // A cut edge joins cliques of different owners.  child (rank r) -> replicated parent: r sends the upward message
    // to EVERY other rank, the downward message needs no exchange (each rank's replica forms it; only r uses it).
    auto cut_children = [&](int child_level) {
        std::vector<int> v;                                    // children (ascending) of cut edges at this level
        for (int k : by_level(child_level)) {
            const PNode &ch = hp.pn[k];
            if (ch.parent >= 0 && hp.pn[ch.parent].owner != ch.owner) v.push_back(k);
        }
        return v;
    };
    for (int level = maxdepth; level >= 0; --level) {          // collect
        for (int k : cut_children(level + 1)) {                // receive what this level consumes
            const int po = hp.pn[hp.pn[k].parent].owner;
            if (hp.pn[k].owner != hp.rank && (po == hp.rank || po == ALL)) comm_op(0, hp.pn[k].psep, 1, hp.pn[k].owner);
        }
        if (level >= 1) {
            emit_launches(0, level);
            emit_reduce(0, level);
            emit_rescale(0, level);
        }
        for (int c : cut_children(level)) {                    // send what this level produced
            if (hp.pn[c].owner != hp.rank) continue;
            const int po = hp.pn[hp.pn[c].parent].owner;
            if (po == ALL) {
                for (int peer = 0; peer < hp.n_ranks; ++peer)
                    if (peer != hp.rank) comm_op(1, hp.pn[c].psep, 1, peer);
            } else comm_op(1, hp.pn[c].psep, 1, po);
        }
    }
    for (int level = 0; level <= maxdepth; ++level) {          // distribute
        for (int c : cut_children(level)) {
            const int po = hp.pn[hp.pn[c].parent].owner;
            if (hp.pn[c].owner == hp.rank && po != ALL) comm_op(0, hp.pn[c].psep, 0, po);
        }
        emit_launches(1, level);
        emit_reduce(1, level);
        emit_rescale(1, level);
        for (int k : cut_children(level + 1)) {
            const int po = hp.pn[hp.pn[k].parent].owner;
            if (po == hp.rank && hp.pn[k].owner != hp.rank) comm_op(1, hp.pn[k].psep, 0, hp.pn[k].owner);
        }
    }
    flush_comm();
    return JTP_OK;
}

int PlanBuilder::finish() {
    // ---- dataflow schedule: runs of launches of one phase become one segment --------------------
    for (const Step &st : hp.steps) {
        if (hp.scaled) break;                      // (a scaled plan launches per level: no segments, no flow steps)
        if (st.kind == 1) {
            hp.flow_steps.push_back(st);
            continue;
        }
        const Launch &L = hp.launches[st.first];
        const bool extend = !hp.flow_steps.empty() && hp.flow_steps.back().kind == 0 && hp.segments.back().phase == L.phase;
        if (!extend) {
            Segment sg;
            sg.phase = L.phase;
            sg.first_launch = st.first;
            sg.blk_off = L.blk_off;
            sg.ticket_idx = JT_SYNC_HDR + (int)hp.segments.size();
            Step fs;
            fs.kind = 0;
            fs.first = (int)hp.segments.size();
            fs.count = 1;
            hp.segments.push_back(sg);
            hp.flow_steps.push_back(fs);
        }
        Segment &sg = hp.segments.back();
        sg.n_launch++;
        sg.nblocks += L.nblocks;
        sg.lds_bytes = std::max(sg.lds_bytes, L.lds_bytes);
    }
    // Both phases in one launch (jt_propagate_flow): where the distribute segment follows the collect segment directly (no
    // exchange in between) and the messages are small beside the tables - every message of a merged launch is read
    // through to memory, which costs where staging is a large share of the traffic (config 3) and buys nothing on chains.
    {
        const bool merge = hp.knobs.merge_phases == 1 ||
                           (hp.knobs.merge_phases < 0 && !hp.multiset && !hp.chain_plan && !hp.tmix &&
                            // (plans of mostly unit cliques: no tables to speak of - one launch.  Measured the same as two launches once
                            //  the distribute segment ran the two-phase kernel, whose build is the faster one: jtp_engine.hip, get_flow)
                            (hp.staging_bytes * 8.0 <= hp.table_bytes || hp.unit_dominated));
        if (merge && !hp.multiset && !hp.tmix) {
            std::vector<Segment> segs;
            std::vector<Step> fsteps;
            for (const Step &st : hp.flow_steps) {
                if (st.kind == 0 && !fsteps.empty() && fsteps.back().kind == 0 && segs.back().phase == 0 && hp.segments[st.first].phase == 1) {
                    const Segment &b = hp.segments[st.first];
                    Segment &a = segs.back();
                    a.phase = 2;
                    a.n_launch += b.n_launch;
                    a.nblocks += b.nblocks;
                    a.lds_bytes = std::max(a.lds_bytes, b.lds_bytes);
                    continue;
                }
                Step fs = st;
                if (st.kind == 0) {
                    fs.first = (int)segs.size();
                    segs.push_back(hp.segments[st.first]);
                    segs.back().ticket_idx = JT_SYNC_HDR + (int)segs.size() - 1;
                }
                fsteps.push_back(fs);
            }
            hp.segments = segs;
            hp.flow_steps = fsteps;
        }
    }
    // JtMsg::same_launch: the producer of an incoming message runs in the same dataflow launch as its consumer - then the
    // consumer reads the entries through to memory and waits on their "unwritten" markers; messages finished by an earlier
    // launch (or received by an exchange) are read with ordinary loads.
    {
        std::vector<int> seg_of(hp.tasks.size(), -1);
        for (size_t g = 0; g < hp.segments.size(); ++g)
            for (int i = hp.segments[g].first_launch; i < hp.segments[g].first_launch + hp.segments[g].n_launch; ++i)
                for (int t : hp.launches[i].tasks) seg_of[t] = (int)g;
        for (size_t t = 0; t < hp.tasks.size(); ++t) {
            JtTask &tk = hp.tasks[t];
            const std::vector<int> &prod = hp.task_producers[t];
            for (int k = 0; k < tk.n_in && k < (int)prod.size(); ++k)
                tk.msg[k].same_launch = (prod[k] >= 0 && seg_of[t] >= 0 && seg_of[prod[k]] == seg_of[t]) ? 1 : 0;
        }
    }
    hp.sync_words = JT_SYNC_HDR + (int)hp.segments.size();
    if (hp.knobs.debug & 2) {     // time-stamp region, JT_NSTAMP doubles per workgroup (+ one spare set), for -DJT_STAMPS builds
        hp.dbg_base = hp.msg_doubles;
        hp.msg_doubles += ((int64_t)hp.blocks.size() + 1) * 16;
        for (const Launch &L : hp.launches)
            for (int t : L.tasks) hp.tasks[t].dbg_off = hp.dbg_base;
    }
    hp.n_messages = 0;
    for (int c = 0; c < N; ++c)
        if (c != hp.root && (hp.owner[c] == hp.rank || (hp.owner[c] == ALL && hp.rank == 0))) hp.n_messages += 2;
    // Lean records (round 6, JtLean): every field of every task is final here
    for (JtTask &tk : hp.tasks) jtp_make_lean(hp, tk, hp.itab, tk.fold != 0);
    // (a folded marginal task runs as a lean task or not at all: without a record - fold_marginals asks for what jtp_make_lean asks for,
    //  so this does not happen - its requests are the read-out's)
    for (HostPlan::FoldReq &fr : hp.folded)
        if (fr.task >= 0 && hp.tasks[fr.task].lean_off <= 0) fr.task = -1;
    for (JtBlock &b : hp.blocks) {
        const int64_t at = hp.tasks[b.task].lean_off;
        if (hp.tasks[b.task].fold) b.flags |= JT_BLOCK_FOLD;
        if (at > 0) b.flags |= JT_BLOCK_LEAN, b.first_x[5] = (uint32_t)hp.tasks[b.task].pnode, b.first_x[6] = (uint32_t)at, b.first_x[7] = (uint32_t)((uint64_t)at >> 32);
    }
    return JTP_OK;
}

int PlanBuilder::sampling() {
    // ---- sampling schedule (jtp_sample): a root-to-leaves sweep over the tree AS THE CALLER DESCRIBED IT.  A clique conditions on the
    //      variables it shares with its parent clique (K; by the running-intersection property exactly those of its variables some
    //      clique nearer the root has drawn) and draws the others (F).  Host only: nothing here depends on layouts, so the schedule -
    //      and with it the order every slice is summed in - is the same whatever the plan's flags.
    std::vector<int> depth(N, 0), order;
    std::vector<std::vector<int>> kids(N);
    int croot = -1;
    for (int c = 0; c < N; ++c) {
        if (hp.parent_clique[c] < 0) croot = c;
        else kids[hp.parent_clique[c]].push_back(c);
    }
    order.push_back(croot);
    for (size_t i = 0; i < order.size(); ++i)
        for (int k : kids[order[i]]) depth[k] = depth[order[i]] + 1, order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return depth[a] != depth[b] ? depth[a] < depth[b] : a < b; });
    hp.sample.clear();
    hp.sample_depths.clear();
    for (int c : order) {
        SampleClique sc;
        sc.clique = c;
        sc.depth = depth[c];
        const int par = hp.parent_clique[c];
        for (int v : hp.node_vars[c]) {
            if (par >= 0 && find_var(hp.node_vars[par], v) >= 0) sc.K.push_back(v);
            else sc.F.push_back(v), sc.R *= hp.card[v];
        }
        if ((int)hp.sample_depths.size() <= sc.depth) hp.sample_depths.resize(sc.depth + 1);
        hp.sample_depths[sc.depth].push_back((int)hp.sample.size());
        hp.sample.push_back(sc);
    }
    hp.sample_refused.clear();
    if (hp.multiset) hp.sample_refused = "a multi-set plan keeps no belief tables: sample from a plan made without JTP_MULTISET (one evidence set per pass)";
    else if (hp.n_ranks > 1) hp.sample_refused = "sampling from a plan shared by several ranks is not built: make the plan with n_ranks = 1";
    else
        for (int c = 0; c < N; ++c)
            if (hp.pn[c].unit) {
                hp.sample_refused = "clique " + std::to_string(c) + " keeps no table on the device: make the plan without `cover`";
                break;
            }
    return JTP_OK;
}
