// Planner, unit 4 of 6 (jtp_plan_build.h has the map): the tasks of the propagate and of the read-out.  Which tables a task of a clique
// reads, in which order, where each lives and who writes it is stated ONCE - task_inputs and input_place - and every user derives
// its part from there: the views plan_loops works on (make_tasks, the read-out tasks), JtMsg::off / npart / fixed / src_task
// (messages, the read-out tasks) and HostPlan::task_producers (messages, fold_marginals).
#include "jtp_plan_build.h"

namespace {

// a table (separator message, static table, requested marginal) seen from the clique: which clique bits it has, and where
template <typename Table>
MsgView make_view(const PNode &p, const Table &s, int psep, bool up) {
    MsgView mv;
    mv.psep = psep;
    mv.up = up;
    mv.msg_bits = s.nbits;
    for (int i = 0; i < 32; ++i) mv.dst[i] = -1;
    for (size_t i = 0; i < s.vars.size(); ++i) {
        int j = find_var(p.vars, s.vars[i]);
        for (int t = 0; t < s.nb[i]; ++t) {
            mv.dst[p.pos[j] + t] = (int8_t)(s.pos[i] + t);
            mv.mask |= 1u << (p.pos[j] + t);
        }
    }
    return mv;
}

std::vector<TaskInput> task_inputs(const HostPlan &hp, const PNode &p, bool with_parent, int skip_child = -1) {
    std::vector<TaskInput> in;
    if (with_parent && p.psep >= 0) in.push_back({TaskInput::PARENT, p.psep, -1});
    if (p.stat >= 0) in.push_back({TaskInput::STATIC, p.stat, -1});
    for (int i = 0; i < (int)p.children.size(); ++i)
        if (i != skip_child) in.push_back({TaskInput::CHILD, hp.pn[p.children[i]].psep, p.children[i]});
    return in;
}

std::vector<MsgView> input_views(const HostPlan &hp, const PNode &p, const std::vector<TaskInput> &in) {
    std::vector<MsgView> v;
    for (const TaskInput &i : in)
        v.push_back(i.kind == TaskInput::STATIC ? make_view(p, hp.statics[i.index], -1, true)
                                                : make_view(p, hp.ps[i.index], i.index, i.kind == TaskInput::CHILD));
    return v;
}

// Where an input lives - what consumers read: the reduced sum where a reduce task exists -, how many partial copies, in which arena,
// the collect task that forms it (JtMsg::src_task of an upward message: tells the engine whose arena a multi-set plan's read-out takes
// it from, readout_redirect) and the task that writes what the consumer reads (HostPlan::task_producers; -1: nobody's product).
struct InputPlace {
    int64_t off;
    int npart, fixed, src_task, producer;
};

// the task that forms a downward message (multi-set plans and unit cliques: a task per child, PSep::dn_task)
int down_writer(const HostPlan &hp, const PSep &sp) { return sp.dn_task >= 0 ? sp.dn_task : hp.pn[sp.parent].distribute_task; }

InputPlace input_place(const HostPlan &hp, const TaskInput &in) {
    if (in.kind == TaskInput::STATIC) return {hp.statics[in.index].off, 1, 1, -1, -1};       // (off -1: the clique is another rank's)
    const PSep &sp = hp.ps[in.index];
    if (in.kind == TaskInput::CHILD)
        return {sp.up_roff, sp.up_rnpart, 0, hp.pn[in.child].collect_task, sp.up_red_task >= 0 ? sp.up_red_task : hp.pn[in.child].collect_task};
    return {sp.dn_roff, sp.dn_rnpart, 0, -1, sp.dn_red_task >= 0 ? sp.dn_red_task : down_writer(hp, sp)};
}

// JtMsg::off / npart / fixed / src_task of every input.  same_launch stays 0: whether the producer runs in the consumer's launch is the
// caller's to say.  A task of the propagate names the collect task behind an upward message and leaves src_task of the others 0, a
// read-out task says -1 there (readout_redirect reads the field); the propagate's tasks of another rank's clique - placeholders that
// never run - keep a static table's offset inside the arena.
void place_inputs(const HostPlan &hp, const std::vector<TaskInput> &in, JtTask &tk, bool readout) {
    for (size_t k = 0; k < in.size(); ++k) {
        const InputPlace at = input_place(hp, in[k]);
        tk.msg[k].off = at.fixed && !readout ? std::max<int64_t>(at.off, 0) : at.off;
        tk.msg[k].npart = at.npart;
        tk.msg[k].fixed = at.fixed;
        if (readout || in[k].kind == TaskInput::CHILD) tk.msg[k].src_task = at.src_task;
    }
}

std::vector<int> input_producers(const HostPlan &hp, const std::vector<TaskInput> &in) {
    std::vector<int> prod;
    for (const TaskInput &i : in) prod.push_back(input_place(hp, i).producer);
    return prod;
}

}  // namespace

// A task of clique tk.pnode with these inputs, forming the messages of `out_seps` (collect: the upward message of the clique's own
// separator; distribute: downward messages): its loops planned - multi-set plans: within the small LDS share of an evidence set, else
// the large one -, its iteration table appended, the task and its kernel variant pushed.  The task is hp.tasks.back() afterwards.
int PlanBuilder::add_task(JtTask tk, int phase, const std::vector<TaskInput> &in, const std::vector<int> &out_seps, int block_log2, double share, int variant) {
    const PNode &p = hp.pn[tk.pnode];
    const std::vector<MsgView> ins = input_views(hp, p, in);
    if ((int)ins.size() > JT_MAX_IN) FAIL(JTP_EUNSUPPORTED, "internal: clique %d has %zu incoming tables", p.real, ins.size());
    std::vector<MsgView> outs;
    for (int k : out_seps) outs.push_back(make_view(p, hp.ps[k], k, phase == 0));
    std::vector<int32_t> itab;
    int rc = plan_loops(hp, p, tk, itab, ins, outs, block_log2, err, hp.multiset ? JT_SETB_SMALL : 0, share);
    if (rc != JTP_OK && hp.multiset) rc = plan_loops(hp, p, tk, itab, ins, outs, block_log2_for(phase, p.depth, p.owner), err, JT_SETB_LARGE);
    if (rc != JTP_OK) return rc;
    tk.itab_off = (int64_t)hp.itab.size();
    hp.itab.insert(hp.itab.end(), itab.begin(), itab.end());
    hp.tasks.push_back(tk);
    hp.task_variant.push_back(variant);
    return JTP_OK;
}

// algorithmic bytes of the incoming messages that are the caller's (virtual separators and static tables are not)
double PlanBuilder::message_bytes(const std::vector<TaskInput> &in) const {
    double mb = 0;
    for (const TaskInput &i : in)
        if (i.kind != TaskInput::STATIC && hp.ps[i.index].node >= 0) mb += host_elems(hp.ps[i.index].vars) * 8;
    return mb;
}

int PlanBuilder::make_tasks() {
    // ---- tasks ------------------------------------------------------------------------------
    task_bytes.clear();
    for (int c = 0; c < NP; ++c) {
        PNode &p = hp.pn[c];
        int nch = (int)p.children.size();
        for (int phase = 0; phase < 2; ++phase) {
            if (phase == 0 && c == hp.root) continue;
            JtTask tk;
            memset(&tk, 0, sizeof tk);
            tk.pnode = c;
            tk.bel_off = -1;
            // One marginalisation per child instead of a distribute pass, down_k = sum psi * down_parent * prod_{j != k} up_j (mode 0; a
            // leaf has no task at all).  Multi-set plans: no belief table is written; beliefs and marginals are formed on demand
            // (jtp_plan_belief_task).  Unit cliques: their distribute pass writes no belief either - what is left of it is the downward
            // messages, and one pass that folds every child's sums on every row costs 3.5 x a row of such a task (163 against 50 vector
            // instructions, the epilogue of the first message on every row).  What differs between the two: the size of a workgroup,
            // the share of the level, the kernel, how the bytes are booked.
            const bool unit_down = p.unit && !hp.knobs.unit_joint_down;
            if (phase == 1 && (hp.multiset || unit_down)) {
                tk.psi_off = hp.multiset ? p.arena_off : 0;
                tk.unit = hp.multiset ? 0 : 1;
                for (int j = 0; j < nch; ++j) {
                    const std::vector<TaskInput> in = task_inputs(hp, p, true, j);
                    const int ks = hp.pn[p.children[j]].psep;
                    const double share = std::min(1.0, (double)p.phys_elems / std::max(1.0, lvl_elems[phase][p.owner][p.depth]));
                    const int blg = block_log2_for(0, p.depth, p.owner, p.layout != 4);
                    const int rc = hp.multiset ? add_task(tk, phase, in, {ks}, block_log2_for(phase, p.depth, p.owner), 1.0, JT_K_MULTI_DISTRIBUTE)
                                               : add_task(tk, phase, in, {ks}, hp.block_log2 > 0 ? std::max(hp.block_log2, hp.TB) : blg, share, JT_K_DISTRIBUTE_LEVEL);
                    if (rc != JTP_OK) return rc;
                    const int ti = (int)hp.tasks.size() - 1;
                    p.down_tasks.push_back(ti);
                    hp.ps[ks].dn_task = ti;
                    hp.ps[ks].dn_npart = hp.tasks[ti].msg[JT_MAX_IN].npart;
                    double b = 0, mb = hp.ps[ks].node >= 0 ? host_elems(hp.ps[ks].vars) * 8 * 2 : 0.0;      // down message + separator belief
                    if (hp.multiset) {
                        if (p.real >= 0) b += host_elems(hp.node_vars[p.real]) * esize;
                        mb += message_bytes(in);
                        hp.alg_table_bytes += b;
                        hp.alg_msg_bytes += mb;
                    } else {
                        // (algorithmic bytes of the clique's downward step, counted once: the static table, the parent's message and every
                        //  child's upward message read - booked on the first task - and each child's downward message and separator belief)
                        if (j == 0) {
                            if (p.stat >= 0) b += host_elems(p.cover) * 8;
                            mb += message_bytes(task_inputs(hp, p, true));
                        }
                        double full = 0;
                        if (p.real >= 0 && j == 0) full += host_elems(hp.node_vars[p.real]) * esize * 2;
                        if (mine(c)) hp.alg_bytes_full += full + mb;
                    }
                    task_bytes.push_back(b + mb);
                }
                continue;
            }
            tk.mode = phase;
            tk.psi_off = mine(c) && !p.unit ? p.arena_off : 0;          // other ranks' tasks are not executed here
            tk.bel_off = phase == 1 && !p.unit ? (mine(c) ? p.arena_off : 0) : -1;   // virtual cliques that keep a table too (scratch)
            tk.unit = p.unit ? 1 : 0;
            // (distribute: the inputs that are not children come first - the parent's message, the clique's static table)
            const std::vector<TaskInput> in = task_inputs(hp, p, phase == 1);
            std::vector<int> out_seps;
            if (phase == 0) out_seps.push_back(p.psep);
            else for (int k : p.children) out_seps.push_back(hp.pn[k].psep);
            const double steps_scale = p.tmix && p.trow > 0 ? (double)(1 << hp.TB) / (double)p.trow : 1.0;     // (as in level_work)
            const double share = std::min(1.0, (double)p.phys_elems * steps_scale / std::max(1.0, lvl_elems[phase][p.owner][p.depth]));
            // (mixed-radix rows are a quarter of a full row or less, and whole variables - 2 or 3 bits - go in or out of the
            //  loops together: such cliques may always use the 64 rows a workgroup can hold)
            const int blg = p.tmix ? hp.TB + JT_MAX_ITER_LOG2 : block_log2_for(phase, p.depth, p.owner, p.layout != 4);
            const int variant = phase == 0 ? (hp.multiset ? JT_K_MULTI_COLLECT : JT_K_COLLECT0 + nch) : JT_K_DIST_P0C0 + 4 * (p.psep >= 0 ? 1 : 0) + nch;
            const int rc = add_task(tk, phase, in, out_seps, hp.block_log2 > 0 ? std::max(hp.block_log2, hp.TB) : blg, share, variant);
            if (rc != JTP_OK) return rc;
            const int ti = (int)hp.tasks.size() - 1;
            (phase == 0 ? p.collect_task : p.distribute_task) = ti;
            for (size_t j = 0; j < out_seps.size(); ++j) (phase == 0 ? hp.ps[out_seps[j]].up_npart : hp.ps[out_seps[j]].dn_npart) = hp.tasks[ti].msg[JT_MAX_IN + j].npart;
            // algorithmic bytes: clique table read (+ belief written), messages.  A unit clique counts what its
            // potential IS - the static table (doubles), read once per pass, and no belief; `full` counts every clique at its
            // full shape in the storage type, read and belief written (8d to the letter)
            double b = 0, full = 0;
            if (p.real >= 0) full += host_elems(hp.node_vars[p.real]) * esize * (phase == 1 ? 2 : 1);
            if (p.real >= 0 && !p.unit) b += host_elems(hp.node_vars[p.real]) * esize * (phase == 1 ? 2 : 1);
            if (p.stat >= 0) b += host_elems(p.cover) * 8;
            double mb = message_bytes(in);
            for (int k : out_seps) if (hp.ps[k].node >= 0) mb += host_elems(hp.ps[k].vars) * 8 * (phase == 1 ? 2 : 1);
            b += mb;
            if (mine(c)) hp.alg_bytes_full += full + mb;
            task_bytes.push_back(b);
            if (hp.multiset) {
                const double tb = p.real >= 0 ? host_elems(hp.node_vars[p.real]) * esize : 0.0;
                hp.alg_table_bytes += tb;
                hp.alg_msg_bytes += b - tb;
            }
        }
    }

    return JTP_OK;
}

int PlanBuilder::messages() {
    // Settle in place (jt_msg_settle): plans whose cliques mostly sit on latency-bound levels - a clique or two - (chains),
    // and (round 3) the tasks of any plan's NARROW levels - the top of a tree, a rank's share of one - where the hand-over
    // between dependent levels is what the level costs (a rank's share of config 4 at 8 ranks: 201.5 -> 195 us, config 4
    // itself +-0; A/B on one box).  Not on streaming levels: there the re-loads of thousands of waiting workgroups cost more
    // than the round trips they save (round 2).  Tried on top of it and dropped: a two-stage wait - one lane polls an entry
    // the PRODUCER waits for, then every thread spins on its own entries - so that a message is taken one load after it
    // becomes visible: config 2 5.47 -> 5.87 ms, the rank share 195 -> 199 us (the spinning threads of a whole level cost
    // the producers more than the saved round trip).
    for (JtTask &tk : hp.tasks) {
        if (tk.kind != 0) continue;
        const PNode &p = hp.pn[tk.pnode];
        const int phase = ((int)(&tk - hp.tasks.data()) == p.collect_task) ? 0 : 1;
        tk.settle = (hp.chain_plan || lvl_elems[phase][p.owner][p.depth] <= hp.knobs.settle_level_elems) ? 1 : 0;
    }
    // ---- message arena ----------------------------------------------------------------------
    // A message written as many partial copies costs every consuming workgroup (sub-box x copies)
    // loads before it can start, on the critical path of the small levels near the root.  From
    // `red_min` copies on, a reduce task behind the producer sums them once and consumers read the sum.
    // (multi-set plans: 2 and 8 measured within 4 % of each other on the width-20 tree, 8 ahead)
    // Single-set plans (round 2, with eight entry loads in flight per staging thread): only messages of 64 copies get a
    // reduce task - config 3 13.3 -> 12.8 ms, config 4 within noise for any threshold from 8 up.
    // Chains keep 8: there a reduce task between two levels beats every consumer summing eight copies (config 2 6.5 against 6.85 ms).
    const int red_min = hp.knobs.reduce_min >= 0 ? hp.knobs.reduce_min : (hp.multiset || hp.chain_plan ? 8 : 64);
    hp.msg_doubles = 0;
    for (auto &s : hp.ps) {
        if (!mine(s.child) && !mine(s.parent)) continue;
        int64_t n = (int64_t)1 << s.nbits;
        s.up_off = s.up_roff = hp.msg_doubles;
        hp.msg_doubles += n * s.up_npart;
        s.dn_off = s.dn_roff = hp.msg_doubles;
        hp.msg_doubles += n * s.dn_npart;
        s.up_rnpart = s.up_npart;
        s.dn_rnpart = s.dn_npart;
        for (int up = 0; up < 2; ++up) {
            const int npart = up ? s.up_npart : s.dn_npart;
            if (red_min <= 0 || npart < red_min) continue;
            (up ? s.up_roff : s.dn_roff) = hp.msg_doubles;
            (up ? s.up_rnpart : s.dn_rnpart) = 1;
            hp.msg_doubles += n;
            JtTask rt;
            memset(&rt, 0, sizeof rt);
            rt.kind = 1;
            rt.pnode = up ? s.child : s.parent;              // the producer: its rank runs the reduction
            rt.nbits = s.nbits;
            rt.n_in = rt.n_out = 1;
            rt.bel_off = -1;
            rt.msg[0].off = up ? s.up_off : s.dn_off;
            rt.msg[0].npart = npart;
            rt.msg[0].pstride = (int32_t)n;
            rt.msg[0].same_launch = 1;
            rt.msg[JT_MAX_IN].off = up ? s.up_roff : s.dn_roff;
            rt.msg[JT_MAX_IN].npart = 1;
            rt.msg[JT_MAX_IN].pstride = (int32_t)n;
            while (((int64_t)JT_REDUCE_ENTRIES << rt.nF) < n) {
                rt.f_x[rt.nF] = (uint32_t)JT_REDUCE_ENTRIES << rt.nF;
                rt.nF++;
            }
            (up ? s.up_red_task : s.dn_red_task) = (int)hp.tasks.size();
            hp.tasks.push_back(rt);
            hp.task_variant.push_back(JT_K_REDUCE_LEVEL);
            task_bytes.push_back(0.0);
        }
        hp.msg_doubles = (hp.msg_doubles + 1) & ~(int64_t)1;
    }
    // who writes what each task reads (finish() turns it into JtMsg::same_launch once the launches are known)
    hp.task_producers.assign(hp.tasks.size(), std::vector<int>());
    for (const PSep &sp : hp.ps) {
        if (sp.up_red_task >= 0) hp.task_producers[sp.up_red_task] = {hp.pn[sp.child].collect_task};
        if (sp.dn_red_task >= 0) hp.task_producers[sp.dn_red_task] = {down_writer(hp, sp)};
    }
    for (size_t t = 0; t < hp.tasks.size(); ++t) {
        JtTask &tk = hp.tasks[t];
        if (tk.kind != 0) continue;
        const PNode &p = hp.pn[tk.pnode];
        const bool collect = (int)t == p.collect_task;
        int served = -1;                                         // a downward-message task (multi-set plans, unit cliques): which child?
        if (!collect)
            for (size_t j = 0; j < p.down_tasks.size(); ++j)
                if (p.down_tasks[j] == (int)t) served = (int)j;
        const std::vector<TaskInput> in = task_inputs(hp, p, !collect, served);
        hp.task_producers[t] = input_producers(hp, in);
        place_inputs(hp, in, tk, false);
        // same_launch: the producer runs in the same dataflow launch as this consumer (same phase, same
        // rank).  Upward messages read during distribute were finished by the collect launch, messages
        // of other ranks arrive by an exchange between launches: those are read with ordinary loads.
        for (size_t k = 0; k < in.size(); ++k) {
            // (a downward-message task: the parent's message is formed by the parent's task in this phase; else: a replicated
            //  parent forms the message on this rank, in this phase, with no exchange in between)
            if (in[k].kind == TaskInput::PARENT) tk.msg[k].same_launch = served >= 0 || hp.pn[p.parent].owner == p.owner || hp.pn[p.parent].owner == ALL;
            if (in[k].kind == TaskInput::CHILD) tk.msg[k].same_launch = collect && hp.pn[in[k].child].owner == p.owner;
        }
        if (served >= 0) tk.msg[JT_MAX_IN].off = hp.ps[hp.pn[p.children[served]].psep].dn_off;
        else if (collect) tk.msg[JT_MAX_IN].off = hp.ps[p.psep].up_off;
        else
            for (size_t j = 0; j < p.children.size(); ++j) tk.msg[JT_MAX_IN + j].off = hp.ps[hp.pn[p.children[j]].psep].dn_off;
    }
    return fold_marginals();
}

// Marginals named at plan creation (jtp_tree_desc.fold_*; round 6).  `JunctionTree.propagate` returns factor marginals only
// (junctiontree/junctiontree.py:264-274, 327-331), and a clique that keeps no table has no belief to take them from: the read-out forms
// psi x (every incoming table) again, per request list, after the propagate - on a tree of such cliques a third of a propagate's work,
// run behind it.  Here the same tasks (jtp_plan_marginal_task: up to three requests of one clique per pass) become tasks OF the
// propagate: on the level of the clique's downward messages - their inputs are the final messages, the parent's produced one level up
// in this launch - where the dependent levels leave slots idle, writing partial copies into a region of the message arena that
// jtp_get_marginals unpacks.  Only the lean pass runs them (jt_unit_lean<..., NOUT>): single-set plans of one rank, no mixed-radix
// rows, not a chain (whose distribute kernel is built without them); the engine falls back to the read-out wherever they did not run.
int PlanBuilder::fold_marginals() {
    if (hp.folded.empty() || hp.multiset || hp.n_ranks != 1 || hp.tmix || hp.chain_plan || hp.knobs.no_fold || hp.knobs.no_lean || (hp.knobs.debug & ~2)) return JTP_OK;
    const int n = (int)hp.folded.size();
    if (hp.knobs.fold < 0) {
        // Where the folded tasks pay (measured, profiles/r06_ab_fold_placement.txt): their workgroups are free where the levels of the
        // distribute phase leave resident slots of the chip idle (the column-sweep tree of config 3: every level under 1 024 workgroups,
        // marginals 3.7 -> 0.24 ms for 1.4 ms more propagate), and cost their own work where the levels fill the chip (the min-fill tree:
        // 6 % of the levels under 1 024; +0.28 ms of propagate for 0.21 ms less read-out, wherever in the launch they are put) - there the
        // read-out's launch, which waits for nobody, does the same work no slower.  So: fold where at least half of the distribute
        // levels are under `fold_slots` workgroups (256 CUs x 4).  JTP_FOLD=1: wherever possible; 0: nowhere.
        std::vector<long> level_blocks(maxdepth + 1, 0);
        for (int c = 0; c < NP; ++c) {
            const PNode &p = hp.pn[c];
            if (!mine(c)) continue;
            if (!p.down_tasks.empty()) {
                for (int t : p.down_tasks) level_blocks[p.depth] += 1L << hp.tasks[t].nF;
            } else if (p.distribute_task >= 0) level_blocks[p.depth] += 1L << hp.tasks[p.distribute_task].nF;
        }
        int levels = 0, idle = 0;
        for (long b : level_blocks)
            if (b > 0) ++levels, idle += b < hp.knobs.fold_slots ? 1 : 0;
        if (2 * idle < levels) return JTP_OK;
    }
    std::vector<int32_t> wanted(hp.fold_cliques);            // (-1: a clique with a belief table - jt_marginals reads that)
    for (int i = 0; i < n; ++i)
        if (!hp.pn[wanted[i]].unit || hp.pn[wanted[i]].real < 0 || !mine(wanted[i])) wanted[i] = -1;
    const std::vector<std::vector<int>> groups = jtp_group_requests(wanted.data(), n, hp.knobs.marg_group, false);
    for (const std::vector<int> &grp : groups) {
        const int c = hp.fold_cliques[grp[0]];
        const PNode &p = hp.pn[c];
        std::vector<std::vector<int>> ovs;
        bool ok = true;
        for (int i : grp) {
            std::vector<int> ov(hp.fold_var_ids.begin() + hp.fold_var_off[i], hp.fold_var_ids.begin() + hp.fold_var_off[i + 1]);
            for (size_t a = 0; a < ov.size(); ++a) {
                ok = ok && find_var(p.vars, ov[a]) >= 0;
                for (size_t b = 0; b < a; ++b) ok = ok && ov[a] != ov[b];
            }
            ovs.push_back(ov);
        }
        if (!ok) continue;                                   // (a malformed request: jtp_get_marginals will say so)
        JtTask tk;
        std::vector<int32_t> tab;
        std::vector<int> out_bits, npart;
        std::vector<JtBlock> blk;
        std::string err2;
        if (jtp_plan_marginal_task(hp, c, ovs, tk, tab, out_bits, npart, blk, err2, true) != JTP_OK) continue;
        if (tk.n_in > JT_MAX_IN || tk.n_out > JT_MAX_OUT || tk.vgroups) continue;
        tk.fold = 1;
        tk.debug = hp.knobs.debug;
        tk.itab_off = (int64_t)hp.itab.size();
        if (tk.tmap_off >= 0) tk.tmap_off += tk.itab_off;
        hp.itab.insert(hp.itab.end(), tab.begin(), tab.end());
        const int t = (int)hp.tasks.size();
        for (size_t j = 0; j < grp.size(); ++j) {
            HostPlan::FoldReq &fr = hp.folded[grp[j]];
            fr.task = t, fr.j = (int)j, fr.npart = npart[j], fr.out_bits = out_bits[j], fr.off = hp.msg_doubles;
            tk.msg[JT_MAX_IN + j].off = hp.msg_doubles;
            hp.msg_doubles += ((int64_t)1 << out_bits[j]) * npart[j];
            hp.msg_doubles = (hp.msg_doubles + 1) & ~(int64_t)1;
        }
        hp.tasks.push_back(tk);
        hp.task_variant.push_back(JT_K_DISTRIBUTE_LEVEL);
        task_bytes.push_back(0.0);
        hp.task_producers.push_back(input_producers(hp, task_inputs(hp, p, true)));      // (finish(): JtMsg::same_launch)
        hp.pn[c].fold_tasks.push_back(t);
    }
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------

std::vector<std::vector<int>> jtp_group_requests(const int32_t *cliques, int n, int per_group, bool one_each) {
    std::vector<std::vector<int>> groups;
    std::map<int, int> open;                                 // clique -> its group that still has room
    for (int i = 0; i < n; ++i) {
        const int c = cliques[i];
        if (c < 0) continue;
        auto it = open.find(c);
        if (one_each || it == open.end() || (int)groups[it->second].size() >= per_group) {
            open[c] = (int)groups.size();
            groups.push_back(std::vector<int>());
        }
        groups[open[c]].push_back(i);
    }
    return groups;
}

// What the two read-out tasks share.  Their inputs are the clique's final incoming tables - the parent's downward message, the static
// table, every child's upward message - read where consumers read them, never from a launch that is still running (same_launch 0).
// Loops, then the task's own table buffer (the clique's thread map behind its rows), the inputs' places, the workgroup records.
static int finish_readout_task(const HostPlan &hp, JtTask &tk, std::vector<int32_t> &itab, const std::vector<TaskInput> &in,
                               const std::vector<MsgView> &outs, int block_log2, std::vector<JtBlock> &blocks, std::string &err) {
    const PNode &p = hp.pn[tk.pnode];
    const std::vector<MsgView> ins = input_views(hp, p, in);
    if ((int)ins.size() > JT_MAX_IN) FAIL(JTP_EUNSUPPORTED, "clique with %zu neighbours", ins.size());
    int rc = plan_loops(hp, p, tk, itab, ins, outs, block_log2, err);
    tk.itab_off = 0;
    if (rc != JTP_OK) return rc;
    if (hp.tmix || p.unit) {
        tk.tmap_off = (int64_t)itab.size();
        itab.insert(itab.end(), p.tmap.begin(), p.tmap.end());
        itab.insert(itab.end(), p.vmap.begin(), p.vmap.end());
    }
    place_inputs(hp, in, tk, true);
    blocks.clear();
    for (uint32_t f = 0; f < (1u << tk.nF); ++f) blocks.push_back(jtp_make_block(hp, tk, 0u, f));
    return JTP_OK;
}

int jtp_plan_marginal_task(const HostPlan &hp, int pnode, const std::vector<std::vector<int>> &out_vars,
                           JtTask &tk, std::vector<int32_t> &itab, std::vector<int> &out_bits, std::vector<int> &npart,
                           std::vector<JtBlock> &blocks, std::string &err, bool with_neighbours) {
    const PNode &p = hp.pn[pnode];
    if (out_vars.empty() || (int)out_vars.size() > JT_MAX_OUT) FAIL(JTP_EINVAL, "internal: %zu marginals in one task", out_vars.size());
    if (with_neighbours && out_vars.size() != 1 && !p.unit) FAIL(JTP_EINVAL, "internal: several marginals in one task of a multi-set plan");
    if (p.unit && !with_neighbours) FAIL(JTP_EINVAL, "internal: a unit clique keeps no belief table to marginalise");
    std::vector<PSep> seps(out_vars.size());
    out_bits.clear();
    for (size_t j = 0; j < out_vars.size(); ++j) {
        PSep &s = seps[j];
        s.vars.assign(out_vars[j].rbegin(), out_vars[j].rend());       // last requested variable = lowest bits
        int bit = 0;
        for (int v : s.vars) {
            if (find_var(p.vars, v) < 0) FAIL(JTP_EINVAL, "variable %d is not in clique %d", v, p.real);
            s.pos.push_back(bit);
            s.nb.push_back(hp.vbits[v]);
            bit += hp.vbits[v];
        }
        s.nbits = bit;
        if (bit > 28) FAIL(JTP_EUNSUPPORTED, "marginal with %d index bits", bit);
        out_bits.push_back(bit);
    }
    memset(&tk, 0, sizeof tk);
    tk.pnode = pnode;
    tk.psi_off = p.unit ? 0 : p.arena_off;
    tk.bel_off = -1;
    tk.unit = p.unit ? 1 : 0;
    tk.mode = 0;                                 // (several outputs: every one of them the sum over its own complement)
    // multi-set plans keep no belief table: the marginal is taken of psi * (every incoming message) directly
    const std::vector<TaskInput> in = with_neighbours ? task_inputs(hp, p, true) : std::vector<TaskInput>();
    std::vector<MsgView> outs;
    for (const PSep &s : seps) outs.push_back(make_view(p, s, -1, true));
    // (a pass over a belief table with nothing to stage: the longest workgroups the loop allows, fewest partial copies)
    const int rc = finish_readout_task(hp, tk, itab, in, outs, with_neighbours ? 14 : (hp.knobs.marg_block_log2 > 0 ? hp.knobs.marg_block_log2 : hp.TB + JT_MAX_ITER_LOG2), blocks, err);
    if (rc != JTP_OK) return rc;
    npart.clear();
    for (size_t j = 0; j < out_vars.size(); ++j) npart.push_back(tk.msg[JT_MAX_IN + j].npart);
    return JTP_OK;
}

int jtp_plan_belief_task(const HostPlan &hp, int pnode, JtTask &tk, std::vector<int32_t> &itab,
                         std::vector<JtBlock> &blocks, std::string &err) {
    const PNode &p = hp.pn[pnode];
    memset(&tk, 0, sizeof tk);
    tk.pnode = pnode;
    tk.psi_off = p.unit ? 0 : p.arena_off;
    tk.bel_off = p.arena_off;                    // (a unit clique: its place in the scratch arena, PlanBuilder::arenas)
    tk.unit = p.unit ? 1 : 0;
    tk.mode = 1;
    return finish_readout_task(hp, tk, itab, task_inputs(hp, p, true), {}, 14, blocks, err);
}
