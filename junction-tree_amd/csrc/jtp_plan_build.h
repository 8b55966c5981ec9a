// The planner's units (internal; jtp_plan.h is the planner's face to the engine).  jtp_build_plan runs the stages of PlanBuilder in order:
//   jtp_plan.cpp           knobs (jtp_read_knobs); the tree stages - read_description, link_nodes, reroot, decide_units, binarise, depths,
//                          arenas, level_work - and block_log2_for; jtp_build_plan
//   jtp_plan_layout.cpp    layouts, searched_order: the bit order of every clique and separator table
//   jtp_plan_loops.cpp     the cost model of one task and its search (search_loops), plan_loops: the F / A / R split and every index
//                          table of a task; jtp_make_block, jtp_make_lean
//   jtp_plan_tasks.cpp     the ONE description of a task's incoming tables (task_inputs: which, in which order; input_place: where each
//                          lives and who writes it) and everything derived from it: make_tasks, messages, fold_marginals, the two read-out
//                          entry points (jtp_plan_marginal_task, jtp_plan_belief_task); jtp_group_requests
//   jtp_plan_schedule.cpp  schedule, finish, sampling
//   jtp_plan_json.cpp      jtp_plan_to_json
#pragma once
#include "jtp_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>

#define FAIL(code, ...)                                   \
    do {                                                  \
        char _b[512];                                     \
        snprintf(_b, sizeof _b, __VA_ARGS__);             \
        err = _b;                                         \
        return code;                                      \
    } while (0)

static inline int ceil_log2(int k) {
    int b = 0;
    while ((1 << b) < k) ++b;
    return b;
}

static inline int popc(uint32_t x) { return __builtin_popcount(x); }

// variable -> (pos, nb) lookup inside a node layout
static inline int find_var(const std::vector<int> &vars, int v) {
    for (size_t i = 0; i < vars.size(); ++i)
        if (vars[i] == v) return (int)i;
    return -1;
}

struct MsgView {
    int psep = -1;
    bool up = true;              // which buffer of the separator
    int8_t dst[32];              // clique bit -> message bit, -1 if the bit is not in the message
    uint32_t mask = 0;           // clique bits that are in the message
    int msg_bits = 0;
};

// ---- jtp_plan_loops.cpp ---------------------------------------------------------------------------------------------------
struct CostEnv {
    int TB = 10, EB = 2, nbits = 0;
    bool dist = false;           // distribute pass: the table is written as well as read
    bool unit = false;           // unit clique: no table rows are loaded or stored, no element ring in LDS
    int max_iter_log2 = JT_MAX_ITER_LOG2;
    double share = 1.0;          // part of the chip this clique can count on (its share of the level's elements)
    double fill = 1.0;           // rows that exist / rows of the index space (variables stored at their true cardinality)
    long lds_cap = 150 * 1024;
    int red_log2 = 6;            // partial copies from 2^red_log2 on are summed by a reduce task, fewer by the consumers
    bool chain = false;          // latency-bound plan: a consumer that waits for several producers pays a staging attempt each
    int min_loop_log2 = JT_MIN_ITER_LOG2;   // chains: JT_MIN_LOOP_LOG2 (two-iteration workgroups: config 2 6.46 -> 5.75 ms; at the top
                                            // of a tree they cost 3 %: an 8-rank share of config 4 205 -> 212 us)
    std::vector<uint32_t> units; // atomic groups of bits above the thread part (a compact variable stays together)
};

struct LoopChoice {
    uint32_t L = 0;
    double us = 1e30;
    long lds = 0;
};

// best loop set of one task: every subset of the units with 2..max_iter_log2 bits (`exhaustive`), or units added
// one at a time, cheapest first
LoopChoice search_loops(const CostEnv &e, const std::vector<uint32_t> &ins, const std::vector<uint32_t> &outs, bool exhaustive);
// What the cost model takes one workgroup's life for - start, staging and flush (`fix_us`), a row of the distribute pass (`iter_us`) -
// and its streaming rate: the constants schedule() tells a bandwidth-bound level from a narrow one by (JtTask::keep_rows).
void jtp_keep_cost(double &fix_us, double &iter_us, double &bytes_per_us);
// Choose the F / A / R split of the high bits of a task of clique `p` and fill every index table of the task.
int plan_loops(const HostPlan &hp, const PNode &p, JtTask &tk, std::vector<int32_t> &itab, const std::vector<MsgView> &ins,
               const std::vector<MsgView> &outs, int block_log2, std::string &err, int strict_budget = 0, double share = 1.0);

// ---- jtp_plan_tasks.cpp ---------------------------------------------------------------------------------------------------
// One incoming table of a task.  The rule, for every task of clique p: the parent's downward message (if the task takes it and p has
// a parent), the clique's static table (a unit clique's potential, seen as one more message: JtMsg::fixed), the children's upward
// messages in child order - minus the one child a per-child task forms the downward message of.
struct TaskInput {
    enum Kind { PARENT, STATIC, CHILD } kind;
    int index;                   // PARENT, CHILD: the separator (HostPlan::ps); STATIC: HostPlan::statics
    int child;                   // CHILD: its pnode
};

// The planner proper: one method per stage of jtp_build_plan, run in order; what the stages share lives here.
struct PlanBuilder {
    const jtp_tree_desc *d;
    HostPlan &hp;
    std::string &err;
    int N = 0, NP = 0, esize = 4, ALL = 1, maxdepth = 0;
    std::vector<std::vector<double>> lvl_elems[2];       // [phase][owner][level]: elements, to size workgroups
    std::vector<double> task_bytes;                      // algorithmic bytes of every task

    PlanBuilder(const jtp_tree_desc *desc, HostPlan &plan, std::string &e) : d(desc), hp(plan), err(e) {}
    bool mine(int pnode) const { return hp.pn[pnode].owner == hp.rank || hp.pn[pnode].owner == ALL; }
    double host_elems(const std::vector<int> &vars) const {
        double e = 1;
        for (int v : vars) e *= hp.card[v];
        return e;
    }
    int block_log2_for(int phase, int level, int owner, bool tiny_rule = true) const;
    int read_description();      // validate and copy the caller's description
    int link_nodes();            // cliques, separators, reachability, replicated part
    int fold_marginals();        // marginal tasks named at plan creation, behind messages()
    int reroot();                // single rank: root at the tree's centre
    int decide_units();          // which cliques keep no table (all ones, or their factors' product as a static table)
    int binarise();              // at most three children per node (virtual all-ones cliques)
    int depths();
    int layouts();               // bit order of every clique and separator table
    bool searched_order(int c, const std::vector<int> &host, const std::vector<int> &seps, std::vector<int> &order);   // layout policy 4
    bool wants_static(const PNode &p) const { return p.unit && p.real >= 0 && !p.cover.empty(); }
    int arenas();                // table offsets, host<->device conversion records
    int level_work();
    int make_tasks();            // one task per (clique, phase) - multi-set plans and unit cliques: per (clique, child) in distribute
    int add_task(JtTask tk, int phase, const std::vector<TaskInput> &in, const std::vector<int> &out_seps, int block_log2, double share, int variant);
    double message_bytes(const std::vector<TaskInput> &in) const;
    int messages();              // message arena, reduce tasks, message offsets of every task
    int schedule();              // launches, workgroup records, exchange schedule
    int finish();                // dataflow segments, sync words, time-stamp region
    int sampling();              // sampling schedule over the caller's tree (jtp_sample)
    int run() {
        int (PlanBuilder::*stages[])() = {&PlanBuilder::read_description, &PlanBuilder::link_nodes, &PlanBuilder::reroot,
                                          &PlanBuilder::decide_units, &PlanBuilder::binarise, &PlanBuilder::depths, &PlanBuilder::layouts,
                                          &PlanBuilder::arenas, &PlanBuilder::level_work, &PlanBuilder::make_tasks,
                                          &PlanBuilder::messages, &PlanBuilder::schedule, &PlanBuilder::finish, &PlanBuilder::sampling};
        for (auto stage : stages) {
            const int rc = (this->*stage)();
            if (rc != JTP_OK) return rc;
        }
        return JTP_OK;
    }
};
