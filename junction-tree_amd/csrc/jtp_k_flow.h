// Message kernels, families `flow`, `both` and `bothm` (jtp_inst_flow_*.hip, jtp_inst_both_*.hip, jtp_inst_bothm_*.hip): the
// dataflow launches of single-set plans - one per phase (jt_collect_flow, jt_distribute_flow, jt_distribute_flow_chain) or one per
// propagate (jt_propagate_flow, jt_propagate_flow_marg); the ticket and the order they rest on: jtp_k_common.h, jt_flow_ticket
// (map of the units: jtp_kernels.hip.h).
#pragma once
#include "jtp_kernels.hip.h"
#include "jtp_k_reduce.h"
#include "jtp_k_unit.h"

#ifndef JT_FLOW_WAVES
#define JT_FLOW_WAVES 4          // (A/B builds: -DJT_FLOW_WAVES=5 / 6 - fewer registers, more workgroups per CU)
#endif
template <typename T>
__global__ __launch_bounds__(JT_THREADS, JT_FLOW_WAVES) void jt_collect_flow(const JtTask *__restrict__ tasks,
                                                              const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                              const T *__restrict__ psi, T *__restrict__ bel,
                                                              double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];        // ticket, wait flags and candidates, parked flush records
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
    const uint32_t ticket = jt_flow_ticket(fl, flow_ctl);
    const JtBlock &bk = blk[ticket];
    if (jt_lean_block<T>(bk, itab, msg, fl, flow_ctl)) return;
    const JtTask &tk = tasks[bk.task];
    if (tk.kind != 0) {
        jt_reduce<true>(tk, bk, msg, fl);
        return;
    }
    if (tk.unit) {
        jt_unit_collect<T, true, false>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
        return;
    }
    switch (tk.n_in) {
        case 0: jt_pass<T, 0, 1, 0, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 1: jt_pass<T, 1, 1, 0, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 2: jt_pass<T, 2, 1, 0, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        default: jt_pass<T, 3, 1, 0, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
    }
}

// jt_collect_flow with KEEP = true: the row loads carry the workgroup's cache policy (JtTask::keep_rows).  The collect launch of plans
// that keep rows and launch their phases separately (a rank's share of a tree): the distribute launch - jt_propagate_flow - finds in
// the Infinity Cache what this one left there.  A kernel of its own: chains and plans that keep nothing run jt_collect_flow, whose row
// loop has no choice to make.
template <typename T>
__global__ __launch_bounds__(JT_THREADS, JT_FLOW_WAVES) void jt_collect_flow_keep(const JtTask *__restrict__ tasks,
                                                                   const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                                   const T *__restrict__ psi, T *__restrict__ bel,
                                                                   double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
    const uint32_t ticket = jt_flow_ticket(fl, flow_ctl);
    const JtBlock &bk = blk[ticket];
    if (jt_lean_block<T>(bk, itab, msg, fl, flow_ctl)) return;
    const JtTask &tk = tasks[bk.task];
    if (tk.kind != 0) {
        jt_reduce<true>(tk, bk, msg, fl);
        return;
    }
    if (tk.unit) {
        jt_unit_collect<T, true, false>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
        return;
    }
    switch (tk.n_in) {
        case 0: jt_pass<T, 0, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 1: jt_pass<T, 1, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 2: jt_pass<T, 2, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        default: jt_pass<T, 3, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
    }
}

template <typename T, bool EARLY = false>
__device__ __forceinline__ void jt_distribute_flow_body(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                        const int *__restrict__ itab, const T *__restrict__ psi, T *__restrict__ bel,
                                                        double *__restrict__ msg, const JtFlow &fl, uint32_t *flow_ctl) {
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
    const uint32_t ticket = jt_flow_ticket(fl, flow_ctl);
    const JtBlock &bk = blk[ticket];
    if (jt_lean_block<T>(bk, itab, msg, fl, flow_ctl)) return;
    const JtTask &tk = tasks[bk.task];
    if (tk.kind != 0) {
        jt_reduce<true>(tk, bk, msg, fl);
        return;
    }
    if (tk.unit) {           // (a unit clique's downward messages are marginalisations of their own: mode 0 in the distribute phase)
        if (tk.mode == 0) jt_unit_collect<T, true, false>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
        else jt_unit_distribute<T, true, false>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
        return;
    }
    switch ((tk.n_in - tk.n_out) * 4 + tk.n_out) {
        case 0: jt_pass<T, 0, 0, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 1: jt_pass<T, 1, 1, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 2: jt_pass<T, 2, 2, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 3: jt_pass<T, 3, 3, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 4: jt_pass<T, 1, 0, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 5: jt_pass<T, 2, 1, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 6: jt_pass<T, 3, 2, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        default: jt_pass<T, 4, 3, 1, true, EARLY>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
    }
}

// Both phases in ONE launch (round 3; plans whose phases follow each other without an exchange in between, and whose
// messages are small beside their tables - jtp_plan.cpp: finish()): the block list of the distribute phase simply
// follows that of the collect phase, and the root's distribute workgroups wait for the last upward messages like any
// other consumer.  Saves the second launch's cold start and the gap between the launches (~10 us of 620 on the width-20
// tree); every message is then read through to memory (JtMsg::same_launch), also the upward messages the distribute
// tasks read, because their producers ran in THIS launch.
// FOLD: the build that also runs the marginal tasks folded into the propagate (jt_propagate_flow_marg: plans that have such tasks).  A
// kernel of its own because the plans without them - every hot path of bench.py - pay for the code otherwise: config 3 5.92 -> 6.07 ms
// with one kernel for both (A/B on one box, profiles/r06_ab_fold_hot_path.txt).
template <typename T, bool FOLD>
__device__ __forceinline__ void jt_propagate_flow_body(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                       const int *__restrict__ itab, const T *__restrict__ psi, T *__restrict__ bel,
                                                       double *__restrict__ msg, const JtFlow &fl, uint32_t *flow_ctl) {
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
    const uint32_t ticket = jt_flow_ticket(fl, flow_ctl);
    const JtBlock &bk = blk[ticket];
    if (jt_lean_block<T, FOLD>(bk, itab, msg, fl, flow_ctl)) return;
    const JtTask &tk = tasks[bk.task];
    if (tk.kind != 0) {
        jt_reduce<true>(tk, bk, msg, fl);
        return;
    }
    if (tk.unit) {
        if (tk.mode == 0) jt_unit_collect<T, true, false>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
        else jt_unit_distribute<T, true, false>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
        return;
    }
    if (tk.mode == 0) {
        switch (tk.n_in) {
            case 0: jt_pass<T, 0, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
            case 1: jt_pass<T, 1, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
            case 2: jt_pass<T, 2, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
            default: jt_pass<T, 3, 1, 0, true, true, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        }
        return;
    }
    switch ((tk.n_in - tk.n_out) * 4 + tk.n_out) {
        case 0: jt_pass<T, 0, 0, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 1: jt_pass<T, 1, 1, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 2: jt_pass<T, 2, 2, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 3: jt_pass<T, 3, 3, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 4: jt_pass<T, 1, 0, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 5: jt_pass<T, 2, 1, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        case 6: jt_pass<T, 3, 2, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
        default: jt_pass<T, 4, 3, 1, true, false, false, true>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry); break;
    }
}

template <typename T>
__global__ __launch_bounds__(JT_THREADS, JT_FLOW_WAVES) void jt_propagate_flow(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                                   const int *__restrict__ itab, const T *__restrict__ psi,
                                                                   T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];
    jt_propagate_flow_body<T, false>(tasks, blk, itab, psi, bel, msg, fl, flow_ctl);
}

template <typename T>
__global__ __launch_bounds__(JT_THREADS, JT_FLOW_WAVES) void jt_propagate_flow_marg(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                                        const int *__restrict__ itab, const T *__restrict__ psi,
                                                                        T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];
    jt_propagate_flow_body<T, true>(tasks, blk, itab, psi, bel, msg, fl, flow_ctl);
}

// Two builds of the distribute pass.  Compiled for four waves per SIMD (128 registers, a few spills) a CU holds four
// workgroups instead of three and a third more table rows are in flight: config 4 0.4505 -> 0.4385 ms (A/B on one box).
// On plans made of latency-bound levels (chains, JtTask::settle) the spills sit on the dependent path - config 2
// 3.56 -> 3.69 ms - so those run the build without (168 registers, three waves).
template <typename T>
__global__ __launch_bounds__(JT_THREADS, JT_FLOW_WAVES) void jt_distribute_flow(const JtTask *__restrict__ tasks,
                                                                    const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                                    const T *__restrict__ psi, T *__restrict__ bel,
                                                                    double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];        // ticket, wait flags and candidates, parked flush records
    jt_distribute_flow_body<T>(tasks, blk, itab, psi, bel, msg, fl, flow_ctl);
}

#ifndef JT_CHAIN_WAVES
#define JT_CHAIN_WAVES 3
#endif
template <typename T>
__global__ __launch_bounds__(JT_THREADS, JT_CHAIN_WAVES) void jt_distribute_flow_chain(const JtTask *__restrict__ tasks,
                                                                          const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                                          const T *__restrict__ psi, T *__restrict__ bel,
                                                                          double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];        // ticket, wait flags and candidates, parked flush records
    jt_distribute_flow_body<T, true>(tasks, blk, itab, psi, bel, msg, fl, flow_ctl);   // (flush records kept in registers)
}
