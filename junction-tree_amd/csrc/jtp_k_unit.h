// Message kernels: the dispatch of unit tasks - jt_unit_collect, jt_unit_distribute, jt_unit_single - to the generic pass
// (JT_UNIT_PASS, JT_UNIT_BELIEF) or the lean one (map of the units: jtp_kernels.hip.h).
#pragma once
#include "jtp_k_lean.h"
#include "jtp_k_pass.h"

// Unit tasks (JtTask::unit): their shapes differ from the table-keeping tasks' - the static table is one more incoming one
// (collect: up to three children, or the static table and two; distribute: the parent's message and / or the static table, then
// up to three children) - so they are dispatched here, by every kernel that may meet one.
#define JT_UNIT_PASS(NIN, NOUT, MODE) jt_pass<T, NIN, NOUT, MODE, FLOW, true, TMIX, false, true, false>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry)
#define JT_UNIT_BELIEF(NIN) jt_pass<T, NIN, 0, 1, FLOW, true, TMIX, false, true, true>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry)
template <typename T, bool FLOW, bool TMIX, bool FOLD = false>
__device__ __forceinline__ void jt_unit_collect(const JtTask &tk, const JtBlock &bk, const int *__restrict__ itab, const T *__restrict__ psi,
                                                T *__restrict__ bel, double *__restrict__ msg, const JtFlow &fl, uint32_t bindex,
                                                uint32_t *flow_ctl, uint64_t t_entry) {
    if constexpr (FOLD && !TMIX && !FLOW) {
        // a marginal task folded into the propagate: the lean pass or nothing.  Only the per-level distribute kernel meets one here
        // (FOLD): dataflow workgroups of such tasks are taken by jt_lean_block, and no other launch list holds them.
        if (tk.fold) {
            if (tk.lean_off > 0 && (fl.ev == nullptr || fl.ev[2 * tk.pnode] == 0))
                jt_unit_lean_readout<T, false>(*reinterpret_cast<const JtLean *>(itab + tk.lean_off), bk, itab, msg, fl);
            return;
        }
    }
    if constexpr (!TMIX) {
        // (round 6) a task of one outgoing message and single-copy inputs on a clique that hosts no observed variable of this
        // evidence set (the engine passes no table at all when nothing is observed): the lean pass
        if (tk.lean_off > 0 && (fl.ev == nullptr || fl.ev[2 * tk.pnode] == 0)) {
            jt_unit_lean_dispatch<T, FLOW>(*reinterpret_cast<const JtLean *>(itab + tk.lean_off), bk, itab, msg, fl, flow_ctl);
            return;
        }
    }
    switch (tk.n_in) {
        case 0: JT_UNIT_PASS(0, 1, 0); break;
        case 1: JT_UNIT_PASS(1, 1, 0); break;
        case 2: JT_UNIT_PASS(2, 1, 0); break;
        default: JT_UNIT_PASS(3, 1, 0); break;
    }
}
template <typename T, bool FLOW, bool TMIX>
__device__ __forceinline__ void jt_unit_distribute(const JtTask &tk, const JtBlock &bk, const int *__restrict__ itab, const T *__restrict__ psi,
                                                   T *__restrict__ bel, double *__restrict__ msg, const JtFlow &fl, uint32_t bindex,
                                                   uint32_t *flow_ctl, uint64_t t_entry) {
    switch ((tk.n_in - tk.n_out) * 4 + tk.n_out) {        // (inputs that are not children) x children
        case 0: JT_UNIT_PASS(0, 0, 1); break;
        case 1: JT_UNIT_PASS(1, 1, 1); break;
        case 2: JT_UNIT_PASS(2, 2, 1); break;
        case 3: JT_UNIT_PASS(3, 3, 1); break;
        case 4: JT_UNIT_PASS(1, 0, 1); break;
        case 5: JT_UNIT_PASS(2, 1, 1); break;
        case 6: JT_UNIT_PASS(3, 2, 1); break;
        case 7: JT_UNIT_PASS(4, 3, 1); break;
        case 8: JT_UNIT_PASS(2, 0, 1); break;
        case 9: JT_UNIT_PASS(3, 1, 1); break;
        default: JT_UNIT_PASS(4, 2, 1); break;
    }
}
// read-out tasks of unit cliques (no launch waits on anything): one to three marginals of psi x every incoming table per pass,
// or the belief itself into the scratch arena
template <typename T, bool TMIX>
__device__ __forceinline__ void jt_unit_single(const JtTask &tk, const JtBlock &bk, const int *__restrict__ itab, const T *__restrict__ psi,
                                               T *__restrict__ bel, double *__restrict__ msg, const JtFlow &fl, uint32_t bindex) {
    constexpr bool FLOW = false;
    uint32_t *flow_ctl = nullptr;
    const uint64_t t_entry = 0;
    if (tk.mode == 0) {
        switch (tk.n_out * 8 + tk.n_in) {
            case 8: JT_UNIT_PASS(0, 1, 0); break;
            case 9: JT_UNIT_PASS(1, 1, 0); break;
            case 10: JT_UNIT_PASS(2, 1, 0); break;
            case 11: JT_UNIT_PASS(3, 1, 0); break;
            case 12: JT_UNIT_PASS(4, 1, 0); break;
            case 16: JT_UNIT_PASS(0, 2, 0); break;
            case 17: JT_UNIT_PASS(1, 2, 0); break;
            case 18: JT_UNIT_PASS(2, 2, 0); break;
            case 19: JT_UNIT_PASS(3, 2, 0); break;
            case 20: JT_UNIT_PASS(4, 2, 0); break;
            case 24: JT_UNIT_PASS(0, 3, 0); break;
            case 25: JT_UNIT_PASS(1, 3, 0); break;
            case 26: JT_UNIT_PASS(2, 3, 0); break;
            case 27: JT_UNIT_PASS(3, 3, 0); break;
            default: JT_UNIT_PASS(4, 3, 0); break;
        }
    } else {
        switch (tk.n_in) {            // (the belief itself, into the scratch arena)
            case 0: JT_UNIT_BELIEF(0); break;
            case 1: JT_UNIT_BELIEF(1); break;
            case 2: JT_UNIT_BELIEF(2); break;
            case 3: JT_UNIT_BELIEF(3); break;
            default: JT_UNIT_BELIEF(4); break;
        }
    }
}
