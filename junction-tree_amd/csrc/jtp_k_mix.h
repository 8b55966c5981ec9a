// Message kernels, families `mix` and `mixc` (jtp_inst_mix_*.hip, jtp_inst_mixc_*.hip): the passes of plans with a mixed-radix
// thread part, one row per step (VG = false) or two (the compact form, VG = true) (map of the units: jtp_kernels.hip.h).
#pragma once
#include "jtp_kernels.hip.h"
#include "jtp_k_reduce.h"
#include "jtp_k_unit.h"

#ifndef JT_MIX_WAVES
#define JT_MIX_WAVES 4          // waves per SIMD the dataflow *_mix kernels are compiled for (3: no spills, and 6-16 % slower on cardinality 3 / 5 trees, 3 % faster on cardinality 6 - A/B on one box)
#endif

// Kernels of plans with a mixed-radix thread part (HostPlan::tmix: some clique stores the variables of its low index
// bits at their TRUE cardinalities): the same passes with TMIX = true - a thread reaches its elements through the
// clique's thread map (JtTask::tmap_off) - for every launch style the engine uses with such plans: one launch per
// phase (dataflow), one per level, and the read-out task lists.
template <typename T, bool FLOW, bool VG>
__device__ __forceinline__ void jt_collect_mix_v(const JtTask &tk, const JtBlock &bk, const int *__restrict__ itab, const T *__restrict__ psi,
                                               T *__restrict__ bel, double *__restrict__ msg, const JtFlow &fl, uint32_t bindex,
                                               uint32_t *flow_ctl, uint64_t t_entry) {
    if (tk.unit) {
        if constexpr (FLOW) jt_unit_collect<T, true, true>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry);
        else jt_unit_single<T, true>(tk, bk, itab, psi, bel, msg, fl, bindex);      // (level launches and read-out lists)
        return;
    }
    if (tk.n_out > 1) {                        // read-out tasks: several marginals of one belief table per pass
        if (tk.n_out == 2) jt_pass<T, 0, 2, 0, FLOW, true, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry);
        else jt_pass<T, 0, 3, 0, FLOW, true, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry);
        return;
    }
    switch (tk.n_in) {
        case 0: jt_pass<T, 0, 1, 0, FLOW, true, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        case 1: jt_pass<T, 1, 1, 0, FLOW, true, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        case 2: jt_pass<T, 2, 1, 0, FLOW, true, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        case 3: jt_pass<T, 3, 1, 0, FLOW, true, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        default: jt_pass<T, 4, 1, 0, FLOW, true, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
    }
}
template <typename T, bool FLOW, bool VG>
__device__ __forceinline__ void jt_distribute_mix_v(const JtTask &tk, const JtBlock &bk, const int *__restrict__ itab, const T *__restrict__ psi,
                                                  T *__restrict__ bel, double *__restrict__ msg, const JtFlow &fl, uint32_t bindex,
                                                  uint32_t *flow_ctl, uint64_t t_entry) {
    if (tk.unit) {
        if (tk.mode == 0) jt_collect_mix_v<T, FLOW, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry);      // (a downward message of a unit clique: its own marginalisation)
        else if (tk.n_out == 0 && !FLOW) jt_unit_single<T, true>(tk, bk, itab, psi, bel, msg, fl, bindex);       // (read-out: up to four incoming tables)
        else jt_unit_distribute<T, FLOW, true>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry);
        return;
    }
    if (tk.n_out == 0) {                       // belief only (leaves, and the read-out of multi-neighbour cliques)
        switch (tk.n_in) {
            case 0: jt_pass<T, 0, 0, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
            case 1: jt_pass<T, 1, 0, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
            case 2: jt_pass<T, 2, 0, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
            case 3: jt_pass<T, 3, 0, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
            default: jt_pass<T, 4, 0, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        }
        return;
    }
    switch ((tk.n_in - tk.n_out) * 4 + tk.n_out) {
        case 1: jt_pass<T, 1, 1, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        case 2: jt_pass<T, 2, 2, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        case 3: jt_pass<T, 3, 3, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        case 5: jt_pass<T, 2, 1, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        case 6: jt_pass<T, 3, 2, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
        default: jt_pass<T, 4, 3, 1, FLOW, false, true, false, false, true, VG>(tk, bk, itab, psi, bel, msg, fl, bindex, flow_ctl, t_entry); break;
    }
}

// (VG: the compact form of the rows, two per step - JtTask::vgroups == 2 on every table-keeping task of the plan, HostPlan::tmix_compact -
//  is a kernel of its own: built into one kernel with the one-row form, either lost 10-20 %)
template <typename T, bool VG>
__global__ __launch_bounds__(JT_THREADS, 3) void jt_collect_level_mix(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                                      const int *__restrict__ itab, const T *__restrict__ psi,
                                                                      T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    jt_collect_mix_v<T, false, VG>(tasks[bk.task], bk, itab, psi, bel, msg, fl, blockIdx.x, nullptr, 0);
}
template <typename T, bool VG>
__global__ __launch_bounds__(JT_THREADS, 3) void jt_distribute_level_mix(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                                         const int *__restrict__ itab, const T *__restrict__ psi,
                                                                         T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    jt_distribute_mix_v<T, false, VG>(tasks[bk.task], bk, itab, psi, bel, msg, fl, blockIdx.x, nullptr, 0);
}
// (read-out task lists: marginals - mode 0 - and beliefs of multi-neighbour cliques - mode 1)
template <typename T, bool VG>
__global__ __launch_bounds__(JT_THREADS, 3) void jt_single_mix(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                               const int *__restrict__ itab, const T *__restrict__ psi,
                                                               T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    const JtTask &tk = tasks[bk.task];
    if (tk.mode == 0) jt_collect_mix_v<T, false, VG>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x, nullptr, 0);
    else jt_distribute_mix_v<T, false, VG>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x, nullptr, 0);
}
template <typename T, bool VG>
__global__ __launch_bounds__(JT_THREADS, JT_MIX_WAVES) void jt_collect_flow_mix(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                                     const int *__restrict__ itab, const T *__restrict__ psi,
                                                                     T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
    const uint32_t ticket = jt_flow_ticket(fl, flow_ctl);
    const JtBlock &bk = blk[ticket];
    const JtTask &tk = tasks[bk.task];
    if (tk.kind != 0) jt_reduce<true>(tk, bk, msg, fl);
    else jt_collect_mix_v<T, true, VG>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
}
template <typename T, bool VG>
__global__ __launch_bounds__(JT_THREADS, JT_MIX_WAVES) void jt_distribute_flow_mix(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                                        const int *__restrict__ itab, const T *__restrict__ psi,
                                                                        T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
    const uint32_t ticket = jt_flow_ticket(fl, flow_ctl);
    const JtBlock &bk = blk[ticket];
    const JtTask &tk = tasks[bk.task];
    if (tk.kind != 0) jt_reduce<true>(tk, bk, msg, fl);
    else jt_distribute_mix_v<T, true, VG>(tk, bk, itab, psi, bel, msg, fl, ticket, flow_ctl, t_entry);
}
