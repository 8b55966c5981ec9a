// Message kernels, family `level` (jtp_inst_level_*.hip): one launch per tree level - jt_reduce_level, jt_collect_level,
// jt_distribute_level - and the read-out task lists jt_single, jt_lean_single and jt_marginals (map of the units: jtp_kernels.hip.h).
#pragma once
#include "jtp_kernels.hip.h"
#include "jtp_k_reduce.h"
#include "jtp_k_unit.h"

template <typename T>
__global__ __launch_bounds__(JT_THREADS) void jt_reduce_level(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                              const int *__restrict__ itab, const T *__restrict__ psi,
                                                              T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    jt_reduce<false>(tasks[bk.task], bk, msg, fl);
}

// Entry points (these names appear in rocprofv3 traces).  One launch covers every clique of
// one tree level, whatever its number of neighbours: the workgroup dispatches on its task.
template <typename T>
__global__ __launch_bounds__(JT_THREADS, 4) void jt_collect_level(const JtTask *__restrict__ tasks,
                                                               const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                               const T *__restrict__ psi, T *__restrict__ bel,
                                                               double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    const JtTask &tk = tasks[bk.task];
    if (tk.unit) {
        jt_unit_collect<T, false, false>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x, nullptr, 0);
        return;
    }
    switch (tk.n_in) {
        case 0: jt_pass<T, 0, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 1: jt_pass<T, 1, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 2: jt_pass<T, 2, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        default: jt_pass<T, 3, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
    }
}

template <typename T>
__global__ __launch_bounds__(JT_THREADS, 3) void jt_distribute_level(const JtTask *__restrict__ tasks,
                                                                  const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                                  const T *__restrict__ psi, T *__restrict__ bel,
                                                                  double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    const JtTask &tk = tasks[bk.task];
    if (tk.unit) {           // (a unit clique's downward messages are marginalisations of their own: mode 0 in the distribute phase)
        if (tk.mode == 0) jt_unit_collect<T, false, false, true>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x, nullptr, 0);
        else jt_unit_distribute<T, false, false>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x, nullptr, 0);
        return;
    }
    switch ((tk.n_in - tk.n_out) * 4 + tk.n_out) {
        case 0: jt_pass<T, 0, 0, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 1: jt_pass<T, 1, 1, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 2: jt_pass<T, 2, 2, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 3: jt_pass<T, 3, 3, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 4: jt_pass<T, 1, 0, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 5: jt_pass<T, 2, 1, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 6: jt_pass<T, 3, 2, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        default: jt_pass<T, 4, 3, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
    }
}

// One task list of single-set passes of any shape (read-out of multi-set plans: beliefs and marginals formed on
// demand from the shared table and one set's final messages; up to four incoming messages).
template <typename T>
__global__ __launch_bounds__(JT_THREADS) void jt_single(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                        const int *__restrict__ itab, const T *__restrict__ psi,
                                                        T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    const JtTask &tk = tasks[bk.task];
    if (tk.unit) {
        jt_unit_single<T, false>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x);
        return;
    }
    if (tk.mode == 0) {
        switch (tk.n_in) {
            case 0: jt_pass<T, 0, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            case 1: jt_pass<T, 1, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            case 2: jt_pass<T, 2, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            case 3: jt_pass<T, 3, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            default: jt_pass<T, 4, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        }
    } else {                                   // belief only: psi * every incoming message
        switch (tk.n_in) {
            case 0: jt_pass<T, 0, 0, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            case 1: jt_pass<T, 1, 0, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            case 2: jt_pass<T, 2, 0, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            case 3: jt_pass<T, 3, 0, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
            default: jt_pass<T, 4, 0, 1>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        }
    }
}

// Marginals of unit cliques by the lean pass (round 6): every task of the list has a lean record (jtp_get_marginals makes them) and the
// evidence set observes nothing (the engine sends the list through jt_single otherwise).  A kernel of its own: jt_single holds the
// generic passes of up to four inputs and three outputs, whose registers would halve the occupancy of these loops.
template <typename T>
__global__ __launch_bounds__(JT_THREADS, 4) void jt_lean_single(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                                const int *__restrict__ itab, const T *__restrict__ psi,
                                                                T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    jt_unit_lean_readout<T>(*reinterpret_cast<const JtLean *>(itab + tasks[bk.task].lean_off), bk, itab, msg, fl);
}

// Read-out of single-set plans (jtp_get_marginals, CliqueGraph.marginalize junctiontree.py:229-274): a pass over a BELIEF
// table (the `psi` argument) that forms one to JT_MAX_OUT marginals of it at once - the requests of a model's factors on one
// clique share the read of its table.  Bound: HBM read, sizeof(T) per element.
template <typename T>
__global__ __launch_bounds__(JT_THREADS, 4) void jt_marginals(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                              const int *__restrict__ itab, const T *__restrict__ psi,
                                                              T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    const JtTask &tk = tasks[bk.task];
    switch (tk.n_out) {
        case 1: jt_pass<T, 0, 1, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        case 2: jt_pass<T, 0, 2, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
        default: jt_pass<T, 0, 3, 0>(tk, bk, itab, psi, bel, msg, fl, blockIdx.x); break;
    }
}
