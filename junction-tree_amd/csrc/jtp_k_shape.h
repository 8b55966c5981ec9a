// Message kernels, family `shape` (jtp_inst_shape_*.hip): one kernel per clique shape, jt_collect<T, NCH> and
// jt_distribute<T, HASP, NCH> (map of the units: jtp_kernels.hip.h).
#pragma once
#include "jtp_kernels.hip.h"
#include "jtp_k_pass.h"

// Per-shape entry points, used when the plan is built with JTP_SPLIT_VARIANTS (profiling aid:
// one launch per (level, neighbour count), so rocprofv3 attributes time to each shape).
template <typename T, int NCH>
__global__ __launch_bounds__(JT_THREADS) void jt_collect(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                         const T *__restrict__ psi, T *__restrict__ bel,
                                                         double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    jt_pass<T, NCH, 1, 0>(tasks[bk.task], bk, itab, psi, bel, msg, fl, blockIdx.x);
}

template <typename T, int HASP, int NCH>
__global__ __launch_bounds__(JT_THREADS) void jt_distribute(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk, const int *__restrict__ itab,
                                                            const T *__restrict__ psi, T *__restrict__ bel,
                                                            double *__restrict__ msg, JtFlow fl) {
    const JtBlock &bk = blk[blockIdx.x];
    jt_pass<T, HASP + NCH, NCH, 1>(tasks[bk.task], bk, itab, psi, bel, msg, fl, blockIdx.x);
}
