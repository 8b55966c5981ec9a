// Message kernels: jt_reduce, the sum of a message's partial copies (map of the units: jtp_kernels.hip.h).
#pragma once
#include "jtp_k_common.h"

// Reduce task: entry i of the sum = the sum of the partial copies of entry i, JT_REDUCE_ENTRIES entries per
// workgroup.  Wave w sums copies [w * per, (w + 1) * per) of its lane's entry with ALL its loads in flight at once
// (up to 16 per lane; a message of 64 copies used to cost eight dependent round trips - 40 us on a loaded chip, the
// whole critical path of the top of a tree), the four partial sums are then added in wave order: a fixed order,
// bit-reproducible.  In a dataflow launch the copies may still be in the making: a wave loads until none of its
// entries is the "unwritten" marker (one poller per wave; the producers are the workgroups just ahead in the list).
// MULTI (multi-set plans; their messages have few copies): the four waves take two evidence sets each instead of a
// quarter of the copies - set w, then set w + 4 - and every wave stores its own sums.
template <bool FLOW, bool MULTI = false>
__device__ __forceinline__ void jt_reduce(const JtTask &tk, const JtBlock &bk, double *__restrict__ msg_arena,
                                          const JtFlow &fl, const int sidv = 0) {
    __shared__ double red_part[4][JT_REDUCE_ENTRIES];
    __shared__ uint32_t red_abort;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)1 << tk.nbits;
    const int64_t i = (int64_t)bk.xF + lane;
    const JtMsg &src = tk.msg[0];
    const bool active = i < n;
    const int npart = src.npart;
    if constexpr (MULTI) {
        for (int set = wave; set < JT_MSETS; set += 4) {
            double *arena = msg_arena + (int64_t)__builtin_amdgcn_readlane(sidv, set) * fl.set_stride;      // (MULTI: jt_mpass, `sidv`)
            const double *copies = arena + fl.cur_off + src.off + (active ? i : 0);
            double sum = 0.0;
            uint64_t t0 = 0;
            for (int p0 = 0; p0 < npart; p0 += 16) {
                double c[16];
                for (;;) {
                    const double *unready = nullptr;
#pragma unroll
                    for (int u = 0; u < 16; ++u) c[u] = (active && p0 + u < npart) ? jt_msg_load<FLOW>(copies + (int64_t)(p0 + u) * src.pstride) : 0.0;
#pragma unroll
                    for (int u = 0; u < 16; ++u)
                        if (FLOW && jt_unwritten(c[u])) unready = copies + (int64_t)(p0 + u) * src.pstride;
                    if (!FLOW || (fl.dbg & 4)) break;
                    const uint64_t have = __ballot(unready != nullptr);
                    if (have == 0) break;
                    bool give_up = false;
                    if (lane == (int)__builtin_ctzll(have)) {
                        if (t0 == 0) t0 = __builtin_amdgcn_s_memrealtime();
                        unsigned spins = 0;
                        while (jt_unwritten(jt_msg_load<true>(unready))) {
                            if (spins < 4) __builtin_amdgcn_s_sleep(8);
                            else __builtin_amdgcn_s_sleep(32);
                            if ((++spins & 15u) == 0) {
                                if (__hip_atomic_load(fl.sync + JT_SYNC_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) give_up = true;
                                else if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {
                                    __hip_atomic_store(fl.sync + JT_SYNC_ABORT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    __hip_atomic_store(fl.host_abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                    give_up = true;
                                }
                                if (give_up) break;
                            }
                        }
                    }
                    if (__any(give_up)) return;              // (no barrier below on this path: every wave finds the flag itself)
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) sum += c[u];
            }
            if (active) {
                const int64_t at = tk.msg[JT_MAX_IN].off + i;
                jt_msg_store<FLOW>(arena + fl.cur_off + at, sum);
                if (fl.oth_off >= 0) arena[fl.oth_off + at] = __longlong_as_double((long long)JT_UNWRITTEN);
            }
        }
        return;
    }
    const int per = (npart + 3) >> 2;
    const int p_lo = wave * per, p_hi = (p_lo + per < npart) ? p_lo + per : npart;
    const double *copies = msg_arena + fl.cur_off + src.off + (active ? i : 0);
    const int64_t ps = src.pstride;
    double sum = 0.0;
    uint64_t t0 = 0;
    bool gave_up = false;
    if (threadIdx.x == 0) red_abort = 0;
    for (int p0 = p_lo; p0 < p_hi && !gave_up; p0 += 16) {
        double c[16];
        for (;;) {
            const double *unready = nullptr;
#pragma unroll
            for (int u = 0; u < 16; ++u) c[u] = (active && p0 + u < p_hi) ? jt_msg_load<FLOW>(copies + (int64_t)(p0 + u) * ps) : 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (FLOW && jt_unwritten(c[u])) unready = copies + (int64_t)(p0 + u) * ps;
            if (!FLOW || (fl.dbg & 4)) break;
            const uint64_t have = __ballot(unready != nullptr);
            if (have == 0) break;
            bool give_up = false;
            if (lane == (int)__builtin_ctzll(have)) {
                if (t0 == 0) t0 = __builtin_amdgcn_s_memrealtime();
                unsigned spins = 0;
                while (jt_unwritten(jt_msg_load<true>(unready))) {
                    if (spins < 4) __builtin_amdgcn_s_sleep(8);
                    else __builtin_amdgcn_s_sleep(32);
                    if ((++spins & 15u) == 0) {
                        if (__hip_atomic_load(fl.sync + JT_SYNC_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) give_up = true;
                        else if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {
                            __hip_atomic_store(fl.sync + JT_SYNC_ABORT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(fl.host_abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            give_up = true;
                        }
                        if (give_up) break;
                    }
                }
            }
            if (__any(give_up)) {
                gave_up = true;
                break;
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) sum += c[u];
    }
    __syncthreads();                               // (red_abort = 0 is visible)
    if (gave_up && lane == 0) red_abort = 1;
    red_part[wave][lane] = sum;
    __syncthreads();
    if (red_abort != 0) return;                    // the grid drains; the host runs the propagate again per level
    if (wave == 0 && active) {
        const double total = ((red_part[0][lane] + red_part[1][lane]) + red_part[2][lane]) + red_part[3][lane];
        const int64_t at = tk.msg[JT_MAX_IN].off + i;
        jt_msg_store<FLOW>(msg_arena + fl.cur_off + at, total);
        if (fl.oth_off >= 0) msg_arena[fl.oth_off + at] = __longlong_as_double((long long)JT_UNWRITTEN);
    }
}
