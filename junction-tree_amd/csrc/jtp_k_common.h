// Message kernels, the ground every pass stands on (map of the units: jtp_kernels.hip.h).  Holds the constants of the row ring,
// JtVec, the LDS-DMA load with its hand-counted wait, the lane shuffles and sums, the diagnostic time stamps (JT_STAMP: the slots
// tools/_stamps.py reads), the marker protocol of dataflow launches (jt_msg_load / jt_msg_store / jt_msg_settle), the split of a
// sub-box entry's address (jt_sub_lo / jt_sub_hi), and the control words and the ticket of a dataflow workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "jtp_internal.h"

constexpr int JT_U = 4;         // loop iterations whose element loads are in flight (the row ring: JT_RING_BYTES = JT_U slots of 1 KiB per wave)
constexpr int JT_UT = 4;        // ... of a mixed-radix plan (rows gathered into registers, *_mix kernels); 8 was 2-4 % slower, A/B on one box

template <typename T> struct JtVec;
template <> struct JtVec<float> { using type = float4; };
template <> struct JtVec<double> { using type = double2; };

// LDS-DMA: 16 bytes per lane from global memory straight into LDS at `lds_dst` + lane * 16
// (wave-uniform byte address).  Not tracked by the compiler's s_waitcnt insertion: callers count
// vmcnt themselves (cdna_hip_programming.md section 5.7).
// `reused` (uniform): the row will be read again soon by workgroups of the same XCD - multi-set plans of several groups of
// evidence sets, whose grid puts the groups' workgroups for one record next to each other on one XCD: default cache policy
// there (16 sets 1.78 -> 1.73 ms, 64 sets 6.09 -> 6.04 ms, 8 sets = one group unchanged; A/B on one box); everywhere else a row is read once per pass: non-temporal.
__device__ __forceinline__ void jt_dma16(const void *gsrc, uint32_t lds_dst, bool reused = false) {
    unsigned keep;
    if (reused) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(gsrc), "s"(lds_dst)
                     : "memory");
        return;
    }
    // non-temporal policy on the table stream (rows are read once per phase, by one CU): config 4 0.610 -> 0.5975 ms against the
    // default policy, A/B on one box over three runs each
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}
template <int N>
__device__ __forceinline__ void jt_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ double jt_shfl_xor(double v, int laneMask) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, laneMask, 64);
    hi = __shfl_xor(hi, laneMask, 64);
    return __hiloint2double(hi, lo);
}

// v of lane + N (N = 1, 2, 4, 8; inside a row of 16 lanes, 0.0 beyond it) without a trip through the LDS crossbar: two DPP moves.
// A sum over lane bit b only has to arrive in the lanes whose bit b is clear (the lanes that store it), and lane + 2^b is their
// partner of the butterfly: same operands, same order, same double as acc += shfl_xor(acc, 2^b) there.
template <int N>
__device__ __forceinline__ double jt_row_down(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x100 + N, 0xf, 0xf, true);       // row_shl:N
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x100 + N, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// acc[e] += the partner's acc[e] over every lane bit of red_lane, all elements together (no per-element branch, one wait per bit)
template <int VEC>
__device__ __forceinline__ void jt_lane_sums(double (&a)[VEC], const int red_lane) {
    if (red_lane & 1) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] += jt_row_down<1>(a[e]);
    }
    if (red_lane & 2) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] += jt_row_down<2>(a[e]);
    }
    if (red_lane & 4) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] += jt_row_down<4>(a[e]);
    }
    if (red_lane & 8) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] += jt_row_down<8>(a[e]);
    }
#pragma unroll
    for (int b = 4; b < 6; ++b) {
        if ((red_lane >> b) & 1) {
            double t[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[e] = jt_shfl_xor(a[e], 1 << b);
#pragma unroll
            for (int e = 0; e < VEC; ++e) a[e] += t[e];
        }
    }
}

// Diagnostic time stamps (builds with -DJT_STAMPS only: `python junction-tree_amd/build.py --out stamps.so -DJT_STAMPS`, plans
// made with JTP_DEBUG=2): lane 0 of a workgroup stores the 100 MHz clock at stage boundaries into its JT_NSTAMP slots of the
// time-stamp region (JtTask::dbg_off).  In the product build the macro is empty: no registers, no branches, no stores.
// Slots: 0 entry, 1 first element loads issued, 2 end of the first staging attempt, 3 staged, 4 constants read,
// 5-8 after loop steps 0-3, 9 loop done, 10 epilogues done (barrier), 11 flush stores issued, 12 flush stores retired,
// 13 staging attempts (a count, not a time), 14 end of the last wait for a producer (0: never waited).
#define JT_NSTAMP 16
#ifdef JT_STAMPS
#define JT_STAMP_AT(slot, value) do { if ((dbg & 2) && threadIdx.x == 0) stamp_out[slot] = (double)(value); } while (0)
#else
#define JT_STAMP_AT(slot, value) do { } while (0)
#endif
#define JT_STAMP(slot) JT_STAMP_AT(slot, __builtin_amdgcn_s_memrealtime())

// message-index bit of sub-box index bit b (free_pos[] packed four per word)
#define JT_FPOS(fp, b) (((fp)[(b) >> 2] >> (8 * ((b) & 3))) & 0xffu)

// Dataflow launches (FLOW = true): ONE launch covers all levels of a phase, so a message may still be
// in the making (by workgroups of the same launch) when its consumer starts.  Every message entry
// carries its own "ready" state: the arena half of this propagate holds JT_UNWRITTEN markers until the
// producer stores the value (64-bit stores are single-copy atomic), so the consumer loads its sub-box,
// and while it finds a marker it waits on that entry and loads again.  Loads and stores of message
// entries are agent-scope atomics here (they go through to memory: the L2 caches of the eight XCDs
// are not coherent with each other inside a launch); no fences, no counters.
template <int N, typename F>
__device__ __forceinline__ void jt_static_for(F &&f) {
    if constexpr (N > 0) {
        jt_static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

__device__ __forceinline__ bool jt_unwritten(double v) { return (uint64_t)__double_as_longlong(v) == JT_UNWRITTEN; }

template <bool FLOW>
__device__ __forceinline__ double jt_msg_load(const double *p) {
    if constexpr (FLOW)
        return __longlong_as_double(__hip_atomic_load(reinterpret_cast<const long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    else
        return *p;
}

// (FLOW) through to memory only where the producer may be running in this launch (JtMsg::same_launch)
template <bool FLOW>
__device__ __forceinline__ double jt_msg_load(const double *p, bool through) {
    if constexpr (FLOW) return through ? jt_msg_load<true>(p) : *p;
    else return *p;
}

template <bool FLOW>
__device__ __forceinline__ void jt_msg_store(double *p, double v) {
    if constexpr (FLOW)
        __hip_atomic_store(reinterpret_cast<long long *>(p), __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

// (FLOW) From the second staging attempt on - the producer is known to be flushing: the polled entry has just
// arrived - a thread that finds one of ITS entries still unwritten loads that entry again for up to ~1.5 us
// instead of sending the whole workgroup round the poll-and-reload loop once more (measured: the loop then
// ends at the second attempt nearly always).
template <bool FLOW>
__device__ __forceinline__ double jt_msg_settle(const double *p, double v, bool through, int attempt) {
    if constexpr (FLOW) {
        if (attempt > 0 && through) {
            for (int spins = 0; spins < 24 && jt_unwritten(v); ++spins) {
                __builtin_amdgcn_s_sleep(2);
                v = jt_msg_load<true>(p);
            }
        }
    }
    return v;
}

// Where entry i of a workgroup's sub-box of a message lives in the message: the sub-box index is a bit-deposit of i into the
// message's index (bit b of i lands on message bit free_pos[b]).  The deposit is linear over disjoint bit groups, so the flush
// splits it once per outgoing message into the part of a thread's own low eight index bits (jt_sub_lo: a vector value) and a
// 32-row table of the bits above them, row j in lane j (jt_sub_hi, read with v_readlane): an entry's address costs one add.
// (Round 3 also rebuilt the STAGING loop on this split, every message in lock step: fewer instructions by far, and slower on
//  every config - 2 % on config 4, 1.5 % on config 3, 12 % on config 2, A/B on one box - so staging keeps the loop of round 2.)
__device__ __forceinline__ uint32_t jt_sub_lo(const uint32_t (&fp)[4], int nfree, int i) {
    uint32_t g = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b)
        if (b < nfree) g += (((uint32_t)i >> b) & 1u) << JT_FPOS(fp, b);
    return g;
}
__device__ __forceinline__ uint32_t jt_sub_hi(const uint32_t (&fp)[4], int nfree, int lane) {
    uint32_t g = 0;
#pragma unroll
    for (int b = 8; b < JT_MAX_FREE; ++b)
        if (b < nfree) g += (((uint32_t)lane >> (b - 8)) & 1u) << JT_FPOS(fp, b);
    return g;
}

// flow_ctl, the control words a dataflow kernel keeps in LDS: [0] the ticket, [1] "gave up waiting", [4..27] two sets of wave flags
// and wait candidates (one per staging attempt, alternating), then the flush records a distribute pass parks: [JT_MAX_OUT][8] words
constexpr int JT_CTL_PARK = 28;
constexpr int JT_CTL_WORDS = JT_CTL_PARK + 8 * JT_MAX_OUT;

// Dataflow entry points: ONE launch per phase.  Workgroups take the block list in blockIdx order; the
// waits cannot deadlock as long as no workgroup is dispatched before one with a lower index (then the
// lowest unfinished workgroup is always running, and it never waits on an unfinished one).  That is
// how the hardware dispatches; should it ever not be, the wait times out, the host notices and runs
// the propagate again with one launch per level (jtp_propagate.hip: check_flow).  With JTP_FLOW_TICKETS
// the list position is drawn from an atomic counter instead, which needs no such assumption but costs
// a memory round trip before anything else can start (~10% on the benchmark tree).
__device__ __forceinline__ uint32_t jt_flow_ticket(const JtFlow &fl, uint32_t *flow_ctl) {
    if (fl.ticket_idx == 0xffffffffu) return blockIdx.x;
    if (threadIdx.x == 0)
        flow_ctl[0] = __hip_atomic_fetch_add(fl.sync + fl.ticket_idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - fl.ticket_base;
    __syncthreads();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)flow_ctl[0]);
}
