// Message kernels, family `multi` (jtp_inst_multi_*.hip): jt_mpass, the pass that serves JT_MSETS evidence sets over one read of
// a table, and its dataflow entry point jt_multi_flow (map of the units: jtp_kernels.hip.h).
#pragma once
#include "jtp_kernels.hip.h"
#include "jtp_k_reduce.h"

// Multi-set pass (JTP_MULTISET plans): JT_MSETS evidence sets that share ONE copy of
// the clique tables are served by ONE pass over a table.  Per set s of the group
//     out_s[S] = sum_{C \ S} psi[C] * e_s[C] * prod_k in_{k,s}[S_k]
// (collect, every downward message - planned as its own marginalisation with the parent's message and the
// siblings' upward messages as inputs - and every marginal have this shape; e_s = the set's hard evidence).
// A table row travels HBM -> LDS -> registers once and is multiplied into the G sets' message entries:
// HBM bytes per evidence set fall by G, the arithmetic (two to four f64 operations per element and set)
// becomes the bound.  Each set has its own LDS region of SETB bytes with the sub-boxes of its messages at
// the offsets the single-set planner computed; SETB is a compile-time constant so that the G reads of one
// message entry differ only in the instruction's immediate offset.  The sets' message arenas lie
// fl.set_stride doubles apart, their evidence tables fl.ev_stride words apart.
//
// Evidence: the part of a set's (mask, value) that lies in the ROW bits (chunk + loop bits) is uniform per
// row - a row that contradicts it is skipped for that set; the part in the thread bits (16-byte vector, lane,
// wave) is constant over the loop, so it is applied to the register sums in the epilogue, not per element.
// `sidv` (round 6): lane j < G holds the ARENA SLOT of the j-th evidence set this workgroup serves - entries 8 g .. 8 g + 7 of the
// task's active list (JtFlow::act_ids), or simply 8 g + j; `msg0` is the base of ALL the sets' arenas.
template <typename T, int NIN, int SETB, bool ESUM = false>
__device__ __forceinline__ void jt_mpass(const JtTask &tk, const JtBlock &bk, const int *__restrict__ itab,
                                         const T *__restrict__ psi_arena, double *__restrict__ msg0,
                                         const JtFlow &fl, uint32_t *flow_ctl, uint32_t bindex, const int sidv) {
    constexpr int G = JT_MSETS;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int EB = (VEC == 4) ? 2 : 1;
    constexpr int TBITS = EB + 8;
    constexpr int U = JT_U;
    constexpr bool FLOW = true;
    using VT = typename JtVec<T>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const uint32_t xF = bk.xF + (uint32_t)tid * VEC;
    const T *psi = psi_arena + tk.psi_off;
    const int total = tk.total;
    const int rmask = (1 << tk.nR) - 1;
    const int64_t sstride = fl.set_stride;
    int64_t soff[G];                                             // (uniform) where the arena of the s-th set of this workgroup starts
#pragma unroll
    for (int s = 0; s < G; ++s) soff[s] = (int64_t)__builtin_amdgcn_readlane(sidv, s) * sstride;
#ifdef JT_STAMPS
    const int dbg = (fl.dbg & 0x80000000u) ? (tk.debug & ~2) : tk.debug;                      // (time stamps of group 0 only)
    double *stamp_out = msg0 + tk.dbg_off + (int64_t)(fl.blk_base + bindex) * JT_NSTAMP;      // (as in jt_pass)
#else
    const int dbg = tk.debug;
#endif
    JT_STAMP(0);

    const int *gtab = itab + tk.itab_off;
    const T *psi0 = psi_arena + bk.psi_x0 + (uint32_t)tid * VEC;
    const uint32_t ring_lds = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)smem) + (uint32_t)wave * (U * 1024);
    const char *ring = smem + wave * (U * 1024) + lane * 16;
    const T *zero_row = psi_arena + (uint32_t)tid * VEC;         // what rows that do not exist read (JT_NO_ROW)
    const bool chunk_ok = !(bk.flags & JT_BLOCK_INVALID);
#pragma unroll
    for (int u = 0; u < U; ++u)
        jt_dma16(bk.first_x[u] == JT_NO_ROW ? zero_row : psi0 + bk.first_x[u], __builtin_amdgcn_readfirstlane(ring_lds + u * 1024), fl.n_groups > 1);
    int trow[JT_NCOL];
    {
        const int r = lane < total ? lane : total - 1;
        const int4 a = *reinterpret_cast<const int4 *>(gtab + r * JT_NCOL);
        const int4 b = *reinterpret_cast<const int4 *>(gtab + r * JT_NCOL + 4);
        trow[0] = a.x; trow[1] = a.y; trow[2] = a.z; trow[3] = a.w;
        trow[4] = b.x; trow[5] = b.y; trow[6] = b.z; trow[7] = b.w;
    }

    JT_STAMP(1);
    // evidence of the G sets on this clique, set s in lane s of a register pair (read after the first element
    // loads have left: the table is two dependent loads away; kept in vector registers: sixteen more scalars
    // live across the loop made hipcc spill scalars into it)
    uint32_t ev_m = 0, ev_v = 0;
    if (fl.ev != nullptr && lane < G) {
        ev_m = fl.ev[(size_t)sidv * fl.ev_stride + 2 * tk.pnode];
        ev_v = fl.ev[(size_t)sidv * fl.ev_stride + 2 * tk.pnode + 1];
    }
    // ---- stage the incoming sub-boxes of every set (one thread per entry, partial copies summed in copy
    //      order), zero the outgoing ones; wait for entries still marked unwritten (dataflow launches)
    const double *msg_cur = msg0 + fl.cur_off;
    char *sets = smem + JT_RING_BYTES;                       // region of set s: sets + s * SETB
    const JtMsg &mo = tk.msg[JT_MAX_IN];
    uint64_t wait_t0 = 0;
    for (int attempt = 0;; ++attempt) {
        JT_STAMP_AT(13, attempt + 1);
        const double *unready = nullptr;
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            const JtMsg &m = tk.msg[k];
            const int nfree = m.nfree;
            const uint32_t *fpw = reinterpret_cast<const uint32_t *>(m.free_pos);
            const uint32_t fp[4] = {fpw[0], fpw[1], fpw[2], fpw[3]};
            const bool thr_mem = m.same_launch != 0;
            const int n = 1 << nfree;
            // (an upward message whose producer did not run for one of the sets - nothing observed below it: that set's entries are the
            //  evidence-free set's, arena slot 0; bit s of `own` = the producer's list holds the s-th set of this workgroup)
            uint32_t own = 0xffu;
            if (fl.skip != nullptr && m.src_task >= 0)
                own = (uint32_t)__ballot(lane < G && fl.skip[(size_t)m.src_task * fl.cap + (uint32_t)sidv] != 0);
            int64_t from[G];
#pragma unroll
            for (int s = 0; s < G; ++s) from[s] = ((own >> s) & 1u) ? soff[s] : (int64_t)0;
            for (int i = tid; i < n; i += JT_THREADS) {
                int idx = 0;
#pragma unroll
                for (int b = 0; b < JT_MAX_FREE; ++b)
                    if (b < nfree) idx += ((i >> b) & 1) << JT_FPOS(fp, b);
                const double *src = msg_cur + m.off + bk.gbase[k] + idx;
                double sum[G];
#pragma unroll
                for (int s = 0; s < G; ++s) sum[s] = 0.0;
                for (int p = 0; p < m.npart; p += 4) {               // the G sets' copies p .. p+3 in flight together
                    double c[G][4];
#pragma unroll
                    for (int s = 0; s < G; ++s)
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            c[s][u] = (p + u < m.npart) ? jt_msg_load<FLOW>(src + from[s] + (int64_t)(p + u) * m.pstride, thr_mem) : 0.0;
#pragma unroll
                    for (int s = 0; s < G; ++s)
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            sum[s] += c[s][u];
                            if (jt_unwritten(c[s][u])) unready = src + from[s] + (int64_t)(p + u) * m.pstride;
                        }
                }
#pragma unroll
                for (int s = 0; s < G; ++s) reinterpret_cast<double *>(sets + s * SETB + (m.lds_off - JT_RING_BYTES))[i] = sum[s];
            }
        }
        if (attempt == 0) {
            const int n = 1 << mo.nfree;
            for (int i = tid; i < n; i += JT_THREADS)
#pragma unroll
                for (int s = 0; s < G; ++s) reinterpret_cast<double *>(sets + s * SETB + (mo.lds_off - JT_RING_BYTES))[i] = 0.0;
        }
        if constexpr (NIN == 0) {
            __syncthreads();
            break;
        } else {
            if (fl.dbg & 8) unready = msg_cur;                           // fault injection: wait for ever
            uint32_t *slot = flow_ctl + 4 + (attempt & 1) * 12;
            {
                const uint64_t have = __ballot(unready != nullptr);
                if (have != 0 && lane == (int)__builtin_ctzll(have)) {
                    slot[4 + 2 * wave] = (uint32_t)(uintptr_t)unready;
                    slot[5 + 2 * wave] = (uint32_t)((uintptr_t)unready >> 32);
                }
                if (lane == 0) slot[wave] = have != 0 ? 1u : 0u;
            }
            __syncthreads();
            const uint32_t w3 = slot[3], w2 = slot[2], w1 = slot[1], w0 = slot[0];
            if ((w0 | w1 | w2 | w3) == 0) break;
            if (tid == 0) {
                const int cw = w3 ? 3 : (w2 ? 2 : (w1 ? 1 : 0));
                const double *entry = reinterpret_cast<const double *>((uintptr_t)slot[4 + 2 * cw] | ((uintptr_t)slot[5 + 2 * cw] << 32));
                if (wait_t0 == 0) wait_t0 = __builtin_amdgcn_s_memrealtime();
                uint32_t give_up = 0;
                unsigned spins = 0;
                const uint64_t limit = (fl.dbg & 8) ? 2000000ull : 200000000ull;
                while (jt_unwritten(jt_msg_load<true>(entry)) || (fl.dbg & 8)) {
                    if (spins >= 64) __builtin_amdgcn_s_sleep(32);
                    else if (spins >= 16) __builtin_amdgcn_s_sleep(16);
                    if ((++spins & 15u) == 0) {
                        if (__hip_atomic_load(fl.sync + JT_SYNC_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) give_up = 1;
                        else if (__builtin_amdgcn_s_memrealtime() - wait_t0 > limit) {
                            __hip_atomic_store(fl.sync + JT_SYNC_ABORT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(fl.host_abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            give_up = 1;
                        }
                        if (give_up) break;
                    }
                }
                flow_ctl[1] = give_up;
            }
            __syncthreads();
            if (flow_ctl[1] != 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // LDS-DMA loads must land before the wave ends
                return;
            }
        }
    }

    JT_STAMP(3);
    // ---- per-thread constants (read before the first store of the kernel, see jt_pass) ---------------
    int thr_in[NIN > 0 ? NIN : 1], in_lds[NIN > 0 ? NIN : 1], in_edep[NIN > 0 ? NIN : 1];
    int in_ew0[NIN > 0 ? NIN : 1], in_ew1[NIN > 0 ? NIN : 1];
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const JtMsg &m = tk.msg[k];
        int t = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b) t += ((lane >> b) & 1) * m.t_w[b];
#pragma unroll
        for (int b = 0; b < 2; ++b) t += ((wave >> b) & 1) * m.t_w[6 + b];
        thr_in[k] = t;
        in_lds[k] = m.lds_off - JT_RING_BYTES;
        in_edep[k] = m.e_dep;
        in_ew0[k] = m.e_w[0];
        in_ew1[k] = m.e_w[1];
    }
    int thr_out = 0;
    {
#pragma unroll
        for (int b = 0; b < 6; ++b) thr_out += ((lane >> b) & 1) * mo.t_w[b];
#pragma unroll
        for (int b = 0; b < 2; ++b) thr_out += ((wave >> b) & 1) * mo.t_w[6 + b];
    }
    const int o_lds = mo.lds_off - JT_RING_BYTES;
    const int o_rede = mo.red_e, o_redl = mo.red_lane, o_redw = mo.red_wave;
    const int o_ew0 = mo.e_w[0], o_ew1 = mo.e_w[1];
    const int o_nfree = mo.nfree;
    const int64_t o_at = mo.off + (int64_t)bk.pnum[0] * mo.pstride + bk.gbase[JT_MAX_IN];
    const uint32_t *ofpw = reinterpret_cast<const uint32_t *>(mo.free_pos);
    const uint32_t ofp[4] = {ofpw[0], ofpw[1], ofpw[2], ofpw[3]};
    // thread part of the evidence: bit (4 s + e) set = element e of this thread agrees with set s
    constexpr uint32_t TMASK = (1u << TBITS) - 1u;
    uint64_t tmatch = 0;
#pragma unroll
    for (int s = 0; s < G; ++s) {
        const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)ev_m, s) & TMASK, v = (uint32_t)__builtin_amdgcn_readlane((int)ev_v, s);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (((((uint32_t)tid * VEC + e) ^ v) & m) == 0) tmatch |= 1ull << (4 * s + e);
    }
    // row part (chunk and loop bits): lane s keeps set s's mask and value; one compare + ballot per row
    const uint32_t row_m = ev_m & ~TMASK, row_v = ev_v & ~TMASK;
    const bool has_row_ev = __ballot(row_m != 0) != 0;
    uint32_t loop_pos[JT_MAX_ITER_LOG2];                // logical index bit of loop-counter bit t
#pragma unroll
    for (int t = 0; t < JT_MAX_ITER_LOG2; ++t) loop_pos[t] = t < tk.nA + tk.nR ? tk.loop_pos[t] : 31u;
    // ESUM (JtTask::esum): no message and no evidence involves the element bits - the elements of a vector are
    // summed first and ONE accumulator per evidence set is kept
    constexpr int NACC = ESUM ? 1 : VEC;
    double acc[G][NACC];
#pragma unroll
    for (int s = 0; s < G; ++s)
#pragma unroll
        for (int e = 0; e < NACC; ++e) acc[s][e] = 0.0;

    auto epilogue = [&](const int oo) {
        // thread part of the evidence, then the in-thread and cross-lane sums of every set
#pragma unroll
        for (int s = 0; s < G; ++s) {
#pragma unroll
            for (int e = 0; e < NACC; ++e)
                if (!((tmatch >> (4 * s + e)) & 1ull)) acc[s][e] = 0.0;
            if constexpr (!ESUM) {
                if constexpr (VEC == 4) {
                    if (o_rede & 1) {
                        acc[s][0] += acc[s][1];
                        acc[s][2] += acc[s][3];
                    }
                    if (o_rede & 2) {
                        acc[s][0] += acc[s][2];
                        acc[s][1] += acc[s][3];
                    }
                } else {
                    if (o_rede & 1) acc[s][0] += acc[s][1];
                }
            }
        }
        // (lane bits 0-3 through DPP row shifts, every set and element together: jt_lane_sums)
#pragma unroll
        for (int s = 0; s < G; ++s) jt_lane_sums<NACC>(acc[s], o_redl);
        const bool rep = (lane & o_redl) == 0;
        const int slot = oo + thr_out;
        const int nph = 1 << __builtin_popcount((unsigned)o_redw);
        int myph = 0;
        if (o_redw == 1) myph = wave & 1;
        else if (o_redw == 2) myph = wave >> 1;
        else if (o_redw == 3) myph = wave;
        for (int ph = 0; ph < nph; ++ph) {
            if (rep && myph == ph) {
#pragma unroll
                for (int s = 0; s < G; ++s) {
                    double *osub = reinterpret_cast<double *>(sets + s * SETB + o_lds);
#pragma unroll
                    for (int e = 0; e < NACC; ++e) {
                        if ((e & o_rede) == 0) {
                            const int eo = ((e & 1) ? o_ew0 : 0) + ((e & 2) ? o_ew1 : 0);
                            __hip_atomic_fetch_add(&osub[slot + eo], acc[s][e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
            }
            if (nph > 1) __syncthreads();
        }
#pragma unroll
        for (int s = 0; s < G; ++s)
#pragma unroll
            for (int e = 0; e < NACC; ++e) acc[s][e] = 0.0;
    };

#pragma unroll
    for (int c = 0; c < JT_NCOL; ++c) asm volatile("" : "+v"(trow[c]));

    // EDEP: some incoming message depends on the element bits of the 16-byte vector (then every message
    // entry is read per element, four reads; otherwise one read per message serves the four elements).
    // The choice is made once per workgroup, outside the loop: inside, a step has no branch at all, so the
    // LDS reads of one evidence set are in flight while the previous set's products are formed.
    auto step = [&](auto slot_tag, auto edep_tag, auto rowev_tag, const int i) {
        constexpr int SLOT = decltype(slot_tag)::value;
        constexpr bool EDEP = decltype(edep_tag)::value;
        constexpr bool ROWEV = decltype(rowev_tag)::value;      // some set of the group observes a variable on the row bits
        constexpr int NV = EDEP ? VEC : 1;
        jt_wait_vmcnt<U - 1>();
        const VT v = *reinterpret_cast<const VT *>(ring + SLOT * 1024);
        double p[VEC];
        p[0] = (double)v.x;
        p[1] = (double)v.y;
        if constexpr (VEC == 4) {
            p[2] = (double)v.z;
            p[3] = (double)v.w;
        }
        {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int inext = (i + U < total) ? i + U : total - 1;
            const uint32_t xnext = (uint32_t)__builtin_amdgcn_readlane(trow[0], inext);
            jt_dma16((xnext == JT_NO_ROW || !chunk_ok) ? zero_row : psi + (xF + xnext),
                     __builtin_amdgcn_readfirstlane(ring_lds + SLOT * 1024), fl.n_groups > 1);
        }
        uint32_t rowok = 0xffffffffu;                       // bit s: the row agrees with set s
        if constexpr (ROWEV) {
            uint32_t xrow = bk.lxF;                         // LOGICAL index of the row (uniform): chunk + loop bits
#pragma unroll
            for (int t = 0; t < JT_MAX_ITER_LOG2; ++t) xrow += (((uint32_t)i >> t) & 1u) << loop_pos[t];
            rowok = (uint32_t)__ballot(((xrow ^ row_v) & row_m) == 0);
        }
        // byte offsets (inside a set's region) of this thread's entries of every incoming message
        int ad[NIN > 0 ? NIN : 1][NV];
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            const int base = (__builtin_amdgcn_readlane(trow[1 + k], i) + thr_in[k]) * 8 + in_lds[k];
            ad[k][0] = base;
            if constexpr (EDEP) {
                ad[k][1] = base + in_ew0[k] * 8;
                if constexpr (VEC == 4) {
                    ad[k][2] = base + in_ew1[k] * 8;
                    ad[k][3] = base + (in_ew0[k] + in_ew1[k]) * 8;
                }
            }
        }
        auto load_set = [&](const int s, double (&dst)[NIN > 0 ? NIN : 1][NV]) {
            const char *reg = sets + s * SETB;
#pragma unroll
            for (int k = 0; k < NIN; ++k)
#pragma unroll
                for (int e = 0; e < NV; ++e) dst[k][e] = *reinterpret_cast<const double *>(reg + ad[k][e]);
        };
        // A row that contradicts a set's evidence contributes nothing to that set: hard evidence is slicing, so the row never
        // reaches the set's accumulators - a uniform branch on the set's bit of `rowok` skips it.  (A factor rs = 0.0 as the
        // multiplier of the accumulating fma is not the same thing: 0 x inf = NaN where the contradicted row holds inf or NaN,
        // or two finite entries whose product overflows.)  For a row that agrees rs is 1.0 and the arithmetic is what it was.
        // Two-stage pipeline over the sets: the entries of set s + 1 are requested before the products of set s are formed.
        double psum = 0.0;
        if constexpr (ESUM) {
            psum = p[0] + p[1];
            if constexpr (VEC == 4) psum += p[2] + p[3];
        }
        if constexpr (!EDEP) {
            // No message depends on the element bits: one entry per message and set, so the entries of ALL eight sets
            // are requested at once (16 LDS reads in flight for two messages; a look-ahead of one set left every
            // set's products waiting a full LDS latency: 0.57 us per row with three waves per SIMD to hide it) and
            // ONE product of a set's entries serves the four elements (NIN multiplications + VEC fused multiply-adds
            // per set and row; with ESUM one).
            double all[G][NIN > 0 ? NIN : 1];
#pragma unroll
            for (int s = 0; s < G; ++s)
#pragma unroll
                for (int k = 0; k < NIN; ++k) all[s][k] = *reinterpret_cast<const double *>(sets + s * SETB + ad[k][0]);
#pragma unroll
            for (int s = 0; s < G; ++s) {
                // (the factor of a row that contradicts the set's evidence is uniform: built in scalar registers it is
                //  one more multiplication per set, not a select as well; without row evidence in the group - decided
                //  once per workgroup - it is not there at all: 24 instead of 56 vector operations per row with two
                //  incoming messages)
                if constexpr (ROWEV) {
                    if (!((rowok >> s) & 1u)) continue;              // (uniform: `rowok` is a ballot)
                }
                double t = 1.0;
                if constexpr (ROWEV) t = __hiloint2double(__builtin_amdgcn_readfirstlane(((rowok >> s) & 1u) ? 0x3FF00000 : 0), 0);
                if constexpr (NIN > 0 && !ROWEV) {
                    t = all[s][0];
#pragma unroll
                    for (int k = 1; k < NIN; ++k) t *= all[s][k];
                } else {
#pragma unroll
                    for (int k = 0; k < NIN; ++k) t *= all[s][k];
                }
                if constexpr (ESUM) acc[s][0] = __builtin_fma(psum, t, acc[s][0]);
                else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[s][e] = __builtin_fma(p[e], t, acc[s][e]);
                }
            }
        } else {
            double cur[NIN > 0 ? NIN : 1][NV];
#pragma unroll
            for (int s = 0; s < G; ++s) {
                load_set(s, cur);
                if constexpr (ROWEV) {
                    if (!((rowok >> s) & 1u)) continue;              // (uniform; the set's entries were requested, not used)
                    const double rs = __hiloint2double(__builtin_amdgcn_readfirstlane(((rowok >> s) & 1u) ? 0x3FF00000 : 0), 0);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        double w = p[e];
#pragma unroll
                        for (int k = 0; k < NIN; ++k) w *= cur[k][e];
                        acc[s][e] = __builtin_fma(w, rs, acc[s][e]);
                    }
                } else {
                    // (no set of the group observes a variable on the row bits - decided once per workgroup: the last message
                    //  entry is the multiplier of the accumulating fma, NIN operations per element and set instead of NIN + 1)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        if constexpr (NIN == 0) acc[s][e] += p[e];
                        else {
                            double w = p[e];
#pragma unroll
                            for (int k = 0; k + 1 < NIN; ++k) w *= cur[k][e];
                            acc[s][e] = __builtin_fma(w, cur[NIN - 1][e], acc[s][e]);
                        }
                    }
                }
            }
        }
        if ((i & rmask) == rmask) epilogue(__builtin_amdgcn_readlane(trow[1 + JT_MAX_IN], i));
    };

    JT_STAMP(4);
    using std::integral_constant;
    bool any_edep = false;
#pragma unroll
    for (int k = 0; k < NIN; ++k) any_edep = any_edep || in_edep[k] != 0;
    auto loop = [&](auto edep_tag, auto rowev_tag) {
        for (int i0 = 0; i0 < total; i0 += U) {
            step(integral_constant<int, 0>{}, edep_tag, rowev_tag, i0);
            step(integral_constant<int, 1>{}, edep_tag, rowev_tag, i0 + 1);
            step(integral_constant<int, 2>{}, edep_tag, rowev_tag, i0 + 2);
            step(integral_constant<int, 3>{}, edep_tag, rowev_tag, i0 + 3);
        }
    };
    // (ESUM: the planner sets JtTask::esum only where no message has element bits)
    bool plain = true;
    if constexpr (!ESUM) {
        if (any_edep) {
            loop(integral_constant<bool, true>{}, integral_constant<bool, true>{});
            plain = false;
        }
    }
    if (plain) {
        if (has_row_ev) loop(integral_constant<bool, false>{}, integral_constant<bool, true>{});
        else loop(integral_constant<bool, false>{}, integral_constant<bool, false>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the ring's last (repeated) loads land before LDS is given back
    JT_STAMP(9);

    // ---- flush every set's outgoing sub-box as this chunk's partial copy --------------------------------
    __syncthreads();
    {
        const int n = 1 << o_nfree;
        const bool mark = fl.oth_off >= 0;
        for (int i = tid; i < n; i += JT_THREADS) {
            int idx = 0;
#pragma unroll
            for (int b = 0; b < JT_MAX_FREE; ++b)
                if (b < o_nfree) idx += ((i >> b) & 1) << JT_FPOS(ofp, b);
#pragma unroll
            for (int s = 0; s < G; ++s) {
                double *base = msg0 + soff[s] + o_at + idx;
                jt_msg_store<FLOW>(base + fl.cur_off, reinterpret_cast<const double *>(sets + s * SETB + o_lds)[i]);
                if (mark) base[fl.oth_off] = __longlong_as_double((long long)JT_UNWRITTEN);
            }
        }
    }
    JT_STAMP(11);
#ifdef JT_STAMPS
    if (dbg & 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        JT_STAMP(12);
    }
#endif
}

// Multi-set entry point: the GROUP of JT_MSETS evidence sets is folded into the 1-D block index; the block list is that of a
// whole phase (dataflow launch) or of one tree level.  A workgroup waits for workgroups earlier in the list - of its own group,
// and, where sets share the messages of evidence-free subtrees (JtFlow::act_ids / JtFlow::skip), of the group that holds arena
// slot 0 or the slot on the producer's active list.  The ticket counters are per group, so these waits across groups rest on
// in-order dispatch and on the host's abort (JtFlow::host_abort).
#ifndef JT_MULTI_WAVES
#define JT_MULTI_WAVES 3
#endif
template <typename T>
__global__ __launch_bounds__(JT_THREADS, JT_MULTI_WAVES) void jt_multi_flow(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk,
                                                            const int *__restrict__ itab, const T *__restrict__ psi,
                                                            T *__restrict__ bel, double *__restrict__ msg, JtFlow fl) {
    __shared__ uint32_t flow_ctl[JT_CTL_WORDS];        // ticket, wait flags and candidates, parked flush records
    // 1-D grid, the GROUP index inside the record index: workgroups b .. b+7 of group g, then the same eight records for
    // group g+1, ...  The groups of evidence sets stream the SAME table rows; dispatched next to each other - and, with the
    // round-robin placement of consecutive workgroups over the eight XCDs, on the same XCD - the second to last group find
    // the rows the first one fetched in the L2 / Infinity Cache instead of fetching 1 GiB of tables again per group
    // (round 2: grid.y = group, every group a sweep of its own over all tables).  Order inside a group is unchanged
    // (record index ascending with blockIdx), which is all the dataflow waits need.
    const uint32_t octet = blockIdx.x / (8u * fl.n_groups), within = blockIdx.x % (8u * fl.n_groups);
    const uint32_t grp = within / 8u, rec = octet * 8u + (within & 7u);
    if (rec >= fl.n_blocks) return;
    if (grp != 0) fl.dbg |= 0x80000000u;                     // (diagnostic builds: group 0 writes the time stamps)
    fl.sync += (size_t)grp * fl.sync_stride;
    double *msg0 = msg;                                      // (the sets' arenas: slot x set_stride doubles from here)
    const uint32_t ticket = fl.ticket_idx == 0xffffffffu ? rec : jt_flow_ticket(fl, flow_ctl);
    const JtBlock &bk = blk[ticket];
    if (bk.flags & JT_BLOCK_NULL) return;                    // (padding of a level's records to a multiple of eight)
    const JtTask &tk = tasks[bk.task];
    // Which evidence sets: entries 8 g .. 8 g + 7 of the task's active list (a shorter last run repeats its last entry: the same
    // values are then stored twice), or - without lists - arena slots 8 g .. 8 g + 7.  Nothing on the list for this group: done.
    int sidv = (int)(grp * 8u + (threadIdx.x & 7u));
    bool esum_ok = ((tk.esum_groups >> (grp & 63u)) & 1ull) != 0;
    if (fl.act_n != nullptr) {
        const int n_act = fl.act_n[bk.task];
        if ((int)(grp * 8u) >= n_act) return;
        const int j = (int)(grp * 8u + (threadIdx.x & 7u));
        sidv = (int)fl.act_ids[(size_t)bk.task * fl.cap + (uint32_t)(j < n_act ? j : n_act - 1)];
        esum_ok = fl.esum_oct[(size_t)bk.task * fl.n_groups + grp] != 0;
    }
    if (tk.kind != 0) {
        jt_reduce<true, true>(tk, bk, msg0, fl, sidv);
        return;
    }
    if (tk.setb <= JT_SETB_SMALL && (tk.esum & 1) && esum_ok) {
        switch (tk.n_in) {
            case 0: jt_mpass<T, 0, JT_SETB_SMALL, true>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            case 1: jt_mpass<T, 1, JT_SETB_SMALL, true>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            case 2: jt_mpass<T, 2, JT_SETB_SMALL, true>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            default: jt_mpass<T, 3, JT_SETB_SMALL, true>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
        }
    } else if (tk.setb <= JT_SETB_SMALL) {
        switch (tk.n_in) {
            case 0: jt_mpass<T, 0, JT_SETB_SMALL>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            case 1: jt_mpass<T, 1, JT_SETB_SMALL>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            case 2: jt_mpass<T, 2, JT_SETB_SMALL>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            default: jt_mpass<T, 3, JT_SETB_SMALL>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
        }
    } else {
        switch (tk.n_in) {
            case 0: jt_mpass<T, 0, JT_SETB_LARGE>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            case 1: jt_mpass<T, 1, JT_SETB_LARGE>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            case 2: jt_mpass<T, 2, JT_SETB_LARGE>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
            default: jt_mpass<T, 3, JT_SETB_LARGE>(tk, bk, itab, psi, msg0, fl, flow_ctl, ticket, sidv); break;
        }
    }
}
