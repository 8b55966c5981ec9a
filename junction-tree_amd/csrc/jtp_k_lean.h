// Message kernels: the lean unit pass - jt_unit_lean, its two dispatchers (a propagate's tasks: jt_unit_lean_dispatch, read-out
// tasks: jt_unit_lean_readout) and jt_lean_block, the short way of a dataflow workgroup to its lean record (map of the units:
// jtp_kernels.hip.h).
#pragma once
#include "jtp_k_common.h"

// The lean unit pass (round 6; JtLean, jtp_internal.h).  A unit task of ONE outgoing message whose incoming tables have one copy each,
// run for an evidence set that observes nothing:
//     out[S] = sum_{C \ S} prod_k in_k[S_k]          (computation.py:79-88 for a clique the reference keeps as length-1 axes,
//                                                     junctiontree.py:52-61; every downward message of such a clique likewise)
// Same sub-boxes, same LDS offsets, same iteration table, same marker protocol and the same epilogue as jt_pass<..., UNIT> - what is
// gone is the interpretation: no bit-deposit loops over free_pos[] (the host stored the weights), no branch per message and row on
// e_dep (the tables that depend on a thread's element bits come first and their number NE is a template parameter), no table row,
// no evidence, no belief, no ring, one read of a 704-byte record instead of scattered reads of a 2.3 KB one.  Where no incoming
// table depends on the element bits (NE = 0) the VEC elements of a thread share ONE product and one accumulator.
// Product order: in[0] * in[1] * ... in the RECORD's order (element-dependent tables first) - a fixed order, the same in every
// launch mode; the generic pass multiplies in JtTask order, so the two agree to rounding, not bit for bit.
// NOUT > 1 (read-out tasks only, jt_unit_single: up to three marginals of psi x every incoming table of a unit clique in one pass): every
// output accumulates the same product and folds after its own runs of rows; outputs 1 and 2 are described by the JtLeanMore record
// behind the lean record.
// COPIES (read-out tasks only): an incoming message may have several partial copies (JtLeanMsg::w_hi[5]), summed in copy order.
template <typename T, int NIN, int NE, bool FLOW, int NOUT = 1, bool COPIES = false>
__device__ __forceinline__ void jt_unit_lean(const JtLean &ln, const JtBlock &bk, const int *__restrict__ itab,
                                             double *__restrict__ msg_arena, const JtFlow &fl, uint32_t *flow_ctl) {
    constexpr int VEC = 16 / sizeof(T);               // elements of a thread per row (the plan's thread part: 256 threads x VEC)
    constexpr int NI = NIN > 0 ? NIN : 1;
    constexpr int NACC = NE > 0 ? VEC : 1;
    const JtLeanMore &lx = *reinterpret_cast<const JtLeanMore *>(&ln + 1);       // (read only where NOUT > 1)
    auto outm = [&](auto j_tag) -> const JtLeanMsg & {
        constexpr int j = decltype(j_tag)::value;
        if constexpr (j == 0) return ln.out;
        else return lx.out[j - 1];
    };
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = ln.total;

    // ---- everything that does not depend on a message: the iteration table (row r in lane r), the thread's validity
    int trow[JT_NCOL];
    {
        const int *gtab = itab + ln.itab_off;
        const int r = lane < total ? lane : total - 1;
        const int4 a = *reinterpret_cast<const int4 *>(gtab + r * JT_NCOL);
        const int4 b = *reinterpret_cast<const int4 *>(gtab + r * JT_NCOL + 4);
        trow[0] = a.x; trow[1] = a.y; trow[2] = a.z; trow[3] = a.w;
        trow[4] = b.x; trow[5] = b.y; trow[6] = b.z; trow[7] = b.w;
    }
    uint32_t dead = 0;                                // bit e: element e of this thread names no entry of the clique
    if (ln.some_invalid) {
        const int *tm = itab + ln.tmap_off + tid * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) dead |= tm[e] < 0 ? 1u << e : 0u;
    }
    const bool chunk_ok = !(bk.flags & JT_BLOCK_INVALID);

    // a sub-box entry's place in its message: weights . bits of (round, thread)
    auto lo_of = [&](const JtLeanMsg &m) {
        uint32_t g = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) g += (((uint32_t)tid >> b) & 1u) * (uint32_t)m.w_lo[b];
        return g;
    };
    auto hi_of = [&](const JtLeanMsg &m) {            // (lane j: round j)
        uint32_t g = 0;
#pragma unroll
        for (int b = 0; b < JT_MAX_FREE - 8; ++b) g += (((uint32_t)lane >> b) & 1u) * (uint32_t)m.w_hi[b];
        return g;
    };

    // ---- stage the incoming sub-boxes, all of them in lock step: four rounds of 256 entries of every message in flight together
    const double *msg_cur = msg_arena + fl.cur_off;
    const double *src[NI];
    uint32_t lo[NI], hiv[NI];
    int nent[NI];
    bool thr_mem[NI];
    int rounds = 0;
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const JtLeanMsg &m = ln.in[k];
        const int gb = m.src == 0 ? bk.gbase[0] : (m.src == 1 ? bk.gbase[1] : (m.src == 2 ? bk.gbase[2] : bk.gbase[3]));
        src[k] = msg_cur + (m.off + gb + ((m.flags & 2) ? fl.fix_shift : 0));
        lo[k] = lo_of(m);
        hiv[k] = hi_of(m);
        nent[k] = 1 << m.nfree;
        thr_mem[k] = (m.flags & 1) != 0;
        const int r = (nent[k] + JT_THREADS - 1) >> 8;
        rounds = r > rounds ? r : rounds;
    }
    uint32_t out_lo[NOUT], out_hiv[NOUT];
    jt_static_for<NOUT>([&](auto j_tag) {
        constexpr int j = decltype(j_tag)::value;
        out_lo[j] = lo_of(outm(j_tag));
        out_hiv[j] = hi_of(outm(j_tag));
    });
    uint64_t wait_t0 = 0;
    for (int attempt = 0;; ++attempt) {
        const int settle_attempt = ln.settle ? attempt : 0;
        const double *unready = nullptr;
        for (int it0 = 0; it0 < rounds; it0 += 4) {
            double c[NI][4];
            const double *at[NI][4];
#pragma unroll
            for (int k = 0; k < NIN; ++k)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    at[k][u] = src[k] + (lo[k] + (uint32_t)__builtin_amdgcn_readlane((int)hiv[k], it0 + u));
                    c[k][u] = (it0 + u) * JT_THREADS + tid < nent[k] ? jt_msg_load<FLOW>(at[k][u], thr_mem[k]) : 0.0;
                }
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                double *sub = reinterpret_cast<double *>(smem + ln.in[k].lds_off);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if ((it0 + u) * JT_THREADS + tid >= nent[k]) continue;
                    if (FLOW) c[k][u] = jt_msg_settle<FLOW>(at[k][u], c[k][u], thr_mem[k], settle_attempt);
                    if (FLOW && jt_unwritten(c[k][u])) unready = at[k][u];
                    double sum = 0.0 + c[k][u];
                    if constexpr (COPIES) {
                        const int ncopy = ln.in[k].w_hi[5];
                        const int64_t cstride = ln.in[k].w_hi[6];
                        for (int p0 = 1; p0 < ncopy; p0 += 4) {
                            double d[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) d[q] = p0 + q < ncopy ? jt_msg_load<FLOW>(at[k][u] + (int64_t)(p0 + q) * cstride, thr_mem[k]) : 0.0;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                if (p0 + q >= ncopy) continue;
                                if constexpr (FLOW) {         // (folded marginals: the copies are in the making like the first one)
                                    const double *ap = at[k][u] + (int64_t)(p0 + q) * cstride;
                                    d[q] = jt_msg_settle<FLOW>(ap, d[q], thr_mem[k], settle_attempt);
                                    if (jt_unwritten(d[q])) unready = ap;
                                }
                                sum += d[q];
                            }
                        }
                    }
                    sub[(it0 + u) * JT_THREADS + tid] = sum;
                }
            }
        }
        if (attempt == 0) {
            jt_static_for<NOUT>([&](auto j_tag) {
                double *sub = reinterpret_cast<double *>(smem + outm(j_tag).lds_off);
                const int n = 1 << outm(j_tag).nfree;
                for (int s = tid; s < n; s += JT_THREADS) sub[s] = 0.0;
            });
        }
        if constexpr (!FLOW || NIN == 0) {
            __syncthreads();
            break;
        } else {
            // (the wait of jt_pass: one lane polls one entry that was not ready, with back-off; it gives up after 2 s or when another
            //  workgroup did, so that the grid always drains)
            if (fl.dbg & 4) unready = nullptr;
            if (fl.dbg & 8) unready = msg_cur;
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
            if (flow_ctl[1] != 0) return;
        }
    }

    // ---- per-thread constants: the byte address inside LDS of this thread's entry of every incoming sub-box (a row adds its offset)
    auto slot_of = [&](const JtLeanMsg &m) {
        int t = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b) t += ((lane >> b) & 1) * m.t_w[b];
#pragma unroll
        for (int b = 0; b < 2; ++b) t += ((wave >> b) & 1) * m.t_w[6 + b];
        return t;
    };
    uint32_t ua[NI][NE > 0 ? VEC : 1];
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const JtLeanMsg &m = ln.in[k];
        const int t = slot_of(m);
        ua[k][0] = (uint32_t)m.lds_off + 8u * (uint32_t)t;
        if constexpr (NE > 0) {
            if (k < NE) {
#pragma unroll
                for (int e = 1; e < VEC; ++e) ua[k][e] = ua[k][0] + 8u * (uint32_t)(((e & 1) ? m.e_w[0] : 0) + ((e & 2) ? m.e_w[1] : 0));
            }
        }
    }
    double *out_sub[NOUT];
    int thr_out[NOUT], o_ew0[NOUT], o_ew1[NOUT], red_e[NOUT], red_lane[NOUT], red_wave[NOUT], rmask[NOUT], nph[NOUT], myph[NOUT];
    bool rep[NOUT];
    jt_static_for<NOUT>([&](auto j_tag) {
        constexpr int j = decltype(j_tag)::value;
        const JtLeanMsg &m = outm(j_tag);
        out_sub[j] = reinterpret_cast<double *>(smem + m.lds_off);
        thr_out[j] = slot_of(m);
        o_ew0[j] = m.e_w[0], o_ew1[j] = m.e_w[1];
        red_e[j] = j == 0 ? ln.red_e : lx.red_e[j > 0 ? j - 1 : 0];
        red_lane[j] = j == 0 ? ln.red_lane : lx.red_lane[j > 0 ? j - 1 : 0];
        red_wave[j] = j == 0 ? ln.red_wave : lx.red_wave[j > 0 ? j - 1 : 0];
        rmask[j] = j == 0 ? ln.rmask : lx.rmask[j > 0 ? j - 1 : 0];
        rep[j] = (lane & red_lane[j]) == 0;
        nph[j] = 1 << __builtin_popcount((unsigned)red_wave[j]);
        myph[j] = 0;
        if (red_wave[j] == 1) myph[j] = wave & 1;
        else if (red_wave[j] == 2) myph[j] = wave >> 1;
        else if (red_wave[j] == 3) myph[j] = wave;
    });

    double acc[NOUT][NACC];
#pragma unroll
    for (int j = 0; j < NOUT; ++j)
#pragma unroll
        for (int e = 0; e < NACC; ++e) acc[j][e] = 0.0;
    // (the record orders the tables its own way; a table's column of the iteration table is its place in JtTask::msg - picked once)
    int tcol[NI];
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const int sk = ln.in[k].src;
        tcol[k] = sk == 0 ? trow[1] : (sk == 1 ? trow[2] : (sk == 2 ? trow[3] : trow[4]));
    }

    // fold this thread's sums of one run of rows into outgoing sub-box j (jt_pass: same sums, same order)
    auto epilogue = [&](auto j_tag, const int oo) {
        constexpr int j = decltype(j_tag)::value;
        double a[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = ((dead >> e) & 1u) ? 0.0 : acc[j][NE > 0 ? e : 0];
        if constexpr (VEC == 4) {
            if (red_e[j] & 1) {
                a[0] += a[1];
                a[2] += a[3];
            }
            if (red_e[j] & 2) {
                a[0] += a[2];
                a[1] += a[3];
            }
        } else {
            if (red_e[j] & 1) a[0] += a[1];
        }
        jt_lane_sums<VEC>(a, red_lane[j]);
        const int slot = oo + thr_out[j];
        for (int ph = 0; ph < nph[j]; ++ph) {
            if (rep[j] && myph[j] == ph) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if ((e & red_e[j]) == 0) {
                        const int eo = ((e & 1) ? o_ew0[j] : 0) + ((e & 2) ? o_ew1[j] : 0);
                        __hip_atomic_fetch_add(&out_sub[j][slot + eo], a[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
            if (nph[j] > 1) __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < NACC; ++e) acc[j][e] = 0.0;
    };

#pragma unroll
    for (int c = 0; c < JT_NCOL; ++c) asm volatile("" : "+v"(trow[c]));
#pragma unroll
    for (int k = 0; k < NIN; ++k) asm volatile("" : "+v"(tcol[k]));

    // ---- the rows: nothing but look-ups and products.  The entries of row i + 1 are asked for before those of row i are used (one
    //      LDS round trip per row otherwise, and nothing to do in it).  CHECK: some row of the loop nest does not exist (a digit
    //      beyond a cardinality: JT_NO_ROW) - such a row adds nothing; plans of power-of-two cardinalities never look.
    struct Entries {
        double e[NE > 0 ? NE : 1][VEC], c[NIN - NE > 0 ? NIN - NE : 1];
    };
    auto fetch = [&](const int i, Entries &x) {
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            const uint32_t rb = (uint32_t)__builtin_amdgcn_readlane(tcol[k], i) << 3;
            if constexpr (NE > 0) {
                if (k < NE) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) x.e[k < NE ? k : 0][e] = *reinterpret_cast<const double *>(smem + (ua[k][e] + rb));
                    continue;
                }
            }
            x.c[k - NE >= 0 ? k - NE : 0] = *reinterpret_cast<const double *>(smem + (ua[k][0] + rb));
        }
    };
    auto use = [&](const Entries &x) {
        if constexpr (NIN == 0) {
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[j][0] += 1.0;
        } else if constexpr (NE == 0) {
            double w = x.c[0];
#pragma unroll
            for (int k = 1; k < NIN; ++k) w *= x.c[k];
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[j][0] += w;
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                double w = x.e[0][e];
#pragma unroll
                for (int k = 1; k < NE; ++k) w *= x.e[k][e];
#pragma unroll
                for (int k = NE; k < NIN; ++k) w *= x.c[k - NE];
#pragma unroll
                for (int j = 0; j < NOUT; ++j) acc[j][e] += w;
            }
        }
    };
    auto rows = [&](auto check_tag) {
        constexpr bool CHECK = decltype(check_tag)::value;
        Entries cur, nxt;
        fetch(0, cur);
        for (int i = 0; i < total; ++i) {
            fetch(i + 1 < total ? i + 1 : i, nxt);
            if (!CHECK || (uint32_t)__builtin_amdgcn_readlane(trow[0], i) != JT_NO_ROW) use(cur);
            jt_static_for<NOUT>([&](auto j_tag) {
                constexpr int j = decltype(j_tag)::value;
                if ((i & rmask[j]) == rmask[j]) epilogue(j_tag, __builtin_amdgcn_readlane(trow[1 + JT_MAX_IN + j], i));
            });
            cur = nxt;
        }
    };
    if (chunk_ok) {                                       // (a chunk whose own digits do not exist writes its zeros and nothing else)
        if (ln.some_norow) rows(std::integral_constant<bool, true>{});
        else rows(std::integral_constant<bool, false>{});
    }

    // ---- flush the outgoing sub-boxes as this chunk's partial copies; the same entries of the other arena half become "unwritten"
    __syncthreads();
    jt_static_for<NOUT>([&](auto j_tag) {
        constexpr int j = decltype(j_tag)::value;
        const JtLeanMsg &m = outm(j_tag);
        const int64_t at = m.off + (int64_t)bk.pnum[j] * (j == 0 ? ln.out_pstride : lx.out_pstride[j > 0 ? j - 1 : 0]) + bk.gbase[JT_MAX_IN + j];
        double *dst = msg_arena + fl.cur_off + at + fl.out_shift;
        double *oth = msg_arena + fl.oth_off + at;
        const bool mark = fl.oth_off >= 0;
        const int n = 1 << m.nfree;
        for (int s = tid, it = 0; s < n; s += JT_THREADS, ++it) {
            const uint32_t idx = out_lo[j] + (uint32_t)__builtin_amdgcn_readlane((int)out_hiv[j], it);
            jt_msg_store<FLOW>(dst + idx, out_sub[j][s]);
            if (mark) oth[idx] = __longlong_as_double((long long)JT_UNWRITTEN);
        }
    });
}

// (which of the ten row loops: incoming tables x those among them that depend on the element bits)
template <typename T, bool FLOW>
__device__ __forceinline__ void jt_unit_lean_dispatch(const JtLean &ln, const JtBlock &bk, const int *__restrict__ itab,
                                                      double *__restrict__ msg, const JtFlow &fl, uint32_t *flow_ctl) {
#define JT_LEAN(NIN, NE) jt_unit_lean<T, NIN, NE, FLOW>(ln, bk, itab, msg, fl, flow_ctl); break
    switch (ln.n_in * 8 + ln.n_e) {
        case 0: JT_LEAN(0, 0);
        case 8: JT_LEAN(1, 0);
        case 9: JT_LEAN(1, 1);
        case 16: JT_LEAN(2, 0);
        case 17: JT_LEAN(2, 1);
        case 18: JT_LEAN(2, 2);
        case 24: JT_LEAN(3, 0);
        case 25: JT_LEAN(3, 1);
        case 26: JT_LEAN(3, 2);
        default: JT_LEAN(3, 3);                           // (jtp_make_lean: at most three incoming tables)
    }
#undef JT_LEAN
}

// Read-out tasks of unit cliques (jtp_get_marginals -> jt_single; no launch waits on anything): up to four incoming tables - the parent's
// message, the static table and two children, all of them - and one to three marginals per pass.
// FLOW: the same tasks FOLDED into a propagate's dataflow launch (JtTask::fold, jtp_plan.cpp fold_marginals): their inputs are messages of
// this launch, waited for like any other.
template <typename T, bool FLOW = false>
__device__ __forceinline__ void jt_unit_lean_readout(const JtLean &ln, const JtBlock &bk, const int *__restrict__ itab,
                                                     double *__restrict__ msg, const JtFlow &fl, uint32_t *flow_ctl = nullptr) {
#define JT_LEAN_OUT(NIN, NE)                                                                          \
    if (ln.n_out == 1) jt_unit_lean<T, NIN, NE, FLOW, 1, true>(ln, bk, itab, msg, fl, flow_ctl);            \
    else if (ln.n_out == 2) jt_unit_lean<T, NIN, NE, FLOW, 2, true>(ln, bk, itab, msg, fl, flow_ctl);       \
    else jt_unit_lean<T, NIN, NE, FLOW, 3, true>(ln, bk, itab, msg, fl, flow_ctl);                          \
    break
    switch (ln.n_in * 8 + ln.n_e) {
        case 0: JT_LEAN_OUT(0, 0);
        case 8: JT_LEAN_OUT(1, 0);
        case 9: JT_LEAN_OUT(1, 1);
        case 16: JT_LEAN_OUT(2, 0);
        case 17: JT_LEAN_OUT(2, 1);
        case 18: JT_LEAN_OUT(2, 2);
        case 24: JT_LEAN_OUT(3, 0);
        case 25: JT_LEAN_OUT(3, 1);
        case 26: JT_LEAN_OUT(3, 2);
        case 27: JT_LEAN_OUT(3, 3);
        case 32: JT_LEAN_OUT(4, 0);
        case 33: JT_LEAN_OUT(4, 1);
        case 34: JT_LEAN_OUT(4, 2);
        case 35: JT_LEAN_OUT(4, 3);
        default: JT_LEAN_OUT(4, 4);
    }
#undef JT_LEAN_OUT
}

// A dataflow workgroup whose record says "lean" (JT_BLOCK_LEAN) goes from its workgroup record straight to the task's lean record:
// one dependent scalar round trip less than through the task record.  (A clique that hosts an observed variable runs the generic pass;
// first_x[5] = the task's planner node, the index of its entry of the evidence table.)
// FOLD: the kernel can run folded marginal tasks (JT_BLOCK_FOLD; jt_propagate_flow_marg only - the other dataflow kernels end such a
// workgroup at once, as every kernel does where the clique hosts an observed variable: the engine then forms those marginals by
// the read-out, jtp_get_marginals).
template <typename T, bool FOLD = false>
__device__ __forceinline__ bool jt_lean_block(const JtBlock &bk, const int *__restrict__ itab, double *__restrict__ msg, const JtFlow &fl,
                                              uint32_t *flow_ctl) {
    if (!(bk.flags & JT_BLOCK_LEAN)) return false;        // (a folded task always has a lean record: jtp_plan.cpp finish())
    const bool observed = fl.ev != nullptr && fl.ev[2 * bk.first_x[5]] != 0;
    const int64_t at = (int64_t)((uint64_t)bk.first_x[6] | ((uint64_t)bk.first_x[7] << 32));
    if (bk.flags & JT_BLOCK_FOLD) {
        if constexpr (FOLD) {
            if (!observed) jt_unit_lean_readout<T, true>(*reinterpret_cast<const JtLean *>(itab + at), bk, itab, msg, fl, flow_ctl);
        }
        return true;
    }
    if (observed) return false;                          // (this clique hosts an observed variable: the generic pass)
    jt_unit_lean_dispatch<T, true>(*reinterpret_cast<const JtLean *>(itab + at), bk, itab, msg, fl, flow_ctl);
    return true;
}
