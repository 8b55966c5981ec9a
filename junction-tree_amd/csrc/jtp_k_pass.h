// Message kernels: jt_pass, the one body of the table-keeping passes (map of the units: jtp_kernels.hip.h).
//
// `jt_pass` covers the reference's per-clique work in both traversal directions (junctiontree/computation.py):
//   collect    (:47-96)   up[S_p]     = sum_{C \ S_p} psi * prod_k up_k
//   distribute (:140-224) down_k[S_k] = sum_{C \ S_k} psi * down_p * prod_{j != k} up_j
//                         belief[C]   = psi * down_p * prod_k up_k
// i.e. the einsum call sites K1..K5 and K7 of SURVEY.md section 2.1 fused into ONE pass
// over the clique table per phase.  The divide-out of `remove_message` (:99-136) does not
// exist here: the all-but-one products are formed directly.
//
// Bound: HBM.  Per clique element the kernel reads sizeof(T) bytes (collect) or reads and
// writes sizeof(T) (distribute); everything else (messages) lives in LDS.  See DESIGN.md.
//
// Work decomposition (jtp_internal.h): a workgroup of 256 threads owns one chunk (fixed F
// bits) of one clique.  Thread t loads VEC consecutive elements (16 bytes) at
//   x = xF + xA(a) + xR(r) + t*VEC
// so a wave reads 1 KiB contiguous per instruction.  Incoming messages are staged once per
// workgroup into LDS as the sub-box this chunk can touch (partial copies summed on the
// way); per element the message entry is one ds_read at  thread_offset + uniform_offset.
// Outgoing sums are kept in VEC registers per message over the R loop, then reduced
// in-thread (e bits), by wave shuffles (lane bits) and through the LDS sub-box (wave bits
// and A loop), and written once per workgroup as one partial copy.  No float atomics: results
// are bit-reproducible.
#pragma once
#include "jtp_k_common.h"

// UNIT (JtTask::unit): the clique keeps NO table - every entry that exists counts as 1 (a clique without factors, a virtual
// clique of the binarisation, or a clique whose factors cover few of its variables: their product is then one of the incoming
// tables, JtMsg::fixed, staged like a message).  No row is loaded and no element ring is kept: which entries of a row exist
// says the clique's thread map (read once), which rows exist the iteration table; the belief is stored only where the task
// names a place for it (read-out tasks).  The reference never materialises such axes either (junctiontree.py:52-61).
// BEL (unit tasks only): the belief is stored - by read-out tasks; the passes of a propagate leave it out at compile time (the
// conversions and the store were a tenth of the distribute step's vector instructions).
template <typename T, int NIN, int NOUT, int MODE, bool FLOW = false, bool EARLY_FLUSH = (MODE == 0), bool TMIX = false, bool KEEP = false, bool UNIT = false, bool BEL = !UNIT, bool VG = false>
__device__ __forceinline__ void jt_pass(const JtTask &tk, const JtBlock &bk, const int *__restrict__ itab,
                                        const T *__restrict__ psi_arena, T *__restrict__ bel_arena,
                                        double *__restrict__ msg_arena, const JtFlow &fl,
                                        uint32_t bindex, uint32_t *flow_ctl = nullptr, uint64_t t_entry = 0) {
    constexpr int VEC = 16 / sizeof(T);
    constexpr int EB = (VEC == 4) ? 2 : 1;
    constexpr int NMSG = NIN + NOUT;
    constexpr int NPAR = NIN - NOUT * (MODE == 1);   // distribute: leading inputs that are not children
    constexpr int U = JT_U;                          // element loads in flight per wave
    // (mixed-radix rows are gathered into registers, a few hundred bytes each; JT_UT = 8 - twice the rows in flight - was tried: slower)
    constexpr int UT = TMIX ? JT_UT : U;
    static_assert(U == 4 && (1 << JT_MIN_ITER_LOG2) == 4 && JT_RING_BYTES == U * 4096, "the loop groups below are written out for four slots");
    using VT = typename JtVec<T>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    // Mixed-radix rows, compact form (JtTask::vgroups == 2, round 5): at most 128 of the 256 logical threads of the thread part own
    // an entry that exists (cardinality 3: 81), so two waves serve a row and the workgroup works on TWO rows at a time - threads
    // 0..127 on rows 0, 2, 4, ..., threads 128..255 on rows 1, 3, 5, ...; which logical thread a thread stands for says the clique's
    // list behind its thread map (vt).  Everything that indexes by the thread part (message look-ups, thread map, evidence) uses
    // vt; staging and flush - plain copies - keep the physical thread; sums over thread-part variables go through LDS adds in wave
    // order (the lanes of a logical variable are no longer an XOR apart).
    // (VG: instantiated by the *_mix kernels for such tasks only - jt_collect_mix / jt_distribute_mix)
    static_assert(!VG || TMIX, "row groups are a form of mixed-radix rows");
    constexpr int ngrp = VG ? 2 : 1;
    int vt = tid, grp = 0;
    if constexpr (VG) {
        vt = (itab + tk.tmap_off + (1 << (EB + 8)))[tid & 127];
        grp = __builtin_amdgcn_readfirstlane(tid >> 7);
    }
    const int vlane = vt & 63, vwave = vt >> 6;

    const uint32_t xF = bk.xF + (uint32_t)tid * VEC;
    const T *psi = psi_arena + tk.psi_off;
    T *bel = bel_arena + (MODE == 1 ? tk.bel_off : 0);   // distribute always stores (virtual cliques: scratch)
    const int total = tk.total;                       // loop iterations of this workgroup (>= U)
    const int dbg = tk.debug;
#ifdef JT_STAMPS
    double *stamp_out = msg_arena + tk.dbg_off + (int64_t)(fl.blk_base + bindex) * JT_NSTAMP;
#endif
    JT_STAMP_AT(0, FLOW ? t_entry : __builtin_amdgcn_s_memrealtime());
    // What staging needs from the task record, read HERE: the element loads below are issued by inline assembly that the
    // compiler treats as a barrier for memory operations - left where they are used, these scalar loads would be one more
    // dependent round trip between the workgroup's start and its message loads.
    constexpr int NI = NIN > 0 ? NIN : 1, NO = NOUT > 0 ? NOUT : 1;
    int64_t sm_off[NI], sm_ps[NI];
    int sm_npart[NI], sm_nfree[NI], sm_lds[NI];
    bool sm_same[NI];
    uint32_t sm_fp[NI][4], sm_hiv[NI];
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const JtMsg &m = tk.msg[k];
        const uint32_t *fpw = reinterpret_cast<const uint32_t *>(m.free_pos);
        const uint32_t fp[4] = {fpw[0], fpw[1], fpw[2], fpw[3]};
        sm_off[k] = m.off + bk.gbase[k] + (m.fixed ? fl.fix_shift : 0);
        sm_ps[k] = m.pstride;
        sm_npart[k] = m.npart;
        sm_nfree[k] = m.nfree;
        sm_lds[k] = m.lds_off;
        sm_same[k] = m.same_launch != 0;
        sm_fp[k][0] = fp[0], sm_fp[k][1] = fp[1], sm_fp[k][2] = fp[2], sm_fp[k][3] = fp[3];
        sm_hiv[k] = jt_sub_hi(fp, m.nfree, lane);
    }
    // ... and what the flush needs.  Collect pass: kept in registers (read after the loop these are one more dependent round
    // trip on the hand-over to the parent: config 2 collect 2.52 -> 2.40 ms).  Distribute pass: the registers they would occupy
    // through the loop cost more (spills) than they save, so lane 0 parks the few words in LDS (flow_ctl) and the flush reads
    // them back from there - round 2 read the task record again, a dependent trip to memory of 1.0-1.6 us in front of the
    // stores of every hand-over.
    constexpr bool EARLY_OUT = EARLY_FLUSH;      // (the chain build of the distribute pass has the registers too)
    int64_t so_at[NO];
    int so_nfree[NO];
    uint32_t so_glo[NO], so_hiv[NO], so_fp[NO][4];
    uint32_t *park = flow_ctl != nullptr ? flow_ctl + JT_CTL_PARK : nullptr;       // [NOUT][8]: at (2 words), nfree, free_pos (4 words)
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        const JtMsg &m = tk.msg[JT_MAX_IN + j];
        const uint32_t *fpw = reinterpret_cast<const uint32_t *>(m.free_pos);
        const uint32_t fp[4] = {fpw[0], fpw[1], fpw[2], fpw[3]};
        const int64_t at = m.off + (int64_t)bk.pnum[j] * m.pstride + bk.gbase[JT_MAX_IN + j];
        if constexpr (EARLY_OUT) {
            so_at[j] = at;
            so_nfree[j] = m.nfree;
            so_fp[j][0] = fp[0], so_fp[j][1] = fp[1], so_fp[j][2] = fp[2], so_fp[j][3] = fp[3];
        } else if (park != nullptr && tid == 0) {
            park[8 * j + 0] = (uint32_t)at, park[8 * j + 1] = (uint32_t)((uint64_t)at >> 32), park[8 * j + 2] = (uint32_t)m.nfree;
            park[8 * j + 3] = fp[0], park[8 * j + 4] = fp[1], park[8 * j + 5] = fp[2], park[8 * j + 6] = fp[3];
        }
    }
    // outgoing message j's epilogue follows every 2^run_j iterations (JtTask::out_run)
    int rmask[NOUT > 0 ? NOUT : 1];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) rmask[j] = (1 << ((tk.out_run >> (8 * j)) & 0xffu)) - 1;
    // hard evidence of this evidence set on this clique (jtp_set_evidence): table entries whose index
    // contradicts it count as zero (read here, before the first store: see the scalar-cache note below)
    uint32_t ev_mask = 0, ev_val = 0;
    if (fl.ev != nullptr) {
        ev_mask = fl.ev[2 * tk.pnode];
        ev_val = fl.ev[2 * tk.pnode + 1];
    }
    uint32_t loop_pos[JT_MAX_ITER_LOG2];                // logical index bit of loop-counter bit t (beyond the loop: bit 31, never set)
#pragma unroll
    for (int t = 0; t < JT_MAX_ITER_LOG2; ++t) loop_pos[t] = t < tk.nA + tk.nR ? tk.loop_pos[t] : 31u;
    T *junk_row = bel_arena + ((size_t)1 << (EB + 8)) + (uint32_t)tid * VEC;
    const bool wr_bel = MODE == 1 && tk.bel_off >= 0;      // (unit tasks: a belief is stored by read-out tasks only)

    // ---- element loads run U iterations ahead of their use.  Iteration i's offsets are row i of
    //      the task's iteration table (host built, held in registers below): the loops do no index
    //      arithmetic beyond one v_readlane per column.
    const int *gtab = itab + tk.itab_off;
    // the first U loads use offsets stored in the task record, so they leave immediately
    // (addresses come from the workgroup record alone: one dependent load after launch)
    // Element vectors travel global -> LDS by LDS-DMA into a wave-private ring of U slots of 1 KiB
    // and are read back with ds_read_b128: no register is a load destination, so the U loads stay
    // in flight across loop iterations whatever the register allocator does; waits are counted by
    // hand (vmcnt counts loads and stores in issue order on CDNA4).
    const T *psi0 = psi_arena + bk.psi_x0 + (uint32_t)tid * VEC;
    // rows that do not exist (JT_NO_ROW: a digit beyond a variable's cardinality, a padding bit) read the arena's
    // zero row; their belief stores go to the row behind it (jtp_internal.h).  The whole chunk may be such.
    const T *zero_row = psi_arena + (uint32_t)tid * VEC;
    const bool chunk_ok = !(bk.flags & JT_BLOCK_INVALID);
    // (uniform) default cache policy for this workgroup's table rows, see JtTask::keep_rows.  KEEP: only the kernel that runs both
    // phases in one launch looks at the flag (jt_propagate_flow: the plans with levels that both passes visit close together in
    // time) - in every kernel, the uniform branch around the two forms of the FIRST loads cost config 2's chain kernels 1.5 % for
    // nothing, around the refills in the row loop 3.5 % (round 4).  The distribute pass's read of a kept row is its last use and
    // still takes the default policy: read non-temporally it was slower at every budget (docs/EXPERIMENTS.md, "Cache residency")
    const bool keep_rows = KEEP && (bk.flags & JT_BLOCK_KEEP_ROWS) != 0;
    const uint32_t ring_lds = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)smem) + (uint32_t)wave * (U * 1024);
    const char *ring = smem + wave * (U * 1024) + lane * 16;
    // The workgroup's iteration table (<= 64 rows of JT_NCOL ints, host built) lives in registers,
    // row r in lane r; a step reads "row i, column c" with v_readlane: no memory latency on the
    // critical path of a step except the message entries themselves.
    int trow[JT_NCOL];
    // (Vector-memory operations return in issue order, so the staging loads issued behind the first table rows only come
    //  back after them.  Issuing the first round of message loads AHEAD of the rows was tried in round 3: config 4 +-0,
    //  config 3 - whose staging loads are a quarter of its traffic - 12.5 -> 13.1 ms, A/B on one box: the rows go first.)
    // TMIX (plans with a mixed-radix thread part, HostPlan::tmix): the elements of a thread's logical index tid * VEC + e lie
    // at tmap[...] inside a row (-1: no such entry).  Rows are then gathered element by element into registers - ordinary
    // loads the compiler counts itself - instead of the 16-byte LDS-DMA ring; everything downstream (message look-ups,
    // butterflies, epilogues) works on the logical index and is unchanged.
    // (Entries that do not exist load the row's first element - every lane then executes every load, no per-element branch -
    //  and count as zero when the row is consumed; `row0` is a register copy of JtBlock::xF: read through `bk` inside the
    //  loop it was a scalar load and a wait in front of every element load, the belief stores could alias it.)
    int tpo[VEC];
    T tbuf[TMIX ? UT : 1][VEC];
    const uint32_t row0 = bk.xF;
    auto gather_row = [&](const int slot, const uint32_t xrow, const bool ok) {
        if constexpr (TMIX) {
            const T *row = ok ? psi + (row0 + xrow) : psi_arena;             // (uniform; psi_arena: the zero row)
#pragma unroll
            for (int e = 0; e < VEC; ++e) tbuf[slot][e] = row[tpo[e] >= 0 ? tpo[e] : 0];
        }
    };
    auto issue_tables = [&]() {
        if constexpr (UNIT) {
            const int *tm = itab + tk.tmap_off + tid * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) tpo[e] = tm[e];
        } else if constexpr (TMIX) {
            const int *tm = itab + tk.tmap_off + vt * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) tpo[e] = tm[e];
#pragma unroll
            for (int u = 0; u < UT; ++u) {
                const uint32_t x = bk.first_x[u * ngrp + grp];          // (rows 0..7: UT * ngrp <= 8)
                gather_row(u, x, x != JT_NO_ROW);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
                jt_dma16(bk.first_x[u] == JT_NO_ROW ? zero_row : psi0 + bk.first_x[u], __builtin_amdgcn_readfirstlane(ring_lds + u * 1024), keep_rows);
        }
        const int r = lane < total ? lane : total - 1;
        const int4 a = *reinterpret_cast<const int4 *>(gtab + r * JT_NCOL);
        const int4 b = *reinterpret_cast<const int4 *>(gtab + r * JT_NCOL + 4);
        trow[0] = a.x; trow[1] = a.y; trow[2] = a.z; trow[3] = a.w;
        trow[4] = b.x; trow[5] = b.y; trow[6] = b.z; trow[7] = b.w;
        JT_STAMP(1);
    };
    issue_tables();
    if constexpr (EARLY_OUT) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            so_glo[j] = jt_sub_lo(so_fp[j], so_nfree[j], tid);
            so_hiv[j] = jt_sub_hi(so_fp[j], so_nfree[j], lane);
        }
    }

    // ---- stage incoming sub-boxes (summing partial copies), zero outgoing sub-boxes -----
    // (the first element loads leave behind the first round of message loads).  Sub-boxes smaller than the workgroup
    // split their partial copies over 256/n thread groups; the loads of ALL such messages are
    // issued together (one round trip to L2 for the whole staging), group sums are combined
    // through LDS in group order (deterministic).  Larger sub-boxes: one thread per entry.
    double *scratch = reinterpret_cast<double *>(smem + tk.itab_lds - JT_STAGE_SCRATCH * NIN);
    const double *msg_cur = msg_arena + fl.cur_off;
    uint64_t wait_t0 = 0;
    for (int attempt = 0;; ++attempt) {
        JT_STAMP_AT(13, attempt + 1);
        // (only in plans made of latency-bound levels, JtTask::settle: chains gain 6 %; next to streaming
        //  levels the extra loads of waiting workgroups cost 1-2 % - both measured)
        const int settle_attempt = tk.settle ? attempt : 0;
        const double *unready = nullptr;          // (FLOW) an entry this thread found not written yet
        // (TMIX: a chunk that does not exist - JT_BLOCK_INVALID - stages nothing, waits for nobody and runs no row: it writes
        //  its all-zero sub-boxes, which the consumers sum and whose entries of the other arena half it re-arms, and ends)
        if (!TMIX || chunk_ok) {
            const double *src[NIN > 0 ? NIN : 1];
            int idx_t[NIN > 0 ? NIN : 1], gp0[NIN > 0 ? NIN : 1], gp1[NIN > 0 ? NIN : 1];
            int64_t ps[NIN > 0 ? NIN : 1];
            bool grouped[NIN > 0 ? NIN : 1], thr_mem[NIN > 0 ? NIN : 1];
            double psum[NIN > 0 ? NIN : 1];
            int maxper = 0;
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                const int nfree = sm_nfree[k];
                const uint32_t fp[4] = {sm_fp[k][0], sm_fp[k][1], sm_fp[k][2], sm_fp[k][3]};
                src[k] = msg_cur + sm_off[k];
                ps[k] = sm_ps[k];
                idx_t[k] = 0;
#pragma unroll
                for (int b = 0; b < 8; ++b)
                    if (b < nfree) idx_t[k] += ((tid >> b) & 1) << JT_FPOS(fp, b);
                thr_mem[k] = sm_same[k];
                grouped[k] = nfree < 8 && sm_npart[k] > 1;
                psum[k] = 0.0;
                gp0[k] = gp1[k] = 0;
                if (grouped[k]) {
                    const int groups = JT_THREADS >> nfree;   // >= 2
                    const int per = (sm_npart[k] + groups - 1) / groups;
                    gp0[k] = (tid >> nfree) * per;
                    gp1[k] = (gp0[k] + per < sm_npart[k]) ? gp0[k] + per : sm_npart[k];
                    maxper = per > maxper ? per : maxper;
                }
            }
            // Sub-boxes of a workgroup's size and more: one thread per entry and round of 256 entries.  Where entry `it` * 256 + tid
            // of message k's sub-box lies in the message (copy pc):
            // (round 6: the part of the bits above the thread's own eight comes from a 32-row table, row j in lane j - jt_sub_hi, as in
            //  the flush; the scalar deposit loop this replaces ran for every entry of every message: ~20 scalar instructions each)
            auto entry_at = [&](auto k_tag, int it, int pc) {
                constexpr int k = decltype(k_tag)::value;
                const int idx = idx_t[k] + __builtin_amdgcn_readlane((int)sm_hiv[k], it);
                return src[k] + ((int64_t)pc * ps[k] + idx);
            };
            // ... single-copy messages first, ALL of them in lock step: the loads of a round - up to eight entries per thread and
            // message (four when there are three messages or more: registers) - leave together, so a task with two or three
            // such messages pays one round trip to memory where it paid one per message (round 5: the unit tasks of config 3 are
            // two 1024-entry sub-boxes and a few cheap rows each - staging was a third of a workgroup's life).
            {
                constexpr int SU = NIN >= 3 ? 4 : 8;
                int nmax = 0;
#pragma unroll
                for (int k = 0; k < NIN; ++k)
                    if (!grouped[k] && sm_npart[k] == 1) nmax = (1 << sm_nfree[k]) > nmax ? (1 << sm_nfree[k]) : nmax;
                for (int it0 = 0; it0 * JT_THREADS < nmax; it0 += SU) {
                    double c[NIN > 0 ? NIN : 1][SU];
                    jt_static_for<NIN>([&](auto k_tag) {
                        constexpr int k = decltype(k_tag)::value;
                        const int n = (!grouped[k] && sm_npart[k] == 1) ? 1 << sm_nfree[k] : 0;
#pragma unroll
                        for (int u = 0; u < SU; ++u)
                            c[k][u] = (it0 + u) * JT_THREADS + tid < n ? jt_msg_load<FLOW>(entry_at(k_tag, it0 + u, 0), thr_mem[k]) : 0.0;
                    });
                    jt_static_for<NIN>([&](auto k_tag) {
                        constexpr int k = decltype(k_tag)::value;
                        const int n = (!grouped[k] && sm_npart[k] == 1) ? 1 << sm_nfree[k] : 0;
                        double *sub = reinterpret_cast<double *>(smem + sm_lds[k]);
#pragma unroll
                        for (int u = 0; u < SU; ++u) {
                            if ((it0 + u) * JT_THREADS + tid >= n) continue;
                            if (FLOW) c[k][u] = jt_msg_settle<FLOW>(entry_at(k_tag, it0 + u, 0), c[k][u], thr_mem[k], settle_attempt);
                            if (FLOW && jt_unwritten(c[k][u])) unready = entry_at(k_tag, it0 + u, 0);
                            sub[(it0 + u) * JT_THREADS + tid] = 0.0 + c[k][u];
                        }
                    });
                }
            }
            // ... then the messages of several copies, one after the other: 2^plog copies of 8 >> plog entries in flight per thread.
            // Every entry's copies are summed in ascending order from 0.0.
            jt_static_for<NIN>([&](auto k_tag) {
                constexpr int k = decltype(k_tag)::value;
                if (grouped[k] || sm_npart[k] == 1) return;
                const int nfree = sm_nfree[k];
                {
                    double *sub = reinterpret_cast<double *>(smem + sm_lds[k]);
                    const int n = 1 << nfree;
                    const int npart = sm_npart[k];
                    {
                        const int plog = npart >= 8 ? 3 : (npart >= 4 ? 2 : 1);
                        const int pmask = (1 << plog) - 1, E = 8 >> plog;
                        for (int it0 = 0; it0 * JT_THREADS < n; it0 += E) {
                            double sum[4] = {0.0, 0.0, 0.0, 0.0};
                            for (int p0 = 0; p0 < npart; p0 += 1 << plog) {
                                double c[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int e = u >> plog, pc = p0 + (u & pmask);
                                    const bool ok = (it0 + e) * JT_THREADS + tid < n && pc < npart;
                                    c[u] = ok ? jt_msg_load<FLOW>(entry_at(k_tag, it0 + e, pc), thr_mem[k]) : 0.0;
                                }
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int e = u >> plog, pc = p0 + (u & pmask);
                                    const bool ok = (it0 + e) * JT_THREADS + tid < n && pc < npart;
                                    if (FLOW && ok) c[u] = jt_msg_settle<FLOW>(entry_at(k_tag, it0 + e, pc), c[u], thr_mem[k], settle_attempt);
                                    if (FLOW && jt_unwritten(c[u])) unready = entry_at(k_tag, it0 + e, pc);
                                }
                                // (plog is uniform: the entry a value belongs to is picked with compile-time indices)
                                if (plog == 1) {
#pragma unroll
                                    for (int u = 0; u < 8; ++u) sum[u >> 1] += c[u];
                                } else if (plog == 2) {
#pragma unroll
                                    for (int u = 0; u < 8; ++u) sum[u >> 2] += c[u];
                                } else {
#pragma unroll
                                    for (int u = 0; u < 8; ++u) sum[0] += c[u];
                                }
                            }
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (e < E && (it0 + e) * JT_THREADS + tid < n) sub[(it0 + e) * JT_THREADS + tid] = sum[e];
                        }
                    }
                }
            });
            // grouped messages: every thread sums its range of copies of its entry, all messages at once
            constexpr int GC = NIN >= 3 ? 4 : 8;          // copies in flight per message (register budget)
            for (int p = 0; p < maxper; p += GC) {
                double c[NIN > 0 ? NIN : 1][GC];
#pragma unroll
                for (int k = 0; k < NIN; ++k)
#pragma unroll
                    for (int u = 0; u < GC; ++u)
                        c[k][u] = (grouped[k] && gp0[k] + p + u < gp1[k]) ? jt_msg_load<FLOW>(src[k] + ((int64_t)(gp0[k] + p + u) * ps[k] + idx_t[k]), thr_mem[k]) : 0.0;
#pragma unroll
                for (int k = 0; k < NIN; ++k)
#pragma unroll
                    for (int u = 0; u < GC; ++u) {
                        if (FLOW && grouped[k] && gp0[k] + p + u < gp1[k])
                            c[k][u] = jt_msg_settle<FLOW>(src[k] + ((int64_t)(gp0[k] + p + u) * ps[k] + idx_t[k]), c[k][u], thr_mem[k], settle_attempt);
                        psum[k] += c[k][u];
                        if (FLOW && jt_unwritten(c[k][u])) unready = src[k] + ((int64_t)(gp0[k] + p + u) * ps[k] + idx_t[k]);
                    }
            }
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (grouped[k]) scratch[k * JT_THREADS + tid] = psum[k];
        }
        if (attempt == 0) {
#pragma unroll
            for (int k = 0; k < NOUT; ++k) {
                const JtMsg &m = tk.msg[JT_MAX_IN + k];
                double *sub = reinterpret_cast<double *>(smem + m.lds_off);
                const int n = 1 << m.nfree;
                for (int s = tid; s < n; s += JT_THREADS) sub[s] = 0.0;
            }
            JT_STAMP(2);
        }
        if constexpr (!FLOW || NIN == 0) {
            __syncthreads();
            break;
        } else {
            // Some entry was not ready: ONE lane of the workgroup waits on one such entry (polling with
            // back-off: thousands of workgroups may be waiting at the top of a tree, and their polls
            // share the memory system with the workgroups they wait for), then everybody loads again.
            // The poller gives up after 2 s (100 MHz clock) or when another workgroup did, so that the
            // grid always drains; the host then reports the propagate as failed.
            if (fl.dbg & 4) unready = nullptr;
            if (fl.dbg & 8) unready = msg_cur;                           // fault injection: wait for ever
            uint32_t *slot = flow_ctl + 4 + (attempt & 1) * 12;          // [0..3] wave flags, [4..11] wave candidates
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
                const int cw = w3 ? 3 : (w2 ? 2 : (w1 ? 1 : 0));          // later waves hold later partial copies
                const double *entry = reinterpret_cast<const double *>((uintptr_t)slot[4 + 2 * cw] | ((uintptr_t)slot[5 + 2 * cw] << 32));
                if (wait_t0 == 0) wait_t0 = __builtin_amdgcn_s_memrealtime();
                uint32_t give_up = 0;
                unsigned spins = 0;
                const uint64_t limit = (fl.dbg & 8) ? 2000000ull : 200000000ull;
                while (jt_unwritten(jt_msg_load<true>(entry)) || (fl.dbg & 8)) {
                    // one load in flight per workgroup is no traffic to speak of: poll back to back while the
                    // wait is young (a short wait is a producer about to finish), then every ~0.5 us, ~1 us
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
                JT_STAMP(14);                                         // (the last poll's end: what follows is re-staging)
            }
            __syncthreads();
            if (flow_ctl[1] != 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // LDS-DMA loads must land before the wave ends
                return;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const int nfree = sm_nfree[k];
        if (nfree < 8 && sm_npart[k] > 1 && tid < (1 << nfree)) {
            const int groups = JT_THREADS >> nfree;
            double sum = 0.0;
            for (int g = 0; g < groups; ++g) sum += scratch[k * JT_THREADS + (g << nfree) + tid];
            reinterpret_cast<double *>(smem + sm_lds[k])[tid] = sum;
        }
    }
    __syncthreads();

    JT_STAMP(3);
    // ---- per-thread constants ---------------------------------------------------------------
    int thr[NMSG > 0 ? NMSG : 1];
    const double *in_sub[NIN > 0 ? NIN : 1];
    double *out_sub[NOUT > 0 ? NOUT : 1];
    int in_ew0[NIN > 0 ? NIN : 1], in_ew1[NIN > 0 ? NIN : 1], in_edep[NIN > 0 ? NIN : 1];
    // outgoing-message constants are read here, before the first store of the kernel: later
    // loads of the task record could not use the scalar cache and would drain vmcnt
    int o_rede[NOUT > 0 ? NOUT : 1], o_redl[NOUT > 0 ? NOUT : 1], o_redw[NOUT > 0 ? NOUT : 1];
    int o_ew0[NOUT > 0 ? NOUT : 1], o_ew1[NOUT > 0 ? NOUT : 1];
#pragma unroll
    for (int k = 0; k < NMSG; ++k) {
        const JtMsg &m = tk.msg[k < NIN ? k : JT_MAX_IN + (k - NIN)];
        int t = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b) t += ((vlane >> b) & 1) * m.t_w[b];
#pragma unroll
        for (int b = 0; b < 2; ++b) t += ((vwave >> b) & 1) * m.t_w[6 + b];
        thr[k] = t;
        if (k < NIN) {
            in_sub[k < NIN ? k : 0] = reinterpret_cast<const double *>(smem + m.lds_off);
            in_ew0[k < NIN ? k : 0] = m.e_w[0];
            in_ew1[k < NIN ? k : 0] = m.e_w[1];
            in_edep[k < NIN ? k : 0] = m.e_dep;
        } else {
            const int j = k >= NIN ? k - NIN : 0;
            out_sub[j] = reinterpret_cast<double *>(smem + m.lds_off);
            o_rede[j] = m.red_e;
            o_redl[j] = m.red_lane;
            o_redw[j] = m.red_wave;
            o_ew0[j] = m.e_w[0];
            o_ew1[j] = m.e_w[1];
        }
    }

    // (unit tasks: a row is nothing but message look-ups, so every instruction of one counts - the byte address of element e's
    //  entry of message k inside the sub-box is formed HERE, a row adds its offset: one vector add per LDS read)
    uint32_t ua[UNIT ? NI : 1][VEC];
    if constexpr (UNIT) {
#pragma unroll
        for (int k = 0; k < NIN; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                ua[k][e] = (uint32_t)tk.msg[k].lds_off + 8u * (uint32_t)(thr[k] + ((e & 1) ? in_ew0[k] : 0) + ((e & 2) ? in_ew1[k] : 0));
    }

    double acc[NOUT > 0 ? NOUT : 1][VEC];
#pragma unroll
    for (int j = 0; j < NOUT; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[j][e] = 0.0;

    // fold this thread's sums for outgoing message j (one run of iterations) into its sub-box
    auto epilogue = [&](auto j_tag, const int oo_j, const bool mine) {
        {
            constexpr int j = decltype(j_tag)::value;
            const int red_e = o_rede[j], red_lane = o_redl[j], red_wave = o_redw[j];
            constexpr bool compact = VG;
            if (compact && !mine) {
                // (compact mixed-radix rows: the other group's sums are due, this wave's run goes on - its sums stay as they are;
                //  the four barriers of the turns below)
                for (int ph = 0; ph < 4; ++ph) __syncthreads();
                return;
            }
            if constexpr ((UNIT || TMIX) && MODE == 0) {
                // (which entries of the thread part exist does not change from row to row: applied to the sums of a run, not to
                //  every product; mixed-radix rows: an entry that does not exist was gathered from the row's first element)
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (tpo[e] < 0) acc[j][e] = 0.0;
            }
            if constexpr (VEC == 4) {
                if (red_e & 1) {
                    acc[j][0] += acc[j][1];
                    acc[j][2] += acc[j][3];
                }
                if (red_e & 2) {
                    acc[j][0] += acc[j][2];
                    acc[j][1] += acc[j][3];
                }
            } else {
                if (red_e & 1) acc[j][0] += acc[j][1];
            }
            if constexpr (compact) {
                // compact mixed-radix rows: the threads that share an output slot are wherever the clique's list put them - every
                // thread adds its own sums to its slot, the LDS serialises the lanes of one wave, the waves take turns (a fixed order)
                const int slot_c = oo_j + thr[NIN + j];
                for (int ph = 0; ph < 4; ++ph) {
                    if (wave == ph) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            if ((e & red_e) == 0) {
                                const int eo = ((e & 1) ? o_ew0[j] : 0) + ((e & 2) ? o_ew1[j] : 0);
                                __hip_atomic_fetch_add(&out_sub[j][slot_c + eo], acc[j][e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                    }
                    __syncthreads();
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[j][e] = 0.0;
                return;
            }
            // (all elements take part, also those folded away above: no branch per element - their sums are not stored)
            if (!(dbg & 4)) jt_lane_sums<VEC>(acc[j], red_lane);
            const bool rep = (lane & red_lane) == 0;
            const int slot = oo_j + thr[NIN + j];
            const int nph = (dbg & 8) ? 1 : 1 << __builtin_popcount((unsigned)red_wave);
            // waves that share slots (wave bits not in the message) take turns, in wave order
            int myph = 0;
            if (red_wave == 1) myph = wave & 1;
            else if (red_wave == 2) myph = wave >> 1;
            else if (red_wave == 3) myph = wave;
            for (int ph = 0; ph < nph; ++ph) {
                if (rep && myph == ph) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        if ((e & red_e) == 0) {
                            const int eo = ((e & 1) ? o_ew0[j] : 0) + ((e & 2) ? o_ew1[j] : 0);
                            // one slot, one lane per phase: an LDS add without return (ds_add_f64) is the same
                            // sum in the same order as read-add-write, minus the wait for the read
                            __hip_atomic_fetch_add(&out_sub[j][slot + eo], acc[j][e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
                if (nph > 1) __syncthreads();
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[j][e] = 0.0;
        }
    };

    // make the table rows "arrived" for the compiler before the loop (they came by vector loads;
    // otherwise every use inside the loop would be guarded by a vmcnt(0) wait)
#pragma unroll
    for (int c = 0; c < JT_NCOL; ++c) asm volatile("" : "+v"(trow[c]));

    // one iteration: consume `slot`, refill it for iteration i + U, multiply, accumulate
    // SLOT = i mod U (static), YOUNGER = vector-memory operations issued after the DMA of iteration i
    // that may still be outstanding when iteration i is consumed
    // (compact mixed-radix rows: a step serves row i * ngrp + grp of the iteration table - nit steps in all)
    const int nit = TMIX ? (total + ngrp - 1) / ngrp : total;
    auto step = [&](auto slot_tag, auto younger_tag, const int i) {
        constexpr int SLOT = decltype(slot_tag)::value;
        constexpr int YOUNGER = decltype(younger_tag)::value;
        double p[VEC];
        if constexpr (UNIT) {
            // (filled in below, once the row is known to exist)
        } else if constexpr (TMIX) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) p[e] = (MODE == 0 || tpo[e] >= 0) ? (double)tbuf[SLOT][e] : 0.0;
            const int inext = (i + UT < nit) ? i + UT : nit - 1;
            const int rnext = inext * ngrp + grp;                       // (uniform per wave)
            const uint32_t xnext = (uint32_t)__builtin_amdgcn_readlane(trow[0], rnext < total ? rnext : total - 1);
            gather_row(SLOT, xnext, xnext != JT_NO_ROW && chunk_ok && i + UT < nit && rnext < total);
        } else {
        jt_wait_vmcnt<YOUNGER>();
        const VT v = *reinterpret_cast<const VT *>(ring + SLOT * 1024);
        p[0] = (double)v.x;
        p[1] = (double)v.y;
        if constexpr (VEC == 4) {
            p[2] = (double)v.z;
            p[3] = (double)v.w;
        }
        {   // refill the slot for iteration i + U (the ds_read above has returned: `v` was converted).
            // Past the end the last row is loaded again (cache resident) so that the count of
            // operations in flight stays the same in every step.
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int inext = (i + U < total) ? i + U : total - 1;
            const uint32_t xnext = (uint32_t)__builtin_amdgcn_readlane(trow[0], inext);
            // (KEEP builds: the refill carries the workgroup's policy like the first loads - a kept level's workgroups have 8-16 rows,
            //  and a row loaded non-temporally is a row the other pass fetches from HBM.  Every other build: always non-temporal, no
            //  choice in this loop - the 3.5 % of the note at `keep_rows` above)
            if constexpr (KEEP)
                jt_dma16((xnext == JT_NO_ROW || !chunk_ok) ? zero_row : psi + (xF + xnext),
                         __builtin_amdgcn_readfirstlane(ring_lds + SLOT * 1024), keep_rows);
            else
                jt_dma16((xnext == JT_NO_ROW || !chunk_ok) ? zero_row : psi + (xF + xnext),
                         __builtin_amdgcn_readfirstlane(ring_lds + SLOT * 1024));
        }
        }
        // (compact mixed-radix rows: the second group's last step may have no row - an odd number of rows)
        const int lraw = TMIX ? i * ngrp + grp : i;
        const bool row_there = !TMIX || lraw < total;          // (uniform per wave)
        const int li = row_there ? lraw : total - 1;
        const uint32_t xoff = (uint32_t)__builtin_amdgcn_readlane(trow[0], li);
        const bool row_ok = xoff != JT_NO_ROW && chunk_ok && row_there;   // (uniform)
        if constexpr (TMIX && !UNIT) {
            if (!row_there) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) p[e] = 0.0;
            }
        }
        // TMIX: the table holds existing rows only; the row's place in the full loop nest and the ends of the outgoing
        // messages' runs come with it (jtp_plan.cpp, plan_loops)
        const uint32_t rowinfo = TMIX ? (uint32_t)__builtin_amdgcn_readlane(trow[1 + JT_MAX_IN], li) : 0u;
        const uint32_t inest = TMIX ? (rowinfo >> 16) & 63u : (uint32_t)i;
        if constexpr (UNIT && MODE == 0) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) p[e] = 1.0;          // (entries that do not exist: see the epilogue; rows: below)
        } else if constexpr (UNIT) {
            const double one = row_ok ? 1.0 : 0.0;             // (uniform)
#pragma unroll
            for (int e = 0; e < VEC; ++e) p[e] = tpo[e] >= 0 ? one : 0.0;
        }
        if (ev_mask != 0) {                                // (uniform: no vector instruction is spent without evidence)
            // LOGICAL index of this thread's first element (evidence masks are over index bits, element offsets are
            // physical): chunk bits + the row's loop bits + thread part
            uint32_t x0 = bk.lxF + (uint32_t)vt * VEC;
#pragma unroll
            for (int t = 0; t < JT_MAX_ITER_LOG2; ++t) x0 += ((inest >> t) & 1u) << loop_pos[t];
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (((x0 + e) & ev_mask) != ev_val) p[e] = 0.0;
        }
        int ioff[4], ooff[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) ioff[k] = k < NIN ? __builtin_amdgcn_readlane(trow[1 + k], li) : 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) ooff[j] = j < NOUT ? __builtin_amdgcn_readlane(trow[1 + JT_MAX_IN + j], li) : 0;
        if constexpr (TMIX && NOUT > 0) ooff[0] &= 0xffff;
        double in[NIN > 0 ? NIN : 1][VEC];
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            if constexpr (UNIT) {
                const uint32_t rb = (uint32_t)ioff[k] << 3;        // (scalar)
                if (in_edep[k]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) in[k][e] = *reinterpret_cast<const double *>(smem + (ua[k][e] + rb));
                } else {
                    const double t = *reinterpret_cast<const double *>(smem + (ua[k][0] + rb));
#pragma unroll
                    for (int e = 0; e < VEC; ++e) in[k][e] = t;
                }
                continue;
            }
            const int base = ioff[k] + thr[k];
            if (in_edep[k]) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int eo = ((e & 1) ? in_ew0[k] : 0) + ((e & 2) ? in_ew1[k] : 0);
                    in[k][e] = in_sub[k][base + eo];
                }
            } else {
                const double t = in_sub[k][base];
#pragma unroll
                for (int e = 0; e < VEC; ++e) in[k][e] = t;
            }
        }
        if constexpr (UNIT) {
            // A unit clique's own values arrive as one more incoming table (the static table), so an entry that contradicts the
            // evidence is cut out of the INPUTS: p = 0 alone would meet it in a product, and 0 x inf is NaN.  (Table-keeping
            // cliques: p is the entry itself, replaced above; their inputs are messages, exactly 0 there and finite.)
            if (ev_mask != 0) {                                // (uniform)
#pragma unroll
                for (int e = 0; e < VEC; ++e)
#pragma unroll
                    for (int k = 0; k < NIN; ++k)
                        if (p[e] == 0.0) in[k][e] = 0.0;
            }
        }
        if constexpr (MODE == 0 && UNIT) {
            // a row that does not exist (uniform) adds nothing; without evidence an element is the product of its message
            // entries and nothing else (p = 1 is folded away: (1 * a) * b and a * b are the same double)
            if (row_ok) {
                if (ev_mask == 0) {                            // (uniform)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        double w = NIN > 0 ? in[0][e] : 1.0;
#pragma unroll
                        for (int k = 1; k < NIN; ++k) w *= in[k][e];
#pragma unroll
                        for (int j = 0; j < NOUT; ++j) acc[j][e] += w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        double w = p[e];
#pragma unroll
                        for (int k = 0; k < NIN; ++k) w *= in[k][e];
#pragma unroll
                        for (int j = 0; j < NOUT; ++j) acc[j][e] += w;
                    }
                }
            }
        } else if constexpr (MODE == 0) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                double w = p[e];
#pragma unroll
                for (int k = 0; k < NIN; ++k) w *= in[k][e];
                // (several outputs - read-out tasks only, jt_marginals: every one the sum over its own complement)
#pragma unroll
                for (int j = 0; j < NOUT; ++j) acc[j][e] += w;
            }
        } else {
            double b[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                double pre = p[e];
#pragma unroll
                for (int k = 0; k < NPAR; ++k) pre *= in[k][e];
                // all-but-one products over the children: prefix * suffix
                double suf[NOUT + 1];
                suf[NOUT] = 1.0;
#pragma unroll
                for (int j = NOUT - 1; j >= 0; --j) suf[j] = suf[j + 1] * in[NPAR + j][e];
                double pref = pre;
#pragma unroll
                for (int j = 0; j < NOUT; ++j) {
                    acc[j][e] += pref * suf[j + 1];
                    pref *= in[NPAR + j][e];
                }
                b[e] = pref;
            }
            if constexpr (BEL) if (!UNIT || wr_bel) {
                // beliefs are written once and not read again by this propagate: a streaming store
                // keeps them from sitting dirty in the last-level cache, where the next collect's
                // reads would have to push them out (measured: collect 0.25 -> 0.22 ms)
                typedef T ext_t __attribute__((ext_vector_type(VEC)));
                ext_t ov;
                ov[0] = (T)b[0];
                ov[1] = (T)b[1];
                if constexpr (VEC == 4) {
                    ov[2] = (T)b[2];
                    ov[3] = (T)b[3];
                }
                if constexpr (TMIX) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        if (row_ok && tpo[e] >= 0) __builtin_nontemporal_store(ov[e], bel + (row0 + xoff + (uint32_t)tpo[e]));
                } else
                __builtin_nontemporal_store(ov, reinterpret_cast<ext_t *>(row_ok ? bel + (xF + xoff) : junk_row));
            }
        }
        if constexpr (NOUT > 0) {
            if (!(dbg & 1)) {
                constexpr bool compact = VG;
                if constexpr (compact) {
                    // Two rows per step: a group's sums of a run are complete when the run ends at its own row or at the next one (the
                    // other group's); the epilogue has barriers, so EVERY wave goes through it when either group's are - the first
                    // group's rows are 2 i, 2 i + 2, ..., the second's 2 i + 1, ... (run-end flags beyond the last row: none)
                    auto endbit = [&](const int r, const int j) {
                        return r < total ? ((uint32_t)__builtin_amdgcn_readlane(trow[1 + JT_MAX_IN], r) >> (24 + j)) & 1u : 0u;
                    };
                    auto both = [&](auto j_tag) {
                        constexpr int j = decltype(j_tag)::value;
                        const uint32_t e0 = endbit(2 * i, j), e1 = endbit(2 * i + 1, j), e2 = endbit(2 * i + 2, j);
                        if (e0 | e1 | e2) epilogue(j_tag, ooff[j], grp == 0 ? (e0 | e1) != 0 : (row_there && (e1 | e2) != 0));
                    };
                    both(std::integral_constant<int, 0>{});
                    if constexpr (NOUT > 1) both(std::integral_constant<int, 1>{});
                    if constexpr (NOUT > 2) both(std::integral_constant<int, 2>{});
                } else {
                auto run_ends = [&](const int j) { return TMIX ? ((rowinfo >> (24 + j)) & 1u) != 0 : (i & rmask[j]) == rmask[j]; };
                if (run_ends(0)) epilogue(std::integral_constant<int, 0>{}, ooff[0], true);
                if constexpr (NOUT > 1)
                    if (run_ends(1)) epilogue(std::integral_constant<int, 1>{}, ooff[1], true);
                if constexpr (NOUT > 2)
                    if (run_ends(2)) epilogue(std::integral_constant<int, 2>{}, ooff[2], true);
                }
            }
        }
    };

    JT_STAMP(4);
    // Younger operations when iteration i is consumed: the U-1 later element loads, plus (distribute)
    // one belief store per step already executed since that load was issued: U of them in steady
    // state, k in step k of the first group (its loads were issued in the prologue, before any store).
    constexpr int ST = (MODE == 1) ? 1 : 0;
    using std::integral_constant;
    if constexpr (TMIX) {
        // any number of rows from 1 to 64 (the rows that exist); none at all for a chunk that does not
        if (chunk_ok)
            for (int i0 = 0; i0 < nit; i0 += UT) {
                step(integral_constant<int, 0>{}, integral_constant<int, 0>{}, i0);
                if (i0 + 1 < nit) step(integral_constant<int, 1>{}, integral_constant<int, 0>{}, i0 + 1);
                if (i0 + 2 < nit) step(integral_constant<int, 2>{}, integral_constant<int, 0>{}, i0 + 2);
                if (i0 + 3 < nit) step(integral_constant<int, 3>{}, integral_constant<int, 0>{}, i0 + 3);
            }
    } else {
    {
        step(integral_constant<int, 0>{}, integral_constant<int, U - 1 + 0 * ST>{}, 0);
        JT_STAMP(5);
        step(integral_constant<int, 1>{}, integral_constant<int, U - 1 + 1 * ST>{}, 1);
        JT_STAMP(6);
        if (total > 2) {              // (a workgroup of two iterations - searched splits on latency-bound levels: the
                                      //  other slots hold repeats of its last row)
            step(integral_constant<int, 2>{}, integral_constant<int, U - 1 + 2 * ST>{}, 2);
            JT_STAMP(7);
            step(integral_constant<int, 3>{}, integral_constant<int, U - 1 + 3 * ST>{}, 3);
            JT_STAMP(8);
        }
    }
    for (int i0 = U; i0 < total; i0 += U) {
        step(integral_constant<int, 0>{}, integral_constant<int, U - 1 + U * ST>{}, i0);
        step(integral_constant<int, 1>{}, integral_constant<int, U - 1 + U * ST>{}, i0 + 1);
        step(integral_constant<int, 2>{}, integral_constant<int, U - 1 + U * ST>{}, i0 + 2);
        step(integral_constant<int, 3>{}, integral_constant<int, U - 1 + U * ST>{}, i0 + 3);
    }
    }
    JT_STAMP(9);

    // ---- flush outgoing sub-boxes as this chunk's partial copy ----------------------------------
    if constexpr (NOUT > 0) {
        if (dbg & 1) {
            if (acc[0][0] == 12345.678) msg_arena[0] = acc[0][0];     // keep the sums alive
            return;
        }
        __syncthreads();
        JT_STAMP(10);
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            if constexpr (!EARLY_OUT) {
                uint32_t fp[4];
                if (park != nullptr) {                     // parked in LDS at the start (dataflow kernels); uniform: back into scalars
                    auto word = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)park[8 * j + i]); };
                    so_at[j] = (int64_t)((uint64_t)word(0) | ((uint64_t)word(1) << 32));
                    so_nfree[j] = (int)word(2);
                    fp[0] = word(3), fp[1] = word(4), fp[2] = word(5), fp[3] = word(6);
                } else {
                    const JtMsg &m = tk.msg[JT_MAX_IN + j];
                    const uint32_t *fpw = reinterpret_cast<const uint32_t *>(m.free_pos);
                    so_at[j] = m.off + (int64_t)bk.pnum[j] * m.pstride + bk.gbase[JT_MAX_IN + j];
                    so_nfree[j] = m.nfree;
                    fp[0] = fpw[0], fp[1] = fpw[1], fp[2] = fpw[2], fp[3] = fpw[3];
                }
                so_glo[j] = jt_sub_lo(fp, so_nfree[j], tid);
                so_hiv[j] = jt_sub_hi(fp, so_nfree[j], lane);
            }
            const int64_t at = so_at[j];
            double *dst = msg_arena + fl.cur_off + at + fl.out_shift;
            double *oth = msg_arena + fl.oth_off + at;          // the half the next propagate will use
            const bool mark = fl.oth_off >= 0;
            const int n = 1 << so_nfree[j];
            for (int s = tid, it = 0; s < n; s += JT_THREADS, ++it) {
                const uint32_t idx = so_glo[j] + (uint32_t)__builtin_amdgcn_readlane((int)so_hiv[j], it);
                jt_msg_store<FLOW>(dst + idx, out_sub[j][s]);
                if (mark) oth[idx] = __longlong_as_double((long long)JT_UNWRITTEN);
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
