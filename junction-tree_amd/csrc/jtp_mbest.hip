// The M most probable assignments on the device: jtp_map_best.
#include "jtp_maxprod.h"

// jtp_map_best runs the upward pass of jtp_map with a LIST per message entry - the CAP largest values, non-increasing, zero past
// their count - and a place (r, t) per element: entry r of the clique's slice, element t of that entry's list.  An entry's list is a
// fold over the children in ascending clique number, E_0 = [psi], E_i = the CAP largest positive products E_{i-1}[a] * m_i[b]; a
// product can only be among them where (a + 1) * (b + 1) <= CAP, and then no earlier than at place (a + 1) * (b + 1) - 1 (the
// products at (a' <= a, b' <= b) are no smaller and come first).  CAP is a template parameter and every list lives in registers:
// all loops over a list are unrolled, every index is a constant, nothing is indexed at run time (so nothing goes to scratch; the
// resource report is in profiles/mbest_resources.txt).  A call for m assignments runs the smallest CAP >= m of 1, 4, 16: the first
// m of a longer list are the shorter list (an element with a >= m or b >= m has m before it).
// jt_mbest_level: a wave64 per (clique, k, segment of r), a lane per contiguous block of r, as jt_max_level walks it; the lane
// keeps the CAP best (value, r, t) of its block - ascending r, so equal values stay in ascending (r, t) - and the wave takes the
// best head of its 64 lanes CAP times, the lower lane among equals (its r are smaller).  jt_mbest_merge does the same over the
// segments' lists.  jt_mbest_decode: a workgroup per solution s; the thread of a clique reads (r, t) at its rank (the root's: s),
// writes the digits of F, forms the fold of that one entry again - same operations, same order: the same bits - this time with the
// (a, b) of every element, and walks back from element t: b is the child's rank, a the element of the fold before.
struct JtMbestWork {                 // one evidence set; `cap` elements per list
    double *raw, *part_w;            // [(raw_off + k) * cap + j]; [(part_off + k * nseg + seg) * cap + j]
    unsigned long long *rt, *part_rt;    // beside them: (r << 4) | t
    unsigned long long *top;         // [ord]: bit pattern of the largest first element of the clique's lists
    const void **psi;                // [1]: the set's potential arena
    int32_t *ev, *states, *rank;     // [n_vars]; [m * n_vars]; [m * n_rec]: the rank solution s takes of each clique's list
    int32_t *flag;
    unsigned char *bp;               // [(s * n_kids + child) * cap + j]: (a << 4) | b of element j of the fold up to that child
    size_t bytes;
};
static JtMbestWork mbest_work(char *base, size_t cap, size_t m, size_t entries, size_t parts, size_t n_rec, size_t n_kids, size_t n_vars) {
    JtMbestWork w;
    size_t at = 0;
    auto take = [&](size_t n) { char *p = base + at; at += n; return p; };
    w.raw = (double *)take(entries * cap * 8);
    w.part_w = (double *)take(parts * cap * 8);
    w.rt = (unsigned long long *)take(entries * cap * 8);
    w.part_rt = (unsigned long long *)take(parts * cap * 8);
    w.top = (unsigned long long *)take(n_rec * 8);
    w.psi = (const void **)take(8);
    w.ev = (int32_t *)take(n_vars * 4);
    w.states = (int32_t *)take(m * n_vars * 4);
    w.rank = (int32_t *)take(m * n_rec * 4);
    w.flag = (int32_t *)take(4);
    w.bp = (unsigned char *)take(m * n_kids * cap);
    w.bytes = at;
    return w;
}

// p into the non-increasing list V from place `from` on (what lies before is known to be no smaller), behind its equals; the last
// element drops out.  The tag travels with its value: once p has taken a place, everything behind moves down by one.
template <int CAP, typename Tag>
__device__ __forceinline__ void jt_mbest_insert(double (&V)[CAP], Tag (&G)[CAP], double p, Tag g, int from) {
    bool moved = false;
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        if (i < from) continue;
        moved = moved || p > V[i];
        if (moved) {
            const double v = V[i];
            const Tag t = G[i];
            V[i] = p, G[i] = g;
            p = v, g = t;
        }
    }
}
// one step of the fold, values alone (equal values need no order among themselves): E = the CAP largest positive E[a] * msg[b]
template <int CAP>
__device__ __forceinline__ void jt_mbest_fold(double (&E)[CAP], const double (&msg)[CAP]) {
    double N[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) N[i] = 0.0;
#pragma unroll
    for (int a = 0; a < CAP; ++a) {
#pragma unroll
        for (int b = 0; b < CAP / (a + 1); ++b) {
            double p = E[a] * msg[b];
            if (p > N[CAP - 1]) {                         // (0 and NaN never are)
#pragma unroll
                for (int i = (a + 1) * (b + 1) - 1; i < CAP; ++i)
                    if (p > N[i]) {
                        const double v = N[i];
                        N[i] = p;
                        p = v;
                    }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i) E[i] = N[i];
}
// ... and with the (a << 4) | b of every element: descending value, equal values in ascending (a, b) - the order they are formed in
template <int CAP>
__device__ __forceinline__ void jt_mbest_fold_tagged(double (&E)[CAP], const double (&msg)[CAP], unsigned (&G)[CAP]) {
    double N[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) N[i] = 0.0, G[i] = 0u;
#pragma unroll
    for (int a = 0; a < CAP; ++a) {
#pragma unroll
        for (int b = 0; b < CAP / (a + 1); ++b) {
            const double p = E[a] * msg[b];
            if (p > N[CAP - 1]) jt_mbest_insert<CAP, unsigned>(N, G, p, (unsigned)(a << 4 | b), (a + 1) * (b + 1) - 1);
        }
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i) E[i] = N[i];
}
// The lists of a wave's 64 lanes - lane l's places all before lane l + 1's - into one, CAP times the best head; lane 0 writes it to
// out_v / out_rt.  Returns the first element's value (in every lane).
template <int CAP>
__device__ __forceinline__ double jt_mbest_wave_store(double (&V)[CAP], unsigned long long (&G)[CAP], int lane, double *out_v, unsigned long long *out_rt) {
    double first = 0.0;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        double bv = V[0];
        int bl = lane;
        for (int d = 32; d >= 1; d >>= 1) {
            const double ow = __shfl_xor(bv, d, 64);
            const int ol = __shfl_xor(bl, d, 64);
            if (ow > bv || (ow == bv && ol < bl)) bv = ow, bl = ol;
        }
        unsigned long long g = __shfl(G[0], bl, 64);
        if (!(bv > 0.0)) bv = 0.0, g = 0ull;             // (the lists are exhausted)
        if (j == 0) first = bv;
        if (lane == 0) out_v[j] = bv, out_rt[j] = g;
        if (lane == bl) {
#pragma unroll
            for (int i = 0; i + 1 < CAP; ++i) V[i] = V[i + 1], G[i] = G[i + 1];
            V[CAP - 1] = 0.0, G[CAP - 1] = 0ull;
        }
    }
    return first;
}
// the largest first element of a clique's lists, kept as jt_maxprod_keep_top keeps a maximum (written out: through that function
// jt_mbest_level compiled to 2 to 4 other instructions, and jtp_map_best for m = 1 on the wide tree took 0.734 ms where it takes 0.721)
__device__ __forceinline__ void jt_mbest_top(const JtMap &rec, const JtMbestWork &wk, double first) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(first);
    unsigned long long *top = wk.top + rec.ord;
    if (__atomic_load_n(top, __ATOMIC_RELAXED) < bits) atomicMax(top, bits);
}

template <typename T, int CAP>
__global__ __launch_bounds__(256) void jt_mbest_level(const JtMap *__restrict__ recs, const JtMapChild *__restrict__ kids, JtMbestWork wk, int n_vars) {
    __shared__ int digs[JT_MAX_VARS][256];             // digit j of thread t's counter: a column per thread (K digits: the wave's, in every column)
    __shared__ JtSampleVar sv[JT_MAX_VARS];
    __shared__ int obs[4][JT_MAX_VARS];                // per wave: the observed state of v[j], -1: none
    // the first JT_QUERY_KIDS children, staged as jt_map_collect_level stages them
    __shared__ uint32_t kstride[JT_QUERY_KIDS][JT_MAX_VARS];
    __shared__ int64_t kraw[JT_QUERY_KIDS];
    __shared__ int kord[JT_QUERY_KIDS];
    __shared__ uint32_t kbase[4][JT_QUERY_KIDS];
    __shared__ int kexp[4][JT_QUERY_KIDS];
    const JtMap &rec = recs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nK = rec.nK, nF = rec.nF, nv = nK + nF;
    jt_query_stage_vars(sv, rec.v, nv, tid);
    const int n_kids = rec.child_end - rec.child_begin;
    const int n_staged = jt_query_stage_kids(kstride, kids + rec.child_begin, n_kids, tid);
    if (tid < n_staged) kraw[tid] = kids[rec.child_begin + tid].raw_off, kord[tid] = kids[rec.child_begin + tid].ord;
    __syncthreads();
    const JtSampleVar *fv = sv + nK;
    const uint32_t R = rec.R, nk = rec.nk, nseg = rec.nseg;
    const uint32_t seg_len = (R + nseg - 1u) / nseg;
    const int64_t n_items = (int64_t)nk * nseg;
    const T *tab = (const T *)wk.psi[0];
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < n_items; item += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const uint32_t seg = (uint32_t)(item % nseg), k = (uint32_t)(item / nseg);
        __builtin_amdgcn_wave_barrier();                // (the wave's row of `obs` is rewritten: its reads of the last item are done)
        if (lane < nv) obs[wave][lane] = wk.ev[sv[lane].col];
        __builtin_amdgcn_wave_barrier();
        bool dead = false, obs_f = false;
        int64_t base = rec.psi_off;
        for (int j = 0; j < nK; ++j) {
            const int dg = (int)((k / sv[j].radix) % (uint32_t)sv[j].card), o = obs[wave][j];
            digs[j][tid] = dg;
            if (o >= 0 && o != dg) dead = true;
            base += jt_sample_at(sv[j], dg);
        }
        for (int j = nK; j < nv; ++j) obs_f = obs_f || obs[wave][j] >= 0;
        if (lane < n_staged) {                             // (the K digits are in every lane's column)
            kbase[wave][lane] = jt_query_kid_at(0u, kstride[lane], digs, tid, 0, nK);
            kexp[wave][lane] = jt_map_exp(wk.top[kord[lane]]);
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t lo = min(seg * seg_len, R), end = min(lo + seg_len, R);
        const auto [a, e, B] = jt_query_cut(lo, end, 64u, (uint32_t)lane);
        double V[CAP];                                     // the lane's best: values and (r << 4) | t
        unsigned long long G[CAP];
#pragma unroll
        for (int i = 0; i < CAP; ++i) V[i] = 0.0, G[i] = 0ull;
        bool bad = false;
        if (!dead && a < e) {
            uint32_t off = jt_query_walk_start(fv, nF, digs + nK, tid, a);
            for (uint32_t q = a;;) {
                int contra = 0;                            // digits of F that contradict the evidence
                if (obs_f)
                    for (int j = nK; j < nv; ++j) {
                        const int o = obs[wave][j];
                        contra += (o >= 0 && o != digs[j][tid]) ? 1 : 0;
                    }
                if (contra == 0) {
                    const T x = tab[base + off];
                    bad = bad || !(x >= (T)0);
                    double E[CAP], msg[CAP];
#pragma unroll
                    for (int i = 0; i < CAP; ++i) E[i] = 0.0;
                    if (x > (T)0) E[0] = (double)x;
                    for (int c = 0; c < n_kids; ++c) {     // (ascending clique number; the ones beyond the staged are read where they lie)
                        const double *list;
                        int ex;
                        if (c < n_staged) {
                            list = wk.raw + (kraw[c] + jt_query_kid_at(kbase[wave][c], kstride[c], digs, tid, nK, nv)) * CAP;
                            ex = kexp[wave][c];
                        } else {
                            const JtMapChild &kid = kids[rec.child_begin + c];
                            list = wk.raw + (kid.raw_off + jt_query_kid_at(kid, digs, tid, nv)) * CAP;
                            ex = jt_map_exp(wk.top[kid.ord]);
                        }
#pragma unroll
                        for (int i = 0; i < CAP; ++i) msg[i] = ldexp(list[i], -ex);
                        jt_mbest_fold<CAP>(E, msg);
                    }
#pragma unroll
                    for (int t = 0; t < CAP; ++t)          // (ascending r, then t: equal values stay in that order)
                        if (E[t] > V[CAP - 1]) jt_mbest_insert<CAP, unsigned long long>(V, G, E[t], (unsigned long long)q << 4 | (unsigned)t, 0);
                }
                if (++q == e) break;
                off = jt_query_walk_next(fv, nF, digs + nK, tid, off);
            }
        }
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == 0 && any_bad) atomicOr(wk.flag, 1);
        if (nseg > 1) {
            const int64_t p = (rec.part_off + (int64_t)k * nseg + seg) * CAP;
            jt_mbest_wave_store<CAP>(V, G, lane, wk.part_w + p, wk.part_rt + p);
        } else {
            const int64_t p = (rec.raw_off + k) * CAP;
            const double first = jt_mbest_wave_store<CAP>(V, G, lane, wk.raw + p, wk.rt + p);
            if (lane == 0) jt_mbest_top(rec, wk, first);
        }
    }
}

// cliques cut into segments: a wave per (clique, k); a lane takes a contiguous run of segments, in ascending order
template <int CAP>
__global__ __launch_bounds__(256) void jt_mbest_merge(const JtMap *__restrict__ recs, JtMbestWork wk) {
    const JtMap &rec = recs[blockIdx.y];
    const uint32_t nseg = rec.nseg, nk = rec.nk;
    if (nseg <= 1) return;
    const int lane = threadIdx.x & 63;
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < (int64_t)nk; k += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const int64_t p0 = rec.part_off + k * nseg;
        const auto [a, e, B] = jt_query_cut(0u, nseg, 64u, (uint32_t)lane);
        double V[CAP];
        unsigned long long G[CAP];
#pragma unroll
        for (int i = 0; i < CAP; ++i) V[i] = 0.0, G[i] = 0ull;
        for (uint32_t s = a; s < e; ++s) {
            const double *pv = wk.part_w + (p0 + s) * CAP;
            const unsigned long long *pg = wk.part_rt + (p0 + s) * CAP;
#pragma unroll
            for (int t = 0; t < CAP; ++t) {
                const double v = pv[t];
                if (v > V[CAP - 1]) jt_mbest_insert<CAP, unsigned long long>(V, G, v, pg[t], 0);
            }
        }
        const int64_t p = (rec.raw_off + k) * CAP;
        const double first = jt_mbest_wave_store<CAP>(V, G, lane, wk.raw + p, wk.rt + p);
        if (lane == 0) jt_mbest_top(rec, wk, first);
    }
}

// a workgroup per solution: threads over the cliques of a depth, a barrier between depths; the solution's rows are this workgroup's alone
template <typename T, int CAP>
__global__ __launch_bounds__(256) void jt_mbest_decode(const JtMap *__restrict__ recs, const JtMapChild *__restrict__ kids, const int32_t *__restrict__ depth_begin,
                                                        int n_depths, JtMbestWork wk, int n_vars, int n_rec, int n_kids) {
    const int s = blockIdx.x, tid = threadIdx.x;
    int32_t *row = wk.states + (int64_t)s * n_vars;
    int32_t *rank = wk.rank + (int64_t)s * n_rec;
    unsigned char *bp = wk.bp + (int64_t)s * n_kids * CAP;
    int fail = wk.flag[0] != 0;
    for (int c = tid; c < n_rec; c += 256) fail |= jt_map_bad(wk.top[c]) ? 1 : 0;
    fail = __syncthreads_or(fail);
    if (fail || !(wk.raw[recs[0].raw_off * CAP + s] > 0.0)) {       // (s < m <= CAP; no s-th assignment of positive value)
        for (int v = tid; v < n_vars; v += 256) row[v] = -1;
        return;
    }
    if (tid == 0) rank[0] = s;
    __syncthreads();
    const T *tab = (const T *)wk.psi[0];
    for (int d = 0; d < n_depths; ++d) {
        for (int c = depth_begin[d] + tid; c < depth_begin[d + 1]; c += 256) {
            const JtMap &rec = recs[c];
            const int nv = rec.nK + rec.nF;
            uint32_t k = 0;
            for (int j = 0; j < rec.nK; ++j) k += (uint32_t)row[rec.v[j].col] * rec.v[j].radix;
            const unsigned long long g = wk.rt[(rec.raw_off + k) * CAP + rank[c]];
            const uint32_t r = (uint32_t)(g >> 4);
            for (int j = rec.nK; j < nv; ++j) row[rec.v[j].col] = (int)((r / rec.v[j].radix) % (uint32_t)rec.v[j].card);
            if (rec.child_begin == rec.child_end) continue;
            // the fold of entry (k, r) once more, keeping where every element came from
            int64_t off = rec.psi_off;
            for (int j = 0; j < nv; ++j) off += jt_sample_at(rec.v[j], row[rec.v[j].col]);
            const T x = tab[off];
            double E[CAP], msg[CAP];
            unsigned tags[CAP];
#pragma unroll
            for (int i = 0; i < CAP; ++i) E[i] = 0.0;
            if (x > (T)0) E[0] = (double)x;
            for (int ch = rec.child_begin; ch < rec.child_end; ++ch) {
                const JtMapChild &kid = kids[ch];
                uint32_t at = 0;
                for (int j = 0; j < nv; ++j) at += (uint32_t)row[rec.v[j].col] * kid.stride[j];
                const double *list = wk.raw + (kid.raw_off + at) * CAP;
                const int ex = jt_map_exp(wk.top[kid.ord]);
#pragma unroll
                for (int i = 0; i < CAP; ++i) msg[i] = ldexp(list[i], -ex);
                jt_mbest_fold_tagged<CAP>(E, msg, tags);
#pragma unroll
                for (int i = 0; i < CAP; ++i) bp[(int64_t)ch * CAP + i] = (unsigned char)tags[i];
            }
            int cur = (int)(g & 15ull);
            for (int ch = rec.child_end - 1; ch >= rec.child_begin; --ch) {
                const unsigned tag = bp[(int64_t)ch * CAP + cur];
                rank[kids[ch].ord] = (int)(tag & 15u);
                cur = (int)(tag >> 4);
            }
        }
        __syncthreads();
    }
}

// the launches of jtp_map_best for lists of CAP elements
template <int CAP>
static void mbest_launch(const HostPlan &hp, const MapMem &up, const JtMbestWork &wk, int m, size_t n_kids, hipStream_t s) {
    const int n_vars = hp.n_vars, n_rec = (int)hp.sample.size(), n_depths = (int)hp.sample_depths.size();
    maxprod_upward(hp, up, 1, [&](const JtMap *recs, dim3 grid, dim3 mgrid, bool merge) {
        if (hp.dtype == JTP_F32) hipLaunchKernelGGL((jt_mbest_level<float, CAP>), grid, dim3(256), 0, s, recs, up.kids.get(), wk, n_vars);
        else hipLaunchKernelGGL((jt_mbest_level<double, CAP>), grid, dim3(256), 0, s, recs, up.kids.get(), wk, n_vars);
        if (merge) hipLaunchKernelGGL(jt_mbest_merge<CAP>, mgrid, dim3(256), 0, s, recs, wk);
    });
    if (hp.dtype == JTP_F32)
        hipLaunchKernelGGL((jt_mbest_decode<float, CAP>), dim3((unsigned)m), dim3(256), 0, s, up.recs.get(), up.kids.get(), up.depth_begin.get(), n_depths, wk, n_vars, n_rec, (int)n_kids);
    else
        hipLaunchKernelGGL((jt_mbest_decode<double, CAP>), dim3((unsigned)m), dim3(256), 0, s, up.recs.get(), up.kids.get(), up.depth_begin.get(), n_depths, wk, n_vars, n_rec, (int)n_kids);
}

extern "C" int jtp_map_best(jtp_plan *pl, int32_t batch, int32_t m, int32_t *states, double *log_value, int32_t *n_found) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if ((rc = maxprod_refuse("jtp_map_best", hp, batch, batch + 1))) return rc;      // (check_ready has seen to the one set's range)
    if (m < 1 || m > JTP_MBEST_MAX) return set_err(JTP_EINVAL, "jtp_map_best: m = %d, not in [1,%d]", m, JTP_MBEST_MAX);
    if (!states || !log_value || !n_found) return set_err(JTP_EINVAL, "null argument");
    const size_t n_vars = (size_t)hp.n_vars, n_rec = hp.sample.size();
    const size_t cap = m <= 1 ? 1 : m <= 4 ? 4 : 16;
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_map_best");
    // (the potentials may have been written on any of the plan's streams; a propagate in flight only reads them, as this does)
    for (auto st : pl->streams) HIP_TRY(hipStreamSynchronize(st));
    hipStream_t s = pl->streams[0];
    // (jtp_map's records, made here if no call has yet, and a larger work area are built into locals and moved into the plan once
    //  complete - a call that fails an allocation leaves the plan as it found it)
    MapMem fresh_map(&pl->mem);
    MbestMem fresh(&pl->mem);
    const bool need_map = !pl->map.recs;
    if ((rc = map_upward_records(pl, fresh_map))) return rc;
    const MapMem &lay = need_map ? fresh_map : pl->map;    // (whose sizes hold)
    const size_t entries = (size_t)lay.entries, parts = (size_t)lay.parts, n_kids = lay.kids.size();
    const size_t need = mbest_work(nullptr, cap, (size_t)m, entries, parts, n_rec, n_kids, n_vars).bytes;
    if (pl->mbest.work.size() < need) HIP_TRY(fresh.work.alloc(need));
    if (need_map) pl->map = std::move(fresh_map);          // (no work area, room for no set: jtp_map allocates its own at its next call)
    if (fresh.work) pl->mbest.work = std::move(fresh.work);
    const JtMbestWork wk = mbest_work(pl->mbest.work.get(), cap, (size_t)m, entries, parts, n_rec, n_kids, n_vars);
    std::vector<const void *> psi(1);
    std::vector<int32_t> ev(n_vars, -1);
    if ((rc = maxprod_stage_sets(pl, (size_t)batch, 1, psi, ev, wk.psi, wk.ev, wk.top, wk.flag, s))) return rc;
    if (n_vars) HIP_TRY(hipMemsetAsync(wk.states, 0, (size_t)m * n_vars * sizeof(int32_t), s));      // (a variable of no clique stays 0)
    if (cap == 1) mbest_launch<1>(hp, pl->map, wk, m, n_kids, s);
    else if (cap == 4) mbest_launch<4>(hp, pl->map, wk, m, n_kids, s);
    else mbest_launch<16>(hp, pl->map, wk, m, n_kids, s);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> top(n_rec);
    std::vector<double> root(cap);
    int32_t flag = 0;
    if (n_vars) HIP_TRY(hipMemcpyAsync(states, wk.states, (size_t)m * n_vars * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(top.data(), wk.top, n_rec * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    // (record 0 is the root: it shares nothing with a parent, its one list is the first of the raw table)
    HIP_TRY(hipMemcpyAsync(root.data(), wk.raw, cap * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&flag, wk.flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // log_value[s]: of the s-th element of the root's list, with the exponents taken out of the messages as jtp_map sums them
    const MaxprodValue val = maxprod_value(top.data(), n_rec, flag != 0);
    *n_found = 0;
    for (int i = 0; i < m; ++i) {
        if (!val.failed && root[i] > 0.0) {
            log_value[i] = maxprod_log(root[i], val.esum);
            ++*n_found;
        } else
            log_value[i] = -INFINITY;
    }
    if (val.failed)
        return set_err(JTP_EINVAL, "jtp_map_best: evidence set %d has no assignment of positive finite value (a negative or NaN entry, "
                                   "or a maximum that is zero or not finite: evidence of probability zero?); its states are -1, its log_value -inf", batch);
    return JTP_OK;
}
