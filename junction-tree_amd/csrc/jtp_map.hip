// The max-product unit: the most probable joint assignment (jtp_map, an upward sweep over the clique potentials and a decode),
// max-propagation (jtp_max_marginals, the same upward sweep, a downward one and a read-out of max-marginals) and the M most probable
// assignments (jtp_map_best, an upward sweep of the same shape over lists and a decode per solution), on the device.
#include <cmath>

#include <algorithm>
#include <cstring>
#include <vector>

#include "jtp_engine.h"
#include "jtp_query.h"

// jtp_map works on the sampling schedule (HostPlan::sample: the caller's tree by depth, then clique number; K the variables a clique
// shares with its parent, F the others in host axis order, R = prod card(F)) and on the potentials alone - no propagate is needed or
// touched.  Upward, one launch per depth, deepest first (jt_map_collect_level): a wave64 per (clique, evidence set, assignment k of
// K, segment of r).  Every lane walks a contiguous block of r - a mixed-radix counter over F, its digits in LDS, moves the table
// offset - and forms, for every entry that agrees with the set's evidence,
//     w(k, r) = ((double)psi[k, r] * m_1) * m_2 * ...          the children in ascending clique number, float64, left to right
//     m_d = ldexp(raw_d[k_d], -e_d),  e_d = ilogb(max raw_d)   so the largest entry of every message read lies in [1, 2)
// keeping (largest w, first r that has it); six shuffle steps give the wave's.  raw_c[k] = that maximum, arg_c[k] = that r (0 and 0
// where k contradicts the evidence), and the maximum of raw_c is kept as an integer maximum over bit patterns - non-negative doubles
// order like their bits, so it is exact whatever the order.  Cliques of many entries per k are cut into segments of r, a wave each;
// jt_map_merge takes the segments in ascending order.  Nothing depends on the stored layout but the offsets jt_sample_at gives, nor
// on how r was cut: equal potentials give equal assignments whatever the plan's flags.  Downward, jt_map_decode: a workgroup per
// set reads arg_c[k] at the digits the cliques above wrote and writes the digits of F_c.
// A set fails where an entry that agrees with its evidence is negative or NaN, or where a clique's maximum is zero or not finite
// (the root's then is): its states are -1.

// ilogb of the finite double >= 0 with this bit pattern (0 for 0.0)
__host__ __device__ static inline int jt_map_exp(unsigned long long bits) {
    const int ex = (int)(bits >> 52) & 0x7ff;
    if (ex) return ex - 1023;
    return bits ? -1011 - __builtin_clzll(bits) : 0;
}
// ... and whether it is one a set fails on: zero, infinite
__host__ __device__ static inline bool jt_map_bad(unsigned long long bits) { return bits == 0ull || ((bits >> 52) & 0x7ffull) == 0x7ffull; }

// the work area of one chunk of `sets` evidence sets (MapMem::work): 8-byte items first
struct JtMapWork {
    double *raw, *part_w;
    unsigned long long *top;         // [set * n_rec + ord]: bit pattern of the largest entry of the clique's raw table
    const void **psi;                // [set]: the set's potential arena
    uint32_t *arg, *part_r;
    int32_t *ev, *states, *flag;
    size_t bytes;
};
static JtMapWork map_work(char *base, size_t sets, size_t entries, size_t parts, size_t n_rec, size_t n_vars) {
    JtMapWork w;
    size_t at = 0;
    auto take = [&](size_t n) { char *p = base + at; at += n; return p; };
    w.raw = (double *)take(sets * entries * 8);
    w.part_w = (double *)take(sets * parts * 8);
    w.top = (unsigned long long *)take(sets * n_rec * 8);
    w.psi = (const void **)take(sets * 8);
    w.arg = (uint32_t *)take(sets * entries * 4);
    w.part_r = (uint32_t *)take(sets * parts * 4);
    w.ev = (int32_t *)take(sets * n_vars * 4);
    w.states = (int32_t *)take(sets * n_vars * 4);
    w.flag = (int32_t *)take(sets * 4);
    w.bytes = at;
    return w;
}

// the wave's (largest w, smallest r among equals), in every lane: six shuffle steps
__device__ __forceinline__ void jt_map_wave_best(double &best, uint32_t &best_r) {
    for (int d = 32; d >= 1; d >>= 1) {
        const double ow = __shfl_xor(best, d, 64);
        const uint32_t orr = __shfl_xor(best_r, d, 64);
        if (ow > best || (ow == best && orr < best_r)) best = ow, best_r = orr;
    }
}

// lane 0 of a wave: raw_c[k], arg_c[k] and the clique's running maximum
__device__ __forceinline__ void jt_map_store(const JtMap &rec, const JtMapWork &wk, int set, uint32_t k, double best, uint32_t best_r, int n_rec, int64_t entries) {
    if (!(best >= 0.0)) best = 0.0, best_r = 0;          // (nothing looked at: k contradicts the evidence)
    best = fabs(best);                                   // (-0.0: its bit pattern would be the largest of all)
    const int64_t p = (int64_t)set * entries + rec.raw_off + k;
    wk.raw[p] = best;
    wk.arg[p] = best_r;
    unsigned long long *top = wk.top + (int64_t)set * n_rec + rec.ord;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(best);
    if (__atomic_load_n(top, __ATOMIC_RELAXED) < bits) atomicMax(top, bits);       // (the maximum only grows: most waves need no atomic)
}

template <typename T>
__global__ __launch_bounds__(256) void jt_map_collect_level(const JtMap *__restrict__ recs, const JtMapChild *__restrict__ kids, JtMapWork wk,
                                                            int n_vars, int n_rec, int n_chunk, int64_t entries, int64_t parts) {
    __shared__ int digs[JT_MAX_VARS][256];             // digit j of thread t's counter: a column per thread (K digits: the wave's, in every column)
    __shared__ JtSampleVar sv[JT_MAX_VARS];
    __shared__ int obs[4][JT_MAX_VARS];                // per wave: the observed state of v[j] in the wave's set, -1: none
    // the first JT_QUERY_KIDS children: strides, place of the raw table and record, staged once; per wave and item the part of the
    // index the K digits fix and the exponent of the child's maximum (read from global memory per entry, each of these is a
    // dependent scalar load: 12 000 cycles an entry on the width-20 tree)
    __shared__ uint32_t kstride[JT_QUERY_KIDS][JT_MAX_VARS];
    __shared__ int64_t kraw[JT_QUERY_KIDS];
    __shared__ int kord[JT_QUERY_KIDS];
    __shared__ uint32_t kbase[4][JT_QUERY_KIDS];
    __shared__ int kexp[4][JT_QUERY_KIDS];
    const JtMap &rec = recs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nK = rec.nK, nF = rec.nF, nv = nK + nF;
    jt_query_stage_vars(sv, rec.v, nv, tid);
    const int n_staged = jt_query_stage_kids(kstride, kids + rec.child_begin, rec.child_end - rec.child_begin, tid);
    if (tid < n_staged) kraw[tid] = kids[rec.child_begin + tid].raw_off, kord[tid] = kids[rec.child_begin + tid].ord;
    __syncthreads();
    const JtSampleVar *fv = sv + nK;
    const uint32_t R = rec.R, nk = rec.nk, nseg = rec.nseg;
    const uint32_t seg_len = (R + nseg - 1u) / nseg;
    const int64_t n_items = (int64_t)n_chunk * nk * nseg;
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < n_items; item += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const uint32_t seg = (uint32_t)(item % nseg), k = (uint32_t)((item / nseg) % nk);
        const int set = (int)(item / ((int64_t)nseg * nk));
        const int32_t *evr = wk.ev + (int64_t)set * n_vars;
        __builtin_amdgcn_wave_barrier();                // (the wave's row of `obs` is rewritten: its reads of the last item are done)
        if (lane < nv) obs[wave][lane] = evr[sv[lane].col];
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
        const T *tab = (const T *)wk.psi[set];
        const double *raw_set = wk.raw + (int64_t)set * entries;
        const unsigned long long *top_set = wk.top + (int64_t)set * n_rec;
        if (lane < n_staged) {                             // (the K digits are in every lane's column)
            kbase[wave][lane] = jt_query_kid_at(0u, kstride[lane], digs, tid, 0, nK);
            kexp[wave][lane] = jt_map_exp(top_set[kord[lane]]);
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t lo = min(seg * seg_len, R), end = min(lo + seg_len, R);
        const auto [a, e, B] = jt_query_cut(lo, end, 64u, (uint32_t)lane);
        double best = -1.0;                                // (nothing looked at yet: every w >= 0 beats it)
        uint32_t best_r = 0xffffffffu;
        bool bad = false;
        if (!dead && a < e) {
            // (the walk of jtp_query.h, written out: the count of contradictions is kept with the digits - see the note there)
            uint32_t off = 0;
            int contra = 0;                                // digits of F that contradict the evidence
            for (int j = 0; j < nF; ++j) {
                const int dg = (int)((a / fv[j].radix) % (uint32_t)fv[j].card), o = obs[wave][nK + j];
                digs[nK + j][tid] = dg;
                off += jt_sample_at(fv[j], dg);
                contra += (o >= 0 && o != dg) ? 1 : 0;
            }
            for (uint32_t q = a;;) {
                if (contra == 0) {
                    const T x = tab[base + off];
                    bad = bad || !(x >= (T)0);
                    double w = (double)x;
                    for (int c = 0; c < n_staged; ++c) {
                        const uint32_t at = jt_query_kid_at(kbase[wave][c], kstride[c], digs, tid, nK, nv);
                        w *= ldexp(raw_set[kraw[c] + at], -kexp[wave][c]);
                    }
                    for (int c = rec.child_begin + n_staged; c < rec.child_end; ++c) {      // (more children than are staged: ascending order still)
                        const JtMapChild &kid = kids[c];
                        w *= ldexp(raw_set[kid.raw_off + jt_query_kid_at(kid, digs, tid, nv)], -jt_map_exp(top_set[kid.ord]));
                    }
                    if (w > best) best = w, best_r = q;    // (ascending r: the first of equals stays; a NaN is never taken)
                }
                if (++q == e) break;
                for (int j = nF - 1; j >= 0; --j) {         // the next assignment in C order
                    const JtSampleVar v = fv[j];
                    const int dg = digs[nK + j][tid];
                    const int o = obs_f ? obs[wave][nK + j] : -1;
                    if (dg + 1 < v.card) {
                        off += jt_sample_at(v, dg + 1) - jt_sample_at(v, dg);
                        digs[nK + j][tid] = dg + 1;
                        if (o >= 0) contra += (o != dg + 1 ? 1 : 0) - (o != dg ? 1 : 0);
                        break;
                    }
                    off -= jt_sample_at(v, dg);
                    digs[nK + j][tid] = 0;
                    if (o >= 0) contra += (o != 0 ? 1 : 0) - (o != dg ? 1 : 0);
                }
            }
        }
        jt_map_wave_best(best, best_r);
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == 0) {
            if (any_bad) atomicOr(&wk.flag[set], 1);
            if (nseg > 1) {                                // (jt_map_merge: -1 = the segment has no entry that counts)
                const int64_t p = (int64_t)set * parts + rec.part_off + (int64_t)k * nseg + seg;
                wk.part_w[p] = best;
                wk.part_r[p] = best_r;
            } else
                jt_map_store(rec, wk, set, k, best, best_r, n_rec, entries);
        }
    }
}

// cliques cut into segments: a wave per (clique, set, k) puts the segments' results together (a segment's r lie before the next one's)
__global__ __launch_bounds__(256) void jt_map_merge(const JtMap *__restrict__ recs, JtMapWork wk, int n_rec, int n_chunk, int64_t entries, int64_t parts) {
    const JtMap &rec = recs[blockIdx.y];
    const uint32_t nseg = rec.nseg, nk = rec.nk;
    if (nseg <= 1) return;
    const int lane = threadIdx.x & 63;
    const int64_t n_items = (int64_t)n_chunk * nk;
    for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const uint32_t k = (uint32_t)(item % nk);
        const int set = (int)(item / nk);
        const int64_t p0 = (int64_t)set * parts + rec.part_off + (int64_t)k * nseg;
        double best = -1.0;
        uint32_t best_r = 0xffffffffu;
        for (uint32_t s = (uint32_t)lane; s < nseg; s += 64u) {
            const double w = wk.part_w[p0 + s];
            if (w > best) best = w, best_r = wk.part_r[p0 + s];
        }
        jt_map_wave_best(best, best_r);
        if (lane == 0) jt_map_store(rec, wk, set, k, best, best_r, n_rec, entries);
    }
}

// a workgroup per set: threads over the cliques of a depth, a barrier between depths; the set's state row is this workgroup's alone
__global__ __launch_bounds__(256) void jt_map_decode(const JtMap *__restrict__ recs, const int32_t *__restrict__ depth_begin, int n_depths, JtMapWork wk,
                                                     int n_vars, int n_rec, int64_t entries) {
    const int set = blockIdx.x, tid = threadIdx.x;
    int32_t *row = wk.states + (int64_t)set * n_vars;
    const uint32_t *arg_set = wk.arg + (int64_t)set * entries;
    int fail = wk.flag[set] != 0;
    for (int c = tid; c < n_rec; c += 256) fail |= jt_map_bad(wk.top[(int64_t)set * n_rec + c]) ? 1 : 0;
    fail = __syncthreads_or(fail);
    if (fail) {
        for (int v = tid; v < n_vars; v += 256) row[v] = -1;
        return;
    }
    for (int d = 0; d < n_depths; ++d) {
        for (int c = depth_begin[d] + tid; c < depth_begin[d + 1]; c += 256) {
            const JtMap &rec = recs[c];
            uint32_t k = 0;
            for (int j = 0; j < rec.nK; ++j) k += (uint32_t)row[rec.v[j].col] * rec.v[j].radix;
            const uint32_t r = arg_set[rec.raw_off + k];
            for (int j = rec.nK; j < rec.nK + rec.nF; ++j) row[rec.v[j].col] = (int)((r / rec.v[j].radix) % (uint32_t)rec.v[j].card);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ max-propagation: the downward half
// jtp_max_marginals runs the upward pass above as it stands (the arg tables it writes are not used), then, shallowest depth first,
// one launch of jt_max_level per depth over the downward messages INTO that depth, and last one launch over all requests.  A
// record (JtMax) is a maximum over the entries of one clique c, onto K - the separator to a child d, or a request's variables -:
//     out[k] = max over r of ((double)psi_c[k, r] * in_1) * in_2 * ...,   in_i = ldexp(table_i[its digits], -ilogb(max table_i))
// the inputs in list order: D_c first (the clique's own downward table; the root has none), then the upward messages of the
// children of c in ascending clique number, without d's for the message to d.  A wave64 per (record, set, k, segment of r), the
// walker of jtp_query.h, evidence as in jt_map_collect_level; no arg, the maximum alone.  D_d is laid out as raw_d is, and its
// largest entry kept the same way (an integer maximum of bit patterns), so that the records below d read it as they read raw.
// The host adds up the exponents taken out (jtp_max_marginals below).
struct JtMaxWork {
    double *down;                    // [set * entries + raw_off of d + k]: rawdn_d
    double *part;                    // [set * parts + part_off + k * nseg + seg]
    double *out;                     // [set * req_entries + out_off + h]
    unsigned long long *dtop;        // [set * n_rec + ord of d]
    size_t bytes;                    // of the whole work area, jtp_map's first
};
static JtMaxWork max_work(char *base, size_t map_bytes, size_t sets, size_t entries, size_t parts, size_t req_entries, size_t n_rec) {
    JtMaxWork w;
    size_t at = (map_bytes + 7) & ~(size_t)7;
    auto take = [&](size_t n) { char *p = base + at; at += n; return p; };
    w.down = (double *)take(sets * entries * 8);
    w.part = (double *)take(sets * parts * 8);
    w.out = (double *)take(sets * req_entries * 8);
    w.dtop = (unsigned long long *)take(sets * n_rec * 8);
    w.bytes = at;
    return w;
}

// lane 0 of a wave: the entry of the record's output, and the running maximum of a downward table
__device__ __forceinline__ void jt_max_store(const JtMax &rec, const JtMaxWork &mw, int set, uint32_t k, double best, int n_rec, int64_t entries, int64_t req_entries) {
    if (!(best >= 0.0)) best = 0.0;                      // (nothing looked at: k contradicts the evidence)
    best = fabs(best);                                   // (-0.0: its bit pattern would be the largest of all)
    if (rec.ord < 0) {
        mw.out[(int64_t)set * req_entries + rec.out_off + k] = best;
        return;
    }
    mw.down[(int64_t)set * entries + rec.out_off + k] = best;
    unsigned long long *top = mw.dtop + (int64_t)set * n_rec + rec.ord;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(best);
    if (__atomic_load_n(top, __ATOMIC_RELAXED) < bits) atomicMax(top, bits);
}

template <typename T>
__global__ __launch_bounds__(256) void jt_max_level(const JtMax *__restrict__ recs, const JtMapChild *__restrict__ ins, JtMapWork wk, JtMaxWork mw,
                                                    int n_vars, int n_rec, int n_chunk, int64_t entries, int64_t parts, int64_t req_entries) {
    __shared__ int digs[JT_MAX_VARS][256];             // digit j of thread t's counter: a column per thread (K digits: the wave's, in every column)
    __shared__ JtSampleVar sv[JT_MAX_VARS];
    __shared__ int obs[4][JT_MAX_VARS];                // per wave: the observed state of v[j] in the wave's set, -1: none
    // the first JT_QUERY_KIDS inputs, staged as jt_map_collect_level stages a clique's children; `kdown`: the input is a down table
    __shared__ uint32_t kstride[JT_QUERY_KIDS][JT_MAX_VARS];
    __shared__ int64_t kraw[JT_QUERY_KIDS];
    __shared__ int kord[JT_QUERY_KIDS];
    __shared__ int kdown[JT_QUERY_KIDS];
    __shared__ uint32_t kbase[4][JT_QUERY_KIDS];
    __shared__ int kexp[4][JT_QUERY_KIDS];
    const JtMax &rec = recs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nK = rec.nK, nF = rec.nF, nv = nK + nF;
    jt_query_stage_vars(sv, rec.v, nv, tid);
    const int n_staged = jt_query_stage_kids(kstride, ins + rec.in_begin, rec.in_end - rec.in_begin, tid);
    if (tid < n_staged) kraw[tid] = ins[rec.in_begin + tid].raw_off, kord[tid] = ins[rec.in_begin + tid].ord, kdown[tid] = ins[rec.in_begin + tid].down;
    __syncthreads();
    const JtSampleVar *fv = sv + nK;
    const uint32_t R = rec.R, nk = rec.nk, nseg = rec.nseg;
    const uint32_t seg_len = (R + nseg - 1u) / nseg;
    const int64_t n_items = (int64_t)n_chunk * nk * nseg;
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < n_items; item += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const uint32_t seg = (uint32_t)(item % nseg), k = (uint32_t)((item / nseg) % nk);
        const int set = (int)(item / ((int64_t)nseg * nk));
        const int32_t *evr = wk.ev + (int64_t)set * n_vars;
        __builtin_amdgcn_wave_barrier();                // (the wave's row of `obs` is rewritten: its reads of the last item are done)
        if (lane < nv) obs[wave][lane] = evr[sv[lane].col];
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
        const T *tab = (const T *)wk.psi[set];
        const double *raw_set = wk.raw + (int64_t)set * entries, *down_set = mw.down + (int64_t)set * entries;
        const unsigned long long *top_set = wk.top + (int64_t)set * n_rec, *dtop_set = mw.dtop + (int64_t)set * n_rec;
        if (lane < n_staged) {                             // (the K digits are in every lane's column)
            kbase[wave][lane] = jt_query_kid_at(0u, kstride[lane], digs, tid, 0, nK);
            kexp[wave][lane] = jt_map_exp((kdown[lane] ? dtop_set : top_set)[kord[lane]]);
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t lo = min(seg * seg_len, R), end = min(lo + seg_len, R);
        const auto [a, e, B] = jt_query_cut(lo, end, 64u, (uint32_t)lane);
        double best = -1.0;                                // (nothing looked at yet: every w >= 0 beats it)
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
                    double w = (double)x;
                    for (int c = 0; c < n_staged; ++c) {
                        const uint32_t at = jt_query_kid_at(kbase[wave][c], kstride[c], digs, tid, nK, nv);
                        w *= ldexp((kdown[c] ? down_set : raw_set)[kraw[c] + at], -kexp[wave][c]);
                    }
                    for (int c = rec.in_begin + n_staged; c < rec.in_end; ++c) {      // (more inputs than are staged: list order still)
                        const JtMapChild &in = ins[c];
                        w *= ldexp((in.down ? down_set : raw_set)[in.raw_off + jt_query_kid_at(in, digs, tid, nv)], -jt_map_exp((in.down ? dtop_set : top_set)[in.ord]));
                    }
                    if (w > best) best = w;                // (a NaN is never taken)
                }
                if (++q == e) break;
                off = jt_query_walk_next(fv, nF, digs + nK, tid, off);
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const double ow = __shfl_xor(best, d, 64);
            if (ow > best) best = ow;
        }
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == 0) {
            if (any_bad) atomicOr(&wk.flag[set], 1);
            if (nseg > 1) mw.part[(int64_t)set * parts + rec.part_off + (int64_t)k * nseg + seg] = best;      // (-1 = the segment has no entry that counts)
            else jt_max_store(rec, mw, set, k, best, n_rec, entries, req_entries);
        }
    }
}

// records cut into segments: a wave per (record, set, k) takes the largest of the segments' results
__global__ __launch_bounds__(256) void jt_max_merge(const JtMax *__restrict__ recs, JtMaxWork mw, int n_rec, int n_chunk, int64_t entries, int64_t parts, int64_t req_entries) {
    const JtMax &rec = recs[blockIdx.y];
    const uint32_t nseg = rec.nseg, nk = rec.nk;
    if (nseg <= 1) return;
    const int lane = threadIdx.x & 63;
    const int64_t n_items = (int64_t)n_chunk * nk;
    for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const uint32_t k = (uint32_t)(item % nk);
        const int set = (int)(item / nk);
        const int64_t p0 = (int64_t)set * parts + rec.part_off + (int64_t)k * nseg;
        double best = -1.0;
        for (uint32_t s = (uint32_t)lane; s < nseg; s += 64u) {
            const double w = mw.part[p0 + s];
            if (w > best) best = w;
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const double ow = __shfl_xor(best, d, 64);
            if (ow > best) best = ow;
        }
        if (lane == 0) jt_max_store(rec, mw, set, k, best, n_rec, entries, req_entries);
    }
}

// ------------------------------------------------------------------------------------------ the M best assignments
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

// the records of the schedule, on the host
static void map_records(const HostPlan &hp, uint32_t seg, std::vector<JtMap> &recs, std::vector<JtMapChild> &kids, std::vector<int32_t> &depth_begin, MapMem &mm) {
    const size_t n = hp.sample.size();
    recs.assign(n, JtMap());
    std::vector<int> ord_of(hp.n_cliques, -1);
    for (size_t i = 0; i < n; ++i) ord_of[hp.sample[i].clique] = (int)i;
    mm.entries = mm.parts = 0;
    for (size_t i = 0; i < n; ++i) {
        const SampleClique &sc = hp.sample[i];
        JtMap &r = recs[i];
        memset(&r, 0, sizeof r);
        r.psi_off = hp.pack[sc.clique].dev_off;
        r.nK = (int32_t)sc.K.size();
        r.nF = (int32_t)sc.F.size();
        r.R = (uint32_t)sc.R;
        r.ord = (int32_t)i;
        uint32_t radix_k = 1, radix_f = 1;
        for (int j = r.nK + r.nF - 1; j >= 0; --j) {
            JtSampleVar &sv = r.v[j] = jt_query_var(hp, sc.clique, j < r.nK ? sc.K[j] : sc.F[j - r.nK]);
            if (j >= r.nK) sv.radix = radix_f, radix_f *= (uint32_t)sv.card;
            else sv.radix = radix_k, radix_k *= (uint32_t)sv.card;
        }
        r.nk = radix_k;
        // (a wave per k walks R entries, 64 lanes wide: from two segments' worth on, segments of `seg` entries or more - the root of a
        //  wide tree has one k)
        r.nseg = jt_query_nseg(r.R, seg);
        r.raw_off = mm.entries;
        mm.entries += r.nk;
        r.part_off = mm.parts;
        if (r.nseg > 1) mm.parts += (int64_t)r.nk * r.nseg;
    }
    // children: the cliques whose parent_clique is c, ascending clique number
    kids.clear();
    for (size_t i = 0; i < n; ++i) {
        JtMap &r = recs[i];
        r.child_begin = (int32_t)kids.size();
        for (int c = 0; c < hp.n_cliques; ++c) {
            if (hp.parent_clique[c] != hp.sample[i].clique) continue;
            const JtMap &ch = recs[ord_of[c]];
            JtMapChild kd;
            memset(&kd, 0, sizeof kd);
            kd.raw_off = ch.raw_off;
            kd.ord = ch.ord;
            for (int j = 0; j < r.nK + r.nF; ++j)
                for (int jj = 0; jj < ch.nK; ++jj)
                    if (ch.v[jj].col == r.v[j].col) kd.stride[j] = ch.v[jj].radix;
            kids.push_back(kd);
        }
        r.child_end = (int32_t)kids.size();
    }
    depth_begin.clear();
    mm.depth_items.clear();
    mm.depth_merge.clear();
    for (const std::vector<int> &level : hp.sample_depths) {     // (records of a depth are consecutive)
        depth_begin.push_back(level[0]);
        int64_t items = 1;
        char merge = 0;
        for (int i : level) items = std::max<int64_t>(items, (int64_t)recs[i].nk * recs[i].nseg), merge = merge || recs[i].nseg > 1;
        mm.depth_items.push_back(items);
        mm.depth_merge.push_back(merge);
    }
    depth_begin.push_back((int32_t)n);
}

// one record of jtp_max_marginals: the entries of `clique` maximised onto `out_vars` (in that order, C order), the upward message of
// the child whose record is `skip` left out (-1: none is); its inputs are appended to `ins`.  `recs` / `kids`: map_records'.
static JtMax max_record(const HostPlan &hp, const std::vector<JtMap> &recs, const std::vector<JtMapChild> &kids, const std::vector<int> &ord_of,
                        int clique, const int32_t *out_vars, int n_out, int skip, uint32_t seg, std::vector<JtMapChild> &ins) {
    const JtMap &cr = recs[ord_of[clique]];
    JtMax r;
    memset(&r, 0, sizeof r);
    r.psi_off = cr.psi_off;
    std::vector<int> vars(out_vars, out_vars + n_out);
    for (int v : hp.node_vars[clique])
        if (std::find(out_vars, out_vars + n_out, v) == out_vars + n_out) vars.push_back(v);
    r.nK = n_out;
    r.nF = (int32_t)vars.size() - n_out;
    uint32_t radix_k = 1, radix_f = 1;
    for (int j = r.nK + r.nF - 1; j >= 0; --j) {
        JtSampleVar &sv = r.v[j] = jt_query_var(hp, clique, vars[j]);
        if (j >= r.nK) sv.radix = radix_f, radix_f *= (uint32_t)sv.card;
        else sv.radix = radix_k, radix_k *= (uint32_t)sv.card;
    }
    r.nk = radix_k;
    r.R = radix_f;
    r.nseg = jt_query_nseg(r.R, seg);
    r.ord = -1;
    r.in_begin = (int32_t)ins.size();
    const int cn = cr.nK + cr.nF;
    auto place_in_clique = [&](int col) {                 // the variable's place in the clique's own record
        int jj = 0;
        while (cr.v[jj].col != col) ++jj;
        return jj;
    };
    if (hp.parent_clique[clique] >= 0) {                  // D_c, indexed as raw_c is
        JtMapChild in;
        memset(&in, 0, sizeof in);
        in.raw_off = cr.raw_off;
        in.ord = cr.ord;
        in.down = 1;
        for (int j = 0; j < cn; ++j) {
            const int jj = place_in_clique(r.v[j].col);
            if (jj < cr.nK) in.stride[j] = cr.v[jj].radix;
        }
        ins.push_back(in);
    }
    for (int c = cr.child_begin; c < cr.child_end; ++c) {
        if (kids[c].ord == skip) continue;
        JtMapChild in = kids[c];
        for (int j = 0; j < cn; ++j) in.stride[j] = kids[c].stride[place_in_clique(r.v[j].col)];
        ins.push_back(in);
    }
    r.in_end = (int32_t)ins.size();
    return r;
}

// the launches of jtp_map_best for lists of CAP elements
template <int CAP>
static void mbest_launch(const HostPlan &hp, const MapMem &up, const JtMbestWork &wk, int m, size_t n_kids, hipStream_t s) {
    const int n_vars = hp.n_vars, n_rec = (int)hp.sample.size(), n_depths = (int)hp.sample_depths.size();
    for (int d = n_depths - 1; d >= 0; --d) {
        const std::vector<int> &level = hp.sample_depths[d];
        jt_query_slices(level.size(), [&](size_t y0, size_t ny) {
            const int64_t waves = up.depth_items[d];
            const dim3 grid(jt_query_grid_x((waves + 3) / 4, ny), (unsigned)ny);
            const JtMap *recs = up.recs.get() + level[0] + y0;
            if (hp.dtype == JTP_F32) hipLaunchKernelGGL((jt_mbest_level<float, CAP>), grid, dim3(256), 0, s, recs, up.kids.get(), wk, n_vars);
            else hipLaunchKernelGGL((jt_mbest_level<double, CAP>), grid, dim3(256), 0, s, recs, up.kids.get(), wk, n_vars);
            if (up.depth_merge[d]) {
                const dim3 mgrid((unsigned)std::min<int64_t>((waves + 3) / 4, 1024), (unsigned)ny);
                hipLaunchKernelGGL(jt_mbest_merge<CAP>, mgrid, dim3(256), 0, s, recs, wk);
            }
        });
    }
    if (hp.dtype == JTP_F32)
        hipLaunchKernelGGL((jt_mbest_decode<float, CAP>), dim3((unsigned)m), dim3(256), 0, s, up.recs.get(), up.kids.get(), up.depth_begin.get(), n_depths, wk, n_vars, n_rec, (int)n_kids);
    else
        hipLaunchKernelGGL((jt_mbest_decode<double, CAP>), dim3((unsigned)m), dim3(256), 0, s, up.recs.get(), up.kids.get(), up.depth_begin.get(), n_depths, wk, n_vars, n_rec, (int)n_kids);
}

extern "C" {

int jtp_map(jtp_plan *pl, int32_t batch_begin, int32_t batch_end, int32_t *states, double *log_value) {
    int rc = check_ready(pl, batch_begin);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if (hp.multiset) return set_err(JTP_EUNSUPPORTED, "jtp_map: a multi-set plan runs eight evidence sets per pass of the propagate and nothing else: ask a plan made without JTP_MULTISET (JTP_SHARE_POTENTIALS shares the tables as well)");
    if (hp.n_ranks > 1) return set_err(JTP_EUNSUPPORTED, "jtp_map: the sweep over a plan shared by several ranks is not built: make the plan with n_ranks = 1");
    for (int c = 0; c < hp.n_cliques; ++c)
        if (hp.pn[c].unit) return set_err(JTP_EUNSUPPORTED, "jtp_map: clique %d keeps no table on the device: make the plan without `cover`", c);
    if (batch_end <= batch_begin || batch_end > hp.n_batch) return set_err(JTP_EINVAL, "bad batch range [%d,%d)", batch_begin, batch_end);
    if (!states) return set_err(JTP_EINVAL, "null argument");
    const size_t n_sets = (size_t)(batch_end - batch_begin), n_vars = (size_t)hp.n_vars, n_rec = hp.sample.size();
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_map");
    // (the potentials may have been written on any of the plan's streams; a propagate in flight only reads them, as this does)
    for (auto st : pl->streams) HIP_TRY(hipStreamSynchronize(st));
    hipStream_t s = pl->streams[0];
    // (first call, or more sets than the work area holds: everything is built into a local and moved into the plan once complete - a
    //  call that fails an allocation leaves the plan as it found it)
    MapMem fresh(&pl->mem);
    const bool first = !pl->map.recs;
    MapMem &lay = first ? fresh : pl->map;                // (whose sizes hold)
    if (first) {
        std::vector<JtMap> recs;
        std::vector<JtMapChild> kids;
        std::vector<int32_t> depth_begin;
        map_records(hp, (uint32_t)std::min<int64_t>(pl->map_seg > 0 ? pl->map_seg : JT_QUERY_SEG, 1 << 30), recs, kids, depth_begin, fresh);
        HIP_TRY(fresh.recs.upload(recs, 1));
        HIP_TRY(fresh.kids.upload(kids, 1));
        HIP_TRY(fresh.depth_begin.upload(depth_begin, 1));
    }
    const size_t entries = (size_t)lay.entries, parts = (size_t)lay.parts;
    // a chunk: as many sets as keep the raw and arg tables (12 bytes an entry) under 64 MiB
    size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / (12 * std::max<size_t>(entries + parts, 1)));
    chunk = std::min(std::min(chunk, n_sets), (size_t)65535);
    if (pl->map_chunk > 0) chunk = std::min(chunk, (size_t)pl->map_chunk);
    if ((size_t)pl->map.sets < chunk || first) {
        HIP_TRY(fresh.work.alloc(map_work(nullptr, chunk, entries, parts, n_rec, n_vars).bytes));
        fresh.sets = (int64_t)chunk;
    }
    if (first) pl->map = std::move(fresh);
    else if (fresh.work) pl->map.work = std::move(fresh.work), pl->map.sets = fresh.sets;
    MapMem &mm = pl->map;
    const JtMapWork wk = map_work(mm.work.get(), (size_t)mm.sets, entries, parts, n_rec, n_vars);
    const int n_depths = (int)hp.sample_depths.size();
    std::vector<const void *> psi(chunk);
    std::vector<int32_t> ev(chunk * n_vars, -1), flag(chunk);
    std::vector<unsigned long long> top(chunk * n_rec);
    const double ninf = -INFINITY;
    size_t n_failed = 0, first_failed = 0;
    for (size_t at = 0; at < n_sets; at += chunk) {
        const size_t cnt = std::min(chunk, n_sets - at);
        for (size_t i = 0; i < cnt; ++i) {
            const size_t b = (size_t)batch_begin + at + i;
            psi[i] = pl->bufs[b].psi;
            if (!pl->ev_obs.empty()) std::copy_n(pl->ev_obs.begin() + b * n_vars, n_vars, ev.begin() + i * n_vars);
        }
        HIP_TRY(hipMemcpyAsync(wk.psi, psi.data(), cnt * sizeof(void *), hipMemcpyHostToDevice, s));
        if (n_vars) HIP_TRY(hipMemcpyAsync(wk.ev, ev.data(), cnt * n_vars * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(wk.top, 0, cnt * n_rec * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(wk.flag, 0, cnt * sizeof(int32_t), s));
        if (n_vars) HIP_TRY(hipMemsetAsync(wk.states, 0, cnt * n_vars * sizeof(int32_t), s));      // (a variable of no clique stays 0)
        for (int d = n_depths - 1; d >= 0; --d) {
            const std::vector<int> &level = hp.sample_depths[d];
            jt_query_slices(level.size(), [&](size_t y0, size_t ny) {
                const int64_t waves = (int64_t)cnt * mm.depth_items[d];
                const dim3 grid(jt_query_grid_x((waves + 3) / 4, ny), (unsigned)ny);
                const JtMap *recs = mm.recs.get() + level[0] + y0;
                JT_QUERY_LAUNCH(hp.dtype, jt_map_collect_level, grid, s, recs, mm.kids.get(), wk, (int)n_vars, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)parts);
                if (mm.depth_merge[d]) {
                    const dim3 mgrid((unsigned)std::min<int64_t>((waves + 3) / 4, 1024), (unsigned)ny);
                    hipLaunchKernelGGL(jt_map_merge, mgrid, dim3(256), 0, s, recs, wk, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)parts);
                }
            });
        }
        hipLaunchKernelGGL(jt_map_decode, dim3((unsigned)cnt), dim3(256), 0, s, mm.recs.get(), mm.depth_begin.get(), n_depths, wk, (int)n_vars, (int)n_rec, (int64_t)entries);
        HIP_TRY(hipGetLastError());
        if (n_vars) HIP_TRY(hipMemcpyAsync(states + at * n_vars, wk.states, cnt * n_vars * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(top.data(), wk.top, cnt * n_rec * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(flag.data(), wk.flag, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                 // (the work area is the next chunk's)
        // log_value = log(raw_root) + ln 2 * (sum of the exponents taken out of the messages), summed here as scale_from_exps does
        for (size_t i = 0; i < cnt; ++i) {
            const unsigned long long *t = &top[i * n_rec];
            bool failed = flag[i] != 0;
            int64_t esum = 0;
            for (size_t c = 0; c < n_rec; ++c) {
                failed = failed || jt_map_bad(t[c]);
                if (c > 0) esum += jt_map_exp(t[c]);       // (record 0 is the root)
            }
            if (failed) {
                if (n_failed++ == 0) first_failed = (size_t)batch_begin + at + i;
                if (log_value) log_value[at + i] = ninf;
                continue;
            }
            double root;
            memcpy(&root, &t[0], sizeof root);
            if (log_value) log_value[at + i] = std::log(root) + 0.6931471805599453 * (double)esum;
        }
    }
    if (n_failed)
        return set_err(JTP_EINVAL, "jtp_map: %zu of %zu evidence sets have no assignment of positive finite value, the first set %zu (a negative or NaN entry, "
                                   "or a maximum that is zero or not finite: evidence of probability zero?); their states are -1, their log_value -inf",
                       n_failed, n_sets, first_failed);
    return JTP_OK;
}

int jtp_max_marginals(jtp_plan *pl, int32_t batch_begin, int32_t batch_end, int32_t n, const int32_t *cliques, const int32_t *var_off, const int32_t *var_ids,
                      const int64_t *out_off, int64_t set_stride, double *host, int64_t *log2_scale, double *log_value) {
    int rc = check_ready(pl, batch_begin);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if (hp.multiset) return set_err(JTP_EUNSUPPORTED, "jtp_max_marginals: a multi-set plan runs eight evidence sets per pass of the propagate and nothing else: ask a plan made without JTP_MULTISET (JTP_SHARE_POTENTIALS shares the tables as well)");
    if (hp.n_ranks > 1) return set_err(JTP_EUNSUPPORTED, "jtp_max_marginals: the sweep over a plan shared by several ranks is not built: make the plan with n_ranks = 1");
    for (int c = 0; c < hp.n_cliques; ++c)
        if (hp.pn[c].unit) return set_err(JTP_EUNSUPPORTED, "jtp_max_marginals: clique %d keeps no table on the device: make the plan without `cover`", c);
    if (batch_end <= batch_begin || batch_end > hp.n_batch) return set_err(JTP_EINVAL, "bad batch range [%d,%d)", batch_begin, batch_end);
    if (n < 0 || (n > 0 && (!cliques || !var_off || !out_off || !host || !log2_scale))) return set_err(JTP_EINVAL, "null argument");
    if (n > 0 && var_off[n] > var_off[0] && !var_ids) return set_err(JTP_EINVAL, "null argument");
    int64_t req_entries = 0;
    for (int i = 0; i < n; ++i) {
        const int c = cliques[i];
        if (c < 0 || c >= hp.n_cliques) return set_err(JTP_EINVAL, "node %d is not a clique", c);
        if (var_off[i + 1] < var_off[i] || var_off[i + 1] - var_off[i] > JT_MAX_VARS) return set_err(JTP_EINVAL, "bad variable list of request %d", i);
        int64_t ne = 1;
        for (int a = var_off[i]; a < var_off[i + 1]; ++a) {
            const int v = var_ids[a];
            if (std::find(hp.node_vars[c].begin(), hp.node_vars[c].end(), v) == hp.node_vars[c].end()) return set_err(JTP_EINVAL, "variable %d is not in clique %d", v, c);
            if (std::find(var_ids + var_off[i], var_ids + a, v) != var_ids + a) return set_err(JTP_EINVAL, "request %d: variable %d listed twice", i, v);
            ne *= hp.card[v];
        }
        req_entries += ne;
        if (out_off[i] < 0 || out_off[i] + ne > set_stride) return set_err(JTP_EINVAL, "request %d: entries [%lld,%lld) lie outside a set's %lld", i, (long long)out_off[i], (long long)(out_off[i] + ne), (long long)set_stride);
    }
    const size_t n_sets = (size_t)(batch_end - batch_begin), n_vars = (size_t)hp.n_vars, n_rec = hp.sample.size();
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_max_marginals");
    // (the potentials may have been written on any of the plan's streams; a propagate in flight only reads them, as this does)
    for (auto st : pl->streams) HIP_TRY(hipStreamSynchronize(st));
    hipStream_t s = pl->streams[0];
    // Whatever is missing - the upward records (jtp_map's, shared with it), the downward records, the records of this request list, a
    // larger work area - is built into locals and moved into the plan once all of it is there: a call that fails an allocation
    // leaves the plan as it found it.
    std::vector<int32_t> key;
    key.push_back(n);
    if (n > 0) {
        key.insert(key.end(), cliques, cliques + n);
        key.insert(key.end(), var_off, var_off + n + 1);
        key.insert(key.end(), var_ids + var_off[0], var_ids + var_off[n]);
    }
    MapMem fresh_map(&pl->mem);
    MaxMem fresh(&pl->mem);
    const bool need_map = !pl->map.recs, need_down = !pl->maxm.built, need_req = !pl->maxm.req || pl->maxm.key != key;
    const uint32_t seg = (uint32_t)std::min<int64_t>(pl->map_seg > 0 ? pl->map_seg : JT_QUERY_SEG, 1 << 30);
    if (need_map || need_down || need_req) {
        std::vector<JtMap> recs;
        std::vector<JtMapChild> kids, ins;
        std::vector<int32_t> depth_begin;
        map_records(hp, seg, recs, kids, depth_begin, fresh_map);
        std::vector<int> ord_of(hp.n_cliques, -1);
        for (size_t i = 0; i < n_rec; ++i) ord_of[hp.sample[i].clique] = (int)i;
        if (need_map) {
            HIP_TRY(fresh_map.recs.upload(recs, 1));
            HIP_TRY(fresh_map.kids.upload(kids, 1));
            HIP_TRY(fresh_map.depth_begin.upload(depth_begin, 1));
        }
        if (need_down) {                                   // the message into record i >= 1 is downward record i - 1
            std::vector<JtMax> down;
            for (size_t i = 1; i < n_rec; ++i) {
                const SampleClique &sc = hp.sample[i];
                JtMax r = max_record(hp, recs, kids, ord_of, hp.parent_clique[sc.clique], sc.K.data(), (int)sc.K.size(), (int)i, seg, ins);
                r.ord = (int32_t)i;
                r.out_off = recs[i].raw_off;
                r.part_off = fresh.down_parts;
                if (r.nseg > 1) fresh.down_parts += (int64_t)r.nk * r.nseg;
                down.push_back(r);
            }
            for (size_t d = 1; d < hp.sample_depths.size(); ++d) {
                int64_t items = 1;
                char merge = 0;
                for (int i : hp.sample_depths[d]) items = std::max<int64_t>(items, (int64_t)down[i - 1].nk * down[i - 1].nseg), merge = merge || down[i - 1].nseg > 1;
                fresh.depth_items.push_back(items);
                fresh.depth_merge.push_back(merge);
            }
            HIP_TRY(fresh.down.upload(down, 1));
            HIP_TRY(fresh.down_in.upload(ins, 1));
            ins.clear();
        }
        if (need_req) {
            std::vector<JtMax> req;
            fresh.req_out.assign(1, 0);
            for (int i = 0; i < n; ++i) {
                JtMax r = max_record(hp, recs, kids, ord_of, cliques[i], var_ids + var_off[i], var_off[i + 1] - var_off[i], -1, seg, ins);
                r.out_off = fresh.req_out.back();
                r.part_off = fresh.req_parts;              // (behind the downward records': added below)
                if (r.nseg > 1) fresh.req_parts += (int64_t)r.nk * r.nseg, fresh.req_merge = 1;
                fresh.req_items = std::max<int64_t>(fresh.req_items, (int64_t)r.nk * r.nseg);
                fresh.req_out.push_back(r.out_off + r.nk);
                req.push_back(r);
            }
            const int64_t down_parts = need_down ? fresh.down_parts : pl->maxm.down_parts;
            for (JtMax &r : req) r.part_off += down_parts;
            HIP_TRY(fresh.req.upload(req, 1));
            HIP_TRY(fresh.req_in.upload(ins, 1));
        }
    }
    const MapMem &lay = need_map ? fresh_map : pl->map;    // (whose sizes hold)
    const size_t entries = (size_t)lay.entries, parts = (size_t)lay.parts;
    const size_t dparts = (size_t)((need_down ? fresh.down_parts : pl->maxm.down_parts) + (need_req ? fresh.req_parts : pl->maxm.req_parts));
    auto work_bytes = [&](size_t sets) { return max_work(nullptr, map_work(nullptr, sets, entries, parts, n_rec, n_vars).bytes, sets, entries, dparts, (size_t)req_entries, n_rec).bytes; };
    // a chunk: as many sets as keep the work area under 64 MiB
    size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / std::max<size_t>(work_bytes(1), 1));
    chunk = std::min(std::min(chunk, n_sets), (size_t)65535);
    if (pl->map_chunk > 0) chunk = std::min(chunk, (size_t)pl->map_chunk);
    if (pl->maxm.work.size() < work_bytes(chunk)) HIP_TRY(fresh.work.alloc(work_bytes(chunk)));
    // (nothing fails from here on that would leave the plan half changed)
    if (need_map) pl->map = std::move(fresh_map);          // (no work area, room for no set: jtp_map allocates its own at its next call)
    MaxMem &mm = pl->maxm;
    if (need_down) mm.down = std::move(fresh.down), mm.down_in = std::move(fresh.down_in), mm.down_parts = fresh.down_parts, mm.depth_items = fresh.depth_items,
                   mm.depth_merge = fresh.depth_merge, mm.built = true;
    if (need_req) mm.req = std::move(fresh.req), mm.req_in = std::move(fresh.req_in), mm.req_parts = fresh.req_parts, mm.req_items = fresh.req_items,
                  mm.req_merge = fresh.req_merge, mm.req_out = fresh.req_out, mm.key = key;
    if (fresh.work) mm.work = std::move(fresh.work);
    const MapMem &up = pl->map;
    const JtMapWork wk = map_work(mm.work.get(), chunk, entries, parts, n_rec, n_vars);
    const JtMaxWork mw = max_work(mm.work.get(), wk.bytes, chunk, entries, dparts, (size_t)req_entries, n_rec);
    const int n_depths = (int)hp.sample_depths.size();
    std::vector<const void *> psi(chunk);
    std::vector<int32_t> ev(chunk * n_vars, -1), flag(chunk);
    std::vector<unsigned long long> top(chunk * n_rec), dtop(chunk * n_rec);
    std::vector<double> out(chunk * (size_t)req_entries);
    std::vector<int64_t> U(n_rec), V(n_rec), S(n_rec);
    std::vector<int> parent(n_rec, -1), req_ord((size_t)n);
    {
        std::vector<int> ord_of(hp.n_cliques, -1);
        for (size_t i = 0; i < n_rec; ++i) ord_of[hp.sample[i].clique] = (int)i;
        for (size_t i = 1; i < n_rec; ++i) parent[i] = ord_of[hp.parent_clique[hp.sample[i].clique]];
        for (int q = 0; q < n; ++q) req_ord[q] = ord_of[cliques[q]];
    }
    const double ninf = -INFINITY;
    size_t n_failed = 0, first_failed = 0;
    for (size_t at = 0; at < n_sets; at += chunk) {
        const size_t cnt = std::min(chunk, n_sets - at);
        for (size_t i = 0; i < cnt; ++i) {
            const size_t b = (size_t)batch_begin + at + i;
            psi[i] = pl->bufs[b].psi;
            if (!pl->ev_obs.empty()) std::copy_n(pl->ev_obs.begin() + b * n_vars, n_vars, ev.begin() + i * n_vars);
        }
        HIP_TRY(hipMemcpyAsync(wk.psi, psi.data(), cnt * sizeof(void *), hipMemcpyHostToDevice, s));
        if (n_vars) HIP_TRY(hipMemcpyAsync(wk.ev, ev.data(), cnt * n_vars * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(wk.top, 0, cnt * n_rec * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(mw.dtop, 0, cnt * n_rec * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(wk.flag, 0, cnt * sizeof(int32_t), s));
        for (int d = n_depths - 1; d >= 0; --d) {          // upward: jtp_map's launches
            const std::vector<int> &level = hp.sample_depths[d];
            jt_query_slices(level.size(), [&](size_t y0, size_t ny) {
                const int64_t waves = (int64_t)cnt * up.depth_items[d];
                const dim3 grid(jt_query_grid_x((waves + 3) / 4, ny), (unsigned)ny);
                const JtMap *recs = up.recs.get() + level[0] + y0;
                JT_QUERY_LAUNCH(hp.dtype, jt_map_collect_level, grid, s, recs, up.kids.get(), wk, (int)n_vars, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)parts);
                if (up.depth_merge[d]) {
                    const dim3 mgrid((unsigned)std::min<int64_t>((waves + 3) / 4, 1024), (unsigned)ny);
                    hipLaunchKernelGGL(jt_map_merge, mgrid, dim3(256), 0, s, recs, wk, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)parts);
                }
            });
        }
        // downward, then the requests: `count` records from `recs` on, each of at most `items` (entry, segment) pairs a set
        auto launch = [&](const JtMax *recs, const JtMapChild *ins, size_t count, int64_t items, bool merge) {
            jt_query_slices(count, [&](size_t y0, size_t ny) {
                const int64_t waves = (int64_t)cnt * items;
                const dim3 grid(jt_query_grid_x((waves + 3) / 4, ny), (unsigned)ny);
                JT_QUERY_LAUNCH(hp.dtype, jt_max_level, grid, s, recs + y0, ins, wk, mw, (int)n_vars, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)dparts, req_entries);
                if (merge) {
                    const dim3 mgrid((unsigned)std::min<int64_t>((waves + 3) / 4, 1024), (unsigned)ny);
                    hipLaunchKernelGGL(jt_max_merge, mgrid, dim3(256), 0, s, recs + y0, mw, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)dparts, req_entries);
                }
            });
        };
        for (int d = 1; d < n_depths; ++d) {
            const std::vector<int> &level = hp.sample_depths[d];
            launch(mm.down.get() + level[0] - 1, mm.down_in.get(), level.size(), mm.depth_items[d - 1], mm.depth_merge[d - 1] != 0);
        }
        if (n > 0) launch(mm.req.get(), mm.req_in.get(), (size_t)n, mm.req_items, mm.req_merge != 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(top.data(), wk.top, cnt * n_rec * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(dtop.data(), mw.dtop, cnt * n_rec * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(flag.data(), wk.flag, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (req_entries) HIP_TRY(hipMemcpyAsync(out.data(), mw.out, cnt * (size_t)req_entries * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                 // (the work area is the next chunk's)
        for (size_t i = 0; i < cnt; ++i) {
            const unsigned long long *t = &top[i * n_rec], *dt = &dtop[i * n_rec];
            double *dst = host + (int64_t)(at + i) * set_stride;
            int64_t *sc = log2_scale + (at + i) * (size_t)n;
            bool failed = flag[i] != 0;
            int64_t esum = 0;
            for (size_t c = 0; c < n_rec; ++c) {
                failed = failed || jt_map_bad(t[c]) || (c > 0 && jt_map_bad(dt[c]));
                if (c > 0) esum += jt_map_exp(t[c]);       // (record 0 is the root)
            }
            if (failed) {
                if (n_failed++ == 0) first_failed = (size_t)batch_begin + at + i;
                if (log_value) log_value[at + i] = ninf;
                for (int q = 0; q < n; ++q) {
                    std::fill_n(dst + out_off[q], mm.req_out[q + 1] - mm.req_out[q], 0.0);
                    sc[q] = 0;
                }
                continue;
            }
            // U_d: what the upward messages below and at d took out; V_d: the same of D_d; S_c: of a request on c
            std::fill(S.begin(), S.end(), 0);
            for (size_t c = n_rec; c-- > 1;) {             // (a record's children come after it: S[c] = sum of U over the children of c, for now)
                U[c] = jt_map_exp(t[c]) + S[c];
                S[parent[c]] += U[c];
            }
            V[0] = 0;
            for (size_t c = 1; c < n_rec; ++c) V[c] = V[parent[c]] + (S[parent[c]] - U[c]) + jt_map_exp(dt[c]);
            for (size_t c = 0; c < n_rec; ++c) S[c] += V[c];
            for (int q = 0; q < n; ++q) {
                std::copy_n(&out[i * (size_t)req_entries + mm.req_out[q]], mm.req_out[q + 1] - mm.req_out[q], dst + out_off[q]);
                sc[q] = S[req_ord[q]];
            }
            double root;
            memcpy(&root, &t[0], sizeof root);
            if (log_value) log_value[at + i] = std::log(root) + 0.6931471805599453 * (double)esum;
        }
    }
    if (n_failed)
        return set_err(JTP_EINVAL, "jtp_max_marginals: %zu of %zu evidence sets have no assignment of positive finite value, the first set %zu (a negative or NaN entry, "
                                   "or a maximum that is zero or not finite: evidence of probability zero?); their tables and exponents are 0, their log_value -inf",
                       n_failed, n_sets, first_failed);
    return JTP_OK;
}

int jtp_map_best(jtp_plan *pl, int32_t batch, int32_t m, int32_t *states, double *log_value, int32_t *n_found) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if (hp.multiset) return set_err(JTP_EUNSUPPORTED, "jtp_map_best: a multi-set plan runs eight evidence sets per pass of the propagate and nothing else: ask a plan made without JTP_MULTISET (JTP_SHARE_POTENTIALS shares the tables as well)");
    if (hp.n_ranks > 1) return set_err(JTP_EUNSUPPORTED, "jtp_map_best: the sweep over a plan shared by several ranks is not built: make the plan with n_ranks = 1");
    for (int c = 0; c < hp.n_cliques; ++c)
        if (hp.pn[c].unit) return set_err(JTP_EUNSUPPORTED, "jtp_map_best: clique %d keeps no table on the device: make the plan without `cover`", c);
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
    if (need_map) {
        std::vector<JtMap> recs;
        std::vector<JtMapChild> kids;
        std::vector<int32_t> depth_begin;
        map_records(hp, (uint32_t)std::min<int64_t>(pl->map_seg > 0 ? pl->map_seg : JT_QUERY_SEG, 1 << 30), recs, kids, depth_begin, fresh_map);
        HIP_TRY(fresh_map.recs.upload(recs, 1));
        HIP_TRY(fresh_map.kids.upload(kids, 1));
        HIP_TRY(fresh_map.depth_begin.upload(depth_begin, 1));
    }
    const MapMem &lay = need_map ? fresh_map : pl->map;    // (whose sizes hold)
    const size_t entries = (size_t)lay.entries, parts = (size_t)lay.parts, n_kids = lay.kids.size();
    const size_t need = mbest_work(nullptr, cap, (size_t)m, entries, parts, n_rec, n_kids, n_vars).bytes;
    if (pl->mbest.work.size() < need) HIP_TRY(fresh.work.alloc(need));
    if (need_map) pl->map = std::move(fresh_map);          // (no work area, room for no set: jtp_map allocates its own at its next call)
    if (fresh.work) pl->mbest.work = std::move(fresh.work);
    const JtMbestWork wk = mbest_work(pl->mbest.work.get(), cap, (size_t)m, entries, parts, n_rec, n_kids, n_vars);
    const void *psi = pl->bufs[batch].psi;
    std::vector<int32_t> ev(n_vars, -1);
    if (!pl->ev_obs.empty()) std::copy_n(pl->ev_obs.begin() + (size_t)batch * n_vars, n_vars, ev.begin());
    HIP_TRY(hipMemcpyAsync(wk.psi, &psi, sizeof(void *), hipMemcpyHostToDevice, s));
    if (n_vars) HIP_TRY(hipMemcpyAsync(wk.ev, ev.data(), n_vars * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(wk.top, 0, n_rec * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(wk.flag, 0, sizeof(int32_t), s));
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
    // log_value[s] = log(raw_root[0][s]) + ln 2 * (sum of the exponents taken out of the messages), as jtp_map sums it
    bool failed = flag != 0;
    int64_t esum = 0;
    for (size_t c = 0; c < n_rec; ++c) {
        failed = failed || jt_map_bad(top[c]);
        if (c > 0) esum += jt_map_exp(top[c]);                 // (record 0 is the root)
    }
    *n_found = 0;
    for (int i = 0; i < m; ++i) {
        if (!failed && root[i] > 0.0) {
            log_value[i] = std::log(root[i]) + 0.6931471805599453 * (double)esum;
            ++*n_found;
        } else
            log_value[i] = -INFINITY;
    }
    if (failed)
        return set_err(JTP_EINVAL, "jtp_map_best: evidence set %d has no assignment of positive finite value (a negative or NaN entry, "
                                   "or a maximum that is zero or not finite: evidence of probability zero?); its states are -1, its log_value -inf", batch);
    return JTP_OK;
}

}  // extern "C"
