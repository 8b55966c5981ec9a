// The most probable joint assignment on the device (jtp_map: an upward sweep over the clique potentials and a decode), and the host
// steps the three max-product units share (jtp_maxprod.h and jtp_sweep.h declare them; jtp_max.hip and jtp_mbest.hip are the other two;
// jtp_mmap.hip takes those of jtp_sweep.h).
#include "jtp_maxprod.h"

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

// (jt_map_wave_best, the wave's (largest w, smallest r among equals), and jt_map_store, what lane 0 writes: jtp_sweep.h)

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

// ------------------------------------------------------------------------------------------ host: the shared steps

std::vector<int> map_ord_of(const HostPlan &hp) {
    std::vector<int> ord_of(hp.n_cliques, -1);
    for (size_t i = 0; i < hp.sample.size(); ++i) ord_of[hp.sample[i].clique] = (int)i;
    return ord_of;
}

// the records of the schedule, on the host; the sizes they give (entries, segment results, items per depth) into `mm`
static void map_records(const HostPlan &hp, uint32_t seg, std::vector<JtMap> &recs, std::vector<JtMapChild> &kids, std::vector<int32_t> &depth_begin, MapMem &mm) {
    const size_t n = hp.sample.size();
    recs.assign(n, JtMap());
    const std::vector<int> ord_of = map_ord_of(hp);
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

int maxprod_refuse(const char *fn, const HostPlan &hp, int32_t batch_begin, int32_t batch_end) {
    if (hp.multiset) return set_err(JTP_EUNSUPPORTED, "%s: a multi-set plan runs eight evidence sets per pass of the propagate and nothing else: ask a plan made without JTP_MULTISET (JTP_SHARE_POTENTIALS shares the tables as well)", fn);
    if (hp.n_ranks > 1) return set_err(JTP_EUNSUPPORTED, "%s: the sweep over a plan shared by several ranks is not built: make the plan with n_ranks = 1", fn);
    for (int c = 0; c < hp.n_cliques; ++c)
        if (hp.pn[c].unit) return set_err(JTP_EUNSUPPORTED, "%s: clique %d keeps no table on the device: make the plan without `cover`", fn, c);
    if (batch_end <= batch_begin || batch_end > hp.n_batch) return set_err(JTP_EINVAL, "bad batch range [%d,%d)", batch_begin, batch_end);
    return JTP_OK;
}

uint32_t maxprod_seg(const jtp_plan *pl) { return (uint32_t)std::min<int64_t>(pl->map_seg > 0 ? pl->map_seg : JT_QUERY_SEG, 1 << 30); }

int map_upward_records(jtp_plan *pl, MapMem &fresh, std::vector<JtMap> *recs, std::vector<JtMapChild> *kids) {
    const bool need = !pl->map.recs;
    if (!need && !recs) return JTP_OK;
    std::vector<JtMap> my_recs;
    std::vector<JtMapChild> my_kids;
    std::vector<int32_t> depth_begin;
    if (!recs) recs = &my_recs, kids = &my_kids;
    map_records(pl->hp, maxprod_seg(pl), *recs, *kids, depth_begin, fresh);
    if (need) {
        HIP_TRY(fresh.recs.upload(*recs, 1));
        HIP_TRY(fresh.kids.upload(*kids, 1));
        HIP_TRY(fresh.depth_begin.upload(depth_begin, 1));
    }
    return JTP_OK;
}

int maxprod_stage_sets(jtp_plan *pl, size_t first, size_t cnt, std::vector<const void *> &psi, std::vector<int32_t> &ev, const void **d_psi, int32_t *d_ev,
                       unsigned long long *d_top, int32_t *d_flag, hipStream_t s) {
    const size_t n_vars = (size_t)pl->hp.n_vars, n_rec = pl->hp.sample.size();
    for (size_t i = 0; i < cnt; ++i) {
        psi[i] = pl->bufs[first + i].psi;
        if (!pl->ev_obs.empty()) std::copy_n(pl->ev_obs.begin() + (first + i) * n_vars, n_vars, ev.begin() + i * n_vars);
    }
    HIP_TRY(hipMemcpyAsync(d_psi, psi.data(), cnt * sizeof(void *), hipMemcpyHostToDevice, s));
    if (n_vars) HIP_TRY(hipMemcpyAsync(d_ev, ev.data(), cnt * n_vars * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_top, 0, cnt * n_rec * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(d_flag, 0, cnt * sizeof(int32_t), s));
    return JTP_OK;
}

void map_upward_sweep(const HostPlan &hp, const MapMem &up, const JtMapWork &wk, size_t cnt, hipStream_t s) {
    const int n_vars = hp.n_vars, n_rec = (int)hp.sample.size();
    maxprod_upward(hp, up, cnt, [&](const JtMap *recs, dim3 grid, dim3 mgrid, bool merge) {
        map_collect_launch(hp.dtype, recs, up.kids.get(), wk, grid, n_vars, n_rec, (int)cnt, (int64_t)up.entries, (int64_t)up.parts, s);
        if (merge) map_merge_launch(recs, wk, mgrid, n_rec, (int)cnt, (int64_t)up.entries, (int64_t)up.parts, s);
    });
}

void map_collect_launch(int dtype, const JtMap *recs, const JtMapChild *kids, const JtMapWork &wk, dim3 grid, int n_vars, int n_rec, int cnt, int64_t entries, int64_t parts, hipStream_t s) {
    JT_QUERY_LAUNCH(dtype, jt_map_collect_level, grid, s, recs, kids, wk, n_vars, n_rec, cnt, entries, parts);
}

void map_merge_launch(const JtMap *recs, const JtMapWork &wk, dim3 mgrid, int n_rec, int cnt, int64_t entries, int64_t parts, hipStream_t s) {
    hipLaunchKernelGGL(jt_map_merge, mgrid, dim3(256), 0, s, recs, wk, n_rec, cnt, entries, parts);
}

void map_decode_launch(const JtMap *recs, const int32_t *depth_begin, int n_depths, const JtMapWork &wk, size_t cnt, int n_vars, int n_rec, int64_t entries, hipStream_t s) {
    hipLaunchKernelGGL(jt_map_decode, dim3((unsigned)cnt), dim3(256), 0, s, recs, depth_begin, n_depths, wk, n_vars, n_rec, entries);
}

MaxprodValue maxprod_value(const unsigned long long *top, size_t n_rec, bool flagged) {
    MaxprodValue val = {flagged, 0, -INFINITY};
    for (size_t c = 0; c < n_rec; ++c) {
        val.failed = val.failed || jt_map_bad(top[c]);
        if (c > 0) val.esum += jt_map_exp(top[c]);         // (record 0 is the root)
    }
    if (val.failed) return val;
    double root;
    memcpy(&root, &top[0], sizeof root);
    val.log_value = maxprod_log(root, val.esum);
    return val;
}

// ------------------------------------------------------------------------------------------ jtp_map

extern "C" int jtp_map(jtp_plan *pl, int32_t batch_begin, int32_t batch_end, int32_t *states, double *log_value) {
    int rc = check_ready(pl, batch_begin);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if ((rc = maxprod_refuse("jtp_map", hp, batch_begin, batch_end))) return rc;
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
    if ((rc = map_upward_records(pl, fresh))) return rc;
    MapMem &lay = first ? fresh : pl->map;                // (whose sizes hold)
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
    std::vector<const void *> psi(chunk);
    std::vector<int32_t> ev(chunk * n_vars, -1), flag(chunk);
    std::vector<unsigned long long> top(chunk * n_rec);
    size_t n_failed = 0, first_failed = 0;
    for (size_t at = 0; at < n_sets; at += chunk) {
        const size_t cnt = std::min(chunk, n_sets - at);
        if ((rc = maxprod_stage_sets(pl, (size_t)batch_begin + at, cnt, psi, ev, wk.psi, wk.ev, wk.top, wk.flag, s))) return rc;
        if (n_vars) HIP_TRY(hipMemsetAsync(wk.states, 0, cnt * n_vars * sizeof(int32_t), s));      // (a variable of no clique stays 0)
        map_upward_sweep(hp, mm, wk, cnt, s);
        map_decode_launch(mm.recs.get(), mm.depth_begin.get(), (int)hp.sample_depths.size(), wk, cnt, (int)n_vars, (int)n_rec, (int64_t)entries, s);
        HIP_TRY(hipGetLastError());
        if (n_vars) HIP_TRY(hipMemcpyAsync(states + at * n_vars, wk.states, cnt * n_vars * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(top.data(), wk.top, cnt * n_rec * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(flag.data(), wk.flag, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                 // (the work area is the next chunk's)
        for (size_t i = 0; i < cnt; ++i) {
            const MaxprodValue val = maxprod_value(&top[i * n_rec], n_rec, flag[i] != 0);
            if (val.failed && n_failed++ == 0) first_failed = (size_t)batch_begin + at + i;
            if (log_value) log_value[at + i] = val.log_value;
        }
    }
    if (n_failed)
        return set_err(JTP_EINVAL, "jtp_map: %zu of %zu evidence sets have no assignment of positive finite value, the first set %zu (a negative or NaN entry, "
                                   "or a maximum that is zero or not finite: evidence of probability zero?); their states are -1, their log_value -inf",
                       n_failed, n_sets, first_failed);
    return JTP_OK;
}
