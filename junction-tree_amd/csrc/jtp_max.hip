// Max-propagation on the device: jtp_max_marginals, the max-marginals of factors and variables.
#include "jtp_maxprod.h"

// jtp_max_marginals runs the upward sweep of jtp_map as it stands (jtp_map.hip; the arg tables it writes are not used), then,
// shallowest depth first, one launch of jt_max_level per depth over the downward messages INTO that depth, and last one launch over
// all requests.  A record (JtMax) is a maximum over the entries of one clique c, onto K - the separator to a child d, or a request's
// variables -:
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
    jt_maxprod_keep_top(mw.dtop + (int64_t)set * n_rec + rec.ord, best);
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

// one record of jtp_max_marginals: the entries of `clique` maximised onto `out_vars` (in that order, C order), the upward message of
// the child whose record is `skip` left out (-1: none is); its inputs are appended to `ins`.  `recs` / `kids`: the upward records.
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

extern "C" int jtp_max_marginals(jtp_plan *pl, int32_t batch_begin, int32_t batch_end, int32_t n, const int32_t *cliques, const int32_t *var_off, const int32_t *var_ids,
                                 const int64_t *out_off, int64_t set_stride, double *host, int64_t *log2_scale, double *log_value) {
    int rc = check_ready(pl, batch_begin);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if ((rc = maxprod_refuse("jtp_max_marginals", hp, batch_begin, batch_end))) return rc;
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
    const std::vector<int> ord_of = map_ord_of(hp);
    if (need_map || need_down || need_req) {
        const uint32_t seg = maxprod_seg(pl);
        std::vector<JtMap> recs;
        std::vector<JtMapChild> kids, ins;
        if ((rc = map_upward_records(pl, fresh_map, &recs, &kids))) return rc;
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
    for (size_t i = 1; i < n_rec; ++i) parent[i] = ord_of[hp.parent_clique[hp.sample[i].clique]];
    for (int q = 0; q < n; ++q) req_ord[q] = ord_of[cliques[q]];
    size_t n_failed = 0, first_failed = 0;
    for (size_t at = 0; at < n_sets; at += chunk) {
        const size_t cnt = std::min(chunk, n_sets - at);
        if ((rc = maxprod_stage_sets(pl, (size_t)batch_begin + at, cnt, psi, ev, wk.psi, wk.ev, wk.top, wk.flag, s))) return rc;
        HIP_TRY(hipMemsetAsync(mw.dtop, 0, cnt * n_rec * sizeof(unsigned long long), s));
        map_upward_sweep(hp, up, wk, cnt, s);
        // downward, then the requests: `count` records from `recs` on, each of at most `items` (entry, segment) pairs a set
        auto launch = [&](const JtMax *recs, const JtMapChild *ins, size_t count, int64_t items, bool merge) {
            maxprod_slices(count, (int64_t)cnt * items, [&](size_t y0, dim3 grid, dim3 mgrid) {
                JT_QUERY_LAUNCH(hp.dtype, jt_max_level, grid, s, recs + y0, ins, wk, mw, (int)n_vars, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)dparts, req_entries);
                if (merge) hipLaunchKernelGGL(jt_max_merge, mgrid, dim3(256), 0, s, recs + y0, mw, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)dparts, req_entries);
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
            MaxprodValue val = maxprod_value(t, n_rec, flag[i] != 0);
            for (size_t c = 1; c < n_rec; ++c) val.failed = val.failed || jt_map_bad(dt[c]);
            if (val.failed) {
                if (n_failed++ == 0) first_failed = (size_t)batch_begin + at + i;
                if (log_value) log_value[at + i] = -INFINITY;
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
            if (log_value) log_value[at + i] = val.log_value;
        }
    }
    if (n_failed)
        return set_err(JTP_EINVAL, "jtp_max_marginals: %zu of %zu evidence sets have no assignment of positive finite value, the first set %zu (a negative or NaN entry, "
                                   "or a maximum that is zero or not finite: evidence of probability zero?); their tables and exponents are 0, their log_value -inf",
                       n_failed, n_sets, first_failed);
    return JTP_OK;
}
