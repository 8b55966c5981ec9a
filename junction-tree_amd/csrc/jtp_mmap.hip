// Marginal MAP on the device (jtp_marginal_map): the most probable assignment of some variables, the others summed out.
#include "jtp_sweep.h"

// jtp_marginal_map works on the sampling schedule (HostPlan::sample: the caller's tree by depth, then clique number; K the variables a
// clique shares with its parent, F the others in host axis order) and on the potentials alone, as jtp_map does.  M is the query;
// F splits into FM = F n M and FS = F \ M, both in host axis order, Rm = prod card(FM), Rs = prod card(FS).  Upward, one depth at a
// time, deepest first, for every entry that agrees with the set's evidence
//     U_c[k, rm] = sum over rs of ((double)psi[k, rm, rs] * m_1) * m_2 * ...      m_d = ldexp(raw_d[k_d], -e_d), e_d = ilogb(max raw_d)
//     raw_c[k] = max over rm of U_c[k, rm],  arg_c[k] = the smallest rm that has it
// The records are jtp_map's (JtMap: v = K, FM, FS; nF and R those of FM) with a JtMmapExt beside each, and within a depth the
// cliques with Rs = 1 come first: they ARE records of jtp_map and go through its kernels as they stand (jt_map_collect_level,
// jt_map_merge), so a query of all variables is jtp_map launch for launch.  The others go through jt_mmap_level: `lanes` =
// min(64, Rs rounded up to a power of two) lanes share one (k, rm), each adds a contiguous block of rs in ascending order (the
// mixed-radix counter of jtp_query.h, its digits in LDS) and a fixed butterfly adds the lanes, as jtp_joint sums; a wave takes 64 /
// lanes values of rm at a time and keeps (largest U, smallest rm) as jtp_map keeps (w, r).  From Rs >= 2 JT_QUERY_SEG on the sum is
// cut into jt_query_nseg(Rs, JT_QUERY_SEG) segments, a wave each, whose sums jt_mmap_merge adds - lane l those of segments l, l + 64,
// ... in ascending order, then the butterfly - before it takes the maximum over rm.  What is added in which order depends on Rs
// alone; a maximum is exact, so neither the layout nor how rm was cut ("map_seg") nor the chunking changes a bit of the result.
// U is never stored: a (k, rm) lives in registers until the maximum has taken it, and the segment sums of a depth live in a
// scratch sized by the largest depth.  Downward it is jt_map_decode over these records: a clique without FM writes nothing.
// LDS of jt_mmap_level: jt_map_collect_level's to the byte (digs 32 KiB of 35 KiB) - four workgroups, sixteen waves a CU, as there.

// the sum over the `lanes` lanes (a power of two) that share an entry, in every one of them: jtp_joint's butterfly
__device__ __forceinline__ double jt_mmap_lanes_sum(double s, int lanes) {
    for (int d = lanes >> 1; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return s;
}

// cliques with Rs > 1.  Items of a wave: (set, k, segment of rm), or where the sum is cut (set, k, rm, segment of rs)
template <typename T>
__global__ __launch_bounds__(256) void jt_mmap_level(const JtMap *__restrict__ recs, const JtMmapExt *__restrict__ exts, const JtMapChild *__restrict__ kids, JtMapWork wk,
                                                     double *__restrict__ spart, int n_vars, int n_rec, int n_chunk, int64_t entries, int64_t parts, int64_t sparts) {
    __shared__ int digs[JT_MAX_VARS][256];             // digit j of thread t's counter: a column per thread (K digits: the wave's; FM digits: the group's)
    __shared__ JtSampleVar sv[JT_MAX_VARS];
    __shared__ int obs[4][JT_MAX_VARS];                // per wave: the observed state of v[j] in the wave's set, -1: none
    __shared__ uint32_t kstride[JT_QUERY_KIDS][JT_MAX_VARS];
    __shared__ int64_t kraw[JT_QUERY_KIDS];
    __shared__ int kord[JT_QUERY_KIDS];
    __shared__ uint32_t kbase[4][JT_QUERY_KIDS];
    __shared__ int kexp[4][JT_QUERY_KIDS];
    const JtMap &rec = recs[blockIdx.y];
    const JtMmapExt &ext = exts[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nK = rec.nK, nM = rec.nF, nfix = nK + nM, nv = nfix + ext.nS;
    jt_query_stage_vars(sv, rec.v, nv, tid);
    const int n_staged = jt_query_stage_kids(kstride, kids + rec.child_begin, rec.child_end - rec.child_begin, tid);
    if (tid < n_staged) kraw[tid] = kids[rec.child_begin + tid].raw_off, kord[tid] = kids[rec.child_begin + tid].ord;
    __syncthreads();
    const JtSampleVar *mv = sv + nK, *fv = sv + nfix;
    const int nS = ext.nS, lanes = ext.lanes, sub = lane & (lanes - 1), grp = lane / lanes;
    const uint32_t per = 64u / (uint32_t)lanes;
    const uint32_t Rm = rec.R, Rs = ext.Rs, nk = rec.nk, nseg = rec.nseg, sseg = ext.sseg;
    const uint32_t seg_len = (Rm + nseg - 1u) / nseg, sseg_len = (Rs + sseg - 1u) / sseg;
    const int64_t per_k = sseg > 1 ? (int64_t)Rm * sseg : (int64_t)nseg;
    const int64_t n_items = (int64_t)n_chunk * nk * per_k;
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < n_items; item += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const uint32_t part = (uint32_t)(item % per_k), k = (uint32_t)((item / per_k) % nk);
        const int set = (int)(item / (per_k * nk));
        const int32_t *evr = wk.ev + (int64_t)set * n_vars;
        __builtin_amdgcn_wave_barrier();                // (the wave's row of `obs` is rewritten: its reads of the last item are done)
        if (lane < nv) obs[wave][lane] = evr[sv[lane].col];
        __builtin_amdgcn_wave_barrier();
        bool dead = false;
        int64_t base = rec.psi_off;
        for (int j = 0; j < nK; ++j) {
            const int dg = (int)((k / sv[j].radix) % (uint32_t)sv[j].card), o = obs[wave][j];
            digs[j][tid] = dg;
            if (o >= 0 && o != dg) dead = true;
            base += jt_sample_at(sv[j], dg);
        }
        const T *tab = (const T *)wk.psi[set];
        const double *raw_set = wk.raw + (int64_t)set * entries;
        const unsigned long long *top_set = wk.top + (int64_t)set * n_rec;
        if (lane < n_staged) {                             // (the K digits are in every lane's column)
            kbase[wave][lane] = jt_query_kid_at(0u, kstride[lane], digs, tid, 0, nK);
            kexp[wave][lane] = jt_map_exp(top_set[kord[lane]]);
        }
        __builtin_amdgcn_wave_barrier();
        // the wave's rm [lo, end) and, of each, the rs [s_lo, s_end)
        uint32_t lo, end, s_lo = 0u, s_end = Rs;
        if (sseg > 1) {
            lo = part / sseg, end = lo + 1u;
            s_lo = min((part % sseg) * sseg_len, Rs), s_end = min(s_lo + sseg_len, Rs);
        } else
            lo = min(part * seg_len, Rm), end = min(lo + seg_len, Rm);
        double best = -1.0, last = -1.0;                   // (nothing looked at yet: every U >= 0 beats it)
        uint32_t best_r = 0xffffffffu;
        bool bad = false;
        for (uint32_t rm0 = lo; rm0 < end; rm0 += per) {   // (the same turns for every lane: the butterfly needs the whole group)
            const uint32_t rm = rm0 + (uint32_t)grp;
            bool looked = !dead && rm < end;
            uint32_t off_m = 0;
            if (looked) {
                for (int j = 0; j < nM; ++j) {
                    const int dg = (int)((rm / mv[j].radix) % (uint32_t)mv[j].card), o = obs[wave][nK + j];
                    digs[nK + j][tid] = dg;
                    off_m += jt_sample_at(mv[j], dg);
                    if (o >= 0 && o != dg) looked = false;
                }
            }
            const auto [a, e, B] = jt_query_cut(s_lo, s_end, (uint32_t)lanes, (uint32_t)sub);
            double sum = 0.0;
            if (looked && a < e) {
                uint32_t off = off_m;
                int contra = 0;                            // digits of FS that contradict the evidence
                for (int j = 0; j < nS; ++j) {
                    const int dg = (int)((a / fv[j].radix) % (uint32_t)fv[j].card), o = obs[wave][nfix + j];
                    digs[nfix + j][tid] = dg;
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
                        sum += w;                          // (ascending rs)
                    }
                    if (++q == e) break;
                    for (int j = nS - 1; j >= 0; --j) {     // the next assignment in C order
                        const JtSampleVar v = fv[j];
                        const int dg = digs[nfix + j][tid], o = obs[wave][nfix + j];
                        if (dg + 1 < v.card) {
                            off += jt_sample_at(v, dg + 1) - jt_sample_at(v, dg);
                            digs[nfix + j][tid] = dg + 1;
                            if (o >= 0) contra += (o != dg + 1 ? 1 : 0) - (o != dg ? 1 : 0);
                            break;
                        }
                        off -= jt_sample_at(v, dg);
                        digs[nfix + j][tid] = 0;
                        if (o >= 0) contra += (o != 0 ? 1 : 0) - (o != dg ? 1 : 0);
                    }
                }
            }
            sum = jt_mmap_lanes_sum(sum, lanes);
            if (looked) {
                last = sum;
                if (sum > best) best = sum, best_r = rm;   // (ascending rm within a group: the first of equals stays; a NaN is never taken)
            }
        }
        const bool any_bad = __ballot(bad) != 0ull;
        if (sseg > 1) {                                    // (jt_mmap_merge: -1 = this (k, rm) is not looked at)
            if (lane == 0) {
                if (any_bad) atomicOr(&wk.flag[set], 1);
                spart[(int64_t)set * sparts + ext.spart_off + (int64_t)k * per_k + part] = last;
            }
            continue;
        }
        jt_map_wave_best(best, best_r);
        if (lane == 0) {
            if (any_bad) atomicOr(&wk.flag[set], 1);
            if (nseg > 1) {                                // (jt_map_merge: -1 = the segment has no entry that counts)
                const int64_t p = (int64_t)set * parts + rec.part_off + (int64_t)k * nseg + part;
                wk.part_w[p] = best;
                wk.part_r[p] = best_r;
            } else
                jt_map_store(rec, wk, set, k, best, best_r, n_rec, entries);
        }
    }
}

// cliques whose sum is cut into segments: a wave per (clique, set, k, segment of rm) adds the segment sums of every rm in ascending
// order of the segments, then takes the maximum over its rm, the smallest rm among equals
__global__ __launch_bounds__(256) void jt_mmap_merge(const JtMap *__restrict__ recs, const JtMmapExt *__restrict__ exts, JtMapWork wk, const double *__restrict__ spart,
                                                     int n_rec, int n_chunk, int64_t entries, int64_t parts, int64_t sparts) {
    const JtMap &rec = recs[blockIdx.y];
    const JtMmapExt &ext = exts[blockIdx.y];
    const uint32_t sseg = ext.sseg, nseg = rec.nseg, nk = rec.nk, Rm = rec.R;
    if (sseg <= 1) return;
    const int lane = threadIdx.x & 63;
    const uint32_t seg_len = (Rm + nseg - 1u) / nseg;
    const int64_t n_items = (int64_t)n_chunk * nk * nseg;
    for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const uint32_t seg = (uint32_t)(item % nseg), k = (uint32_t)((item / nseg) % nk);
        const int set = (int)(item / ((int64_t)nseg * nk));
        const uint32_t lo = min(seg * seg_len, Rm), end = min(lo + seg_len, Rm);
        double best = -1.0;
        uint32_t best_r = 0xffffffffu;
        for (uint32_t rm = lo; rm < end; ++rm) {
            const double *part = spart + (int64_t)set * sparts + ext.spart_off + ((int64_t)k * Rm + rm) * sseg;
            if (part[0] < 0.0) continue;                   // (not looked at: every segment says so)
            double sum = 0.0;
            for (uint32_t sg = (uint32_t)lane; sg < sseg; sg += 64u) sum += part[sg];
            sum = jt_mmap_lanes_sum(sum, 64);
            if (sum > best) best = sum, best_r = rm;       // (every lane holds the same)
        }
        if (lane == 0) {
            if (nseg > 1) {
                const int64_t p = (int64_t)set * parts + rec.part_off + (int64_t)k * nseg + seg;
                wk.part_w[p] = best;
                wk.part_r[p] = best_r;
            } else
                jt_map_store(rec, wk, set, k, best, best_r, n_rec, entries);
        }
    }
}

// ------------------------------------------------------------------------------------------ host

// the records of a query (in_m[v]: v is maximised) and the sizes they give, into `mm`; JTP_OK, or the refusal of a tree that is not strong
static int mmap_records(const HostPlan &hp, uint32_t seg, const std::vector<char> &in_m, std::vector<JtMap> &recs, std::vector<JtMmapExt> &exts,
                        std::vector<JtMapChild> &kids, std::vector<int32_t> &depth_begin, MmapMem &mm) {
    const size_t n = hp.sample.size();
    // the invariant: a clique that maximises shares only maximised variables with its parent
    for (size_t i = 0; i < n; ++i) {
        const SampleClique &sc = hp.sample[i];
        const auto x = std::find_if(sc.F.begin(), sc.F.end(), [&](int v) { return in_m[v] != 0; });
        const auto y = std::find_if(sc.K.begin(), sc.K.end(), [&](int v) { return in_m[v] == 0; });
        if (x != sc.F.end() && y != sc.K.end())
            return set_err(JTP_EINVAL, "jtp_marginal_map: the tree is not strong for this query: clique %d maximises variable %d below variable %d, which is summed "
                                       "and shared with its parent clique %d", sc.clique, *x, *y, hp.parent_clique[sc.clique]);
    }
    // visit order with, inside a depth, the cliques that sum nothing first (a stable partition)
    std::vector<int> order;
    auto sums = [&](int i) { return std::any_of(hp.sample[i].F.begin(), hp.sample[i].F.end(), [&](int v) { return in_m[v] == 0 && hp.card[v] > 1; }); };
    mm.depths.clear();
    depth_begin.clear();
    for (const std::vector<int> &level : hp.sample_depths) {
        MmapMem::Depth d;
        depth_begin.push_back((int32_t)order.size());
        d.a0 = (int32_t)order.size();
        for (int i : level)
            if (!sums(i)) order.push_back(i);
        d.a1 = (int32_t)order.size();
        for (int i : level)
            if (sums(i)) order.push_back(i);
        d.b1 = (int32_t)order.size();
        mm.depths.push_back(d);
    }
    depth_begin.push_back((int32_t)n);
    std::vector<int> rec_of(hp.n_cliques, -1);
    for (size_t i = 0; i < n; ++i) rec_of[hp.sample[order[i]].clique] = (int)i;
    recs.assign(n, JtMap());
    exts.assign(n, JtMmapExt());
    mm.entries = mm.parts = mm.sparts = 0;
    for (size_t i = 0; i < n; ++i) {
        const SampleClique &sc = hp.sample[order[i]];
        JtMap &r = recs[i];
        JtMmapExt &x = exts[i];
        memset(&r, 0, sizeof r);
        memset(&x, 0, sizeof x);
        std::vector<int> vs = sc.K;
        for (int v : sc.F)
            if (in_m[v]) vs.push_back(v);
        r.nK = (int32_t)sc.K.size();
        r.nF = (int32_t)vs.size() - r.nK;
        for (int v : sc.F)
            if (!in_m[v]) vs.push_back(v);
        x.nS = (int32_t)vs.size() - r.nK - r.nF;
        r.psi_off = hp.pack[sc.clique].dev_off;
        r.ord = (int32_t)i;
        uint32_t radix_k = 1, radix_m = 1, radix_s = 1;
        for (int j = (int)vs.size() - 1; j >= 0; --j) {
            JtSampleVar &sv = r.v[j] = jt_query_var(hp, sc.clique, vs[j]);
            if (j >= r.nK + r.nF) sv.radix = radix_s, radix_s *= (uint32_t)sv.card;
            else if (j >= r.nK) sv.radix = radix_m, radix_m *= (uint32_t)sv.card;
            else sv.radix = radix_k, radix_k *= (uint32_t)sv.card;
        }
        r.nk = radix_k;
        r.R = radix_m;
        x.Rs = radix_s;
        // (a segment of rm is about `seg` entries of the table, as jtp_map's is: seg / Rs values of rm; a maximum does not depend on the cut)
        r.nseg = jt_query_nseg(r.R, std::max<uint32_t>(1u, seg / std::min(x.Rs, seg)));
        x.sseg = jt_query_nseg(x.Rs, JT_QUERY_SEG);          // (of Rs alone: no knob reaches the order of a sum)
        x.lanes = 1;
        while (x.lanes < 64 && (uint32_t)x.lanes < x.Rs) x.lanes <<= 1;
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
            if (hp.parent_clique[c] != hp.sample[order[i]].clique) continue;
            const JtMap &ch = recs[rec_of[c]];
            JtMapChild kd;
            memset(&kd, 0, sizeof kd);
            kd.raw_off = ch.raw_off;
            kd.ord = ch.ord;
            for (int j = 0; j < r.nK + r.nF + exts[i].nS; ++j)
                for (int jj = 0; jj < ch.nK; ++jj)
                    if (ch.v[jj].col == r.v[j].col) kd.stride[j] = ch.v[jj].radix;
            kids.push_back(kd);
        }
        r.child_end = (int32_t)kids.size();
    }
    // per depth: the most waves of a clique in each launch, and the segment sums (a scratch the depths use in turn)
    for (MmapMem::Depth &d : mm.depths) {
        int64_t sp = 0;
        for (int i = d.a0; i < d.b1; ++i) {
            const JtMap &r = recs[i];
            JtMmapExt &x = exts[i];
            const int64_t rm_items = (int64_t)r.nk * r.nseg;
            d.merge = d.merge || r.nseg > 1;
            if (i < d.a1) d.items_a = std::max(d.items_a, rm_items);
            else if (x.sseg > 1) {
                x.spart_off = sp;
                sp += (int64_t)r.nk * r.R * x.sseg;
                d.items_b = std::max(d.items_b, (int64_t)r.nk * r.R * x.sseg);
                d.items_s = std::max(d.items_s, rm_items);
            } else
                d.items_b = std::max(d.items_b, rm_items);
        }
        mm.sparts = std::max(mm.sparts, sp);
    }
    return JTP_OK;
}

extern "C" int jtp_marginal_map(jtp_plan *pl, int32_t batch_begin, int32_t batch_end, int32_t n_query, const int32_t *var_ids, int32_t *states, double *log_value) {
    int rc = check_ready(pl, batch_begin);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if ((rc = maxprod_refuse("jtp_marginal_map", hp, batch_begin, batch_end))) return rc;
    if (n_query < 0) return set_err(JTP_EINVAL, "n_query = %d", n_query);
    if (n_query > 0 && (!var_ids || !states)) return set_err(JTP_EINVAL, "null argument");
    std::vector<char> in_m((size_t)hp.n_vars, 0), held((size_t)hp.n_vars, 0);
    for (const SampleClique &sc : hp.sample)
        for (int v : sc.F) held[v] = 1;                    // (every variable of a clique is in the F of the shallowest clique that holds it)
    for (int i = 0; i < n_query; ++i) {
        const int v = var_ids[i];
        if (v < 0 || v >= hp.n_vars) return set_err(JTP_EINVAL, "jtp_marginal_map: variable %d out of range [0,%d)", v, hp.n_vars);
        if (in_m[v]) return set_err(JTP_EINVAL, "jtp_marginal_map: variable %d listed twice", v);
        in_m[v] = 1;
        if (!held[v])
            return set_err(JTP_EINVAL, "jtp_marginal_map: variable %d is in no clique", v);
    }
    const size_t n_sets = (size_t)(batch_end - batch_begin), n_vars = (size_t)hp.n_vars, n_rec = hp.sample.size(), nq = (size_t)n_query;
    // the records are those of the last query if this is the same set of variables under the same "map_seg"
    std::vector<int32_t> key(1, (int32_t)maxprod_seg(pl));
    key.insert(key.end(), var_ids, var_ids + n_query);
    std::sort(key.begin() + 1, key.end());
    // (whatever is missing is built into a local and moved into the plan once complete - a call that fails an allocation leaves the
    //  plan as it found it; a tree that is not strong is refused before anything touches the device)
    MmapMem fresh(&pl->mem);
    const bool need = !pl->mmap.recs || pl->mmap.key != key;
    std::vector<JtMap> recs;
    std::vector<JtMmapExt> exts;
    std::vector<JtMapChild> kids;
    std::vector<int32_t> depth_begin;
    if (need && (rc = mmap_records(hp, maxprod_seg(pl), in_m, recs, exts, kids, depth_begin, fresh))) return rc;
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_marginal_map");
    // (the potentials may have been written on any of the plan's streams; a propagate in flight only reads them, as this does)
    for (auto st : pl->streams) HIP_TRY(hipStreamSynchronize(st));
    hipStream_t s = pl->streams[0];
    if (need) {
        HIP_TRY(fresh.recs.upload(recs, 1));
        HIP_TRY(fresh.ext.upload(exts, 1));
        HIP_TRY(fresh.kids.upload(kids, 1));
        HIP_TRY(fresh.depth_begin.upload(depth_begin, 1));
    }
    const MmapMem &lay = need ? fresh : pl->mmap;          // (whose sizes hold)
    const size_t entries = (size_t)lay.entries, parts = (size_t)lay.parts, sparts = (size_t)lay.sparts;
    // a chunk: as many sets as keep the raw and arg tables (12 bytes an entry) and the segment sums under 64 MiB
    size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / std::max<size_t>(12 * (entries + parts) + 8 * sparts, 12));
    chunk = std::min(std::min(chunk, n_sets), (size_t)65535);
    if (pl->map_chunk > 0) chunk = std::min(chunk, (size_t)pl->map_chunk);
    auto sums_at = [&](size_t sets) { return (map_work(nullptr, sets, entries, parts, n_rec, n_vars).bytes + 7) & ~(size_t)7; };
    const size_t work_bytes = sums_at(chunk) + chunk * sparts * 8;
    if (pl->mmap.work.size() < work_bytes) HIP_TRY(fresh.work.alloc(work_bytes));
    if (need) {
        DeviceBuf<char> old_work = std::move(pl->mmap.work);
        if (!fresh.work) fresh.work = std::move(old_work);
        fresh.key = key;
        pl->mmap = std::move(fresh);
    } else if (fresh.work)
        pl->mmap.work = std::move(fresh.work);
    const MmapMem &mm = pl->mmap;
    const JtMapWork wk = map_work(mm.work.get(), chunk, entries, parts, n_rec, n_vars);
    double *spart = (double *)(mm.work.get() + sums_at(chunk));
    std::vector<const void *> psi(chunk);
    std::vector<int32_t> ev(chunk * n_vars, -1), flag(chunk), rows(chunk * n_vars);
    std::vector<unsigned long long> top(chunk * n_rec);
    size_t n_failed = 0, first_failed = 0;
    for (size_t at = 0; at < n_sets; at += chunk) {
        const size_t cnt = std::min(chunk, n_sets - at);
        if ((rc = maxprod_stage_sets(pl, (size_t)batch_begin + at, cnt, psi, ev, wk.psi, wk.ev, wk.top, wk.flag, s))) return rc;
        if (n_vars) HIP_TRY(hipMemsetAsync(wk.states, 0, cnt * n_vars * sizeof(int32_t), s));
        for (size_t d = mm.depths.size(); d-- > 0;) {       // deepest first
            const MmapMem::Depth &dp = mm.depths[d];
            // (jtp_map's kernels over the cliques that sum nothing, as jtp_map launches them)
            maxprod_slices((size_t)(dp.a1 - dp.a0), (int64_t)cnt * dp.items_a, [&](size_t y0, dim3 grid, dim3) {
                map_collect_launch(hp.dtype, mm.recs.get() + dp.a0 + y0, mm.kids.get(), wk, grid, (int)n_vars, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)parts, s);
            });
            maxprod_slices((size_t)(dp.b1 - dp.a1), (int64_t)cnt * dp.items_b, [&](size_t y0, dim3 grid, dim3) {
                JT_QUERY_LAUNCH(hp.dtype, jt_mmap_level, grid, s, mm.recs.get() + dp.a1 + y0, mm.ext.get() + dp.a1 + y0, mm.kids.get(), wk, spart, (int)n_vars, (int)n_rec,
                                (int)cnt, (int64_t)entries, (int64_t)parts, (int64_t)sparts);
            });
            if (dp.items_s)
                maxprod_slices((size_t)(dp.b1 - dp.a1), (int64_t)cnt * dp.items_s, [&](size_t y0, dim3, dim3 mgrid) {
                    hipLaunchKernelGGL(jt_mmap_merge, mgrid, dim3(256), 0, s, mm.recs.get() + dp.a1 + y0, mm.ext.get() + dp.a1 + y0, wk, spart, (int)n_rec, (int)cnt,
                                       (int64_t)entries, (int64_t)parts, (int64_t)sparts);
                });
            if (dp.merge)
                maxprod_slices((size_t)(dp.b1 - dp.a0), (int64_t)cnt * std::max(dp.items_a, std::max(dp.items_b, dp.items_s)), [&](size_t y0, dim3, dim3 mgrid) {
                    map_merge_launch(mm.recs.get() + dp.a0 + y0, wk, mgrid, (int)n_rec, (int)cnt, (int64_t)entries, (int64_t)parts, s);
                });
        }
        map_decode_launch(mm.recs.get(), mm.depth_begin.get(), (int)mm.depths.size(), wk, cnt, (int)n_vars, (int)n_rec, (int64_t)entries, s);
        HIP_TRY(hipGetLastError());
        if (n_vars) HIP_TRY(hipMemcpyAsync(rows.data(), wk.states, cnt * n_vars * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(top.data(), wk.top, cnt * n_rec * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(flag.data(), wk.flag, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                 // (the work area is the next chunk's)
        for (size_t i = 0; i < cnt; ++i) {
            const MaxprodValue val = maxprod_value(&top[i * n_rec], n_rec, flag[i] != 0);
            if (val.failed && n_failed++ == 0) first_failed = (size_t)batch_begin + at + i;
            if (log_value) log_value[at + i] = val.log_value;
            for (size_t q = 0; q < nq; ++q) states[(at + i) * nq + q] = rows[i * n_vars + (size_t)var_ids[q]];
        }
    }
    if (n_failed)
        return set_err(JTP_EINVAL, "jtp_marginal_map: %zu of %zu evidence sets have no assignment of positive finite value, the first set %zu (a negative or NaN entry, "
                                   "or a maximum that is zero or not finite: evidence of probability zero?); their states are -1, their log_value -inf",
                       n_failed, n_sets, first_failed);
    return JTP_OK;
}
