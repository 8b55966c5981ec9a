// The joint distribution of a few variables that need not share a clique, from the beliefs a propagate left.
#include <cmath>

#include <algorithm>
#include <cstring>
#include <vector>

#include "jtp_engine.h"
#include "jtp_query.h"

// jtp_joint works on the sampling schedule (HostPlan::sample: the caller's tree by depth, then clique number; K the variables a clique
// shares with its parent, F the others in host axis order, R = prod card(F)) and on the belief tables alone.  The HOME of a query
// variable is the shallowest clique that holds it, the TOP the deepest clique whose subtree holds every home, and the ACTIVE
// cliques are those on the paths from the homes up to the top: nothing else is read.  For an active clique c, C_c = the query
// variables whose home lies in its subtree, in the order of the query, Q_c those whose home is c, F'_c = F_c without Q_c,
// R'_c = prod card(F'_c).  Upward, deepest first, for every active clique but the top, every assignment k of K_c and x of C_c:
//     sigma_c[k] = sum over r < R_c of beta_c[k, r]                                                     (jt_joint_sigma)
//     U_c[k, x]  = sum over r' < R'_c of ((double)beta_c[k, x|Q_c, r'] * M_d1[.]) * M_d2[.] ...         (jt_joint_level)
//     M_c[k, x]  = U_c[k, x] / sigma_c[k], 0 where sigma_c[k] = 0
// the active children d1 < d2 < ... in ascending clique number, float64, left to right, each read at the digits of K_d that
// (k, x, r') fix and at x restricted to C_d.  The top forms the same sum over ALL its variables outside Q_top (those it shares with
// its parent included, host axis order) and does not divide: C_top is the query, so what it writes is the result in the query's
// order.  M_c is P(C_c | K_c) - the power of two a scaled plan keeps per clique cancels in U / sigma - so the result is the top's
// belief marginalised: unnormalised, times 2^-E_top on a scaled plan.
// A sum of n terms is formed by min(64, n rounded up to a power of two) lanes: lane l adds the contiguous block [l B, (l + 1) B) of
// the index, B = ceil(n / lanes), entry by entry (a mixed-radix counter, its digits in LDS, moves the table offset), and a fixed
// tree of shuffles adds the lanes.  What is added in which order depends on n alone - not on the stored layout, of which nothing is
// known here but the offsets jt_sample_at gives - so equal beliefs give bit-equal joints whatever the plan's flags.  A sum of
// n >= 2 JT_QUERY_SEG terms (the root of a wide tree: 2^20 entries behind each of a handful of outputs) is cut into
// min(4096, n / JT_QUERY_SEG) contiguous segments - of n alone again - each summed as above by a wave of its own;
// jt_joint_merge adds the segments' sums, lane l those of segments l, l + 64, ... in ascending order, then the same tree.
// fail[0] counts the (clique, k) pairs that met a negative or NaN entry or whose sigma is not finite, fail[1] keeps the smallest
// visit-order place among them; fail[2] is set where the top met such an entry or a sum of it is not finite (one more pair).

#define JT_JOINT_CAP ((int64_t)64 << 20)      // bytes of the result, and of all sigma, M and segment sums of a call

// the sum over the `lanes` lanes (a power of two) that share an entry, in every one of them: log2(lanes) shuffle steps
__device__ __forceinline__ double jt_joint_lanes_sum(double s, int lanes) {
    for (int d = lanes >> 1; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return s;
}

// one launch over every active clique but the top: a wave64 per (clique, k)
template <typename T>
__global__ __launch_bounds__(256) void jt_joint_sigma(const JtJoint *__restrict__ recs, const T *__restrict__ bel, double *__restrict__ work,
                                                      unsigned long long *__restrict__ fail) {
    __shared__ int digs[JT_MAX_VARS][256];             // digit j of thread t's counter: a column per thread, no barrier needed
    __shared__ JtSampleVar kv[JT_MAX_VARS], fv[JT_MAX_VARS];
    const JtJoint &rec = recs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nK = rec.nK, nF = rec.nFs;
    jt_query_stage_vars(kv, rec.v, nK, tid);
    jt_query_stage_vars(fv, rec.f, nF, tid);
    __syncthreads();
    const uint32_t R = rec.R, nk = rec.nk;
    for (uint32_t k = blockIdx.x * 4u + (uint32_t)(tid >> 6); k < nk; k += gridDim.x * 4u) {      // (a whole wave)
        int64_t base = rec.bel_off;
        for (int j = 0; j < nK; ++j) base += jt_sample_at(kv[j], (int)((k / kv[j].radix) % (uint32_t)kv[j].card));
        const auto [a, e, B] = jt_query_cut(0u, R, 64u, (uint32_t)lane);
        double sum = 0.0;
        bool bad = false;
        if (a < e) {
            uint32_t off = jt_query_walk_start(fv, nF, digs, tid, a);
            for (uint32_t q = a;;) {
                const double w = (double)bel[base + off];
                bad = bad || !(w >= 0.0);
                sum += w;
                if (++q == e) break;
                off = jt_query_walk_next(fv, nF, digs, tid, off);
            }
        }
        sum = jt_joint_lanes_sum(sum, 64);
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == 0) {
            work[rec.sig_off + k] = sum;
            if (any_bad || !(sum < INFINITY)) {
                atomicAdd(&fail[0], 1ull);
                atomicMin(&fail[1], (unsigned long long)rec.ord);
            }
        }
    }
}

// a finished sum: the top's goes to the result as it is, every other clique's is divided by sigma; true where the top's is not finite
__device__ __forceinline__ bool jt_joint_store(const JtJoint &rec, double *work, int64_t entry, double sum) {
    if (rec.top) {
        work[rec.msg_off + entry] = sum;
        return !(sum < INFINITY);
    }
    const double sigma = work[rec.sig_off + entry / rec.X];
    work[rec.msg_off + entry] = sigma == 0.0 ? 0.0 : sum / sigma;
    return false;
}

// one launch per active depth, deepest first: `lanes` lanes per output entry (clique, k, x), 256 / lanes entries per workgroup and turn
template <typename T>
__global__ __launch_bounds__(256) void jt_joint_level(const JtJoint *__restrict__ recs, const JtJointChild *__restrict__ kids, const T *__restrict__ bel,
                                                      double *work, unsigned long long *__restrict__ fail) {
    __shared__ int digs[JT_MAX_VARS][256];             // digit of v[j] in thread t's entry: a column per thread
    __shared__ JtSampleVar sv[JT_MAX_VARS];
    __shared__ JtJointX xs[JT_JOINT_MAXQ];
    // the first JT_QUERY_KIDS active children: strides and place of the message, staged once; per thread and entry the part of the
    // message index that (k, x) fix
    __shared__ uint32_t kstride[JT_QUERY_KIDS][JT_MAX_VARS];
    __shared__ uint32_t kxstride[JT_QUERY_KIDS][JT_JOINT_MAXQ];
    __shared__ int64_t kmsg[JT_QUERY_KIDS];
    __shared__ uint32_t kbase[JT_QUERY_KIDS][256];
    const JtJoint &rec = recs[blockIdx.y];
    const int tid = threadIdx.x;
    const int nK = rec.nK, nQ = rec.nQ, nF = rec.nF, nX = rec.nX, nfix = nK + nQ, nv = nfix + nF;
    jt_query_stage_vars(sv, rec.v, nv, tid);
    for (int i = tid; i < nX * (int)(sizeof(JtJointX) / 4); i += 256) ((int32_t *)xs)[i] = ((const int32_t *)rec.x)[i];
    const int n_staged = jt_query_stage_kids(kstride, kids + rec.child_begin, rec.child_end - rec.child_begin, tid);
    for (int i = tid; i < n_staged * JT_JOINT_MAXQ; i += 256) kxstride[i / JT_JOINT_MAXQ][i % JT_JOINT_MAXQ] = kids[rec.child_begin + i / JT_JOINT_MAXQ].xstride[i % JT_JOINT_MAXQ];
    if (tid < n_staged) kmsg[tid] = kids[rec.child_begin + tid].msg_off;
    __syncthreads();
    const JtSampleVar *fv = sv + nfix;
    const int lanes = rec.lanes, sub = tid & (lanes - 1), per = 256 / lanes;
    const uint32_t Rp = rec.Rp, X = rec.X, nseg = rec.nseg;
    const uint32_t seg_len = (Rp + nseg - 1u) / nseg;
    const int64_t n_items = (int64_t)rec.nk * X * nseg;
    bool bad = false;
    for (int64_t first = (int64_t)blockIdx.x * per; first < n_items; first += (int64_t)gridDim.x * per) {     // (the whole workgroup)
        const int64_t item = first + tid / lanes;
        const bool live = item < n_items;
        const int64_t entry = live ? item / nseg : 0;
        const uint32_t seg = live ? (uint32_t)(item % nseg) : 0u;
        const uint32_t k = (uint32_t)(entry / X), x = (uint32_t)(entry % X);
        const uint32_t lo = min(seg * seg_len, Rp), end = live ? min(lo + seg_len, Rp) : lo;
        const auto [a, e, B] = jt_query_cut(lo, end, (uint32_t)lanes, (uint32_t)sub);
        double sum = 0.0;
        if (a < e) {
            int64_t base = rec.bel_off;
            for (int j = 0; j < nK; ++j) digs[j][tid] = (int)((k / sv[j].radix) % (uint32_t)sv[j].card);
            for (int i = 0; i < nX; ++i)
                if (xs[i].slot >= 0) digs[xs[i].slot][tid] = (int)((x / xs[i].radix) % (uint32_t)xs[i].card);
            for (int j = 0; j < nfix; ++j) base += jt_sample_at(sv[j], digs[j][tid]);
            for (int c = 0; c < n_staged; ++c) {
                uint32_t at = jt_query_kid_at(0u, kstride[c], digs, tid, 0, nfix);
                for (int i = 0; i < nX; ++i) at += ((x / xs[i].radix) % (uint32_t)xs[i].card) * kxstride[c][i];
                kbase[c][tid] = at;
            }
            uint32_t off = jt_query_walk_start(fv, nF, digs + nfix, tid, a);
            for (uint32_t q = a;;) {
                const T b = bel[base + off];
                bad = bad || !(b >= (T)0);
                double w = (double)b;
                for (int c = 0; c < n_staged; ++c) {
                    const uint32_t at = jt_query_kid_at(kbase[c][tid], kstride[c], digs, tid, nfix, nv);
                    w *= work[kmsg[c] + at];
                }
                for (int c = rec.child_begin + n_staged; c < rec.child_end; ++c) {      // (more children than are staged: ascending order still)
                    const JtJointChild &kid = kids[c];
                    uint32_t at = jt_query_kid_at(kid, digs, tid, nv);
                    for (int i = 0; i < nX; ++i) {
                        const uint32_t st = kid.xstride[i];
                        if (st) at += ((x / xs[i].radix) % (uint32_t)xs[i].card) * st;
                    }
                    w *= work[kid.msg_off + at];
                }
                sum += w;
                if (++q == e) break;
                off = jt_query_walk_next(fv, nF, digs + nfix, tid, off);
            }
        }
        sum = jt_joint_lanes_sum(sum, lanes);
        if (live && sub == 0) {
            if (nseg > 1) work[rec.part_off + item] = sum;     // (jt_joint_merge)
            else bad = jt_joint_store(rec, work, entry, sum) || bad;
        }
    }
    // (the other cliques' entries were all looked at by jt_joint_sigma)
    if (rec.top && __ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(&fail[2], 1ull);
}

// cliques cut into segments: a wave per output entry adds the segments' sums
__global__ __launch_bounds__(256) void jt_joint_merge(const JtJoint *__restrict__ recs, double *work, unsigned long long *__restrict__ fail) {
    const JtJoint &rec = recs[blockIdx.y];
    const uint32_t nseg = rec.nseg;
    if (nseg <= 1) return;
    const int lane = threadIdx.x & 63;
    const int64_t n_entries = (int64_t)rec.nk * rec.X;
    bool bad = false;
    for (int64_t entry = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); entry < n_entries; entry += (int64_t)gridDim.x * 4) {      // (a whole wave)
        const double *part = work + rec.part_off + entry * nseg;
        double sum = 0.0;
        for (uint32_t sg = (uint32_t)lane; sg < nseg; sg += 64u) sum += part[sg];
        sum = jt_joint_lanes_sum(sum, 64);
        if (lane == 0) bad = jt_joint_store(rec, work, entry, sum) || bad;
    }
    if (rec.top && __ballot(bad) != 0ull && lane == 0) atomicOr(&fail[2], 1ull);
}

namespace {

struct JointQuery {
    std::vector<JtJoint> recs;
    std::vector<JtJointChild> kids;
    std::vector<std::pair<int, int>> depth_range;    // per active depth, shallowest first: records [first, second)
    std::vector<int64_t> depth_items;                // ... and the most workgroup turns' worth of entries of a clique there
    std::vector<int64_t> depth_merge;                // ... and the most entries of a clique there that is cut into segments (0: none is)
    int64_t work_doubles = 0, result = 0;            // the work area (report, sigma, M, result), the result's entries
    int64_t result_off = 0;
    int top_clique = -1;
    uint32_t max_nk = 1;
};

}  // namespace

// the active set and its records (the work area's layout with them); JTP_OK, or the refusal
static int joint_records(const HostPlan &hp, int n_query, const int32_t *q, JointQuery &jq) {
    const int n = (int)hp.sample.size();
    std::vector<int> ord_of(hp.n_cliques, -1), home(n_query, -1);
    for (int i = 0; i < n; ++i) ord_of[hp.sample[i].clique] = i;
    for (int i = 0; i < n_query; ++i) {
        for (int s = 0; s < n && home[i] < 0; ++s)           // (visit order: the shallowest clique that holds it, where it is in F)
            if (std::find(hp.sample[s].F.begin(), hp.sample[s].F.end(), q[i]) != hp.sample[s].F.end()) home[i] = s;
        if (home[i] < 0) return set_err(JTP_EINVAL, "jtp_joint: variable %d is in no clique", q[i]);
    }
    auto parent_of = [&](int s) { const int p = hp.parent_clique[hp.sample[s].clique]; return p < 0 ? -1 : ord_of[p]; };
    // homes below every record; the top: the deepest record that has them all
    std::vector<int> below(n, 0);
    for (int i = 0; i < n_query; ++i)
        for (int s = home[i]; s >= 0; s = parent_of(s)) ++below[s];
    int top = home[0];
    while (below[top] < n_query) top = parent_of(top);
    std::vector<int> act;                                    // active records, visit order: the top first
    for (int s = top; s < n; ++s) {
        if (!below[s]) continue;
        int a = s;
        while (a >= 0 && a != top) a = parent_of(a);
        if (a == top) act.push_back(s);
    }
    std::vector<int> rec_of(n, -1);
    for (size_t i = 0; i < act.size(); ++i) rec_of[act[i]] = (int)i;
    // C_c per active record: query positions, in the order of the query
    std::vector<std::vector<int>> carried(act.size());
    for (int i = 0; i < n_query; ++i)
        for (int s = home[i];; s = parent_of(s)) {
            carried[rec_of[s]].push_back(i);
            if (s == top) break;
        }
    for (auto &c : carried) std::sort(c.begin(), c.end());
    jq.recs.assign(act.size(), JtJoint());
    jq.top_clique = hp.sample[top].clique;
    jq.result = 1;
    for (int i = 0; i < n_query; ++i) {
        jq.result *= hp.card[q[i]];
        if (jq.result * 8 > JT_JOINT_CAP)
            return set_err(JTP_EUNSUPPORTED, "jtp_joint: the joint of these %d variables has more than %lld entries: a result beyond 64 MiB is not formed", n_query,
                           (long long)(JT_JOINT_CAP / 8));
    }
    int64_t at = 4;                                          // (the failure report: three words, and one of padding)
    const int64_t report = at;
    for (size_t i = 0; i < act.size(); ++i) {
        const SampleClique &sc = hp.sample[act[i]];
        JtJoint &r = jq.recs[i];
        memset(&r, 0, sizeof r);
        r.bel_off = hp.pack[sc.clique].dev_off;
        r.ord = act[i];
        r.top = i == 0;
        std::vector<int> own;                                // positions in the query of Q_c
        for (int p : carried[i])
            if (home[p] == act[i]) own.push_back(p);
        // v: K (not the top's), Q_c, the others in host axis order
        std::vector<int> vs;
        if (!r.top) vs = sc.K;
        r.nK = (int32_t)vs.size();
        for (int p : own) vs.push_back(q[p]);
        r.nQ = (int32_t)own.size();
        for (int v : hp.node_vars[sc.clique])
            if (std::find(vs.begin(), vs.end(), v) == vs.end()) vs.push_back(v);
        r.nF = (int32_t)vs.size() - r.nK - r.nQ;
        uint32_t radix_k = 1, radix_f = 1;
        for (int j = (int)vs.size() - 1; j >= 0; --j) {
            r.v[j] = jt_query_var(hp, sc.clique, vs[j]);
            if (j >= r.nK + r.nQ) r.v[j].radix = radix_f, radix_f *= (uint32_t)r.v[j].card;
            else if (j < r.nK) r.v[j].radix = radix_k, radix_k *= (uint32_t)r.v[j].card;
        }
        r.nk = radix_k;
        r.Rp = radix_f;
        r.nFs = (int32_t)sc.F.size();
        uint32_t radix = 1;
        for (int j = r.nFs - 1; j >= 0; --j) r.f[j] = jt_query_var(hp, sc.clique, sc.F[j]), r.f[j].radix = radix, radix *= (uint32_t)r.f[j].card;
        r.R = radix;
        r.lanes = 1;
        while (r.lanes < 64 && (uint32_t)r.lanes < r.Rp) r.lanes <<= 1;
        // x: C_c in the order of the query
        r.nX = (int32_t)carried[i].size();
        int64_t X = 1;
        for (int j = r.nX - 1; j >= 0; --j) {
            const int p = carried[i][j];
            JtJointX &jx = r.x[j];
            jx.card = hp.card[q[p]];
            jx.radix = (uint32_t)X;
            jx.slot = -1;
            for (int o = 0; o < r.nQ; ++o)
                if (own[o] == p) jx.slot = r.nK + o;
            X *= jx.card;
        }
        r.X = (uint32_t)X;                                   // (at most the result's entries)
        r.nseg = jt_query_nseg(r.Rp, JT_QUERY_SEG);
        const int64_t msg = (int64_t)r.nk * X;
        if (!r.top) {
            r.sig_off = at;
            r.msg_off = at + r.nk;
            at += r.nk + msg;
        }
        if (r.nseg > 1) r.part_off = at, at += msg * r.nseg;
        if ((at - report) * 8 > JT_JOINT_CAP)
            return set_err(JTP_EUNSUPPORTED, "jtp_joint: the tables carried up to the top pass 64 MiB at clique %d, whose message over %d query variables and its %u "
                                             "separator assignments has %lld entries (%.1f MiB; %u segment sums behind each): ask for fewer variables, or for variables nearer each other",
                           sc.clique, r.nX, r.nk, (long long)msg, (double)msg * 8.0 / 1048576.0, r.nseg > 1 ? r.nseg : 0u);
        if (!r.top) jq.max_nk = std::max(jq.max_nk, r.nk);
    }
    jq.result_off = at;
    jq.recs[0].msg_off = at;
    jq.work_doubles = at + jq.result;
    // active children: the active records whose parent clique is c (visit order within a depth is ascending clique number)
    jq.kids.clear();
    for (size_t i = 0; i < act.size(); ++i) {
        JtJoint &r = jq.recs[i];
        r.child_begin = (int32_t)jq.kids.size();
        for (size_t c = i + 1; c < act.size(); ++c) {
            if (parent_of(act[c]) != act[i]) continue;
            const JtJoint &ch = jq.recs[c];
            JtJointChild kd;
            memset(&kd, 0, sizeof kd);
            kd.msg_off = ch.msg_off;
            int64_t reach = 0;                               // the largest index this parent can form
            for (int j = 0; j < r.nK + r.nQ + r.nF; ++j)
                for (int jj = 0; jj < ch.nK; ++jj)
                    if (ch.v[jj].col == r.v[j].col) kd.stride[j] = ch.v[jj].radix * ch.X, reach += (int64_t)(r.v[j].card - 1) * kd.stride[j];
            for (int j = 0; j < r.nX; ++j)
                for (int jj = 0; jj < ch.nX; ++jj)
                    if (carried[c][jj] == carried[i][j]) kd.xstride[j] = ch.x[jj].radix, reach += (int64_t)(r.x[j].card - 1) * kd.xstride[j];
            if (reach != (int64_t)ch.nk * ch.X - 1)
                return set_err(JTP_EHIP, "jtp_joint: internal: clique %d indexes %lld entries of the message of clique %d, which has %lld", hp.sample[act[i]].clique,
                               (long long)reach + 1, hp.sample[act[c]].clique, (long long)ch.nk * ch.X);
            jq.kids.push_back(kd);
        }
        r.child_end = (int32_t)jq.kids.size();
    }
    jq.depth_range.clear();
    jq.depth_items.clear();
    jq.depth_merge.clear();
    for (size_t i = 0; i < act.size();) {
        size_t j = i;
        int64_t turns = 1, merge = 0;
        while (j < act.size() && hp.sample[act[j]].depth == hp.sample[act[i]].depth) {
            const JtJoint &r = jq.recs[j];
            turns = std::max(turns, ((int64_t)r.nk * r.X * r.nseg * r.lanes + 255) / 256);
            if (r.nseg > 1) merge = std::max(merge, (int64_t)r.nk * r.X);
            ++j;
        }
        jq.depth_range.push_back({(int)i, (int)j});
        jq.depth_items.push_back(turns);
        jq.depth_merge.push_back(merge);
        i = j;
    }
    return JTP_OK;
}

extern "C" {

int jtp_joint(jtp_plan *pl, int32_t batch, int32_t n_query, const int32_t *var_ids, double *host, int64_t *log2_scale) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    HostPlan &hp = pl->hp;
    if (!hp.sample_refused.empty()) return set_err(JTP_EUNSUPPORTED, "jtp_joint: %s", hp.sample_refused.c_str());
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    if (n_query < 1) return set_err(JTP_EINVAL, "n_query = %d: at least one variable", n_query);
    if (!var_ids || !host) return set_err(JTP_EINVAL, "null argument");
    if (n_query > JT_JOINT_MAXQ) return set_err(JTP_EUNSUPPORTED, "jtp_joint: %d query variables: at most %d in one call", n_query, JT_JOINT_MAXQ);
    for (int i = 0; i < n_query; ++i) {
        if (var_ids[i] < 0 || var_ids[i] >= hp.n_vars) return set_err(JTP_EINVAL, "jtp_joint: variable %d out of range [0,%d)", var_ids[i], hp.n_vars);
        for (int j = 0; j < i; ++j)
            if (var_ids[j] == var_ids[i]) return set_err(JTP_EINVAL, "jtp_joint: variable %d listed twice", var_ids[i]);
    }
    BatchBuffers &b = pl->bufs[batch];
    if (b.epoch == 0) return set_err(JTP_EINVAL, "evidence set %d has not been propagated: there are no beliefs to form a joint from", batch);
    JointQuery jq;
    rc = joint_records(hp, n_query, var_ids, jq);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_joint");
    rc = settle(pl, batch);
    if (rc) return rc;
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    // (buffers that must grow are built into locals and moved into the plan once everything the call allocates is there - a call
    //  that fails leaves the plan as it found it)
    const size_t rec_bytes = jq.recs.size() * sizeof(JtJoint), kid_bytes = jq.kids.size() * sizeof(JtJointChild);
    DeviceBuf<char> recs_dev(&pl->mem);
    DeviceBuf<double> work_dev(&pl->mem);
    if (pl->joint.recs.size() < rec_bytes + kid_bytes) HIP_TRY(recs_dev.alloc(rec_bytes + kid_bytes));
    if (pl->joint.work.size() < (size_t)jq.work_doubles) HIP_TRY(work_dev.alloc((size_t)jq.work_doubles));
    if (recs_dev) pl->joint.recs = std::move(recs_dev);
    if (work_dev) pl->joint.work = std::move(work_dev);
    char *blob = pl->joint.recs.get();
    const JtJoint *recs = (const JtJoint *)blob;
    const JtJointChild *kids = (const JtJointChild *)(blob + rec_bytes);
    double *work = pl->joint.work.get();
    unsigned long long *dfail = (unsigned long long *)work;
    HIP_TRY(hipMemcpyAsync(blob, jq.recs.data(), rec_bytes, hipMemcpyHostToDevice, s));
    if (kid_bytes) HIP_TRY(hipMemcpyAsync(blob + rec_bytes, jq.kids.data(), kid_bytes, hipMemcpyHostToDevice, s));
    const unsigned long long fail0[4] = {0ull, ~0ull, 0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(dfail, fail0, sizeof fail0, hipMemcpyHostToDevice, s));
    const size_t n_rec = jq.recs.size();
    jt_query_slices(n_rec - 1, [&](size_t y0, size_t ny) {    // (sigma does not depend on the depth: every clique but the top - record 0, always there - at once)
        const dim3 grid(jt_query_grid_x(((int64_t)jq.max_nk + 3) / 4, ny), (unsigned)ny);
        JT_QUERY_LAUNCH(hp.dtype, jt_joint_sigma, grid, s, recs + 1 + y0, (const T *)b.bel, work, dfail);
    });
    for (size_t d = jq.depth_range.size(); d-- > 0;) {
        const int y0 = jq.depth_range[d].first, ny = jq.depth_range[d].second - y0;      // (at most one clique per query variable)
        const dim3 grid(jt_query_grid_x(jq.depth_items[d], (size_t)ny), (unsigned)ny);
        JT_QUERY_LAUNCH(hp.dtype, jt_joint_level, grid, s, recs + y0, kids, (const T *)b.bel, work, dfail);
        if (jq.depth_merge[d]) {
            const dim3 mgrid((unsigned)std::min<int64_t>((jq.depth_merge[d] + 3) / 4, 1024), (unsigned)ny);
            hipLaunchKernelGGL(jt_joint_merge, mgrid, dim3(256), 0, s, recs + y0, work, dfail);
        }
    }
    HIP_TRY(hipGetLastError());
    unsigned long long fail[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(host, work + jq.result_off, (size_t)jq.result * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(fail, dfail, sizeof fail, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    rc = check_flow(pl, batch);
    if (rc) return rc;
    if (log2_scale) {
        rc = jtp_get_log2_scale(pl, batch, jq.top_clique, log2_scale);
        if (rc) return rc;
    }
    if (fail[0] || fail[2]) {
        const int c = fail[2] ? jq.top_clique : fail[1] < hp.sample.size() ? hp.sample[(size_t)fail[1]].clique : -1;      // (the top is the first of the active cliques)
        return set_err(JTP_EINVAL, "jtp_joint: %llu (clique, k) pairs met a negative or NaN belief entry or a sum that is not finite, the first at clique %d; "
                                   "the joint is written as it came out (tables that overflowed on a plan without JTP_SCALED?)", fail[0] + (fail[2] ? 1ull : 0ull), c);
    }
    return JTP_OK;
}

}  // extern "C"
