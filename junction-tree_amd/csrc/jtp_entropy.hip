// Entropy of the posterior, and cross-entropy against another evidence set of the plan, from the beliefs a propagate left.
#include <cmath>

#include <algorithm>
#include <cstring>
#include <vector>

#include "jtp_engine.h"
#include "jtp_query.h"

// jtp_entropy works on the sampling schedule (HostPlan::sample: K_c the variables clique c shares with its parent, F_c the others,
// R_c = prod card(F_c), nk = prod card(K_c)) and on the belief tables alone, ALL of them: one streaming pass.  For a set a and a
// reference set b, per clique c (include/jtprop.h has the definitions):
//     t_c(a, b) = sum_k [ sum_r beta^a[k, r] ln beta^b[k, r]  -  sigma^a[k] ln sigma^b[k] ],   sigma[k] = sum_r beta[k, r]
//     h_c = -t_c(a, a) / S_c,   x_c = -t_c(a, b) / S_c,   S_c = sum_k sigma^a[k]
// SINGLE PASS: jt_entropy_sums reads every entry once and forms, per (set, clique, k), sigma^a and sum_r beta^a ln beta^a - with a
// reference also sigma^b and sum_r beta^a ln beta^b, from the two tables at the same offset -; jt_entropy_finish adds the segments,
// takes sigma ln sigma off, adds over k and divides.  (The two-pass form, sigma first and then sum beta ln(beta / sigma), reads every
// belief twice; it was not needed to meet the tests' bound.)
// ORDER OF THE SUMS.  F_c is listed in ascending device stride, the first variable the fastest digit of r.  `lanes` = min(64, R_c
// rounded up to a power of two) lanes share a (k, segment) and 256 / lanes of those make a workgroup turn; lane l adds r = lo + l,
// lo + l + lanes, ... one after the other (a mixed-radix counter, its digits in LDS, moves the table offset by `lanes` a turn), and a
// fixed tree of shuffles adds the lanes.  R_c >= 2 JT_QUERY_SEG: r is cut into jt_query_nseg contiguous segments, a wave each; the
// finish adds a k's segment sums by a wave, lane l those of segments l, l + 64, ... in ascending order, then the same tree.  Over k:
// nseg = 1: thread t of 256 adds k = t, t + 256, ..., a shuffle tree adds the lanes of a wave; nseg > 1: wave w adds k = w, w + 4,
// ...; the four waves' sums are added in ascending order.  Nothing here depends on timing - the only atomics are ORs of flag bits -
// so two calls on the same beliefs agree bit for bit; the order DOES depend on the stored layout (which r a lane meets), so plans
// of different layout agree to rounding only.  That is the price of coalesced reads.
// A term is left out by a select on beta^a > 0 (sigma^a > 0): the logarithm's value at 0 never reaches a sum.  Flags per (set,
// clique): 1 = a negative or NaN entry in either table, or a sigma^b that is not finite; 2 = beta^a > 0 met beta^b = 0 (x_c = +inf).

#define JT_ENTROPY_CAP ((int64_t)64 << 20)    // bytes of the per-k and segment sums of a chunk of evidence sets

__device__ __forceinline__ double jt_entropy_lanes_sum(double s, int lanes) {
    for (int d = lanes >> 1; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return s;
}

// the counter of thread `tid` moves on by `lanes` entries of r - digit j by step[j] and the carry -: the offset there.  Digits
// below step_lo do not move; above step_hi only a carry does.
__device__ __forceinline__ uint32_t jt_entropy_walk_add(const JtSampleVar *fv, const int32_t *step, int nF, int step_lo, int step_hi, int (*digs)[256], int tid,
                                                        uint32_t off) {
    int carry = 0;
    for (int j = step_lo; j < nF; ++j) {
        if (j >= step_hi && !carry) break;
        const JtSampleVar v = fv[j];
        const int dg = digs[j][tid];
        int nd = dg + step[j] + carry;
        carry = nd >= v.card;
        if (carry) nd -= v.card;
        off += jt_sample_at(v, nd) - jt_sample_at(v, dg);
        digs[j][tid] = nd;
    }
    return off;
}

// one launch over all cliques (blockIdx.y) and all evidence sets of the chunk (blockIdx.z)
template <typename T, bool REF>
__device__ __forceinline__ void jt_entropy_sums_body(const JtEntropy *__restrict__ recs, const void *const *__restrict__ tables, double *__restrict__ ksum,
                                                     double *__restrict__ part, unsigned long long *__restrict__ res, int rec0, int n_rec, int64_t entries,
                                                     int64_t parts) {
    constexpr int NV = REF ? 4 : 2;
    __shared__ int digs[JT_MAX_VARS][256];             // digit j of thread t's counter: a column per thread, no barrier needed
    __shared__ JtSampleVar sv[JT_MAX_VARS];
    __shared__ int32_t step[JT_MAX_VARS];
    const JtEntropy &rec = recs[blockIdx.y];
    const int tid = threadIdx.x, set = blockIdx.z;
    const int nK = rec.nK, nF = rec.nF;
    jt_query_stage_vars(sv, rec.v, nK + nF, tid);
    if (tid < nF) step[tid] = rec.step[tid];
    __syncthreads();
    const T *__restrict__ bel_a = (const T *)tables[2 * set];
    const T *__restrict__ bel_b = (const T *)tables[2 * set + 1];
    const JtSampleVar *fv = sv + nK;
    const int lanes = rec.lanes, sub = tid & (lanes - 1), per = 256 / lanes;
    const int step_lo = rec.step_lo, step_hi = rec.step_hi;
    const uint32_t R = rec.R, nseg = rec.nseg;
    const uint32_t seg_len = (R + nseg - 1u) / nseg;
    const int64_t n_items = (int64_t)rec.nk * nseg;
    double *out = nseg > 1 ? part + ((int64_t)set * parts + rec.part_off) * NV : ksum + ((int64_t)set * entries + rec.k_off) * NV;
    bool bad = false, inf = false;
    for (int64_t first = (int64_t)blockIdx.x * per; first < n_items; first += (int64_t)gridDim.x * per) {     // (the whole workgroup)
        const int64_t item = first + tid / lanes;
        const bool live = item < n_items;
        const uint32_t k = live ? (uint32_t)(item / nseg) : 0u, seg = live ? (uint32_t)(item % nseg) : 0u;
        const uint32_t lo = min(seg * seg_len, R), end = live ? min(lo + seg_len, R) : lo;
        double s_a = 0.0, t_aa = 0.0, s_b = 0.0, t_ab = 0.0;
        if (end - lo > (uint32_t)sub) {
            int64_t base = rec.bel_off;
            for (int j = 0; j < nK; ++j) base += jt_sample_at(sv[j], (int)((k / sv[j].radix) % (uint32_t)sv[j].card));
            uint32_t q = lo + (uint32_t)sub;
            uint32_t off = jt_query_walk_start(fv, nF, digs, tid, q);
            for (;;) {
                const double a = (double)bel_a[base + off];
                bad = bad || !(a >= 0.0);
                s_a += a;
                t_aa += a > 0.0 ? a * log(a) : 0.0;
                if (REF) {
                    const double b = (double)bel_b[base + off];
                    bad = bad || !(b >= 0.0);
                    s_b += b;
                    t_ab += a > 0.0 && b > 0.0 ? a * log(b) : 0.0;
                    inf = inf || (a > 0.0 && b == 0.0);
                }
                if (end - q <= (uint32_t)lanes) break;
                q += (uint32_t)lanes;
                off = jt_entropy_walk_add(fv, step, nF, step_lo, step_hi, digs, tid, off);
            }
        }
        s_a = jt_entropy_lanes_sum(s_a, lanes);
        t_aa = jt_entropy_lanes_sum(t_aa, lanes);
        if (REF) s_b = jt_entropy_lanes_sum(s_b, lanes), t_ab = jt_entropy_lanes_sum(t_ab, lanes);
        if (live && sub == 0) {
            double *o = out + item * NV;               // (nseg = 1: item = k)
            o[0] = s_a, o[1] = t_aa;
            if (REF) o[2] = s_b, o[3] = t_ab;
        }
    }
    const unsigned long long bits = (__ballot(bad) != 0ull ? 1ull : 0ull) | (__ballot(inf) != 0ull ? 2ull : 0ull);
    if (bits && (tid & 63) == 0) atomicOr(&res[((int64_t)set * n_rec + rec0 + blockIdx.y) * 4 + 3], bits);
}

// (the two kernels: entropy alone, and entropy with the cross-entropy against the second table)
template <typename T>
__global__ __launch_bounds__(256) void jt_entropy_sums(const JtEntropy *__restrict__ recs, const void *const *__restrict__ tables, double *__restrict__ ksum,
                                                       double *__restrict__ part, unsigned long long *__restrict__ res, int rec0, int n_rec, int64_t entries,
                                                       int64_t parts) {
    jt_entropy_sums_body<T, false>(recs, tables, ksum, part, res, rec0, n_rec, entries, parts);
}
template <typename T>
__global__ __launch_bounds__(256) void jt_entropy_sums_ref(const JtEntropy *__restrict__ recs, const void *const *__restrict__ tables, double *__restrict__ ksum,
                                                           double *__restrict__ part, unsigned long long *__restrict__ res, int rec0, int n_rec, int64_t entries,
                                                           int64_t parts) {
    jt_entropy_sums_body<T, true>(recs, tables, ksum, part, res, rec0, n_rec, entries, parts);
}

// sigma ln sigma taken off one k's sums `v`, and the k added to the clique's
template <bool REF>
__device__ __forceinline__ void jt_entropy_add_k(const double *v, double &S, double &t_aa, double &t_ab, bool &inf, bool &bad) {
    const double sa = v[0];
    S += sa;
    t_aa += v[1] - (sa > 0.0 ? sa * log(sa) : 0.0);
    if (REF) {
        const double sb = v[2];
        t_ab += v[3] - (sa > 0.0 && sb > 0.0 ? sa * log(sb) : 0.0);
        inf = inf || (sa > 0.0 && sb == 0.0);
        bad = bad || !(sb < INFINITY);                   // (the reference's tables overflowed: its logarithms say nothing)
    }
}

// a workgroup per (clique, set): res = h_c, x_c, S_c; the flags word is ORed into as jt_entropy_sums does
template <bool REF>
__global__ __launch_bounds__(256) void jt_entropy_finish(const JtEntropy *__restrict__ recs, const double *__restrict__ ksum, const double *__restrict__ part,
                                                         unsigned long long *__restrict__ res, int n_rec, int64_t entries, int64_t parts) {
    constexpr int NV = REF ? 4 : 2;
    __shared__ double wsum[4][3];
    __shared__ int winf[4];
    const JtEntropy &rec = recs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, set = blockIdx.y;
    const uint32_t nk = rec.nk, nseg = rec.nseg;
    double S = 0.0, t_aa = 0.0, t_ab = 0.0;
    bool inf = false, bad = false;
    if (nseg > 1) {
        const double *pt = part + ((int64_t)set * parts + rec.part_off) * NV;
        for (uint32_t k = (uint32_t)wave; k < nk; k += 4u) {             // (a whole wave; every lane ends with the wave's sums)
            double v[NV];
            for (int i = 0; i < NV; ++i) v[i] = 0.0;
            for (uint32_t sg = (uint32_t)lane; sg < nseg; sg += 64u)
                for (int i = 0; i < NV; ++i) v[i] += pt[((int64_t)k * nseg + sg) * NV + i];
            for (int i = 0; i < NV; ++i) v[i] = jt_entropy_lanes_sum(v[i], 64);
            jt_entropy_add_k<REF>(v, S, t_aa, t_ab, inf, bad);
        }
    } else {
        const double *ks = ksum + ((int64_t)set * entries + rec.k_off) * NV;
        for (uint32_t k = (uint32_t)tid; k < nk; k += 256u) jt_entropy_add_k<REF>(ks + (int64_t)k * NV, S, t_aa, t_ab, inf, bad);
        S = jt_entropy_lanes_sum(S, 64);
        t_aa = jt_entropy_lanes_sum(t_aa, 64);
        if (REF) t_ab = jt_entropy_lanes_sum(t_ab, 64);
    }
    const int bits = (__ballot(bad) != 0ull ? 1 : 0) | (__ballot(inf) != 0ull ? 2 : 0);
    if (lane == 0) wsum[wave][0] = S, wsum[wave][1] = t_aa, wsum[wave][2] = t_ab, winf[wave] = bits;
    __syncthreads();
    if (tid == 0) {
        S = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
        t_aa = ((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1];
        t_ab = ((wsum[0][2] + wsum[1][2]) + wsum[2][2]) + wsum[3][2];
        double *o = (double *)(res + ((int64_t)set * n_rec + blockIdx.x) * 4);
        o[0] = (0.0 - t_aa) / S;
        o[1] = (0.0 - t_ab) / S;
        o[2] = S;
        const int bits = winf[0] | winf[1] | winf[2] | winf[3];
        if (bits) atomicOr(&res[((int64_t)set * n_rec + blockIdx.x) * 4 + 3], (unsigned long long)bits);
    }
}

// the plan's records, and the sizes of a set's sums with them
static void entropy_records(const HostPlan &hp, std::vector<JtEntropy> &recs, EntropyMem &em) {
    recs.assign(hp.sample.size(), JtEntropy());
    em.entries = em.parts = 0;
    em.max_items = 1;
    for (size_t i = 0; i < recs.size(); ++i) {
        const SampleClique &sc = hp.sample[i];
        JtEntropy &r = recs[i];
        memset(&r, 0, sizeof r);
        r.bel_off = hp.pack[sc.clique].dev_off;
        r.clique = sc.clique;
        r.nK = (int32_t)sc.K.size();
        r.nF = (int32_t)sc.F.size();
        uint32_t radix = 1;
        for (int j = r.nK - 1; j >= 0; --j) r.v[j] = jt_query_var(hp, sc.clique, sc.K[j]), r.v[j].radix = radix, radix *= (uint32_t)r.v[j].card;
        r.nk = radix;
        JtSampleVar *fv = r.v + r.nK;
        for (int j = 0; j < r.nF; ++j) fv[j] = jt_query_var(hp, sc.clique, sc.F[j]);
        std::stable_sort(fv, fv + r.nF, [](const JtSampleVar &x, const JtSampleVar &y) { return x.stride < y.stride; });
        radix = 1;
        for (int j = 0; j < r.nF; ++j) fv[j].radix = radix, radix *= (uint32_t)fv[j].card;
        r.R = radix;
        r.lanes = 1;
        while (r.lanes < 64 && (uint32_t)r.lanes < r.R) r.lanes <<= 1;
        r.nseg = jt_query_nseg(r.R, JT_QUERY_SEG);
        uint32_t rem = (uint32_t)r.lanes;
        r.step_lo = r.nF, r.step_hi = 0;
        for (int j = 0; j < r.nF; ++j) {
            r.step[j] = (int32_t)(rem % (uint32_t)fv[j].card);
            rem /= (uint32_t)fv[j].card;
            if (r.step[j]) r.step_lo = std::min(r.step_lo, j), r.step_hi = j + 1;
        }
        r.k_off = em.entries;
        em.entries += r.nk;
        if (r.nseg > 1) r.part_off = em.parts, em.parts += (int64_t)r.nk * r.nseg;
        em.max_items = std::max(em.max_items, ((int64_t)r.nk * r.nseg * r.lanes + 255) / 256);
    }
}

extern "C" {

int jtp_entropy(jtp_plan *pl, int32_t batch_begin, int32_t batch_end, const int32_t *ref_set, double *entropy, double *cross, double *clique_entropy) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    HostPlan &hp = pl->hp;
    if (!hp.sample_refused.empty()) return set_err(JTP_EUNSUPPORTED, "jtp_entropy: %s", hp.sample_refused.c_str());
    int rc = check_ready(pl, batch_begin);
    if (rc) return rc;
    if (batch_end <= batch_begin || batch_end > hp.n_batch) return set_err(JTP_EINVAL, "bad batch range [%d,%d)", batch_begin, batch_end);
    if (!entropy) return set_err(JTP_EINVAL, "null argument");
    if ((ref_set == nullptr) != (cross == nullptr)) return set_err(JTP_EINVAL, "jtp_entropy: ref_set and cross are both NULL or both given");
    const size_t n_sets = (size_t)(batch_end - batch_begin), n_rec = hp.sample.size();
    for (size_t i = 0; i < n_sets; ++i) {
        const int a = batch_begin + (int)i, b = ref_set ? ref_set[i] : a;
        if (b < 0 || b >= hp.n_batch) return set_err(JTP_EINVAL, "jtp_entropy: reference set %d of set %d out of range [0,%d)", b, a, hp.n_batch);
        for (int x : {a, b})
            if (pl->bufs[x].epoch == 0) return set_err(JTP_EINVAL, "evidence set %d has not been propagated: there are no beliefs to take an entropy of", x);
    }
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_entropy");
    for (size_t i = 0; i < n_sets; ++i)
        for (int x : {batch_begin + (int)i, ref_set ? ref_set[i] : batch_begin + (int)i})
            if ((rc = settle(pl, x))) return rc;
    for (auto st : pl->streams) HIP_TRY(hipStreamSynchronize(st));     // (the sets' beliefs were written on their own streams)
    hipStream_t s = pl->streams[0];
    // (first call, or a chunk the work area does not hold: built into locals and moved into the plan once everything the call
    //  allocates is there - a call that fails an allocation leaves the plan as it found it)
    EntropyMem fresh(&pl->mem);
    const bool first = !pl->entropy.recs;
    if (first) {
        std::vector<JtEntropy> recs;
        entropy_records(hp, recs, fresh);
        HIP_TRY(fresh.recs.upload(recs, 1));
    }
    const EntropyMem &lay = first ? fresh : pl->entropy;  // (whose sizes hold)
    const size_t nv = ref_set ? 4 : 2, entries = (size_t)lay.entries, parts = (size_t)lay.parts;
    const size_t chunk = std::min(std::min<size_t>(n_sets, 65535), std::max<size_t>(1, (size_t)JT_ENTROPY_CAP / (8 * nv * (entries + parts))));
    // the work area, in words of 8 bytes: the tables' addresses, the results, the per-k sums, the segment sums
    const size_t res_at = 2 * chunk, ksum_at = res_at + chunk * n_rec * 4, part_at = ksum_at + chunk * entries * nv, words = part_at + chunk * parts * nv;
    if (pl->entropy.work.size() < words) HIP_TRY(fresh.work.alloc(words));
    if (first) pl->entropy = std::move(fresh);
    else if (fresh.work) pl->entropy.work = std::move(fresh.work);
    EntropyMem &em = pl->entropy;
    double *work = em.work.get();
    unsigned long long *res = (unsigned long long *)(work + res_at);
    std::vector<const void *> tables(2 * chunk);
    std::vector<double> out(chunk * n_rec * 4);
    const double qnan = std::nan("");
    size_t n_failed = 0;
    int first_set = -1, first_clique = -1;
    for (size_t at = 0; at < n_sets; at += chunk) {
        const size_t cnt = std::min(chunk, n_sets - at);
        for (size_t i = 0; i < cnt; ++i) {
            const int a = batch_begin + (int)(at + i);
            tables[2 * i] = pl->bufs[a].bel;
            tables[2 * i + 1] = pl->bufs[ref_set ? ref_set[at + i] : a].bel;
        }
        HIP_TRY(hipMemcpyAsync(work, tables.data(), 2 * cnt * sizeof(void *), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(res, 0, cnt * n_rec * 4 * sizeof(double), s));
        jt_query_slices(n_rec, [&](size_t y0, size_t ny) {
            const dim3 grid(jt_query_grid_x(em.max_items, ny), (unsigned)ny, (unsigned)cnt);
            if (ref_set)
                JT_QUERY_LAUNCH(hp.dtype, jt_entropy_sums_ref, grid, s, em.recs.get() + y0, (const void *const *)work, work + ksum_at, work + part_at, res, (int)y0, (int)n_rec,
                                (int64_t)entries, (int64_t)parts);
            else
                JT_QUERY_LAUNCH(hp.dtype, jt_entropy_sums, grid, s, em.recs.get() + y0, (const void *const *)work, work + ksum_at, work + part_at, res, (int)y0, (int)n_rec,
                                (int64_t)entries, (int64_t)parts);
        });
        const dim3 fgrid((unsigned)n_rec, (unsigned)cnt);
        if (ref_set) hipLaunchKernelGGL(jt_entropy_finish<true>, fgrid, dim3(256), 0, s, em.recs.get(), work + ksum_at, work + part_at, res, (int)n_rec, (int64_t)entries, (int64_t)parts);
        else hipLaunchKernelGGL(jt_entropy_finish<false>, fgrid, dim3(256), 0, s, em.recs.get(), work + ksum_at, work + part_at, res, (int)n_rec, (int64_t)entries, (int64_t)parts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out.data(), res, cnt * n_rec * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                 // (the work area is the next chunk's)
        // H and X: the cliques' terms added in visit order
        for (size_t i = 0; i < cnt; ++i) {
            const double *o = &out[i * n_rec * 4];
            double H = 0.0, X = 0.0;
            bool any_inf = false;
            int failed_at = -1;
            for (size_t c = 0; c < n_rec && failed_at < 0; ++c) {
                unsigned long long flags;
                memcpy(&flags, &o[c * 4 + 3], sizeof flags);
                const double S = o[c * 4 + 2];
                if ((flags & 1ull) || !(S > 0.0) || !(S < INFINITY)) failed_at = (int)c;
                H += o[c * 4];
                X += o[c * 4 + 1];
                any_inf = any_inf || (flags & 2ull);
            }
            double *row = clique_entropy ? clique_entropy + (at + i) * (size_t)hp.n_cliques : nullptr;
            if (failed_at >= 0) {
                if (n_failed++ == 0) first_set = batch_begin + (int)(at + i), first_clique = hp.sample[(size_t)failed_at].clique;
                entropy[at + i] = qnan;
                if (cross) cross[at + i] = qnan;
                for (int c = 0; row && c < hp.n_cliques; ++c) row[c] = qnan;
                continue;
            }
            entropy[at + i] = H;
            if (cross) cross[at + i] = any_inf ? INFINITY : X;
            for (size_t c = 0; row && c < n_rec; ++c) row[hp.sample[c].clique] = o[c * 4];
        }
    }
    if (n_failed)
        return set_err(JTP_EINVAL, "jtp_entropy: %zu of %zu evidence sets failed, the first set %d at clique %d (a negative or NaN belief entry in the set or its reference, "
                                   "or a clique whose beliefs sum to zero or to nothing finite: evidence of probability zero? tables that overflowed on a plan without "
                                   "JTP_SCALED?); their outputs are NaN",
                       n_failed, n_sets, first_set, first_clique);
    return JTP_OK;
}

}  // extern "C"
