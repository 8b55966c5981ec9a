// Joint posterior samples drawn on the device from the propagated beliefs.
#include <cmath>

#include <algorithm>
#include <cstring>
#include <vector>

#include "jtp_engine.h"
#include "jtp_query.h"

// jtp_sample: one launch per depth of the caller's tree (HostPlan::sample_depths), a wave64 per (clique, sample), four per
// workgroup; blockIdx.y = the clique's record, blockIdx.x * 4 + wave = the sample of the chunk.  The wave reads the sample's
// digits of the conditioning variables (drawn by the launches before this one), which fixes a slice of the clique's belief table:
// R entries w_r >= 0, r the C-order index over the drawn variables in host axis order.  It draws the entry at which the running sum
// crosses u * total by a search that narrows a segment [lo, lo + len) of r, starting with the whole slice: lane l sums the block
// [lo + l B, lo + (l + 1) B), B = ceil(len / 64), entry by entry in r order (a mixed-radix counter over the drawn variables, its
// digits in LDS, moves the table offset), an inclusive scan over the lanes (six shuffle steps) gives the running sums at the
// block ends, and the first block WITH MASS whose running sum exceeds the target becomes the next segment, the target less what
// lies before it.  B = 1 ends it.  Which entries are added in which order depends on R alone - not on the table's layout, the chunk
// or the launch - so equal beliefs give equal draws whatever the plan's flags.  A chosen block always has a positive sum, hence a
// positive entry: where rounding lets no block cross the target, the last block with mass is taken, and the entry drawn has
// w_r > 0.  A slice with a negative or NaN entry, or whose total is zero or not finite, fails: the sample's drawn variables are
// set to -1, a clique that finds -1 among its conditioning digits fails without loading anything, and fail[0] counts the failed
// (clique, sample) pairs, fail[1] keeps the smallest visit-order place among them.
#define JT_SAMPLE_SALT 0x53414D504C45ull

template <typename T>
__global__ __launch_bounds__(256) void jt_sample_level(const JtSample *__restrict__ recs, const T *__restrict__ bel, int32_t *__restrict__ states,
                                                       int n_vars, int n_chunk, uint64_t first, uint64_t seed, unsigned long long *__restrict__ fail) {
    __shared__ int digs[JT_MAX_VARS][256];             // digit k of thread t's counter: a column per thread, no barrier needed
    __shared__ JtSampleVar sv[JT_MAX_VARS];
    const JtSample &rec = recs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nK = rec.nK, nF = rec.nF;
    jt_query_stage_vars(sv, rec.v, nK + nF, tid);
    __syncthreads();
    const int local = blockIdx.x * 4 + (tid >> 6);
    if (local >= n_chunk) return;                      // (a whole wave)
    int32_t *row = states + (int64_t)local * n_vars;
    const JtSampleVar *fv = sv + nK;
    bool dead = false;
    int64_t base = rec.bel_off;
    for (int k = 0; k < nK; ++k) {
        const int st = row[sv[k].col];
        if (st < 0 || st >= sv[k].card) dead = true;
        else base += jt_sample_at(sv[k], st);
    }
    const uint64_t key = jt_splitmix64(jt_splitmix64(seed * 0x100000001B3ull + (uint64_t)rec.clique) ^ JT_SAMPLE_SALT);
    const double u = (double)(jt_splitmix64(key + first + (uint64_t)local) >> 11) * (1.0 / 9007199254740992.0);
    uint32_t lo = 0, len = rec.R, r = 0;
    double target = 0.0;
    bool whole = true;
    while (!dead) {
        const uint32_t end = lo + len;
        const auto [a, e, B] = jt_query_cut(lo, end, 64u, (uint32_t)lane);
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
        double inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const double y = __shfl_up(inc, d, 64);
            if (lane >= d) inc += y;
        }
        const double total = __shfl(inc, 63, 64);
        if (whole) {
            whole = false;
            if (__ballot(bad) != 0ull || !(total > 0.0) || !(total < INFINITY)) {
                dead = true;
                break;
            }
            target = u * total;
        }
        double exc = __shfl_up(inc, 1, 64);
        if (lane == 0) exc = 0.0;
        const unsigned long long mass = __ballot(sum > 0.0), hit = mass & __ballot(inc > target);
        if (!mass) {
            dead = true;
            break;
        }
        const int sel = hit ? __builtin_ctzll(hit) : 63 - __builtin_clzll(mass);
        target -= __shfl(exc, sel, 64);
        lo += (uint32_t)sel * B;
        len = min(B, end - lo);
        if (B == 1) {
            r = lo;
            break;
        }
    }
    if (dead && lane == 0) {
        atomicAdd(&fail[0], 1ull);
        atomicMin(&fail[1], (unsigned long long)rec.ord);
    }
    if (lane < nF) row[fv[lane].col] = dead ? -1 : (int)((r / fv[lane].radix) % (uint32_t)fv[lane].card);
}

extern "C" {

int jtp_sample(jtp_plan *pl, int32_t batch, int32_t n_samples, uint64_t seed, int32_t *states) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    HostPlan &hp = pl->hp;
    if (!hp.sample_refused.empty()) return set_err(JTP_EUNSUPPORTED, "jtp_sample: %s", hp.sample_refused.c_str());
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    if (!states) return set_err(JTP_EINVAL, "null argument");
    if (n_samples < 1) return set_err(JTP_EINVAL, "n_samples = %d: at least one sample", n_samples);
    BatchBuffers &b = pl->bufs[batch];
    if (b.epoch == 0) return set_err(JTP_EINVAL, "evidence set %d has not been propagated: there are no beliefs to sample from", batch);
    const int n_vars = hp.n_vars;
    if (n_vars == 0) return JTP_OK;
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_sample");
    rc = settle(pl, batch);
    if (rc) return rc;
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    // (first call: the records and the failure report are built into locals and moved into the plan once everything the call
    //  allocates is there - a call that fails leaves the plan as it found it)
    DeviceBuf<JtSample> recs_dev(&pl->mem);
    DeviceBuf<unsigned long long> fail_dev(&pl->mem);
    if (!pl->sample.recs) {
        std::vector<JtSample> recs(hp.sample.size());
        for (size_t i = 0; i < recs.size(); ++i) {
            const SampleClique &sc = hp.sample[i];
            JtSample &r = recs[i];
            memset(&r, 0, sizeof r);
            r.bel_off = hp.pack[sc.clique].dev_off;
            r.nK = (int32_t)sc.K.size();
            r.nF = (int32_t)sc.F.size();
            r.R = (uint32_t)sc.R;
            r.clique = sc.clique;
            r.ord = (int32_t)i;
            uint32_t radix = 1;
            for (int j = r.nK + r.nF - 1; j >= 0; --j) {
                JtSampleVar &sv = r.v[j] = jt_query_var(hp, sc.clique, j < r.nK ? sc.K[j] : sc.F[j - r.nK]);
                if (j >= r.nK) sv.radix = radix, radix *= (uint32_t)sv.card;
            }
        }
        HIP_TRY(recs_dev.upload(recs, 1));
    }
    if (!pl->sample.fail) HIP_TRY(fail_dev.alloc(2));
    // samples go in chunks through one buffer of state rows (at most 64 MiB of them, 256 .. 65536 rows): the grid stays within
    // limits whatever n_samples is, and there is one copy back per chunk
    const size_t chunk = std::min<size_t>((size_t)n_samples, std::max<size_t>(256, std::min<size_t>(65536, ((size_t)16 << 20) / (size_t)n_vars)));
    HIP_TRY(pl->sample.states.reserve(chunk * (size_t)n_vars));
    if (recs_dev) pl->sample.recs = std::move(recs_dev);
    if (fail_dev) pl->sample.fail = std::move(fail_dev);
    int32_t *rows = pl->sample.states.get();
    unsigned long long *dfail = pl->sample.fail.get();
    HIP_TRY(hipMemsetAsync(dfail, 0, sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(dfail + 1, 0xff, sizeof(unsigned long long), s));
    for (size_t at = 0; at < (size_t)n_samples; at += chunk) {
        const size_t cnt = std::min(chunk, (size_t)n_samples - at);
        HIP_TRY(hipMemsetAsync(rows, 0xff, cnt * (size_t)n_vars * sizeof(int32_t), s));      // (-1: nothing drawn yet)
        for (const std::vector<int> &level : hp.sample_depths)
            jt_query_slices(level.size(), [&](size_t y0, size_t ny) {                                     // (records of a depth are consecutive)
                const dim3 grid((unsigned)((cnt + 3) / 4), (unsigned)ny);
                JT_QUERY_LAUNCH(hp.dtype, jt_sample_level, grid, s, pl->sample.recs.get() + level[0] + y0, (const T *)b.bel, rows, n_vars, (int)cnt, (uint64_t)at, seed, dfail);
            });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(states + at * (size_t)n_vars, rows, cnt * (size_t)n_vars * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                // (the buffer is the next chunk's)
    }
    unsigned long long fail[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(fail, dfail, sizeof fail, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    rc = check_flow(pl, batch);
    if (rc) return rc;
    if (fail[0]) {
        const int c = fail[1] < hp.sample.size() ? hp.sample[(size_t)fail[1]].clique : -1;
        return set_err(JTP_EINVAL, "jtp_sample: %llu (clique, sample) pairs met a slice without mass (zero or non-finite total, or a negative or NaN entry), "
                                   "the first at clique %d; their variables are -1 in the states (evidence of probability zero? tables that overflowed?)", fail[0], c);
    }
    return JTP_OK;
}

}  // extern "C"
