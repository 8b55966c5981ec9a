// Internal header of the units that sweep the sampling schedule upward over the clique potentials, every message scaled by the exponent
// of its largest entry: the three max-product units (through jtp_maxprod.h, which adds what only they share) and jtp_mmap.hip
// (jtp_marginal_map, which sums before it maximises and runs jtp_map's kernels where there is nothing to sum).  The work area and the
// maxima of that sweep, what a wave keeps and stores, and the host steps of an entry point, which jtp_map.hip defines once.  No
// function here is told which query calls it.
#pragma once
#include <cmath>

#include <algorithm>
#include <cstring>
#include <vector>

#include "jtp_engine.h"
#include "jtp_query.h"

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

// `v` >= 0 into the running maximum of a table, kept as an integer maximum over bit patterns - non-negative doubles order like their
// bits, so it is exact whatever the order (the maximum only grows: most waves need no atomic)
__device__ __forceinline__ void jt_maxprod_keep_top(unsigned long long *top, double v) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    if (__atomic_load_n(top, __ATOMIC_RELAXED) < bits) atomicMax(top, bits);
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
    jt_maxprod_keep_top(wk.top + (int64_t)set * n_rec + rec.ord, best);
}

// ------------------------------------------------------------------------------------------ host: the steps of an entry point (jtp_map.hip)

// what every entry point refuses, under the name `fn`: a multi-set plan, several ranks, a clique without a table, a bad batch range
int maxprod_refuse(const char *fn, const HostPlan &hp, int32_t batch_begin, int32_t batch_end);
// entries per segment of r: jtp_debug_set "map_seg", else JT_QUERY_SEG
uint32_t maxprod_seg(const jtp_plan *pl);
// sets [first, first + cnt) of the plan into a work area: their potential arenas and evidence rows (through the caller's host
// buffers), their maxima and flags cleared
int maxprod_stage_sets(jtp_plan *pl, size_t first, size_t cnt, std::vector<const void *> &psi, std::vector<int32_t> &ev, const void **d_psi, int32_t *d_ev,
                       unsigned long long *d_top, int32_t *d_flag, hipStream_t s);
// n records of at most `waves` waves of work each, a slice at a time: fn(first record of the slice, grid of the level kernel, of the merge kernel)
template <typename Fn>
static inline void maxprod_slices(size_t n, int64_t waves, Fn &&fn) {
    jt_query_slices(n, [&](size_t y0, size_t ny) {
        fn(y0, dim3(jt_query_grid_x((waves + 3) / 4, ny), (unsigned)ny), dim3((unsigned)std::min<int64_t>((waves + 3) / 4, 1024), (unsigned)ny));
    });
}
// jtp_map's kernels one by one, over the grid.y records from `recs` on, and its decode over all records (jtp_map's own sweep, and
// jtp_marginal_map over JtMap records of its own: the cliques that sum nothing)
void map_collect_launch(int dtype, const JtMap *recs, const JtMapChild *kids, const JtMapWork &wk, dim3 grid, int n_vars, int n_rec, int cnt, int64_t entries, int64_t parts, hipStream_t s);
void map_merge_launch(const JtMap *recs, const JtMapWork &wk, dim3 mgrid, int n_rec, int cnt, int64_t entries, int64_t parts, hipStream_t s);
void map_decode_launch(const JtMap *recs, const int32_t *depth_begin, int n_depths, const JtMapWork &wk, size_t cnt, int n_vars, int n_rec, int64_t entries, hipStream_t s);
// from a set's downloaded maxima (by record; record 0 is the root) and its flag: whether the set failed, the sum of the exponents
// taken out of the messages, and log_value = log(raw_root) + ln 2 * that sum, summed as scale_from_exps does (-inf: failed)
struct MaxprodValue {
    bool failed;
    int64_t esum;
    double log_value;
};
static inline double maxprod_log(double root, int64_t esum) { return std::log(root) + 0.6931471805599453 * (double)esum; }
MaxprodValue maxprod_value(const unsigned long long *top, size_t n_rec, bool flagged);
