// Internal header of the three max-product units - jtp_map.hip (jtp_map: the most probable assignment), jtp_max.hip (jtp_max_marginals:
// max-propagation) and jtp_mbest.hip (jtp_map_best: the M most probable assignments) - and of nothing else: what they share.  All
// three sweep the sampling schedule upward over the clique potentials, every message scaled by the exponent of its largest entry:
// the work area and the maxima of that sweep, and the host steps of an entry point, which jtp_map.hip defines once.  The level
// kernels keep the set-up of a wave's item as their own text: drawn from functions here it compiled to other instruction streams
// (7 to 19 of about 2200 instructions fewer, a tenth of the lines elsewhere) at no fewer lines of source.  No function here is told
// which query calls it.
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

// ------------------------------------------------------------------------------------------ host: the steps of an entry point (jtp_map.hip)

// what every entry point refuses, under the name `fn`: a multi-set plan, several ranks, a clique without a table, a bad batch range
int maxprod_refuse(const char *fn, const HostPlan &hp, int32_t batch_begin, int32_t batch_end);
// entries per segment of r: jtp_debug_set "map_seg", else JT_QUERY_SEG
uint32_t maxprod_seg(const jtp_plan *pl);
// ord_of[clique]: the clique's place in the visit order, its record
std::vector<int> map_ord_of(const HostPlan &hp);
// The plan's upward records (jtp_map's, which all three sweep over): if it has none, built into `fresh` and uploaded (the caller moves
// `fresh` into the plan once nothing can fail any more).  `recs` and `kids`, if given, get them on the host, built even where the plan has them.
int map_upward_records(jtp_plan *pl, MapMem &fresh, std::vector<JtMap> *recs = nullptr, std::vector<JtMapChild> *kids = nullptr);
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
// the upward launches over `sets` evidence sets, deepest depth first: launch(first record of the slice, the two grids, whether the depth needs the merge)
template <typename Launch>
static inline void maxprod_upward(const HostPlan &hp, const MapMem &up, size_t sets, Launch &&launch) {
    for (int d = (int)hp.sample_depths.size() - 1; d >= 0; --d) {
        const std::vector<int> &level = hp.sample_depths[d];
        maxprod_slices(level.size(), (int64_t)sets * up.depth_items[d],
                       [&](size_t y0, dim3 grid, dim3 mgrid) { launch(up.recs.get() + level[0] + y0, grid, mgrid, up.depth_merge[d] != 0); });
    }
}
// jtp_map's upward sweep (jt_map_collect_level, jt_map_merge) over the `cnt` sets staged in `wk`
void map_upward_sweep(const HostPlan &hp, const MapMem &up, const JtMapWork &wk, size_t cnt, hipStream_t s);
// from a set's downloaded maxima (by record; record 0 is the root) and its flag: whether the set failed, the sum of the exponents
// taken out of the messages, and log_value = log(raw_root) + ln 2 * that sum, summed as scale_from_exps does (-inf: failed)
struct MaxprodValue {
    bool failed;
    int64_t esum;
    double log_value;
};
static inline double maxprod_log(double root, int64_t esum) { return std::log(root) + 0.6931471805599453 * (double)esum; }
MaxprodValue maxprod_value(const unsigned long long *top, size_t n_rec, bool flagged);
