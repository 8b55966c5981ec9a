// Internal header of the three max-product units - jtp_map.hip (jtp_map: the most probable assignment), jtp_max.hip (jtp_max_marginals:
// max-propagation) and jtp_mbest.hip (jtp_map_best: the M most probable assignments) - and of nothing else: what they share.  All
// three sweep the sampling schedule upward over the clique potentials, every message scaled by the exponent of its largest entry:
// the work area and the maxima of that sweep and the host steps of an entry point are in jtp_sweep.h (jtp_marginal_map runs the same
// sweep with a sum in it); here, jtp_map's upward records and sweep, which all three run as they stand.  The level
// kernels keep the set-up of a wave's item as their own text: drawn from functions here it compiled to other instruction streams
// (7 to 19 of about 2200 instructions fewer, a tenth of the lines elsewhere) at no fewer lines of source.  No function here is told
// which query calls it.
#pragma once
#include "jtp_sweep.h"

// ------------------------------------------------------------------------------------------ host: the steps of an entry point (jtp_map.hip)

// ord_of[clique]: the clique's place in the visit order, its record
std::vector<int> map_ord_of(const HostPlan &hp);
// The plan's upward records (jtp_map's, which all three sweep over): if it has none, built into `fresh` and uploaded (the caller moves
// `fresh` into the plan once nothing can fail any more).  `recs` and `kids`, if given, get them on the host, built even where the plan has them.
int map_upward_records(jtp_plan *pl, MapMem &fresh, std::vector<JtMap> *recs = nullptr, std::vector<JtMapChild> *kids = nullptr);
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
