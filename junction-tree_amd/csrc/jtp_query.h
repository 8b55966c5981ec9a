// Internal header of the query units (jtp_sample.hip, jtp_map.hip, jtp_max.hip, jtp_mbest.hip, jtp_joint.hip, jtp_entropy.hip - the three
// max-product ones share more, in jtp_maxprod.h; jtp_engine.h includes it for the
// *Mem holders the plan keeps by value): their records, and what they share - how the digits of a clique's variables address its stored table
// (the one place outside the planner that knows how a compact mixed-radix row stores a variable), the walk of a lane over a block
// of a table's index, the staging of a clique's children, the launch shape.  No function here is told which query calls it.
#pragma once
#include <algorithm>

#include "jtp_device.h"
#include "jtp_plan.h"

#define JT_QUERY_KIDS 8          // children of a clique whose records a workgroup stages in LDS (the others are read where they lie)
#define JT_QUERY_SEG 1024        // entries of a segment (jtp_map: jtp_debug_set "map_seg" overrides it, tools/map_time.py)

// One variable of a record.  A digit's place in the stored table is linear in the digit - the `back` sum of jt_dev_to_host - in two
// parts for the variable across the thread part's top bit of a compact row (JtPackDesc::split_var):
// (digit mod 2^lb) * stride + (digit >> lb) * stride2; every other variable has lb = 31, stride2 = 0.
struct JtSampleVar {                 // 24 bytes
    int32_t col;                     // column of the state row (variable id)
    int32_t card;
    uint32_t stride, stride2;        // device element strides
    int32_t lb;
    uint32_t radix;                  // the variable's C-order weight in the index it is a digit of (the records below say which)
};

// jtp_sample: one record per clique of the sampling schedule (SampleClique), read by the kernel jt_sample_level as it stands.  The
// conditioning variables come first, then the drawn ones, both in host axis order; `radix` of a drawn variable: the product of the
// cardinalities of the drawn variables behind it.
struct JtSample {
    int64_t bel_off;                 // element offset of the clique's table in the belief arena
    int32_t nK, nF;
    uint32_t R;                      // entries of one slice: product of the cardinalities of the drawn variables
    int32_t clique;                  // C-ABI clique number: the random stream's key
    int32_t ord;                     // place in the visit order (the failure report keeps the smallest)
    int32_t pad;
    JtSampleVar v[JT_MAX_VARS];      // [0, nK): conditioning; [nK, nK + nF): drawn
};
// what jtp_sample keeps with the plan: the records (HostPlan::sample, visit order, built once), the state rows of one chunk of
// samples (int32[rows][n_vars], grow-only, reused chunk after chunk) and the failure report (count, smallest visit-order place)
struct SampleMem {
    DeviceBuf<JtSample> recs;
    DeviceBuf<int32_t> states;
    DeviceBuf<unsigned long long> fail;
    explicit SampleMem(MemLedger *m) : recs(m), states(m), fail(m) {}
};

// jtp_map: one record per clique of the sampling schedule (HostPlan::sample, visit order), read by the kernels as it stands.
// v[0, nK): the variables shared with the parent clique, `radix` their C-order weight in the clique's raw / arg table of nk
// entries; v[nK, nK + nF): the others, `radix` their weight in r.  A clique of many entries per k is cut into `nseg` contiguous
// segments of r, a wave each, whose (max, first r) jt_map_merge puts together: the result does not depend on the cut.
struct JtMap {
    int64_t psi_off;                 // element offset of the clique's table in the potential arena
    int64_t raw_off;                 // the clique's place in a set's raw / arg tables (entries)
    int64_t part_off;                // ... and, nseg > 1, in a set's tables of segment results (entry k * nseg + seg)
    int32_t nK, nF;
    uint32_t R, nk;                  // products of the cardinalities of F and of K
    uint32_t nseg;
    int32_t ord;                     // place in the visit order: the slot of the clique's maximum
    int32_t child_begin, child_end;  // the clique's children: a range of the JtMapChild array
    JtSampleVar v[JT_MAX_VARS];
};
struct JtMapChild {
    int64_t raw_off;                 // the child's place in a set's raw table
    int32_t ord;                     // the child's record
    int32_t down;                    // jtp_max_marginals: 1 = the input is the clique's own downward table D (down tables are laid out as raw ones); jtp_map: 0
    uint32_t stride[JT_MAX_VARS];    // per variable v[j] of the PARENT's record: its weight in the child's k (0: not shared with the child)
};
// what jtp_map keeps with the plan: the records (built once) and the work area of one chunk of evidence sets (grow-only) - per set
// the raw and arg tables, the segment results, the cliques' maxima as bit patterns, the evidence row, the state row, a flag
struct MapMem {
    DeviceBuf<JtMap> recs;
    DeviceBuf<JtMapChild> kids;
    DeviceBuf<int32_t> depth_begin;  // records [depth_begin[d], depth_begin[d + 1]) are depth d
    DeviceBuf<char> work;
    int64_t sets = 0;                // evidence sets `work` has room for
    int64_t entries = 0, parts = 0;  // per set: raw / arg entries, segment results
    std::vector<int64_t> depth_items;    // per depth: most (k, segment) pairs of a clique
    std::vector<char> depth_merge;       // ... and whether some clique there is cut into segments
    explicit MapMem(MemLedger *m) : recs(m), kids(m), depth_begin(m), work(m) {}
};

// jtp_marginal_map: the records of a query, read by jtp_map's kernels and by jt_mmap_level.  A record is a JtMap whose F is cut in
// two - v[0, nK): K; v[nK, nK + nF): FM, the clique's own variables that are maximised, `radix` their weight in rm (R = Rm, nseg its
// segments); v[nK + nF, nK + nF + nS): FS, those that are summed, `radix` their weight in rs - with a JtMmapExt beside it.  Inside a
// depth the cliques with Rs = 1 come first: jtp_map's kernels take those as they stand.  A child's stride[] covers all three parts.
struct JtMmapExt {
    int64_t spart_off;               // sseg > 1: the clique's place in a set's segment sums of its depth (entry (k * Rm + rm) * sseg + segment)
    int32_t nS;
    int32_t lanes;                   // lanes that share one (k, rm): min(64, Rs rounded up to a power of two)
    uint32_t Rs;                     // product of the cardinalities of FS
    uint32_t sseg;                   // contiguous segments the sum over rs is cut into, a wave each (jt_query_nseg of Rs alone)
};
// what jtp_marginal_map keeps with the plan: the records of the last query (`key`: the entries per segment of rm they were cut by,
// then the query sorted) and grow-only the work area of one chunk of evidence sets - jtp_map's (map_work), then the segment sums
struct MmapMem {
    struct Depth {
        int32_t a0 = 0, a1 = 0, b1 = 0;  // records [a0, a1): Rs = 1; [a1, b1): the others
        int64_t items_a = 0, items_b = 0;    // most waves of work a set gives a clique in jt_map_collect_level, in jt_mmap_level
        int64_t items_s = 0;             // ... and in jt_mmap_merge (0: no sum of the depth is cut)
        char merge = 0;                  // some clique's rm is cut into segments: jt_map_merge
    };
    DeviceBuf<JtMap> recs;
    DeviceBuf<JtMmapExt> ext;
    DeviceBuf<JtMapChild> kids;
    DeviceBuf<int32_t> depth_begin;
    DeviceBuf<char> work;
    std::vector<int32_t> key;
    int64_t entries = 0, parts = 0;      // per set: raw / arg entries, segment results of rm
    int64_t sparts = 0;                  // per set: segment sums of the depth that has most
    std::vector<Depth> depths;
    explicit MmapMem(MemLedger *m) : recs(m), ext(m), kids(m), depth_begin(m), work(m) {}
};

// jtp_max_marginals: one record per table the downward half of max-propagation forms by a maximum over a clique c's entries - the
// downward message to a child d of c (one per clique but the root, in the visit order of d) and a request (clique c, variables V).
// v[0, nK): the variables of the output - K_d with the weights raw_d has, or V in the requested order, C order -; v[nK, nK + nF):
// the clique's other variables in host axis order, `radix` their weight in r; all of them as clique c stores them (jt_query_var).
// The inputs are multiplied in list order: the clique's own downward table D_c first (JtMapChild::down; absent at the root), then
// the upward messages of the children of c in ascending clique number - all of them for a request, all but d for the message to d.
// An input's stride[j] is the weight of v[j] in that table's index.  Segments as for JtMap.
struct JtMax {
    int64_t psi_off;                 // element offset of the table of clique c in the potential arena
    int64_t out_off;                 // ord >= 0: the place of D_d in a set's down tables (= raw_off of d); else the request's place in a set's outputs
    int64_t part_off;                // nseg > 1: place in a set's segment results (entry k * nseg + seg)
    int32_t nK, nF;
    uint32_t R, nk;                  // products of the cardinalities of F and of K
    uint32_t nseg;
    int32_t ord;                     // the record of d - the slot of the largest entry of rawdn_d - or -1: a request
    int32_t in_begin, in_end;        // the inputs: a range of a JtMapChild array
    JtSampleVar v[JT_MAX_VARS];
};
// what jtp_max_marginals keeps with the plan, grow-only: the downward records (built once), the records of the last request list and
// that list (n, cliques, var_off, var_ids), and the work area of one chunk of evidence sets - jtp_map's (raw, arg, maxima, evidence
// rows, flags), then the down tables, the maxima of theirs, the segment results and the request outputs
struct MaxMem {
    DeviceBuf<JtMax> down, req;
    DeviceBuf<JtMapChild> down_in, req_in;
    DeviceBuf<char> work;
    bool built = false;              // `down` holds the plan's records (a tree of one clique has none)
    std::vector<int32_t> key;        // the request list `req` was made from
    std::vector<int64_t> req_out;    // [n + 1]: the requests' places in a set's outputs
    int64_t down_parts = 0, req_parts = 0;       // per set: segment results of the downward records, of the requests
    int64_t req_items = 1;               // most (entry, segment) pairs of a request
    char req_merge = 0;                  // ... and whether some request is cut into segments
    std::vector<int64_t> depth_items;    // per depth >= 1 (entry d - 1): most (k, segment) pairs of a message into that depth
    std::vector<char> depth_merge;
    explicit MaxMem(MemLedger *m) : down(m), req(m), down_in(m), req_in(m), work(m) {}
};

// what jtp_map_best keeps with the plan beside jtp_map's records (which it reads as they stand), grow-only: the work area of one
// evidence set - per assignment of K_c a list of `cap` values and as many places (r, t), the same per segment result, the cliques'
// maxima, the evidence row, and per solution a state row, the rank it takes of every clique's list and the fold's back-pointers
struct MbestMem {
    DeviceBuf<char> work;
    explicit MbestMem(MemLedger *m) : work(m) {}
};

// jtp_joint: one record per ACTIVE clique of a query (the cliques on the paths from the query variables' homes up to the top), in
// visit order - the top first - built and uploaded per call.  v[0, nK): the variables shared with the parent clique, `radix` their
// C-order weight in k; v[nK, nK + nQ): the query variables whose home the clique is (their digits come from x);
// v[nK + nQ, nK + nQ + nF): the clique's other variables in host axis order, `radix` their weight in r'.  f[0, nFs): ALL variables
// the clique does not share with its parent, host axis order, `radix` their weight in r - what sigma sums over.  x[0, nX): the
// query variables whose home lies in the clique's subtree, in the order of the query, `radix` their C-order weight in x; `slot` the
// place in v of one whose home is this clique, -1 for one carried up from a child.  The top has nK = 0: the variables it shares
// with its parent are among its "other" variables, summed over.
#define JT_JOINT_MAXQ 16         // query variables of a call
struct JtJointX {
    int32_t card;
    uint32_t radix;
    int32_t slot;
    int32_t pad;
};
struct JtJoint {
    int64_t bel_off;                 // element offset of the clique's table in the belief arena
    int64_t sig_off, msg_off;        // places of sigma_c[nk] and of M_c[nk * X] in the work area (doubles); the top: msg_off = the result's
    int64_t part_off;                // nseg > 1: place of the segment sums (entry (k * X + x) * nseg + segment)
    int32_t nK, nQ, nF, nFs, nX;
    int32_t lanes;                   // lanes that share one output entry: min(64, R' rounded up to a power of two)
    uint32_t R, Rp, nk, X;           // prod card of f (R_c), of the "other" variables (R'_c), of K_c, of x (C_c)
    uint32_t nseg;                   // contiguous segments the sum over r' is cut into, a wave each (a function of R'_c alone)
    int32_t ord;                     // place in the visit order of the sampling schedule (the failure report keeps the smallest)
    int32_t top;
    int32_t child_begin, child_end;  // the clique's ACTIVE children, ascending clique number: a range of the JtJointChild array
    JtSampleVar v[JT_MAX_VARS];
    JtSampleVar f[JT_MAX_VARS];
    JtJointX x[JT_JOINT_MAXQ];
};
struct JtJointChild {
    int64_t msg_off;                 // the child's M in the work area
    uint32_t stride[JT_MAX_VARS];    // per variable v[j] of the PARENT's record: its weight in the child's message index (0: not in K_d)
    uint32_t xstride[JT_JOINT_MAXQ]; // per x[i] of the parent's record: its weight there (0: not carried by this child)
};
// what jtp_joint keeps with the plan, grow-only: the records of the last call (JtJoint, then JtJointChild) and the work area - the
// failure report (count, smallest visit-order place, the top's flag), every sigma, M and segment sum, the result
struct JointMem {
    DeviceBuf<char> recs;
    DeviceBuf<double> work;
    explicit JointMem(MemLedger *m) : recs(m), work(m) {}
};

// jtp_entropy: one record per clique of the sampling schedule (HostPlan::sample, visit order), read by the kernels as it stands.
// v[0, nK): the variables shared with the parent clique, host axis order, `radix` their C-order weight in k; v[nK, nK + nF): the
// others in ASCENDING DEVICE STRIDE, the first the fastest digit of r (`radix` 1): the `lanes` lanes that share a k take r = l,
// l + lanes, ..., so on a power-of-two layout whose low strides are F's a wave reads consecutive elements.  step[j]: digit j of
// `lanes` in that mixed radix, what one turn of a lane adds to its counter ([step_lo, step_hi): the digits that are not zero).
struct JtEntropy {
    int64_t bel_off;                 // element offset of the clique's table in the belief arena
    int64_t k_off;                   // the clique's place in a set's per-k sums (entry k)
    int64_t part_off;                // nseg > 1: ... and in a set's segment sums (entry k * nseg + segment)
    int32_t nK, nF;
    uint32_t R, nk;                  // products of the cardinalities of F and of K
    uint32_t nseg;                   // contiguous segments r is cut into, a wave each (jt_query_nseg)
    int32_t lanes;                   // lanes that share a (k, segment): min(64, R rounded up to a power of two)
    int32_t clique;                  // C-ABI clique number
    int32_t step_lo, step_hi;
    int32_t pad;
    JtSampleVar v[JT_MAX_VARS];
    int32_t step[JT_MAX_VARS];
};
// what jtp_entropy keeps with the plan: the records (built once), and grow-only the work area of one chunk of evidence sets - per
// set the two belief arenas' addresses, per (set, clique) four words of result (t(a,a), t(a,b), S, flags), and per set the per-k
// and the segment sums, two doubles an entry without a reference set and four with one
struct EntropyMem {
    DeviceBuf<JtEntropy> recs;
    DeviceBuf<double> work;
    int64_t entries = 0, parts = 0;  // per set: per-k entries, segment results
    int64_t max_items = 1;           // most (k, segment) pairs x lanes of a clique
    explicit EntropyMem(MemLedger *m) : recs(m), work(m) {}
};

// ------------------------------------------------------------------------------------------ host: records and launch shape

// variable `v` of clique `clique` as the kernels address it; `radix` is the caller's to set (1 here)
static inline JtSampleVar jt_query_var(const HostPlan &hp, int clique, int v) {
    const JtPackDesc &d = hp.pack[clique];
    int i_host = 0;                  // the variable's place in the clique's host axis order: the index into the pack record
    while (hp.node_vars[clique][i_host] != v) ++i_host;
    JtSampleVar sv;
    sv.col = v;
    sv.card = d.card[i_host];
    sv.stride = d.dstride[i_host];
    sv.stride2 = 0;
    sv.lb = 31;
    if (d.row_elems > 0 && i_host == d.split_var) sv.lb = d.split_lb, sv.stride2 = d.split_ds2;
    sv.radix = 1;
    return sv;
}

// segments the n entries behind one output are cut into, a wave each: from two segments' worth on, segments of `seg` entries or more
static inline uint32_t jt_query_nseg(uint32_t n, uint32_t seg) { return n >= 2u * seg ? std::min<uint32_t>(4096u, n / seg) : 1u; }
// grid.x of a grid-stride launch that has work for `want` workgroups per record, `ny` records in blockIdx.y
static inline unsigned jt_query_grid_x(int64_t want, size_t ny) { return (unsigned)std::min<int64_t>(want, std::max<int64_t>(64, 32768 / (int64_t)ny)); }
// a run of n consecutive records in slices that fit blockIdx.y: fn(first record of the slice, records in it)
template <typename Fn>
static inline void jt_query_slices(size_t n, Fn &&fn) {
    for (size_t y0 = 0; y0 < n; y0 += 65535) fn(y0, std::min<size_t>(65535, n - y0));
}
// the float / double instantiation of a kernel template, as the plan's dtype asks, 256 threads a workgroup: the arguments are the
// kernel's, written out at the call, and `T` in them is the table type (`(const T *)b.bel`)
#define JT_QUERY_LAUNCH(dtype, kernel, grid, stream, ...)                                                                       \
    do {                                                                                                                        \
        if ((dtype) == JTP_F32) { using T = float; hipLaunchKernelGGL(kernel<T>, grid, dim3(256), 0, stream, __VA_ARGS__); }    \
        else { using T = double; hipLaunchKernelGGL(kernel<T>, grid, dim3(256), 0, stream, __VA_ARGS__); }                      \
    } while (0)

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------ device: the table walk
// element offset of digit `digit` of a variable in a stored table
__device__ __forceinline__ uint32_t jt_sample_at(const JtSampleVar &v, int digit) {
    return ((uint32_t)digit & ((1u << v.lb) - 1u)) * v.stride + ((uint32_t)digit >> v.lb) * v.stride2;
}
// n records of a clique's variables into LDS, by the workgroup's 256 threads (the barrier is the caller's)
__device__ __forceinline__ void jt_query_stage_vars(JtSampleVar *lds, const JtSampleVar *v, int n, int tid) {
    for (int i = tid; i < n * (int)(sizeof(JtSampleVar) / 4); i += 256) ((int32_t *)lds)[i] = ((const int32_t *)v)[i];
}
// [lo, end) in one contiguous block per lane: lane `sub` of `lanes` takes [a, e), B = ceil((end - lo) / lanes) entries or none
struct JtQueryCut { uint32_t a, e, B; };
__device__ __forceinline__ JtQueryCut jt_query_cut(uint32_t lo, uint32_t end, uint32_t lanes, uint32_t sub) {
    const uint32_t B = (end - lo + lanes - 1u) / lanes, a = min(lo + sub * B, end);
    return {a, min(a + B, end), B};
}

// The walk of thread `tid` over a block of the C-order index of fv[0, nF): a mixed-radix counter whose digit j is digs[j][tid] (`digs`:
// the first of the walk's nF rows; a column per thread, no barrier needed) moves the table offset.  jt_map_collect_level does not
// use these two: it keeps a count of the digits that contradict the evidence with them, and neither way of sharing them - the
// count handed in as a callable, or formed in a loop of its own behind the start - left the kernel's code as it was; the build
// that was timed took 4 % longer over 64 evidence sets (profiles/query_units_resources.txt, query_units_ab.txt).  So its start
// and advance are written out there; how a digit moves the offset is jt_sample_at's to say, which that copy calls too.
// Start at index `a`: the offset there ...
__device__ __forceinline__ uint32_t jt_query_walk_start(const JtSampleVar *fv, int nF, int (*digs)[256], int tid, uint32_t a) {
    uint32_t off = 0;
    for (int j = 0; j < nF; ++j) {
        const int dg = (int)((a / fv[j].radix) % (uint32_t)fv[j].card);
        digs[j][tid] = dg;
        off += jt_sample_at(fv[j], dg);
    }
    return off;
}
// ... and on to the next assignment in C order: the offset there
__device__ __forceinline__ uint32_t jt_query_walk_next(const JtSampleVar *fv, int nF, int (*digs)[256], int tid, uint32_t off) {
    for (int j = nF - 1; j >= 0; --j) {
        const JtSampleVar v = fv[j];
        const int dg = digs[j][tid];
        if (dg + 1 < v.card) {
            off += jt_sample_at(v, dg + 1) - jt_sample_at(v, dg);
            digs[j][tid] = dg + 1;
            break;
        }
        off -= jt_sample_at(v, dg);
        digs[j][tid] = 0;
    }
    return off;
}

// A clique's children.  A child's table is indexed by digits of the PARENT's variables: Kid::stride[j] is the weight of the parent's
// v[j] there.  The strides of the first JT_QUERY_KIDS of the clique's n_kids children are staged in LDS once per workgroup (no
// barrier here); returns how many that is ...
template <typename Kid>
__device__ __forceinline__ int jt_query_stage_kids(uint32_t (*kstride)[JT_MAX_VARS], const Kid *kids, int n_kids, int tid) {
    const int n_staged = min(n_kids, JT_QUERY_KIDS);
    for (int i = tid; i < n_staged * JT_MAX_VARS; i += 256) kstride[i / JT_MAX_VARS][i % JT_MAX_VARS] = kids[i / JT_MAX_VARS].stride[i % JT_MAX_VARS];
    return n_staged;
}
// ... where the index is summed in two parts, what the digits fixed during a walk decide and the walked ones on top of it:
// at + sum over j0 <= j < j1 of digs[j][tid] * stride[j] ...
__device__ __forceinline__ uint32_t jt_query_kid_at(uint32_t at, const uint32_t *stride, int (*digs)[256], int tid, int j0, int j1) {
    for (int j = j0; j < j1; ++j) at += (uint32_t)digs[j][tid] * stride[j];
    return at;
}
// ... and a child beyond the staged ones is read where it lies, all nv digits at once
template <typename Kid>
__device__ __forceinline__ uint32_t jt_query_kid_at(const Kid &kid, int (*digs)[256], int tid, int nv) {
    uint32_t at = 0;
    for (int j = 0; j < nv; ++j) {
        const uint32_t st = kid.stride[j];
        if (st) at += (uint32_t)digs[j][tid] * st;
    }
    return at;
}
#endif
