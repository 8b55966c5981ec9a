// Internal header of the engine's translation units (not installed): what they share.
//   jtp_engine.hip     errors, host memory, device queries, plan creation and destruction, zero_padding, jtp_debug_*
//   jtp_upload.hip     potentials in (pack, evaluate, synthetic fill), evidence, the active lists of multi-set plans
//   jtp_propagate.hip  kernel tables and the one launch path, the flight board, jtp_propagate, jtp_sync, check_flow / settle
//   jtp_readout.hip    beliefs, marginals, scale / Z / log Z, expected counts
//   jtp_sample.hip     jtp_sample: joint posterior samples from the beliefs a propagate left        (these three: the queries on the sampling
//                      schedule; jtp_query.h has their records and the table walk, child staging and launch shape they share)
//   jtp_map.hip        jtp_map: the most probable assignment (max-product sweep over the potentials)     (these three: the max-product
//   jtp_max.hip        jtp_max_marginals: max-propagation                                                units; jtp_maxprod.h has the work
//   jtp_mbest.hip      jtp_map_best: the M most probable assignments                                     area and the host steps they share)
//   jtp_mmap.hip       jtp_marginal_map: the most probable assignment of some variables, the others summed (jtp_sweep.h: the upward
//                      sweep's work area and host steps, which it shares with the three above; jtp_map's kernels, and its own)
//   jtp_joint.hip      jtp_joint: the joint of variables of different cliques, from the beliefs a propagate left
//   jtp_entropy.hip    jtp_entropy: posterior entropy and cross-entropy against another evidence set, one streaming pass over all beliefs
//   jtp_profile.cpp    profiling, regions, statistics;    jtp_comm.cpp   RCCL and roctx loaders, jtp_comm_*, the exchange steps
// Every global has one definition, in the unit that owns it; the other units reach it through the functions declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

#include "jtp_device.h"
#include "jtp_plan.h"
#include "jtp_query.h"

// ------------------------------------------------------------------------------------------ errors (jtp_engine.hip)

int set_err(int code, const char *fmt, ...);

// the one failure path of HIP calls and of the buffers of jtp_device.h: out of memory is JTP_ENOMEM (the Python layer evicts
// cached plans and tries again on that), everything else JTP_EHIP
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return set_err(_e == hipErrorOutOfMemory ? JTP_ENOMEM : JTP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// ------------------------------------------------------------------------------------------ RCCL, roctx (jtp_comm.cpp)

struct jtp_plan;
struct BatchBuffers;
namespace rccl {
int size();                     // ranks of the communicator jtp_comm_init made; 0: there is none
int rank();                     // ... and this process's rank in it
// the exchange step `st` of a sharded propagate of evidence set `bb`, on stream `s` (real, or JTP_FAKE_COMM=2: loop-back)
int exchange_step(jtp_plan *pl, BatchBuffers &bb, const JtFlow &fl, const Step &st, hipStream_t s);
}  // namespace rccl

namespace roctx {
void load();
struct Range {                  // a named range while the object lives (plans created with JTP_ROCTX=1; else a no-op)
    bool on;
    Range(bool enabled, const char *name);
    ~Range();
};
}  // namespace roctx

// ------------------------------------------------------------------------------------------ plan object

// Evidence-free subtrees (rounds 5-6).  Arena slot 0 of a multi-set plan holds a set that observes nothing.  The upward message of a
// clique below which a set observes nothing IS slot 0's: the set is not on that collect task's active list (JtFlow::act_ids), consumers
// and the read-out take the message from slot 0 (JtFlow::skip / jtp_readout.hip readout_redirect), and the set's own entries of it stay
// "unwritten" in both arena halves - which jt_multi_fanout (jtp_upload.hip) restores, once, for the (task, set) pairs that LEAVE a list when the evidence changes.
#define JT_FANOUT_RESET 0x20000000
struct JtFanout {
    int64_t off;               // msg-arena offset (doubles) of the entries
    int32_t count;             // doubles
    int32_t flags;             // JT_FANOUT_RESET: the entries of BOTH arena halves of the listed slots become "unwritten"
    uint16_t slot[JT_MSETS];   // the arena slots concerned (0xffff: none)
};

// Memory ownership: the plan owns every allocation (jtp_plan: SetMem per evidence set, the *_all arenas of multi-set plans, the
// tables); BatchBuffers holds plain views of them, set ONCE in jtp_plan_create - where the aliasing is decided (shared psi / fix
// under JTP_SHARE_POTENTIALS, slices of msg_all / ev_all / sync_all in multi-set plans) - and read by the launch code.
struct BatchBuffers {
    void *psi = nullptr;
    void *bel = nullptr;
    double *msg = nullptr;
    double *fix = nullptr;          // fixed arena: the static tables of unit cliques (HostPlan::statics; shared like psi)
    uint32_t *ev = nullptr;         // hard evidence: (mask, value) per planner node, or null (jtp_set_evidence)
    bool ev_any = false;            // ... and it observes something: the kernels get a null table otherwise (single-set plans: the lean
                                    // unit pass takes that for "no evidence anywhere", jt_unit_collect)
    uint32_t *sync = nullptr;       // dataflow launches: abort flag and ticket counters
    // JTP_SCALED plans: log2 of the power of two every message of the last propagate was divided by (slot 2 * psep: upward,
    // + 1: downward), rewritten by every propagate (jt_rescale_level); on the host, once a read-out asks: the exponent E of
    // every planner node and separator - what the device holds for it is the true table x 2^-E (fetch_scale)
    int32_t *exps = nullptr;
    bool scale_fresh = false;
    std::vector<int64_t> node_e, sep_e;
    uint32_t epoch = 0;             // propagates enqueued so far; its parity selects the message arena half
    uint32_t flow_runs = 0;         // of which dataflow
    uint32_t ticket_runs = 0;       // of which in ticket order: the segments' ticket counters only grow, by one launch's workgroups
                                    // per such run (NOT per dataflow run: a plan changes between blockIdx and ticket order as other
                                    // plans come and go)
    bool unchecked = false;         // a dataflow propagate was enqueued and its abort flag not looked at yet
    int64_t cur_off(int64_t half) const { return (epoch & 1u) ? half : 0; }     // half in use by the last propagate
    // JtFlow::fix_shift of a launch that reads this propagate's half: fixed arena - (message arena + cur_off), in doubles
    int64_t fix_shift(int64_t cur) const { return fix ? (int64_t)(((intptr_t)fix - (intptr_t)msg) / 8) - cur : 0; }
};

// device tables of one list of marginal requests (jtp_get_marginals), kept for the next call
struct MargBatch {
    int lean_nblocks = 0, lean_lds = 0;  // the first workgroups of the unit list have a lean record (jt_lean_single)
    // the list is the one the plan was made with (jtp_tree_desc.fold_*) and every request on a clique without a table was folded into
    // the propagate: `d_descs_fold` says where the propagate left them; the unit launches are then skipped (jtp_get_marginals)
    bool folded = false;
    DeviceBuf<JtMargDesc> d_descs_fold;
    std::vector<JtTask> h_tasks;         // multi-set plans with active lists: the records as planned (readout_redirect patches copies of them)
    std::vector<int32_t> key;            // n, cliques, var_off, var_ids
    DeviceBuf<JtTask> d_tasks;
    DeviceBuf<JtBlock> d_blocks;
    DeviceBuf<int> d_itab;
    DeviceBuf<JtMargDesc> d_descs;
    DeviceBuf<double> scratch, stage;
    int n = 0, nblocks = 0, lds = 0, max_grid_x = 1;
    // requests on UNIT cliques (no belief table): psi x every incoming table marginalised directly (kernel jt_single); their
    // workgroup records follow the others' in d_blocks
    int unit_nblocks = 0, unit_lds = 0;
    int64_t total_out = 0;
    std::vector<int64_t> elems;          // host entries of each request
    // jtp_accumulate_marginals (the list then ends with the root's scalar): `slots` slots as large as `scratch`, one per evidence
    // set of a chunk; the patched task records of every slot (lists with h_tasks); per slot the requests' entries, laid out as
    // `stage`, and S per (slot, request); the weights of the range; and what goes back to the host - the accumulators, the root
    // sum of every set of the range, the bad-pair report (count, first set * n + request).  Grow-only, replaced together.
    struct Acc {
        DeviceBuf<double> scratch, entries, sums, weights, out;
        DeviceBuf<JtTask> tasks;
        int64_t slots = 0, range = 0;
        explicit Acc(MemLedger *m) : scratch(m), entries(m), sums(m), weights(m), out(m), tasks(m) {}
    } acc;
    explicit MargBatch(MemLedger *m) : d_descs_fold(m), d_tasks(m), d_blocks(m), d_itab(m), d_descs(m), scratch(m), stage(m), acc(m) {}
};

// what one evidence set of a single-set plan owns (multi-set plans: entry 0 holds the shared psi and the belief scratch)
struct SetMem {
    DeviceBuf<char> psi, bel;
    DeviceBuf<double> msg, fix;
    DeviceBuf<uint32_t> ev, sync;
    DeviceBuf<int32_t> exps;
    explicit SetMem(MemLedger *m) : psi(m), bel(m), msg(m), fix(m), ev(m), sync(m), exps(m) {}
};

struct jtp_plan {
    MemLedger mem;                  // (first: every buffer below books with it, and is destroyed before it)
    HostPlan hp;
    bool device = false;
    bool widened = false;           // asked for float32 tables, made with float64 ones (jtp_plan_create)
    bool inflight = false;          // counted in g_inflight: a dataflow propagate of this plan may still be running
    int launch_mode = 0;            // of the last propagate: 0 one launch per level, 1 dataflow in blockIdx order, 2 dataflow, ticket order
    int tickets_used = 0;           // propagates (per evidence set) that ran in ticket order
    int foreign_seen = 0;           // propagates that found ANOTHER PROCESS with a dataflow propagate in flight on the device
    double device_bytes = 0;        // mem.bytes at the end of jtp_plan_create: everything the plan holds from then on
    int64_t half = 2;               // doubles per half of a message arena (cur_half)
    int flow_propagates = 0;        // propagates (per evidence set) that ran as dataflow launches
    uint32_t flow_debug = 0;        // JTP_FLOW_DEBUG at plan creation, or jtp_debug_set(plan, "flow_debug", v)
    bool env_tickets = false;       // JTP_FLOW_TICKETS at plan creation
    bool roctx = false;             // JTP_ROCTX at plan creation: named ranges around the phases of a propagate
    // multi-set plans (JTP_MULTISET): evidence sets in groups of JT_MSETS, one allocation each for all sets'
    // message arenas, evidence tables and sync areas (bufs[b] point into them; bufs[b].psi/.bel are shared)
    bool multiset = false;
    int n_groups = 0;
    DeviceBuf<double> msg_all{&mem};
    DeviceBuf<uint32_t> ev_all{&mem}, sync_all{&mem};
    int64_t set_stride = 0;         // doubles between consecutive sets' arenas (both halves)
    uint32_t ev_stride = 0;         // uint32 per set's evidence table
    // read-out of multi-set plans: belief task of each clique, built on first use
    std::vector<uint32_t> ev_host;  // host copy of ev_all (which tasks may sum their elements first depends on it)
    // evidence-free subtrees: the first JT_MSETS arena slots are not the caller's (the caller's set b is slot set0 + b); slot 0 runs
    // every collect task without evidence, and a set takes from it the upward message of every clique below which it observes nothing
    int set0 = 0;
    // Round 6: per TASK, not per group - the active list of a collect task holds the arena slots of the sets that observe something below
    // its clique (slot 0, the evidence-free set, first); the list of a downward task every caller's slot (rebuild_active).
    std::vector<uint8_t> member_host;     // [task * cap + slot] != 0: the slot is on the task's list
    std::vector<uint16_t> act_ids_host;   // [task * cap + j]
    std::vector<int32_t> act_n_host;      // [task]
    std::vector<uint8_t> esum_oct_host;   // [task * n_groups + g]: entries 8 g .. 8 g + 7 of the list observe nothing on the clique's element bits
    DeviceBuf<uint8_t> d_member{&mem}, d_esum_oct{&mem};
    DeviceBuf<uint16_t> d_act_ids{&mem};
    DeviceBuf<int32_t> d_act_n{&mem};
    bool act_dirty = false;
    DeviceBuf<JtFanout> d_fanout{&mem};       // (grow-only)
    int n_fanout = 0;
    struct BeliefTask {
        DeviceBuf<JtTask> d_task;
        DeviceBuf<JtBlock> d_blk;
        DeviceBuf<int> d_tab;
        int nblocks = 0, lds = 0;
        JtTask h_task;
        explicit BeliefTask(MemLedger *m = nullptr) : d_task(m), d_blk(m), d_tab(m) {}
    };
    std::vector<BeliefTask> belief_tasks;
    std::vector<hipStream_t> streams;
    std::vector<SetMem> set_mem;
    std::vector<BatchBuffers> bufs;
    DeviceBuf<JtTask> d_tasks{&mem};
    DeviceBuf<JtBlock> d_blocks{&mem};
    DeviceBuf<JtBlock> d_init[2] = {DeviceBuf<JtBlock>(&mem), DeviceBuf<JtBlock>(&mem)};      // HostPlan::init_blocks on the device (mixed-radix plans)
    DeviceBuf<JtRescale> d_rescale{&mem};         // HostPlan::rescale on the device (JTP_SCALED plans)
    DeviceBuf<int> d_itab{&mem};
    DeviceBuf<char> stage{&mem};    // device staging buffer for host<->device conversion (grow-only)
    // uploads (jtp_set_potential): two device staging buffers used in turn, an event each - a call waits only for
    // the pack kernel that last read ITS buffer (two calls back), not for the stream
    DeviceBuf<char> up_stage[2] = {DeviceBuf<char>(&mem), DeviceBuf<char>(&mem)};
    hipEvent_t up_ev[2] = {nullptr, nullptr};
    bool up_busy[2] = {false, false};
    unsigned up_cursor = 0;
    hipEvent_t region_ev[2] = {nullptr, nullptr};      // jtp_region_begin / jtp_region_end
    bool region_open = false;
    int prof_steps = 0;             // 0: off; else ring of this many event sets
    std::vector<hipEvent_t> ev;     // prof_steps x (2 per launch)
    int prof_cursor = 0;            // propagates recorded since profiling was switched on
    int prof_stride = 1;            // every how many propagates one is timed (jtp_set_profiling_stride)
    unsigned prof_calls = 0;        // propagates since profiling was switched on, timed or not
    bool prof_per_launch = false;   // event pair per launch instead of three per propagate
    bool flow = true;               // dataflow launches (one per phase) instead of one per level
    bool chain = false;             // the plan is made of latency-bound levels (JtTask::settle): distribute runs the build without spills
    bool marg_tasks = false;        // some marginal request was folded into the propagate (HostPlan::folded): jt_propagate_flow_marg
    PinnedBuf<uint32_t> host_abort{&mem};     // set by a workgroup that gave up waiting
    int flow_fallbacks = 0;         // times that happened (then: one launch per level from there on)
    int fake_comm = 0;              // JTP_FAKE_COMM: 1 = what a rank would receive is filled with ones, what it would send goes nowhere;
                                    // 2 = the exchange steps run as REAL RCCL groups in loop-back (every ncclSend / ncclRecv of the step
                                    // addressed to this rank itself, on the plan's stream, between the launches as in a sharded run)
    bool esum_dirty = false;        // multi-set plans: JtTask::esum_groups changed on the host since the last upload
    bool psi_dirty = false;         // shared potentials were written (on stream 0) since the last propagate
    std::vector<std::unique_ptr<MargBatch>> marg_cache;
    // factor tables and records on their way to jt_eval_batch: slices of one buffer handed out in turn, so that
    // evaluate calls following each other need no synchronisation until the buffer wraps
    DeviceBuf<char> eval_stage{&mem};    // device
    PinnedBuf<char> eval_host{&mem};     // pinned mirror of the same size: the caller's tables are copied here before the call returns
    size_t eval_cursor = 0;
    DeviceBuf<char> unit_scratch{&mem};  // scratch arena in which the belief of a unit clique is formed on demand (jtp_get_belief)
    SampleMem sample{&mem};         // jtp_sample: records, state rows, failure report
    // jtp_accumulate_marginals: an event per stream (the accumulation waits for the sets' formation launches), made on first use;
    // evidence sets per chunk as jtp_debug_set "acc_chunk" asks (0: as many as fit 64 MiB of partial copies)
    std::vector<hipEvent_t> acc_ev;
    int64_t acc_chunk = 0;
    // jtp_map: the observed state of every variable in every evidence set as jtp_set_evidence was last given it ([set * n_vars + v],
    // -1: not observed; empty: no call yet), the records and the work area, and the sets per chunk jtp_debug_set "map_chunk" asks
    // for (0: as many as fit 64 MiB)
    std::vector<int32_t> ev_obs;
    MapMem map{&mem};
    int64_t map_chunk = 0;
    int64_t map_seg = 0;            // jtp_debug_set "map_seg": entries per segment of r (0: JT_QUERY_SEG); setting it drops the records
    MaxMem maxm{&mem};              // jtp_max_marginals: downward and request records, work area (both knobs govern it too)
    MbestMem mbest{&mem};           // jtp_map_best: work area of one set (jtp_map's records; "map_seg" governs it too)
    MmapMem mmap{&mem};             // jtp_marginal_map: the records of the last query and the work area (both knobs govern it too)
    JointMem joint{&mem};           // jtp_joint: records and work area
    EntropyMem entropy{&mem};       // jtp_entropy: records and work area
    hipStream_t eval_stream = nullptr;   // stream whose kernels may still read the buffer
    bool eval_pending = false;
    int esize = 4;
};

// ------------------------------------------------------------------------------------------ helpers used across units

// offset of the message arena half the last propagate of the evidence set wrote
static inline int64_t cur_half(const jtp_plan *pl, const BatchBuffers &b) { return b.cur_off(pl->half); }

// workgroups of 256 threads of a grid-stride kernel over n elements
static inline int grid_1d(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 4096); }

#ifdef __HIPCC__
__device__ __forceinline__ uint64_t jt_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
#endif

// jtp_engine.hip
int check_ready(jtp_plan *pl, int batch);
int ensure_stage(jtp_plan *pl, size_t bytes);
int zero_padding(jtp_plan *pl, double *msg, int nsets, hipStream_t s, int halves = 3);
// jtp_upload.hip
void launch_virtual_fill(const HostPlan &hp, const JtPackDesc &d, void *psi, hipStream_t s);
int rebuild_active(jtp_plan *pl, hipStream_t s);
// jtp_propagate.hip
bool flow_both();
const void *kernel_fn(const HostPlan &hp, int variant);
const void *flow_fn(const jtp_plan *pl, int phase);
hipError_t raise_lds(const void *func, int bytes);
int launch_readout(jtp_plan *pl, int variant, int nblocks, int lds, hipStream_t s, const JtTask *tasks,
                   const JtBlock *blocks, const int *itab, void *psi, void *bel, double *msg, const JtFlow &fl);
void drop_flight(jtp_plan *pl);
int flight_board_state(int device);
int check_flow(jtp_plan *pl, int synced = -1);
int settle(jtp_plan *pl, int batch);
