// The propagate: which kernel runs a launch (KernelTable), the one path every message-passing launch takes, the count of dataflow
// propagates in flight on a device - in this process and, through the flight board, in the others - jtp_propagate and jtp_sync,
// and what follows a dataflow launch that gave up waiting (check_flow, settle).
#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "jtp_engine.h"
#include "jtp_kernels.hip.h"

// ------------------------------------------------------------------------------------------ kernels of a launch

static inline int mixk(const HostPlan &hp) { return hp.tmix ? (hp.tmix_compact ? 2 : 1) : 0; }

bool flow_both() {
    static const bool on = !(getenv("JTP_FLOW_BOTH") && atoi(getenv("JTP_FLOW_BOTH")) == 0);
    return on;
}

template <typename T>
struct KernelTable {
    typedef void (*fn)(const JtTask *, const JtBlock *, const int *, const T *, T *, double *, JtFlow);
    // (tmix: 0 no mixed-radix rows, 1 one row per step, 2 the compact form - two rows per step, HostPlan::tmix_compact: mixk())
    static fn get(int variant, int tmix) {
        if (tmix == 2) {
            if (variant >= JT_K_COLLECT0 && variant <= JT_K_COLLECT3) return jt_collect_level_mix<T, true>;
            if (variant >= JT_K_DIST_P0C0 && variant <= JT_K_DIST_P1C3) return jt_distribute_level_mix<T, true>;
            if (variant == JT_K_COLLECT_LEVEL) return jt_collect_level_mix<T, true>;
            if (variant == JT_K_DISTRIBUTE_LEVEL) return jt_distribute_level_mix<T, true>;
            if (variant == JT_K_SINGLE || variant == JT_K_MARGINALS) return jt_single_mix<T, true>;
        }
        if (tmix) {                 // plans with a mixed-radix thread part: one kernel per launch style (they dispatch on the task)
            if (variant >= JT_K_COLLECT0 && variant <= JT_K_COLLECT3) return jt_collect_level_mix<T, false>;
            if (variant >= JT_K_DIST_P0C0 && variant <= JT_K_DIST_P1C3) return jt_distribute_level_mix<T, false>;
            if (variant == JT_K_COLLECT_LEVEL) return jt_collect_level_mix<T, false>;
            if (variant == JT_K_DISTRIBUTE_LEVEL) return jt_distribute_level_mix<T, false>;
            if (variant == JT_K_SINGLE || variant == JT_K_MARGINALS) return jt_single_mix<T, false>;
        }
        switch (variant) {
            case JT_K_COLLECT0: return jt_collect<T, 0>;
            case JT_K_COLLECT1: return jt_collect<T, 1>;
            case JT_K_COLLECT2: return jt_collect<T, 2>;
            case JT_K_COLLECT3: return jt_collect<T, 3>;
            case JT_K_DIST_P0C0: return jt_distribute<T, 0, 0>;
            case JT_K_DIST_P0C1: return jt_distribute<T, 0, 1>;
            case JT_K_DIST_P0C2: return jt_distribute<T, 0, 2>;
            case JT_K_DIST_P0C3: return jt_distribute<T, 0, 3>;
            case JT_K_DIST_P1C0: return jt_distribute<T, 1, 0>;
            case JT_K_DIST_P1C1: return jt_distribute<T, 1, 1>;
            case JT_K_DIST_P1C2: return jt_distribute<T, 1, 2>;
            case JT_K_DIST_P1C3: return jt_distribute<T, 1, 3>;
            case JT_K_COLLECT_LEVEL: return jt_collect_level<T>;
            case JT_K_DISTRIBUTE_LEVEL: return jt_distribute_level<T>;
            case JT_K_REDUCE_LEVEL: return jt_reduce_level<T>;
            case JT_K_MULTI_COLLECT: return jt_multi_flow<T>;
            case JT_K_MULTI_DISTRIBUTE: return jt_multi_flow<T>;
            case JT_K_SINGLE: return jt_single<T>;
            case JT_K_MARGINALS: return jt_marginals<T>;
            case JT_K_LEAN_SINGLE: return jt_lean_single<T>;
        }
        return nullptr;
    }
    static fn get_flow(int phase, bool chain, int tmix, bool marg, bool keep) {
        if (tmix == 2) return phase == 0 ? jt_collect_flow_mix<T, true> : jt_distribute_flow_mix<T, true>;
        if (tmix) return phase == 0 ? jt_collect_flow_mix<T, false> : jt_distribute_flow_mix<T, false>;      // (never merged: jtp_plan.cpp finish())
        // (marg: the plan has marginal tasks folded into its distribute phase - the build of the kernel that can run them)
        if (phase == 2) return marg ? jt_propagate_flow_marg<T> : jt_propagate_flow<T>;          // both phases in one launch
        // The kernel that runs both phases dispatches on the task's mode, so it serves a distribute segment alone as well - and its
        // build of the distribute pass is the faster one (round 5, A/B by environment on one box: config 3 in two launches 8.35 -> 8.13 ms,
        // the whole gain of "one launch"; a rank's share of config 4 at 8 ranks 178 -> 176 us).  JTP_FLOW_BOTH=0: jt_distribute_flow as before.
        if (phase == 1 && !chain && flow_both()) return marg ? jt_propagate_flow_marg<T> : jt_propagate_flow<T>;
        // (keep: the plan's collect passes keep table rows for its distribute launch - JtTask::keep_rows, the build that looks at the flag)
        if (phase == 0 && !chain && keep) return jt_collect_flow_keep<T>;
        return phase == 0 ? jt_collect_flow<T> : (chain ? jt_distribute_flow_chain<T> : jt_distribute_flow<T>);
    }
};

static const char *k_names[JT_K_COUNT] = {
    "jt_collect<T, 0>", "jt_collect<T, 1>", "jt_collect<T, 2>", "jt_collect<T, 3>",
    "jt_distribute<T, 0, 0>", "jt_distribute<T, 0, 1>", "jt_distribute<T, 0, 2>", "jt_distribute<T, 0, 3>",
    "jt_distribute<T, 1, 0>", "jt_distribute<T, 1, 1>", "jt_distribute<T, 1, 2>", "jt_distribute<T, 1, 3>",
    "jt_collect_level<T>", "jt_distribute_level<T>", "jt_collect_flow<T>", "jt_distribute_flow<T>", "jt_reduce_level<T>",
    "jt_multi_flow<T>", "jt_multi_flow<T>", "jt_single<T>", "jt_propagate_flow<T>", "jt_marginals<T>", "jt_lean_single<T>",
};

// the kernel function of a launch variant / of a dataflow phase in the plan's storage type (raise_lds wants it untyped)
const void *kernel_fn(const HostPlan &hp, int variant) {
    return hp.dtype == JTP_F32 ? (const void *)KernelTable<float>::get(variant, mixk(hp)) : (const void *)KernelTable<double>::get(variant, mixk(hp));
}
const void *flow_fn(const jtp_plan *pl, int phase) {
    const HostPlan &hp = pl->hp;
    return hp.dtype == JTP_F32 ? (const void *)KernelTable<float>::get_flow(phase, pl->chain, mixk(hp), pl->marg_tasks, hp.keep_bytes[0] > 0)
                               : (const void *)KernelTable<double>::get_flow(phase, pl->chain, mixk(hp), pl->marg_tasks, hp.keep_bytes[0] > 0);
}

// dynamic LDS above 64 KiB must be allowed per kernel function: remember what each function was raised to
// (per device: the attribute belongs to the function on the CURRENT device; under a lock: plans may be created from
//  several host threads)
static std::map<std::pair<int, const void *>, int> g_lds_raised;
static std::mutex g_lds_mutex;
hipError_t raise_lds(const void *func, int bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_lds_mutex);
    int &have = g_lds_raised[std::make_pair(dev, func)];
    if (have >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

// The one launch of a message-passing kernel.  They all take JT_KARGS and differ in T alone (KernelTable keeps the compiler checking
// that), so the function comes untyped from kernel_fn / flow_fn and the arguments go by address: `psi` and `bel` point to tables of
// the plan's storage type either way.  A launch that fails shows in the caller's hipGetLastError.
static void launch_kargs(const void *fn, unsigned grid, int lds, hipStream_t s, const JtTask *tasks, const JtBlock *blocks,
                         const int *itab, const void *psi, void *bel, double *msg, const JtFlow &fl) {
    void *args[] = {&tasks, &blocks, &itab, &psi, &bel, &msg, const_cast<JtFlow *>(&fl)};
    (void)hipLaunchKernel(fn, dim3(grid), dim3(JT_THREADS), args, (size_t)lds, s);
}

static int launch_variant(jtp_plan *pl, int variant, int nblocks, int lds, hipStream_t s, const JtTask *tasks,
                          const JtBlock *blocks, const int *itab, void *psi, void *bel, double *msg, const JtFlow &fl) {
    launch_kargs(kernel_fn(pl->hp, variant), (unsigned)nblocks, lds, s, tasks, blocks, itab, psi, bel, msg, fl);
    return JTP_OK;
}

// read-out launches: their dynamic LDS is only known now, and must be allowed for the kernel first
int launch_readout(jtp_plan *pl, int variant, int nblocks, int lds, hipStream_t s, const JtTask *tasks,
                          const JtBlock *blocks, const int *itab, void *psi, void *bel, double *msg, const JtFlow &fl) {
    HIP_TRY(raise_lds(kernel_fn(pl->hp, variant), lds));
    return launch_variant(pl, variant, nblocks, lds, s, tasks, blocks, itab, psi, bel, msg, fl);
}

// JTP_SCALED plans: the messages one tree level has just produced are divided by a power of two each, in place, before the next
// level reads them.  One workgroup per record (JtRescale: every copy of one message as its consumers read it), one launch per
// kind-2 step.  Pass 1 takes the largest biased exponent field of the entries (an integer maximum: across the lanes of a row by
// DPP row shifts, across rows by ds_bpermute, across the four waves through LDS); pass 2 multiplies every entry by 2^-e, e = that
// field - 1023 clamped to [-1022, 1022] so that 2^-e is a normal double built from bits - the largest entry then lies in [1, 2)
// (or [1, 4) after the clamp).  A field of 0 (all zero or subnormal) or 0x7ff (an inf or NaN somewhere) leaves the message as it
// is, e = 0: a NaN then propagates exactly as on an unscaled plan.  Multiplying by a power of two is exact, zeros stay zeros.
// (`msg`: the half of the evidence set's arena this propagate uses - 16-byte aligned; a record starts at any double.)
__device__ __forceinline__ int jt_exp_field(double v) { return (__double2hiint(v) >> 20) & 0x7ff; }
#define JT_ROW_DOWN_INT(v, N) __builtin_amdgcn_update_dpp(0, (v), 0x100 + (N), 0xf, 0xf, true)      // row_shl:N - lane + N of the row of 16, 0 beyond it

__global__ __launch_bounds__(256) void jt_rescale_level(const JtRescale *__restrict__ recs, double *__restrict__ msg, int32_t *__restrict__ exps) {
    __shared__ int wave_max[4];
    const JtRescale r = recs[blockIdx.x];
    const int tid = threadIdx.x;
    double *p = msg + r.off;
    // 16-byte vectors from the first even arena offset on; at most one entry before them and one behind
    const int64_t head = ((r.off & 1) && r.count > 0) ? 1 : 0;
    const int64_t npair = (r.count - head) >> 1;
    const bool tail = ((r.count - head) & 1) != 0;
    double2 *v = reinterpret_cast<double2 *>(p + head);
    int mx = 0;
    for (int64_t i = tid; i < npair; i += 256) {
        const double2 x = v[i];
        mx = max(mx, max(jt_exp_field(x.x), jt_exp_field(x.y)));
    }
    if (tid == 0 && head) mx = max(mx, jt_exp_field(p[0]));
    if (tid == 1 && tail) mx = max(mx, jt_exp_field(p[r.count - 1]));
    mx = max(mx, JT_ROW_DOWN_INT(mx, 1));
    mx = max(mx, JT_ROW_DOWN_INT(mx, 2));
    mx = max(mx, JT_ROW_DOWN_INT(mx, 4));
    mx = max(mx, JT_ROW_DOWN_INT(mx, 8));              // lane 0 of every row of 16: the row's maximum
    mx = max(mx, __shfl_xor(mx, 16, 64));
    mx = max(mx, __shfl_xor(mx, 32, 64));              // lane 0: the wave's
    if ((tid & 63) == 0) wave_max[tid >> 6] = mx;
    __syncthreads();
    const int field = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
    int e = 0;
    if (field != 0 && field != 0x7ff) e = min(max(field - 1023, -1022), 1022);
    if (tid == 0) exps[r.slot] = e;
    if (e == 0) return;                                // (times 1: nothing to do)
    const double scale = __hiloint2double((1023 - e) << 20, 0);
    for (int64_t i = tid; i < npair; i += 256) {
        double2 x = v[i];
        x.x *= scale;
        x.y *= scale;
        v[i] = x;
    }
    if (tid == 0 && head) p[0] *= scale;
    if (tid == 1 && tail) p[r.count - 1] *= scale;
}

// JTP_FAKE_COMM: stand-in for a received message
__global__ __launch_bounds__(256) void jt_fill_value(double *__restrict__ dst, int64_t n, double v) {
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x) dst[x] = v;
}

// ------------------------------------------------------------------------------------------ propagates in flight

// Plans with a dataflow propagate enqueued and not yet synchronised, per device: dataflow kernels of two plans running
// at once need ticket order (see jtp_propagate).  A plan that merely EXISTS costs the others nothing (round 2 counted
// live plans: a library user with two junction trees paid the ticket round trip - +10 % on config 4 - on every propagate).
static std::atomic<int> g_inflight[64];

// ... and the same across PROCESSES (round 4): every process using this library on a device keeps its count of in-flight
// dataflow propagates in a slot of a small shared-memory board, /dev/shm/jtprop_flight_<PCI bus id>; a process that finds
// another LIVE process's count above zero launches in ticket order, as it does for a second plan of its own.  Round 3 left
// that case to an environment variable (JTP_FLOW_TICKETS) and to the 2 s time-out with its fall-back to level launches.
// Processes that do not share /dev/shm (containers) still cannot see each other: for them the time-out stands.
namespace board {
struct Slot { std::atomic<int32_t> pid, count; };
constexpr int SLOTS = 64;
// Trust model: the board is advisory.  It is world-writable (any local user's process on the device must be able to publish), so
// a hostile local user could pin every process to ticket order (10 % slower) or hide itself - never corrupt a result: a process that
// is not seen falls under the 2 s time-out and its fall-back to level launches.  Liveness is `kill(pid, 0)`: processes in different
// PID namespaces that share /dev/shm cannot check each other and treat every published count as live.
struct Board { Slot *slots = nullptr; int mine = -1; bool tried = false; int32_t owner_pid = 0; };
static Board g_board[64];
static std::mutex g_mutex;

static bool alive(int32_t pid) { return pid > 0 && (kill((pid_t)pid, 0) == 0 || errno == EPERM); }

static Board &open_board(int device) {
    Board &b = g_board[device & 63];
    std::lock_guard<std::mutex> lock(g_mutex);
    if (b.tried && b.owner_pid == (int32_t)getpid()) return b;
    if (b.tried) {                                      // a forked child: the parent's mapping is there, its SLOT is not ours
        b.mine = -1;
        b.owner_pid = (int32_t)getpid();
        if (!b.slots) return b;
    } else {
    b.tried = true;
    b.owner_pid = (int32_t)getpid();
    char bus[64] = "unknown";
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) return b;
    for (char *c = bus; *c; ++c)
        if (*c == ':' || *c == '.') *c = '_';
    char name[128];
    snprintf(name, sizeof name, "/jtprop_flight_%s", bus);
    // an existing board is opened as it is (O_CREAT on another user's file fails under fs.protected_regular); a new one is made
    // exclusively and opened up with fchmod - the process umask is never touched (other threads may be creating files)
    int fd = shm_open(name, O_RDWR, 0);
    if (fd < 0 && errno == ENOENT) {
        fd = shm_open(name, O_RDWR | O_CREAT | O_EXCL, 0600);
        if (fd >= 0) (void)fchmod(fd, 0666);
        else if (errno == EEXIST) fd = shm_open(name, O_RDWR, 0);          // (somebody else was first)
    }
    if (fd < 0) return b;
    struct stat sb;
    if (fstat(fd, &sb) != 0 || ((size_t)sb.st_size < sizeof(Slot) * SLOTS && ftruncate(fd, sizeof(Slot) * SLOTS) != 0)) { close(fd); return b; }
    void *m = mmap(nullptr, sizeof(Slot) * SLOTS, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return b;
    b.slots = static_cast<Slot *>(m);
    }
    const int32_t me = (int32_t)getpid();
    for (int pass = 0; pass < 2 && b.mine < 0; ++pass)
        for (int i = 0; i < SLOTS && b.mine < 0; ++i) {
            int32_t owner = b.slots[i].pid.load();
            if (owner == me) { b.mine = i; break; }                     // (a forked child inherits nothing useful: it has its own pid)
            if (owner != 0 && (pass == 0 || alive(owner))) continue;    // pass 0: free slots only; pass 1: slots of dead processes too
            if (b.slots[i].pid.compare_exchange_strong(owner, me)) {
                b.slots[i].count.store(0);
                b.mine = i;
            }
        }
    return b;
}

// this process has `n` dataflow propagates in flight on the device; returns whether another live process has any
static bool publish(int device, int n) {
    Board &b = open_board(device);
    if (!b.slots || b.mine < 0) return false;
    b.slots[b.mine].count.store(n);
    bool others = false;
    for (int i = 0; i < SLOTS; ++i) {
        if (i == b.mine || b.slots[i].count.load() <= 0) continue;
        const int32_t owner = b.slots[i].pid.load();
        if (alive(owner)) others = true;
        else {                                             // left behind by a process that died in flight: release the slot FIRST, and
            int32_t expect = owner;                        // clear its count only if that release was ours (a new owner may have published)
            if (owner != 0 && b.slots[i].pid.compare_exchange_strong(expect, 0)) b.slots[i].count.store(0);
        }
    }
    return others;
}
}  // namespace board

// Dataflow launches in blockIdx order are safe only while no OTHER dataflow kernel can be resident on the device at the
// same time (jtp_propagate).  A plan enters the count at its first dataflow propagate and leaves it when the host has
// seen all its streams idle (jtp_sync, a read-out's settle, jtp_plan_destroy).
static bool enter_flight(jtp_plan *pl) {          // returns whether ANOTHER plan - of this process or of another - is in flight on the device
    std::atomic<int> &g = g_inflight[pl->hp.device & 63];
    bool mine = false;
    if (!pl->inflight) {
        pl->inflight = true;
        mine = g.fetch_add(1) > 0;
    } else
        mine = g.load() > 1;
    const bool foreign = board::publish(pl->hp.device, g.load());
    if (foreign) pl->foreign_seen++;
    return mine || foreign;
}
// (the plan's streams are idle: leave_flight; jtp_plan_destroy, which has waited for them whatever `unchecked` says)
void drop_flight(jtp_plan *pl) {
    if (!pl->inflight) return;
    pl->inflight = false;
    const int left = --g_inflight[pl->hp.device & 63];
    (void)board::publish(pl->hp.device, left);
}
static void leave_flight(jtp_plan *pl) {
    for (const auto &b : pl->bufs)
        if (b.unchecked) return;                   // some evidence set's stream has not been waited for yet
    drop_flight(pl);
}
// jtp_stats.flight_board: -1 the board was never looked for, 1 this process has a slot on it, 0 it has none
int flight_board_state(int device) {
    const board::Board &bd = board::g_board[device & 63];
    return !bd.tried ? -1 : (bd.slots && bd.mine >= 0 ? 1 : 0);
}

// ------------------------------------------------------------------------------------------ after a dataflow launch

// Called wherever the host has just synchronised with the plan's streams.  A dataflow launch whose
// workgroups gave up waiting (it would take workgroups dispatched out of order, or a stuck device;
// never observed) has left that propagate unfinished: mark the whole arena unwritten again, switch the
// plan to one launch per level for good, and run the affected evidence sets again that way.
// `synced`: the evidence set whose stream the caller has just synchronised (-1: all of them).
int check_flow(jtp_plan *pl, int synced) {
    if (!pl->host_abort) return JTP_OK;
    if (*(volatile uint32_t *)pl->host_abort.get() == 0) {
        // only what has actually finished is known to be good (sets sharing the stream finished with it)
        for (size_t i = 0; i < pl->bufs.size(); ++i)
            if (synced < 0 || i % pl->streams.size() == (size_t)synced % pl->streams.size()) pl->bufs[i].unchecked = false;
        leave_flight(pl);
        return JTP_OK;
    }
    *(volatile uint32_t *)pl->host_abort.get() = 0;
    pl->flow = false;
    pl->flow_fallbacks++;
    if (pl->hp.n_ranks > 1) {
        // the other ranks have moved on with whatever this rank sent them: no local repair is possible
        for (auto s : pl->streams) (void)hipStreamSynchronize(s);
        for (auto &b : pl->bufs) b.unchecked = false;
        leave_flight(pl);
        return set_err(JTP_EHIP, "a dataflow launch of rank %d timed out waiting for a message (is the GPU shared with other "
                                 "work? then set JTP_FLOW_TICKETS=1); the results of this propagate are invalid on every rank; "
                                 "this plan launches per level from now on", pl->hp.rank);
    }
    for (auto s : pl->streams) HIP_TRY(hipStreamSynchronize(s));
    // only the sets that are run again lose their messages: a set whose propagate was already checked keeps
    // its arena (its separator beliefs are read from there), and no later launch of this plan waits on markers
    if (pl->multiset) {                                     // (all sets run together, the padding sets of the last group too)
        // (on the plan's stream, like the zeros that follow: that stream does not synchronise with the null stream)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)pl->msg_all.get(), (int)(uint32_t)(JT_UNWRITTEN & 0xffffffffu), pl->msg_all.bytes() / 4, pl->streams[0]));
        if (int rc = zero_padding(pl, pl->msg_all.get(), pl->n_groups * JT_MSETS, pl->streams[0])) return rc;
        HIP_TRY(hipStreamSynchronize(pl->streams[0]));
        for (auto &b : pl->bufs) b.epoch = 0, b.flow_runs = 0, b.ticket_runs = 0;
    } else
    for (size_t i = 0; i < pl->bufs.size(); ++i) {
        BatchBuffers &b = pl->bufs[i];
        if (!b.unchecked) continue;
        HIP_TRY(hipMemsetAsync(b.sync, 0, (size_t)pl->hp.sync_words * 4, pl->streams[0]));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)b.msg, (int)(uint32_t)(JT_UNWRITTEN & 0xffffffffu), (size_t)pl->half * 4, pl->streams[0]));
        if (int rc = zero_padding(pl, b.msg, 1, pl->streams[0])) return rc;
        HIP_TRY(hipStreamSynchronize(pl->streams[0]));
        b.epoch = 0;
        b.flow_runs = 0;
        b.ticket_runs = 0;
    }
    if (pl->multiset) {
        bool any = false;
        for (auto &b : pl->bufs) any = any || b.unchecked, b.unchecked = false;
        HIP_TRY(hipMemset(pl->sync_all.get(), 0, pl->sync_all.bytes()));
        if (any) {
            int rc = jtp_propagate(pl, 0, pl->hp.n_batch);
            if (rc) return rc;
        }
    } else
    for (size_t i = 0; i < pl->bufs.size(); ++i) {
        if (!pl->bufs[i].unchecked) continue;
        pl->bufs[i].unchecked = false;
        int rc = jtp_propagate(pl, (int32_t)i, (int32_t)i + 1);
        if (rc) return rc;
    }
    for (auto s : pl->streams) HIP_TRY(hipStreamSynchronize(s));
    leave_flight(pl);
    return JTP_OK;
}

// Before anything is read out: if a dataflow propagate of this evidence set has not been checked yet, wait
// for it and look at the abort flag FIRST, so that a propagate that had to be run again per level is run
// again before the read-out kernels copy anything (they used to copy the aborted propagate's data).
int settle(jtp_plan *pl, int batch) {
    if (!pl->bufs[batch].unchecked) return JTP_OK;
    HIP_TRY(hipStreamSynchronize(pl->streams[batch % pl->streams.size()]));
    return check_flow(pl, batch);
}

// ------------------------------------------------------------------------------------------ propagate

// dynamic LDS of a multi-set launch: the ring plus one region per evidence set of the group (reduce tasks: none)
static int multiset_lds(const HostPlan &hp, const Launch &L) {
    int lds = 0;
    for (int t : L.tasks) lds = std::max(lds, hp.tasks[t].kind == 0 ? hp.tasks[t].lds_bytes : 0);
    return lds;
}

// a zeroed JtFlow with what every launch of a propagate of evidence set `bb` carries (after bb.epoch was advanced)
static JtFlow flow_base(const jtp_plan *pl, const BatchBuffers &bb) {
    JtFlow fl;
    memset(&fl, 0, sizeof fl);
    fl.host_abort = pl->host_abort.get();
    fl.cur_off = cur_half(pl, bb);
    fl.dbg = pl->flow_debug;
    return fl;
}

// Profiling: whether this propagate is one of those timed, and where its `events_per_step` events start in the ring - which grows
// here to hold the propagates kept.
static int prof_ring(jtp_plan *pl, size_t events_per_step, bool &prof, size_t &ev_base) {
    prof = pl->prof_steps > 0 && (pl->prof_calls++ % (unsigned)pl->prof_stride) == 0;
    if (prof) while (pl->ev.size() < events_per_step * (size_t)pl->prof_steps) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        pl->ev.push_back(e);
    }
    ev_base = prof ? events_per_step * (size_t)(pl->prof_cursor % pl->prof_steps) : 0;
    return JTP_OK;
}

// Several evidence sets = several dataflow kernels on the device at once.  In blockIdx order that can
// deadlock: kernel A's waiting workgroups fill the XCD on which kernel B's lowest unfinished
// workgroup should start, and the other way round (seen: --batch 4 hit the 2 s time-out).  A
// ticket is drawn by a workgroup that is already running, so the lowest unfinished record of every
// kernel is always being worked on, whatever else shares the device.
// The same holds for two plans of one process whose propagates overlap (plan_for caches plans, each on
// its own stream), hence tickets whenever another plan of this process has a dataflow propagate IN FLIGHT on
// this device (round 2: whenever another plan existed).  The plan that was there first keeps blockIdx order:
// the newcomer's ticket-ordered workgroups always make progress and drain, so it cannot be starved for good.
// (JTP_FLOW_TICKETS=1 in the environment: for processes that share their GPU with other processes)
//
// What the two kinds of propagate share of this: `bb` keeps the counters (evidence set 0 of a multi-set plan, whose sets run
// together and count `n_sets` at once); `force_tickets`: the per-set propagate of a plan with several streams.
struct LaunchMode {
    bool tickets;
    uint32_t ticket_run;            // ticket-ordered runs of the evidence set before this one
};
static LaunchMode launch_mode(jtp_plan *pl, BatchBuffers &bb, bool flow, bool force_tickets, int n_sets) {
    if (flow) bb.flow_runs++;
    const bool others = flow ? enter_flight(pl) : false;
    LaunchMode m;
    m.tickets = (pl->hp.flags & JTP_FLOW_TICKETS) != 0 || force_tickets || pl->env_tickets || others;
    pl->launch_mode = flow ? (m.tickets ? 2 : 1) : 0;
    if (flow) pl->flow_propagates += n_sets, pl->tickets_used += m.tickets ? n_sets : 0;
    m.ticket_run = bb.ticket_runs;
    if (flow && m.tickets) bb.ticket_runs++;
    return m;
}

// the exchange step of a sharded plan: real, loop-back (JTP_FAKE_COMM=2) or - any other JTP_FAKE_COMM - what would arrive filled in
static int comm_step(jtp_plan *pl, BatchBuffers &bb, const JtFlow &fl, const Step &st, hipStream_t s) {
    const HostPlan &hp = pl->hp;
    if (pl->fake_comm == 0 || pl->fake_comm == 2) return rccl::exchange_step(pl, bb, fl, st, s);
    for (int i = st.first; i < st.first + st.count; ++i) {
        const CommOp &op = hp.comm[i];
        if (op.send) continue;
        const int grid = (int)std::min<int64_t>((op.count + 255) / 256, 1024);
        hipLaunchKernelGGL(jt_fill_value, dim3(grid), dim3(256), 0, s, bb.msg + fl.cur_off + op.off, op.count, 1.0);
    }
    return JTP_OK;
}

static int propagate_multiset(jtp_plan *pl, int32_t batch_begin, int32_t batch_end) {
    HostPlan &hp = pl->hp;
    if (batch_begin != 0 || batch_end != hp.n_batch)
        return set_err(JTP_EINVAL, "a multi-set plan propagates all its evidence sets together: pass [0, %d)", hp.n_batch);
    if (pl->prof_per_launch) return set_err(JTP_EINVAL, "per-launch profiling is not available for multi-set plans");
    hipStream_t s = pl->streams[0];
    bool prof;
    size_t ev_base;
    if (int rc = prof_ring(pl, 3, prof, ev_base)) return rc;
    for (auto &bb : pl->bufs) bb.epoch++;
    BatchBuffers &b0 = pl->bufs[0];
    JtFlow fl = flow_base(pl, b0);
    fl.sync = pl->sync_all.get();
    fl.oth_off = pl->half - fl.cur_off;                  // the kernel waits on markers in every launch mode
    fl.ev = pl->ev_all.get();
    fl.set_stride = pl->set_stride;
    fl.ev_stride = pl->ev_stride;
    fl.sync_stride = (uint32_t)hp.sync_words;
    if (pl->act_dirty) {
        if (int rc2 = rebuild_active(pl, s)) return rc2;
    }
    fl.skip = pl->d_member.get();
    fl.act_ids = pl->d_act_ids.get();
    fl.act_n = pl->d_act_n.get();
    fl.esum_oct = pl->d_esum_oct.get();
    fl.cap = (uint32_t)(pl->n_groups * JT_MSETS);
    fl.n_tasks = (uint32_t)hp.tasks.size();
    if (pl->esum_dirty) {
        // which groups may sum a vector's elements first on which task (jtp_set_evidence): the fields of ALL tasks in one
        // strided copy, ordered before the launches below on the plan's stream
        HIP_TRY(hipMemcpy2DAsync(&pl->d_tasks.get()[0].esum_groups, sizeof(JtTask), &hp.tasks[0].esum_groups, sizeof(JtTask), sizeof(uint64_t),
                                 hp.tasks.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpy2DAsync(&pl->d_tasks.get()[0].esum, sizeof(JtTask), &hp.tasks[0].esum, sizeof(JtTask), sizeof(int32_t),
                                 hp.tasks.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));                    // (the source is the plan's own task table: pageable)
        pl->esum_dirty = false;
    }
    const bool flow = pl->flow;
    if (flow)
        for (auto &bb : pl->bufs) bb.unchecked = true;
    const LaunchMode lm = launch_mode(pl, b0, flow, false, hp.n_batch);
    bool mid_done = false;
    if (prof) HIP_TRY(hipEventRecord(pl->ev[ev_base + 0], s));
    const void *kernel = kernel_fn(hp, JT_K_MULTI_COLLECT);       // (jt_multi_flow: it dispatches on the task)
    auto launch = [&](int64_t blk_off, int nblocks, int lds, int ticket_idx, uint32_t ticket_base) {
        fl.ticket_idx = ticket_idx >= 0 ? (uint32_t)ticket_idx : 0xffffffffu;
        fl.ticket_base = ticket_base;
        fl.blk_base = (uint32_t)blk_off;
        fl.n_groups = (uint32_t)pl->n_groups;
        fl.n_blocks = (uint32_t)nblocks;
        // (1-D grid: eight records of group 0, the same eight of group 1, ... - see jt_multi_flow)
        const unsigned grid = (unsigned)((nblocks + 7) / 8) * 8u * (unsigned)pl->n_groups;
        launch_kargs(kernel, grid, lds, s, pl->d_tasks.get(), pl->d_blocks.get() + blk_off, pl->d_itab.get(), b0.psi, b0.bel, pl->msg_all.get(), fl);
    };
    for (const Step &st : (flow ? hp.flow_steps : hp.steps)) {
        if (st.kind != 0) continue;
        const int phase = flow ? hp.segments[st.first].phase : hp.launches[st.first].phase;
        if (prof && !mid_done && phase == 1) {
            HIP_TRY(hipEventRecord(pl->ev[ev_base + 1], s));
            mid_done = true;
        }
        if (flow) {
            const Segment &sg = hp.segments[st.first];
            int lds = 0;
            for (int i = sg.first_launch; i < sg.first_launch + sg.n_launch; ++i) lds = std::max(lds, multiset_lds(hp, hp.launches[i]));
            launch(sg.blk_off, sg.nblocks, lds, lm.tickets ? sg.ticket_idx : -1, lm.ticket_run * (uint32_t)sg.nblocks);
        } else {
            const Launch &L = hp.launches[st.first];
            launch(L.blk_off, L.nblocks, multiset_lds(hp, L), -1, 0u);
        }
    }
    if (prof) {
        if (!mid_done) HIP_TRY(hipEventRecord(pl->ev[ev_base + 1], s));
        HIP_TRY(hipEventRecord(pl->ev[ev_base + 2], s));
        pl->prof_cursor++;
    }
    HIP_TRY(hipGetLastError());
    return JTP_OK;
}

static int propagate_sets(jtp_plan *pl, int32_t batch_begin, int32_t batch_end) {
    HostPlan &hp = pl->hp;
    bool prof;
    size_t ev_base;
    if (int rc = prof_ring(pl, pl->prof_per_launch ? 2 * hp.launches.size() : 3, prof, ev_base)) return rc;
    for (int b = batch_begin; b < batch_end; ++b) {
        hipStream_t s = pl->streams[b % pl->streams.size()];
        BatchBuffers &bb = pl->bufs[b];
        const bool pb = prof && b == batch_begin;
        const bool per_launch = pb && pl->prof_per_launch;
        const bool per_phase = pb && !pl->prof_per_launch;
        bool mid_done = false;
        if (per_phase) HIP_TRY(hipEventRecord(pl->ev[ev_base + 0], s));
        const bool flow = pl->flow && !per_launch;
        const int64_t half = pl->half;
        bb.epoch++;
        bb.scale_fresh = false;
        JtFlow fl = flow_base(pl, bb);
        fl.sync = bb.sync;
        // (a plan that launches per level never waits on entries: it need not mark the other half)
        fl.oth_off = pl->flow ? half - fl.cur_off : -1;
        fl.ev = bb.ev_any ? bb.ev : nullptr;
        fl.fix_shift = bb.fix_shift(fl.cur_off);
        if (flow) bb.unchecked = true;
        const LaunchMode lm = launch_mode(pl, bb, flow, pl->streams.size() > 1, 1);
        for (const Step &st : (flow ? hp.flow_steps : hp.steps)) {
            if (st.kind == 0 && flow) {
                const Segment &sg = hp.segments[st.first];
                if (per_phase && !mid_done && sg.phase >= 1) {       // (a merged launch counts as the second phase)
                    HIP_TRY(hipEventRecord(pl->ev[ev_base + 1], s));
                    mid_done = true;
                }
                fl.ticket_idx = lm.tickets ? (uint32_t)sg.ticket_idx : 0xffffffffu;
                fl.blk_base = (uint32_t)sg.blk_off;
                fl.ticket_base = lm.ticket_run * (uint32_t)sg.nblocks;
                launch_kargs(flow_fn(pl, sg.phase), (unsigned)sg.nblocks, sg.lds_bytes, s, pl->d_tasks.get(), pl->d_blocks.get() + sg.blk_off, pl->d_itab.get(), bb.psi, bb.bel, bb.msg, fl);
            } else if (st.kind == 0) {
                const Launch &L = hp.launches[st.first];
                if (per_phase && !mid_done && L.phase == 1) {
                    HIP_TRY(hipEventRecord(pl->ev[ev_base + 1], s));
                    mid_done = true;
                }
                if (per_launch) HIP_TRY(hipEventRecord(pl->ev[ev_base + 2 * st.first], s));
                fl.blk_base = (uint32_t)L.blk_off;
                launch_variant(pl, L.variant, L.nblocks, L.lds_bytes, s, pl->d_tasks.get(), pl->d_blocks.get() + L.blk_off, pl->d_itab.get(), bb.psi, bb.bel, bb.msg, fl);
                if (per_launch) HIP_TRY(hipEventRecord(pl->ev[ev_base + 2 * st.first + 1], s));
            } else if (st.kind == 2) {
                // (JTP_SCALED: the messages the level before has just produced, a workgroup each)
                hipLaunchKernelGGL(jt_rescale_level, dim3((unsigned)st.count), dim3(256), 0, s, pl->d_rescale.get() + st.first, bb.msg + fl.cur_off, bb.exps);
            } else if (int rc = comm_step(pl, bb, fl, st, s))
                return rc;
        }
        if (per_phase) {
            if (!mid_done) HIP_TRY(hipEventRecord(pl->ev[ev_base + 1], s));
            HIP_TRY(hipEventRecord(pl->ev[ev_base + 2], s));
        }
        if (pb) pl->prof_cursor++;
    }
    HIP_TRY(hipGetLastError());
    return JTP_OK;
}

extern "C" {

const char *jtp_kernel_name(int32_t variant) {
    if (variant < 0 || variant >= JT_K_COUNT) return nullptr;
    return k_names[variant];
}

int jtp_propagate(jtp_plan *pl, int32_t batch_begin, int32_t batch_end) {
    int rc = check_ready(pl, batch_begin);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if (batch_end <= batch_begin || batch_end > hp.n_batch) return set_err(JTP_EINVAL, "bad batch range [%d,%d)", batch_begin, batch_end);
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range whole(pl->roctx, pl->multiset ? "jtp_propagate (multi-set: collect + distribute)" : "jtp_propagate (collect + distribute)");
    if ((hp.flags & JTP_SHARE_POTENTIALS) && pl->psi_dirty) {
        HIP_TRY(hipStreamSynchronize(pl->streams[0]));        // the shared tables were written on stream 0
        pl->psi_dirty = false;
    }
    return pl->multiset ? propagate_multiset(pl, batch_begin, batch_end) : propagate_sets(pl, batch_begin, batch_end);
}

int jtp_sync(jtp_plan *pl) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    if (!pl->device) return JTP_OK;
    HIP_TRY(hipSetDevice(pl->hp.device));
    for (auto s : pl->streams) HIP_TRY(hipStreamSynchronize(s));
    pl->eval_pending = false;
    pl->eval_cursor = 0;
    return check_flow(pl);
}

}  // extern "C"
