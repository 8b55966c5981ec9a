// C ABI of libjtprop.so (declared in include/jtprop.h): device memory, launch schedule,
// RCCL point-to-point exchange at subtree cuts, host<->device layout conversion.
// Plain HIP runtime + RCCL; no PyTorch, no Triton.
// This unit: the error state, version, host memory and device queries, the life of a plan (jtp_engine.h maps the other units).
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "jtp_engine.h"

// ------------------------------------------------------------------------------------------ errors

static thread_local std::string g_err;

int set_err(int code, const char *fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// ------------------------------------------------------------------------------------------ what every unit asks of a plan

int check_ready(jtp_plan *pl, int batch) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    if (!pl->device) return set_err(JTP_EHIP, "plan was created with JTP_PLAN_ONLY: no device work possible");
    if (batch < 0 || batch >= pl->hp.n_batch) return set_err(JTP_EINVAL, "batch %d out of range [0,%d)", batch, pl->hp.n_batch);
    return JTP_OK;
}

int ensure_stage(jtp_plan *pl, size_t bytes) {
    HIP_TRY(pl->stage.reserve(bytes));
    return JTP_OK;
}

// The chunks whose own digits do not exist (a digit beyond a variable's cardinality, a padding bit set) are not in the block
// lists of a single-set plan (HostPlan::init_blocks): whatever their incoming messages, all they would write is their partial
// copies of the outgoing messages, all zeros.  Those zeros are written HERE, once per arena half, on `s`, after the arena was set
// to "unwritten": the entries carry no marker from then on (nobody re-arms them), every propagate finds them written.
__global__ __launch_bounds__(256) void jt_zero_copies(const JtTask *__restrict__ tasks, const JtBlock *__restrict__ blk, double *__restrict__ msg,
                                                      int64_t cur_off, int64_t set_stride) {
    const JtBlock &bk = blk[blockIdx.x];
    const JtTask &tk = tasks[bk.task];
    msg += (int64_t)blockIdx.y * set_stride;               // (multi-set plans: one arena per evidence set)
    for (int j = 0; j < tk.n_out; ++j) {
        const JtMsg &m = tk.msg[JT_MAX_IN + j];
        // (where a workgroup's flush puts entry s of its sub-box: jt_pass / jt_mpass, "flush outgoing sub-boxes")
        const int64_t at = cur_off + m.off + (int64_t)bk.pnum[j] * m.pstride + bk.gbase[JT_MAX_IN + j];
        const int n = 1 << m.nfree;
        for (int s = threadIdx.x; s < n; s += 256) {
            uint32_t idx = 0;
            for (int b = 0; b < m.nfree; ++b) idx += (((uint32_t)s >> b) & 1u) << m.free_pos[b];
            msg[at + idx] = 0.0;
        }
    }
}

// (`msg`, `nsets`: one evidence set's arena, or - multi-set plans - all of them, set_stride doubles apart; `halves`: bit h = arena half h)
int zero_padding(jtp_plan *pl, double *msg, int nsets, hipStream_t s, int halves) {
    const HostPlan &hp = pl->hp;
    for (int m = 0; m < 2; ++m) {
        if (hp.init_blocks[m].empty() || !pl->d_init[m]) continue;
        for (int h = 0; h < 2; ++h)
            if ((halves >> h) & 1)
                hipLaunchKernelGGL(jt_zero_copies, dim3((unsigned)hp.init_blocks[m].size(), (unsigned)nsets), dim3(256), 0, s, pl->d_tasks.get(), pl->d_init[m].get(), msg,
                                   h ? pl->half : (int64_t)0, pl->set_stride);
    }
    HIP_TRY(hipGetLastError());
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------ version, host memory, devices

extern "C" {

const char *jtp_last_error(void) { return g_err.c_str(); }
// JTP_SOURCE_ID: digest of the library's sources, passed in by junction-tree_amd/build.py; profiles/ files carry the id of
// the build they were measured on, and bench.py quotes a traffic figure only from a file whose id matches the running one
#ifndef JTP_SOURCE_ID
#define JTP_SOURCE_ID "unknown"
#endif
const char *jtp_version(void) { return "jtprop 0.8.1 (gfx950, HIP, RCCL p2p) src:" JTP_SOURCE_ID; }

int jtp_host_alloc(void **ptr, size_t bytes) {
    if (!ptr) return set_err(JTP_EINVAL, "null argument");
    *ptr = nullptr;
    HIP_TRY(hipHostMalloc(ptr, std::max<size_t>(bytes, 1), hipHostMallocDefault));
    return JTP_OK;
}

int jtp_host_free(void *ptr) {
    if (!ptr) return JTP_OK;
    HIP_TRY(hipHostFree(ptr));
    return JTP_OK;
}

int jtp_device_count(int32_t *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return set_err(JTP_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return JTP_OK;
}

int jtp_device_memory(int32_t device, uint64_t *free_bytes, uint64_t *total_bytes) {
    size_t f = 0, t = 0;
    int before = 0;
    HIP_TRY(hipGetDevice(&before));
    HIP_TRY(hipSetDevice(device));
    const hipError_t e = hipMemGetInfo(&f, &t);
    (void)hipSetDevice(before);                    // (the caller's current device stays what it was)
    if (e != hipSuccess) return set_err(JTP_EHIP, "hipMemGetInfo failed: %s", hipGetErrorString(e));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------ lifetime

void jtp_plan_destroy(jtp_plan *pl) {
    if (!pl) return;
    std::vector<hipStream_t> streams;
    if (pl->device) {
        (void)hipSetDevice(pl->hp.device);
        for (auto s : pl->streams) (void)hipStreamSynchronize(s);
        drop_flight(pl);
        for (auto e : pl->up_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto e : pl->ev) (void)hipEventDestroy(e);
        for (auto e : pl->acc_ev) (void)hipEventDestroy(e);
        for (auto e : pl->region_ev)
            if (e) (void)hipEventDestroy(e);
        streams.swap(pl->streams);
    }
    delete pl;                      // every buffer: after the streams were waited for, before they are destroyed
    for (auto s : streams) (void)hipStreamDestroy(s);
}

}  // extern "C"

struct PlanDestroyer { void operator()(jtp_plan *pl) const { jtp_plan_destroy(pl); } };

extern "C" {

int jtp_plan_create(const jtp_tree_desc *desc, jtp_plan **out) {
    if (!out) return set_err(JTP_EINVAL, "null output pointer");
    *out = nullptr;
    // (destroyed on every early return; released into *out at the end)
    std::unique_ptr<jtp_plan, PlanDestroyer> owner(new jtp_plan());
    jtp_plan *pl = owner.get();
    auto start_over = [&]() { owner.reset(new jtp_plan()), pl = owner.get(); };
    std::string err;
    int rc = jtp_build_plan(desc, pl->hp, err);
    // Fall-backs of the planner's defaults, tried in turn while the structure is "unsupported":
    //  - multi-set plans: sub-boxes too large for one evidence set's LDS region under the default bit order -> the
    //    order with the smallest sub-boxes;
    //  - a table that cannot be cut into workgroups without splitting a variable stored at its true cardinality ->
    //    every table padded to powers of two (the round-1 layout).
    for (int attempt = 1; attempt < 4 && rc == JTP_EUNSUPPORTED && desc; ++attempt) {
        jtp_tree_desc again = *desc;
        const bool relayout = (attempt & 1) && (desc->flags & JTP_MULTISET) && desc->layout_policy == 0;
        const bool pad = (attempt & 2) && !(desc->flags & JTP_NO_COMPACT);
        if (!relayout && !pad) continue;
        if ((attempt & 1) && !relayout) continue;
        if ((attempt & 2) && !pad) continue;
        if (relayout) again.layout_policy = 2;
        if (pad) again.flags |= JTP_NO_COMPACT;
        std::string err2;
        start_over();
        const int rc2 = jtp_build_plan(&again, pl->hp, err2);
        if (rc2 == JTP_OK) rc = rc2;
        else if (rc2 != JTP_EUNSUPPORTED) rc = rc2, err = err2;
    }
    //  - float32 storage means 1024-element rows: a clique of few rows with four or more neighbours whose separators are
    //    nearly the whole clique then needs more LDS than a CU has ("message sub-boxes do not fit in LDS").  The same tree in
    //    float64 storage (512-element rows) plans: the plan is then made with double tables - twice the device bytes of
    //    what was asked for, the host interface unchanged (every call names its host type) - and says so in
    //    jtp_stats.storage_dtype.  (Round 3 did this in the Python layer only, keyed on the message text.)
    if (rc == JTP_EUNSUPPORTED && desc && desc->dtype == JTP_F32 && !(desc->flags & JTP_MULTISET)) {
        for (int attempt = 0; attempt < 2 && rc == JTP_EUNSUPPORTED; ++attempt) {
            jtp_tree_desc again = *desc;
            again.dtype = JTP_F64;
            if (attempt == 1) {
                if (desc->flags & JTP_NO_COMPACT) break;
                again.flags |= JTP_NO_COMPACT;
            }
            std::string err2;
            start_over();
            const int rc2 = jtp_build_plan(&again, pl->hp, err2);
            if (rc2 == JTP_OK) rc = rc2, pl->widened = true;
            else if (rc2 != JTP_EUNSUPPORTED) rc = rc2, err = err2;
        }
    }
    //  - a clique that keeps no table stages the product of its factors like one more message: where that does not fit (or the
    //    tighter layout rules of such cliques cannot be met) the tree is planned with every table materialised, as rounds 1-4 did
    if (rc == JTP_EUNSUPPORTED && desc && desc->cover_off && !(desc->flags & JTP_MULTISET)) {
        jtp_tree_desc again = *desc;
        again.cover_off = again.cover_ids = nullptr;
        jtp_plan *fresh = nullptr;
        const int rc2 = jtp_plan_create(&again, &fresh);
        if (rc2 == JTP_OK) {
            fresh->hp.lean_refused = err.empty() ? std::string("unsupported") : err;      // (jtp_stats.lean_refused, jtp_plan_describe)
            *out = fresh;
        }
        return rc2;
    }
    if (rc != JTP_OK) return set_err(rc, "%s", err.c_str());
    HostPlan &hp = pl->hp;
    pl->esize = hp.dtype == JTP_F32 ? 4 : 8;
    pl->half = std::max<int64_t>(hp.msg_doubles, 2);
    pl->multiset = hp.multiset;
    if (pl->multiset && !(hp.flags & JTP_SHARE_POTENTIALS))
        return set_err(JTP_EINVAL, "JTP_MULTISET needs JTP_SHARE_POTENTIALS (the evidence sets of a group read one table)");
    // one launch per level when asked for, for per-shape launches and for the JTP_DEBUG experiments
    pl->flow = !(hp.flags & (JTP_LEVEL_LAUNCHES | JTP_SPLIT_VARIANTS)) && !(hp.knobs.debug & 1) && !hp.knobs.force_level_launches;
    // Sub-boxes so large that one or two workgroups fill a CU (config 3: 121 KB): a waiting workgroup
    // then idles a whole CU, and staging is a large share of the traffic, which per-level launches read
    // through L2 while a dataflow launch has to read through to memory.  Measured 39.6 vs 46.9 ms.
    if (hp.max_lds > 64 * 1024 && !pl->multiset && !hp.knobs.force_flow) pl->flow = false;
    pl->chain = hp.chain_plan;
    for (const HostPlan::FoldReq &fr : hp.folded) pl->marg_tasks = pl->marg_tasks || fr.task >= 0;
    if (hp.flags & JTP_PLAN_ONLY) {
        *out = owner.release();
        return JTP_OK;
    }
    // JTP_FAKE_COMM=1 (development aid): run ONE rank's share of a multi-rank plan on its own; what
    // it would receive is filled with ones, what it would send goes nowhere.  Timing only.
    pl->fake_comm = hp.n_ranks > 1 ? hp.knobs.fake_comm : 0;
    if (pl->fake_comm == 2 && rccl::size() != 1)
        return set_err(JTP_ECOMM, "JTP_FAKE_COMM=2 (exchange steps as RCCL groups in loop-back) needs a communicator of ONE rank: jtp_comm_init(0, 1, ...)");
    if (hp.n_ranks > 1 && !pl->fake_comm && (rccl::size() != hp.n_ranks || rccl::rank() != hp.rank))
        return set_err(JTP_ECOMM, "n_ranks=%d but jtp_comm_init was not called with a matching communicator", hp.n_ranks);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return set_err(JTP_EHIP, "no HIP device available (%s); libjtprop has no CPU fallback",
                       e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    pl->device = true;
    pl->mem.fail_in = hp.knobs.fail_alloc;          // (test hook: for the allocations of this function only)
    pl->flow_debug = hp.knobs.flow_debug;
    pl->env_tickets = hp.knobs.flow_tickets != 0;
    pl->roctx = hp.knobs.roctx != 0;
    if (pl->roctx) roctx::load();
    HIP_TRY(hipSetDevice(hp.device));
    const int nstreams = pl->multiset ? 1 : std::min(hp.n_batch, 16);
    pl->streams.resize(nstreams);
    for (auto &s : pl->streams) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipStream_t s0 = pl->streams[0];
    pl->bufs.resize(hp.n_batch);
    const size_t abytes = (size_t)std::max<int64_t>(hp.arena_elems, 256) * pl->esize;
    // two halves, used by alternate propagates (jtp_internal.h: JT_UNWRITTEN)
    const size_t mdoubles = (size_t)pl->half * 2, mbytes = mdoubles * 8;
    const int unwritten = (int)(uint32_t)(JT_UNWRITTEN & 0xffffffffu);
    const bool share_psi = (hp.flags & JTP_SHARE_POTENTIALS) != 0;     // one potential arena for all evidence sets
    // Which evidence set sees which allocation is decided HERE, once: multi-set plans share psi and one belief scratch (set_mem[0])
    // and slice the *_all arenas; single-set plans own everything per set, except psi / fix under JTP_SHARE_POTENTIALS (set 0's).
    const size_t n_own = pl->multiset ? 1 : (size_t)hp.n_batch;
    pl->set_mem.reserve(n_own);
    for (size_t i = 0; i < n_own; ++i) pl->set_mem.emplace_back(&pl->mem);
    if (pl->multiset) {
        // (group 0: the evidence-free sets the others take their untouched upward messages from - one more group through the collect
        //  pass, which pays from eight groups on: measured 64 sets 4.97 -> 4.8 ms, 8 sets 0.91 -> 1.3; JTP_EF_SHARE=1 / JTP_NO_EF_SHARE=1 force it)
        const bool ef = hp.knobs.no_ef_share == 0 && ((hp.n_batch + JT_MSETS - 1) / JT_MSETS >= 8 || hp.knobs.no_ef_share < 0);
        pl->set0 = ef ? JT_MSETS : 0;
        pl->n_groups = (hp.n_batch + JT_MSETS - 1) / JT_MSETS + (pl->set0 ? 1 : 0);
        const size_t nsets = (size_t)pl->n_groups * JT_MSETS;          // (the last group is padded with evidence-free sets)
        pl->set_stride = (int64_t)mdoubles;
        pl->ev_stride = (uint32_t)(2 * hp.pn.size());
        SetMem &m = pl->set_mem[0];
        HIP_TRY(m.psi.alloc(abytes));
        HIP_TRY(m.bel.alloc(abytes));                                  // scratch: one belief table at a time, on demand
        HIP_TRY(hipMemsetAsync(m.psi.get(), 0, abytes, s0));
        HIP_TRY(hipMemsetAsync(m.bel.get(), 0, abytes, s0));
        HIP_TRY(pl->msg_all.alloc(mdoubles * nsets));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)pl->msg_all.get(), unwritten, mbytes * nsets / 4, s0));
        HIP_TRY(pl->ev_all.alloc((size_t)pl->ev_stride * nsets));
        HIP_TRY(hipMemsetAsync(pl->ev_all.get(), 0, pl->ev_all.bytes(), s0));
        HIP_TRY(pl->sync_all.alloc((size_t)hp.sync_words * pl->n_groups));
        HIP_TRY(hipMemsetAsync(pl->sync_all.get(), 0, pl->sync_all.bytes(), s0));
        for (int b = 0; b < hp.n_batch; ++b) {
            BatchBuffers &bb = pl->bufs[b];
            bb.psi = m.psi.get();
            bb.bel = m.bel.get();
            bb.msg = pl->msg_all.get() + (int64_t)(pl->set0 + b) * pl->set_stride;
            bb.ev = pl->ev_all.get() + (size_t)(pl->set0 + b) * pl->ev_stride;
            bb.sync = pl->sync_all.get() + (size_t)((pl->set0 + b) / JT_MSETS) * hp.sync_words;
        }
        if (pl->set0) {
            // (the active lists are made by the first propagate: rebuild_active)
            const size_t cap = (size_t)pl->n_groups * JT_MSETS, nt = hp.tasks.size();
            HIP_TRY(pl->d_member.alloc(nt * cap));
            HIP_TRY(pl->d_act_ids.alloc(nt * cap));
            HIP_TRY(pl->d_act_n.alloc(nt));
            HIP_TRY(pl->d_esum_oct.alloc(nt * (size_t)pl->n_groups));
            pl->act_dirty = true;
        }
    } else
    for (size_t i = 0; i < n_own; ++i) {
        SetMem &m = pl->set_mem[i], &first = pl->set_mem[0];
        BatchBuffers &b = pl->bufs[i];
        const bool own_psi = !share_psi || i == 0;
        if (own_psi) HIP_TRY(m.psi.alloc(abytes));
        HIP_TRY(m.bel.alloc(abytes));
        HIP_TRY(m.msg.alloc(mdoubles));
        if (hp.fix_doubles > 0 && own_psi) {
            HIP_TRY(m.fix.alloc((size_t)hp.fix_doubles));
            HIP_TRY(hipMemsetAsync(m.fix.get(), 0, m.fix.bytes(), s0));
        }
        b.psi = (own_psi ? m : first).psi.get();
        b.fix = (own_psi ? m : first).fix.get();
        b.bel = m.bel.get();
        b.msg = m.msg.get();
        HIP_TRY(hipMemsetAsync(b.psi, 0, abytes, s0));
        HIP_TRY(hipMemsetAsync(b.bel, 0, abytes, s0));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)b.msg, unwritten, mbytes / 4, s0));
        HIP_TRY(m.sync.alloc((size_t)hp.sync_words));
        b.sync = m.sync.get();
        HIP_TRY(hipMemsetAsync(b.sync, 0, m.sync.bytes(), s0));
        if (hp.scaled) {
            HIP_TRY(m.exps.alloc(std::max<size_t>(2 * hp.ps.size(), 1)));
            b.exps = m.exps.get();
            HIP_TRY(hipMemsetAsync(b.exps, 0, m.exps.bytes(), s0));
        }
    }
    HIP_TRY(pl->host_abort.alloc(16, hipHostMallocMapped));
    *pl->host_abort.get() = 0;

    for (auto &b : pl->bufs) {
        if (&b != &pl->bufs[0] && b.psi == pl->bufs[0].psi) continue;          // shared tables: filled once
        for (const VirtualFill &vf : hp.virtual_fills) launch_virtual_fill(hp, vf.d, b.psi, s0);
        HIP_TRY(hipGetLastError());
    }
    if (pl->multiset) {
        pl->ev_host.assign((size_t)pl->ev_stride * pl->n_groups * JT_MSETS, 0u);
        for (JtTask &tk : hp.tasks)
            if (tk.esum & 1) tk.esum |= 2, tk.esum_groups = ~0ull;      // no evidence yet
    }
    HIP_TRY(pl->d_tasks.upload(hp.tasks));
    HIP_TRY(pl->d_blocks.upload(hp.blocks));
    HIP_TRY(pl->d_itab.upload(hp.itab));
    HIP_TRY(pl->d_rescale.upload(hp.rescale));
    for (int m = 0; m < 2; ++m) HIP_TRY(pl->d_init[m].upload(hp.init_blocks[m]));
    // dynamic LDS beyond 64 KiB has to be allowed per kernel function (raise_lds remembers what each one has)
    if (pl->multiset) {
        HIP_TRY(raise_lds(kernel_fn(hp, JT_K_MULTI_COLLECT), JT_RING_BYTES + JT_MSETS * (JT_MSETS > 8 ? JT_SETB_SMALL : JT_SETB_LARGE)));
    } else if (hp.max_lds > 64 * 1024) {
        for (int v = 0; v < JT_K_COUNT; ++v) {
            if (kernel_fn(hp, v) == nullptr) continue;             // (the dataflow kernels: below)
            HIP_TRY(raise_lds(kernel_fn(hp, v), hp.max_lds));
        }
        for (int ph = 0; ph < 3; ++ph) HIP_TRY(raise_lds(flow_fn(pl, ph), hp.max_lds));
    }
    if (pl->multiset) {
        if (int rc = zero_padding(pl, pl->msg_all.get(), pl->n_groups * JT_MSETS, s0)) return rc;
    } else
        for (auto &b : pl->bufs)
            if (int rc = zero_padding(pl, b.msg, 1, s0)) return rc;
    HIP_TRY(hipStreamSynchronize(s0));
    // what the plan holds on the device from now on (the plan cache of the Python layer budgets with it)
    pl->device_bytes = (double)pl->mem.bytes;
    pl->mem.fail_in = 0;
    *out = owner.release();
    return JTP_OK;
}

const char *jtp_plan_describe(jtp_plan *pl) {
    if (!pl) return "";
    if (pl->hp.json.empty()) jtp_plan_to_json(pl->hp, pl->hp.tasks.size() <= 20000);
    return pl->hp.json.c_str();
}

int jtp_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes) {
    if (device_bytes) *device_bytes = g_live_bytes[0].load();
    if (pinned_bytes) *pinned_bytes = g_live_bytes[1].load();
    return JTP_OK;
}

int jtp_debug_set(jtp_plan *pl, const char *knob, int64_t value) {
    if (!pl || !knob) return set_err(JTP_EINVAL, "null argument");
    if (!strcmp(knob, "flow_debug")) pl->flow_debug = (uint32_t)value;      // fault injection (tests): see JtFlow::dbg
    else if (!strcmp(knob, "flow")) pl->flow = value != 0 && !pl->hp.segments.empty();
    else if (!strcmp(knob, "fail_alloc")) pl->mem.fail_in = std::max<int64_t>(value, 0);      // (MemLedger::fail_in)
    else if (!strcmp(knob, "acc_chunk")) pl->acc_chunk = std::max<int64_t>(value, 0);         // (jtp_accumulate_marginals; 0: by size)
    else if (!strcmp(knob, "map_chunk")) pl->map_chunk = std::max<int64_t>(value, 0);         // (jtp_map, jtp_max_marginals; 0: by size)
    else if (!strcmp(knob, "map_seg"))                                                        // (jtp_map, jtp_max_marginals: the records are built again)
        pl->map_seg = std::max<int64_t>(value, 0), pl->map = MapMem(&pl->mem), pl->maxm = MaxMem(&pl->mem);
    else return set_err(JTP_EINVAL, "unknown knob %s", knob);
    return JTP_OK;
}

}  // extern "C"
