// Multi-GPU: the RCCL point-to-point exchange at subtree cuts (library looked up at run time), jtp_comm_*, and the optional
// roctx ranges.  Launches nothing: host code over the HIP runtime.
#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jtp_engine.h"

// ------------------------------------------------------------------------------------------ RCCL (lazy)

namespace rccl {
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
enum { ncclSuccess = 0 };
enum { ncclFloat64 = 8 };
typedef int (*GetUniqueId_t)(ncclUniqueId *);
typedef int (*CommInitRank_t)(ncclComm_t *, int, ncclUniqueId, int);
typedef int (*CommDestroy_t)(ncclComm_t);
typedef int (*Send_t)(const void *, size_t, int, int, ncclComm_t, hipStream_t);
typedef int (*Recv_t)(void *, size_t, int, int, ncclComm_t, hipStream_t);
typedef int (*Group_t)(void);
typedef const char *(*ErrStr_t)(int);
typedef int (*CommQuery_t)(const ncclComm_t, int *);

static void *lib = nullptr;
static GetUniqueId_t GetUniqueId;
static CommInitRank_t CommInitRank;
static CommDestroy_t CommDestroy;
static Send_t Send;
static Recv_t Recv;
static Group_t GroupStart, GroupEnd;
static ErrStr_t GetErrorString;
static CommQuery_t CommCount = nullptr, CommUserRank = nullptr, CommCuDevice = nullptr;      // (optional: what the communicator itself says)
static ncclComm_t comm = nullptr;
static int comm_rank = 0, comm_size = 1;

static int load() {
    if (lib) return JTP_OK;
    // JTP_RCCL_LIB: another library with the same eight entry points (tests/mock_rccl: several processes on
    // one GPU exchanging through /dev/shm, to exercise the multi-rank path where there is no second GPU)
    const char *names[] = {getenv("JTP_RCCL_LIB") ? getenv("JTP_RCCL_LIB") : "librccl.so.1", "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
        lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (lib) break;
    }
    if (!lib) return set_err(JTP_ECOMM, "cannot load librccl: %s", dlerror());
#define SYM(var, name)                                                            \
    var = (decltype(var))dlsym(lib, name);                                        \
    if (!var) return set_err(JTP_ECOMM, "librccl lacks symbol %s", name);
    SYM(GetUniqueId, "ncclGetUniqueId")
    SYM(CommInitRank, "ncclCommInitRank")
    SYM(CommDestroy, "ncclCommDestroy")
    SYM(Send, "ncclSend")
    SYM(Recv, "ncclRecv")
    SYM(GroupStart, "ncclGroupStart")
    SYM(GroupEnd, "ncclGroupEnd")
    SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
    CommCount = (CommQuery_t)dlsym(lib, "ncclCommCount");
    CommUserRank = (CommQuery_t)dlsym(lib, "ncclCommUserRank");
    CommCuDevice = (CommQuery_t)dlsym(lib, "ncclCommCuDevice");
    return JTP_OK;
}
int size() { return comm ? comm_size : 0; }
int rank() { return comm_rank; }
}  // namespace rccl

// ------------------------------------------------------------------------------------------ roctx ranges (lazy, optional)
// phases show up as named ranges in rocprofv3 --marker-trace.  The library is looked up at the
// first propagate of a plan created with JTP_ROCTX=1 in the environment; without it (or without the library) the
// calls are no-ops.
namespace roctx {
typedef int (*Push_t)(const char *);
typedef int (*Pop_t)(void);
static Push_t Push = nullptr;
static Pop_t Pop = nullptr;
static int state = 0;                   // 0 not looked up, 1 available, -1 absent
void load() {
    if (state != 0) return;
    state = -1;
    for (const char *n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
        void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!h) continue;
        Push = (Push_t)dlsym(h, "roctxRangePushA");
        Pop = (Pop_t)dlsym(h, "roctxRangePop");
        if (Push && Pop) {
            state = 1;
            return;
        }
    }
}
Range::Range(bool enabled, const char *name) : on(enabled && state == 1) { if (on) Push(name); }
Range::~Range() { if (on) Pop(); }
}  // namespace roctx

#define NCCL_TRY(expr)                                                                          \
    do {                                                                                        \
        int _r = (expr);                                                                        \
        if (_r != rccl::ncclSuccess)                                                            \
            return set_err(JTP_ECOMM, "%s failed: %s", #expr, rccl::GetErrorString(_r));         \
    } while (0)

// ------------------------------------------------------------------------------------------ exchange steps of a propagate

// (jtp_propagate.hip: comm_step; the third stand-in, JTP_FAKE_COMM=1, fills the receive buffers there and never comes here)
int rccl::exchange_step(jtp_plan *pl, BatchBuffers &bb, const JtFlow &fl, const Step &st, hipStream_t s) {
    const HostPlan &hp = pl->hp;
    if (pl->fake_comm == 2) {
        // loop-back: the step's sends and receives as one RCCL group addressed to this rank itself (RCCL pairs the k-th
        // send to a peer with the k-th receive from it: a receive without a send of its own takes this rank's first
        // outgoing message, a send without a receive lands in a spare buffer) - the real cost of the group on this GPU,
        // without the wire
        std::vector<const CommOp *> sends, recvs;
        for (int i = st.first; i < st.first + st.count; ++i) (hp.comm[i].send ? sends : recvs).push_back(&hp.comm[i]);
        const size_t n = std::max(sends.size(), recvs.size());
        int64_t most = 0;
        for (int i = st.first; i < st.first + st.count; ++i) most = std::max(most, hp.comm[i].count);
        const int rc2 = ensure_stage(pl, (size_t)most * 8 * 2);
        if (rc2) return rc2;
        double *spare = (double *)pl->stage.get();
        NCCL_TRY(rccl::GroupStart());
        for (size_t k = 0; k < n; ++k) {
            const CommOp *sd = k < sends.size() ? sends[k] : nullptr, *rv = k < recvs.size() ? recvs[k] : nullptr;
            const int64_t cnt = rv ? rv->count : sd->count;
            const double *src = sd && sd->count >= cnt ? bb.msg + fl.cur_off + sd->off : spare + most;
            double *dst = rv ? bb.msg + fl.cur_off + rv->off : spare;
            NCCL_TRY(rccl::Send(src, (size_t)cnt, rccl::ncclFloat64, rccl::comm_rank, rccl::comm, s));
            NCCL_TRY(rccl::Recv(dst, (size_t)cnt, rccl::ncclFloat64, rccl::comm_rank, rccl::comm, s));
        }
        NCCL_TRY(rccl::GroupEnd());
        return JTP_OK;
    }
    NCCL_TRY(rccl::GroupStart());
    for (int i = st.first; i < st.first + st.count; ++i) {
        const CommOp &op = hp.comm[i];
        if (op.send) NCCL_TRY(rccl::Send(bb.msg + fl.cur_off + op.off, (size_t)op.count, rccl::ncclFloat64, op.peer, rccl::comm, s));
        else NCCL_TRY(rccl::Recv(bb.msg + fl.cur_off + op.off, (size_t)op.count, rccl::ncclFloat64, op.peer, rccl::comm, s));
    }
    NCCL_TRY(rccl::GroupEnd());
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------ multi-GPU

extern "C" {

int jtp_comm_unique_id(void *id128) {
    int rc = rccl::load();
    if (rc) return rc;
    rccl::ncclUniqueId id;
    NCCL_TRY(rccl::GetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return JTP_OK;
}

int jtp_comm_init(int32_t rank, int32_t n_ranks, const void *id128, int32_t device) {
    int rc = rccl::load();
    if (rc) return rc;
    if (rccl::comm) return set_err(JTP_ECOMM, "communicator already initialised");
    HIP_TRY(hipSetDevice(device));
    rccl::ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    NCCL_TRY(rccl::CommInitRank(&rccl::comm, n_ranks, id, rank));
    rccl::comm_rank = rank;
    rccl::comm_size = n_ranks;
    return JTP_OK;
}

// What the communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice; -1 where the library has no such
// entry point): a multi-rank benchmark line carries it, so that the reader sees RCCL saw N ranks.
int jtp_comm_info(int32_t *n_ranks, int32_t *rank, int32_t *device) {
    if (!rccl::comm) return set_err(JTP_ECOMM, "communicator not initialised");
    int v = -1;
    if (n_ranks) *n_ranks = (rccl::CommCount && rccl::CommCount(rccl::comm, &v) == rccl::ncclSuccess) ? v : -1;
    v = -1;
    if (rank) *rank = (rccl::CommUserRank && rccl::CommUserRank(rccl::comm, &v) == rccl::ncclSuccess) ? v : -1;
    v = -1;
    if (device) *device = (rccl::CommCuDevice && rccl::CommCuDevice(rccl::comm, &v) == rccl::ncclSuccess) ? v : -1;
    return JTP_OK;
}

int jtp_comm_selftest(int32_t n) {
    if (!rccl::comm) return set_err(JTP_ECOMM, "communicator not initialised");
    if (n <= 0) return set_err(JTP_EINVAL, "n must be positive");
    DeviceBuf<double> abuf, bbuf;
    HIP_TRY(abuf.alloc((size_t)n));
    HIP_TRY(bbuf.alloc((size_t)n));
    double *a = abuf.get(), *b = bbuf.get();
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    std::vector<double> h(n), back(n, -1.0);
    for (int i = 0; i < n; ++i) h[i] = 0.5 * i + 1.0;
    HIP_TRY(hipMemcpyAsync(a, h.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b, 0, (size_t)n * 8, s));
    NCCL_TRY(rccl::GroupStart());
    NCCL_TRY(rccl::Send(a, (size_t)n, rccl::ncclFloat64, rccl::comm_rank, rccl::comm, s));
    NCCL_TRY(rccl::Recv(b, (size_t)n, rccl::ncclFloat64, rccl::comm_rank, rccl::comm, s));
    NCCL_TRY(rccl::GroupEnd());
    HIP_TRY(hipMemcpyAsync(back.data(), b, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipStreamDestroy(s);
    for (int i = 0; i < n; ++i)
        if (back[i] != h[i]) return set_err(JTP_ECOMM, "self send/recv mismatch at %d: %g vs %g", i, back[i], h[i]);
    return JTP_OK;
}

int jtp_comm_destroy(void) {
    if (rccl::comm) {
        NCCL_TRY(rccl::CommDestroy(rccl::comm));
        rccl::comm = nullptr;
    }
    return JTP_OK;
}

}  // extern "C"
