// Owning buffers for the engine's device and pinned host memory (the engine's translation units only: jtp_engine.h).
// A buffer is either empty or holds one complete allocation: every operation that fails leaves it empty, so `if (!buf)` is
// a correct "not built yet" test.  Each buffer books its bytes with its plan's MemLedger (jtp_stats.device_bytes) and with the
// process-wide counters behind jtp_debug_live_bytes; the ledger also carries the test hook that makes an allocation fail.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <utility>
#include <vector>

struct MemLedger {
    int64_t bytes = 0;          // held now by the buffers booked here
    int64_t fail_in = 0;        // test hook (JTP_FAIL_ALLOC, jtp_debug_set "fail_alloc"): the fail_in-th allocation from now reports
                                // hipErrorOutOfMemory on the host, without calling HIP; 0: off
};

inline std::atomic<int64_t> g_live_bytes[2];       // [0] device, [1] pinned host: the whole process (ONE object for all units)

template <typename T, bool PINNED>
class MemBuf {
    T *p_ = nullptr;
    size_t n_ = 0;
    MemLedger *ledger_ = nullptr;

public:
    explicit MemBuf(MemLedger *ledger = nullptr) : ledger_(ledger) {}
    MemBuf(const MemBuf &) = delete;
    MemBuf &operator=(const MemBuf &) = delete;
    MemBuf(MemBuf &&o) noexcept : p_(o.p_), n_(o.n_), ledger_(o.ledger_) { o.p_ = nullptr, o.n_ = 0; }
    MemBuf &operator=(MemBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_, ledger_ = o.ledger_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~MemBuf() { reset(); }

    T *get() const { return p_; }
    size_t size() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
    explicit operator bool() const { return p_ != nullptr; }

    void reset() {
        if (!p_) return;
        (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        book(-(int64_t)bytes());
        p_ = nullptr, n_ = 0;
    }
    // n elements, uninitialised (n == 0: the buffer stays empty); `flags`: of hipHostMalloc (pinned buffers)
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
        reset();
        if (n == 0) return hipSuccess;
        if (ledger_ && ledger_->fail_in > 0 && --ledger_->fail_in == 0) return hipErrorOutOfMemory;
        void *q = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&q, n * sizeof(T), flags) : hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(q), n_ = n;
        book((int64_t)bytes());
        return hipSuccess;
    }
    // grow-only: the buffer in place stays when it holds n elements already
    hipError_t reserve(size_t n) { return n_ >= n ? hipSuccess : alloc(n); }
    // max(n, at_least) elements, the first n copied from the host
    hipError_t upload(const T *src, size_t n, size_t at_least = 0) {
        hipError_t e = alloc(n > at_least ? n : at_least);
        if (e == hipSuccess && n > 0) e = hipMemcpy(p_, src, n * sizeof(T), PINNED ? hipMemcpyHostToHost : hipMemcpyHostToDevice);
        if (e != hipSuccess) reset();
        return e;
    }
    hipError_t upload(const std::vector<T> &v, size_t at_least = 0) { return upload(v.data(), v.size(), at_least); }

private:
    void book(int64_t delta) {
        if (ledger_) ledger_->bytes += delta;
        g_live_bytes[PINNED ? 1 : 0] += delta;
    }
};

template <typename T> using DeviceBuf = MemBuf<T, false>;
template <typename T> using PinnedBuf = MemBuf<T, true>;
