// Shared host-side plumbing of libpowdr_gpu: the launch stream, optional
// per-kernel HIP-event timing, error helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace pw {

hipStream_t stream();
void set_stream(hipStream_t s);

// Timing: when enabled every PW_LAUNCH is bracketed by two events recorded on
// the launch stream; report() synchronises and aggregates by kernel name.
bool timing_enabled();
void timing_begin(const char* name, hipEvent_t* e0);
void timing_end(const char* name, hipEvent_t e0);

struct ScopedKernelTimer {
    const char* name;
    hipEvent_t e0 = nullptr;
    bool on;
    explicit ScopedKernelTimer(const char* n) : name(n), on(timing_enabled()) {
        if (on) timing_begin(name, &e0);
    }
    ~ScopedKernelTimer() {
        if (on) timing_end(name, e0);
    }
};

inline int hip_status(hipError_t e) { return (int)e; }

#define PW_HIP_TRY(expr)                          \
    do {                                          \
        hipError_t _e = (expr);                   \
        if (_e != hipSuccess) return (int)_e;     \
    } while (0)

inline unsigned div_up(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// the log height of the smallest trace of at least two rows that holds `rows`
inline uint32_t ceil_log2_at_least_1(unsigned long long rows) {
    uint32_t lh = 1;
    while ((1ull << lh) < rows) ++lh;
    return lh;
}

struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int device = -1;  // the device the buffer lives on: a host thread (thread_local contexts) may have moved to another GPU
    int ensure(size_t need) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return (int)e;
        if (p && dev == device && need <= bytes) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        e = hipMalloc(&p, need);
        if (e != hipSuccess) return (int)e;
        bytes = need;
        device = dev;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() { release(); }  // thread_local owners (per-thread segment contexts) give their memory back when the thread exits
};

// a small host table into a buffer of its own, with `slack` spare entries at its end that kernels may read
template <class T>
inline int upload_table(DeviceBuf& b, const T* v, size_t n, size_t slack = 0) {
    if (int rc = b.ensure((n + slack) * sizeof(T))) return rc;
    if (n) PW_HIP_TRY(hipMemcpy(b.p, v, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// Which code paths the calling thread's library calls took (powdr_gpu_call_stats): parity tests assert that a workload
// really exercised the job forms / kernels it is meant to cover instead of inferring it from sizes.
enum CallStat : int {
    kStatGatherSparseJobs = 0, kStatGatherWholeJobs, kStatGatherChunkJobs, kStatGatherCalls,
    kStatBusFastInteractions, kStatBusInterpretedInteractions, kStatBusBinnedWindows, kStatBusDirectCalls,
    kStatBusXbcCalls, kStatJitKernelLaunches, kStatInterpreterKernelLaunches, kStatNttStridedFixedLaunches, kStatCount = 16
};
uint64_t* call_stats();  // this thread's kStatCount counters

}  // namespace pw
