// mcr_host.h — host-side utilities shared by the translation units of libmcr_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/mcr.h"

namespace mcr {

void set_error(const char* fmt, ...);          // thread-local message for mcr_last_error()
int hip_fail(hipError_t e, const char* what);  // records the HIP error text, returns MCR_ERR_HIP
int use_device(int device);                    // hipSetDevice with range / no-device checks

// Every ABI entry point works on `device` and then puts the calling thread's current device back: a
// caller that holds GPU 3 (one process per GPU under torch.distributed) keeps GPU 3 after calling a
// helper with device 0.
class DeviceScope {
public:
    explicit DeviceScope(int device) : prev_(-1), rc(MCR_OK) {
        if (hipGetDevice(&prev_) != hipSuccess) { (void)hipGetLastError(); prev_ = -1; }
        rc = use_device(device);
        if (rc != MCR_OK || prev_ == device) prev_ = -1;   // nothing to restore
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    ~DeviceScope() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }

private:
    int prev_;

public:
    int rc;
};
#define MCR_ENTER_DEVICE(device)         \
    ::mcr::DeviceScope mcr_scope_(device); \
    if (mcr_scope_.rc != MCR_OK) return mcr_scope_.rc

// RAII bag of device allocations for the rarely used *_host convenience entry points (helpers, shock rows).
class DeviceArena {
public:
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() {
        for (void* p : ptrs_) (void)hipFree(p);
    }
    hipError_t alloc(void** out, size_t bytes) {
        hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        if (e == hipSuccess) ptrs_.push_back(*out);
        return e;
    }

private:
    std::vector<void*> ptrs_;
};

// Context of one host-buffer call (mcr_run_batch_host*): a private NON-BLOCKING stream — concurrent callers (server
// executor threads) do not serialise on the null stream or on a device-wide synchronise — and one scratch block that the
// call carves its device buffers from.  Contexts live in a PROCESS-WIDE pool keyed by device (mutex-guarded): a call
// leases one for its duration (mcr_hip.hip: IdlePool, HostCall) and hands it back, so short-lived caller threads and the per-call shard
// workers of the multi-device entry reuse the same few contexts instead of leaving one behind each (round 2 kept them in
// thread-local storage: one stream + up to 256 MiB of HBM leaked per thread that ever called).  At most
// kHostCtxIdlePerDevice idle contexts per device stay cached, each with a block of at most kHostCtxKeepBytes (larger
// blocks are freed when the call ends); mcr_release_cached() frees the idle ones on demand.  Concurrency is bounded by
// the callers: N simultaneous calls use N contexts.
constexpr size_t kHostCtxKeepBytes = (size_t)256 << 20;
constexpr int kHostCtxIdlePerDevice = 4;
struct HostCtx {
    int device;
    hipStream_t stream;
    void* block;
    size_t capacity;
};

// Fork/join streams for calls that spread independent pieces of work over several HIP streams and join them back onto
// the caller's stream: kForkStreams non-blocking side streams with one "done" event each, and a fork event.  Leased from
// a process-wide pool keyed by device (mcr_hip.hip) for the duration of the call's ENQUEUE; at most
// kStreamForkIdlePerDevice idle sets per device stay cached (mcr_release_cached frees them).
constexpr int kForkStreams = 8;
constexpr int kStreamForkIdlePerDevice = 2;
struct StreamFork {
    int device;
    hipStream_t side[kForkStreams];
    hipEvent_t done[kForkStreams];
    hipEvent_t fork;
};

// Joint outcomes (mcr_aggregate.hip): option k's success mask is a row of joint_mask_words(n_paths) 64-bit words, bit b of
// word w = path 64 w + b of the range.
inline uint64_t joint_mask_words(uint64_t n_paths) { return n_paths / 64 + (n_paths % 64 ? 1 : 0); }
// pack_success_kernel: a uint8 [n_paths] success column -> its mask row (every word written, tail bits 0)
int launch_pack_success(const uint8_t* success, uint64_t n_paths, uint64_t* row, hipStream_t stream);
// joint_counts_kernel: zeroes joint [n][n] and extremes [2] (may be null), then counts the rows (n_paths == 0: zeroes alone)
int launch_joint_counts(const uint64_t* masks, int n, uint64_t n_paths, uint64_t* joint, uint64_t* extremes, hipStream_t stream);

// Outcome probes (mcr_aggregate.hip), per-option route: final_balance[i] = NaN where years_to_ruin[i] is a number (the path failed)
int launch_nan_failed(double* final_balance, const double* years_to_ruin, uint64_t n_paths, hipStream_t stream);

}  // namespace mcr
