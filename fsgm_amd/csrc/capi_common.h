// capi_common.h -- plumbing shared by the C-ABI translation units: error reporting, device selection, the per-device
// plan caches and the event timer of the *_time entry points
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdarg.h>
#include <stdio.h>
#include <vector>
#include "../../include/fsgm.h"

namespace fsgm {

char* last_error_buf();   // thread-local, 512 bytes

inline fsgm_status fail(fsgm_status st, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return st;
}

#define FSGM_HIP(expr)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::fsgm::fail(FSGM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define FSGM_REQUIRE(cond, ...)                                          \
    do {                                                                 \
        if (!(cond)) return ::fsgm::fail(FSGM_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// NOMEM for an allocation that did not fit, HIP for every other failure; the message is "what: <HIP's text>"
inline fsgm_status hip_status(hipError_t e, const char* what = nullptr) {
    if (e == hipSuccess) return FSGM_OK;
    const fsgm_status st = e == hipErrorOutOfMemory ? FSGM_ERR_NOMEM : FSGM_ERR_HIP;
    return what ? fail(st, "%s: %s", what, hipGetErrorString(e)) : fail(st, "%s", hipGetErrorString(e));
}

inline fsgm_status device_count(int* ndev) {
    *ndev = 0;
    if (hipGetDeviceCount(ndev) != hipSuccess || *ndev == 0)
        return fail(FSGM_ERR_HIP, "no HIP device available (libfsgm_hip has no CPU fallback)");
    return FSGM_OK;
}
// makes `device` current (entry points call it after their argument checks: it is the first thing that needs a GPU)
inline fsgm_status use_device(int device) {
    int ndev;
    const fsgm_status st = device_count(&ndev);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
    FSGM_HIP(hipSetDevice(device));
    return FSGM_OK;
}

// The host-pointer entry points keep their cached plans / arenas PER DEVICE and hold that device's lock for the length of a
// call: calls on different devices run side by side (fsgm_*_batch_devices_host starts one host thread per device of its
// list), calls on one device take turns -- they would share the GPU anyway.
constexpr int FSGM_MAX_DEVICES = 64;
template <class T>
struct PerDevice {
    std::mutex mu[FSGM_MAX_DEVICES];
    T v[FSGM_MAX_DEVICES];
};
#define FSGM_DEVICE_SLOT(dev) FSGM_REQUIRE((dev) >= 0 && (dev) < ::fsgm::FSGM_MAX_DEVICES, "device %d out of range", (int)(dev))

// The plans behind the host- and device-pointer entry points of one kind: per device the last `cap` that were made, oldest
// evicted first.  find / insert want the device's lock held (mu(device), for the length of the call that uses the plan).
// pinned (may be null): a plan it answers true for is never evicted -- a captured graph names its buffers, its stream and its
// events --, does not count against `cap`, and lives until clear().
template <class P>
struct PlanCache {
    PerDevice<std::vector<P*>> plans;
    const size_t cap;
    void (*const destroy)(P*);
    bool (*const pinned)(const P*);
    PlanCache(size_t cap_, void (*destroy_)(P*), bool (*pinned_)(const P*) = nullptr) : cap(cap_), destroy(destroy_), pinned(pinned_) {}

    std::mutex& mu(int device) { return plans.mu[device]; }
    template <class Match>
    P* find(int device, Match&& match) {
        for (P* p : plans.v[device])
            if (match(p)) return p;
        return nullptr;
    }
    void insert(int device, P* p) {
        std::vector<P*>& v = plans.v[device];
        size_t loose = 0;
        for (P* q : v) loose += !(pinned && pinned(q));
        if (loose >= cap) {                                      // the oldest plan that no graph names
            for (auto it = v.begin(); it != v.end(); ++it)
                if (!(pinned && pinned(*it))) { destroy(*it); v.erase(it); break; }
        }
        v.push_back(p);
    }
    void clear() {
        for (int d = 0; d < FSGM_MAX_DEVICES; d++) {
            std::lock_guard<std::mutex> lk(plans.mu[d]);
            for (P* p : plans.v[d]) destroy(p);
            plans.v[d].clear();
        }
    }
};

// ms_avg = the time of one enqueue() (a callable returning fsgm_status that queues work on `stream`), averaged over
// `iters` of them behind `warmup` untimed ones
template <class Enqueue>
fsgm_status time_enqueues(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, int warmup, int iters, Enqueue&& enqueue, float* ms_avg) {
    for (int i = -warmup; i < iters; i++) {
        if (i == 0) FSGM_HIP(hipEventRecord(ev0, stream));
        const fsgm_status st = enqueue();
        if (st != FSGM_OK) return st;
    }
    FSGM_HIP(hipEventRecord(ev1, stream));
    FSGM_HIP(hipEventSynchronize(ev1));
    float ms = 0;
    FSGM_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    *ms_avg = ms / iters;
    return FSGM_OK;
}

// cmax[f] = the largest byte of frame f of n host volumes of `voxels` bytes each (the sgm(C) / sgm2d(C) host forms' u8 volumes);
// a frame that holds one above the call's declared cost_bound is refused
inline fsgm_status frame_cost_maxima(const char* who, const uint8_t* C, int n, size_t voxels, int cost_bound, int* cmax) {
    for (int f = 0; f < n; f++) {
        const uint8_t* v = C + (size_t)f * voxels;
        int m = 0;
        for (size_t i = 0; i < voxels; i++) m = v[i] > m ? v[i] : m;
        FSGM_REQUIRE(m <= cost_bound, "%s: frame %d holds a cost of %d, above cost_bound %d", who, f, m, cost_bound);
        cmax[f] = m;
    }
    return FSGM_OK;
}

// Scope guard for host-pointer entry points: work queued on `st` may still read the caller's input
// buffers or write its output buffers (async copies), so every exit that is not the normal one
// (which has synchronised already and calls dismiss()) drains the stream before the caller gets
// control back.
struct StreamGuard {
    hipStream_t st;
    bool armed = true;
    explicit StreamGuard(hipStream_t s) : st(s) {}
    void dismiss() { armed = false; }
    ~StreamGuard() { if (armed) (void)hipStreamSynchronize(st); }
    StreamGuard(const StreamGuard&) = delete;
    StreamGuard& operator=(const StreamGuard&) = delete;
};

}  // namespace fsgm
