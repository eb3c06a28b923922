// The lifetime of a library handle, stated once (host code only).
//
// A handle derives from VrxQueue, which owns the handle's device, its non-blocking stream and its timing
// events.  vrx_X_create builds the handle inside a VrxOwned<vrx_X>, so that every error return releases it, and
// hands it out with release(); vrx_X_destroy is vrx_destroy.  The rule of teardown: the device is made current
// and the stream has drained BEFORE anything is freed or destroyed -- then the events and the stream go, then
// the handle's own destructor runs and its DevBuf members free their memory.  A queue that was never opened
// (no stream) tears down to nothing.
#pragma once

#include <memory>

#include "vrx_common.h"

#define VRX_TRY(expr)                                                                   \
    do {                                                                                \
        if (int rc__ = (expr)) return rc__;                                             \
    } while (0)

struct VrxQueue {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    VrxQueue() = default;
    VrxQueue(const VrxQueue&) = delete;
    VrxQueue& operator=(const VrxQueue&) = delete;
    // what every create does: the device checked and current, a stream of its own, n_events timing events
    int open(const char* who, int dev, int n_events) {
        VRX_TRY(vrx_use_device(who, dev));
        device = dev;
        VRX_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return events(n_events);
    }
    // events alone, for timing on a borrowed stream (vrx_problem_ambient)
    int events(int n_events) {
        VRX_REQUIRE(n_events <= 5, "a handle holds at most 5 events");
        for (int i = 0; i < n_events; ++i) VRX_HIP(hipEventCreate(&ev[i]));
        return VRX_OK;
    }
    // what every later entry point begins with
    int use() const {
        VRX_HIP(hipSetDevice(device));
        return VRX_OK;
    }
    // milliseconds from event a to event b (both reached); out may be null
    int ms(int a, int b, double* out) const {
        if (!out) return VRX_OK;
        float t = 0.f;
        VRX_HIP(hipEventElapsedTime(&t, ev[a], ev[b]));
        *out = t;
        return VRX_OK;
    }
    void close() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
        }
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
    ~VrxQueue() { close(); }
};

template <class H>
void vrx_destroy(H* h) {
    if (!h) return;
    h->close();
    delete h;
}

struct VrxDelete {
    template <class H>
    void operator()(H* h) const {
        vrx_destroy(h);
    }
};
template <class H>
using VrxOwned = std::unique_ptr<H, VrxDelete>;

// Room for count items; a buffer that has to grow takes an eighth more than asked.
template <typename T>
hipError_t vrx_reserve(DevBuf<T>& b, size_t count) {
    return b.n >= count ? hipSuccess : b.alloc(count + count / 8);
}

// One hipCUB call from one spelling of its arguments: VRX_CUB_CALL binds everything behind the temporary
// storage, vrx_cub asks the call for its size, grows the caller's buffer to it and runs it.  A unit that wants
// its storage in place ahead of a timed region sizes there (VRX_CUB_SIZE) and runs the same call later in the
// storage it sized (VRX_CUB_SIZED: no query, nothing on the host between two launches).
#define VRX_CUB_CALL(algo, ...) \
    [&](void* tmp__, size_t& bytes__) { return hipcub::algo(tmp__, bytes__, __VA_ARGS__); }

enum VrxCub { VRX_CUB_RUN, VRX_CUB_SIZE, VRX_CUB_SIZED };

template <typename T, class Call>
hipError_t vrx_cub(DevBuf<T>& tmp, Call call, VrxCub mode = VRX_CUB_RUN) {
    static_assert(sizeof(T) == 1, "temporary storage is counted in bytes");
    size_t bytes = tmp.n;
    if (mode != VRX_CUB_SIZED) {
        bytes = 0;
        hipError_t e = call(nullptr, bytes);
        if (e == hipSuccess) e = vrx_reserve(tmp, bytes ? bytes : 1);
        if (e != hipSuccess || mode == VRX_CUB_SIZE) return e;
    }
    return call(tmp.p, bytes);
}
