// What every device workspace of libplenum_verify.so is made of (host code): the early-return macro,
// grow-only device and pinned buffers, the event hand-over between caller streams, and the 256-byte
// staging layout. Callers serialise use of a workspace on its own mutex.
#ifndef PV_WORKSPACE_H
#define PV_WORKSPACE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/plenum_verify.h"

// Records `msg` as the calling thread's pv_last_error() and returns `code`.
int pv_fail(int code, const std::string& msg);

#define PV_HIP(call, code)                                                                             \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return pv_fail(code, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline uint64_t pv_up256(uint64_t x) { return (x + 255) & ~255ull; }

// off[0..n] is non-decreasing (no early exit: the loop vectorises, and valid input is the common case).
inline bool pv_offsets_monotone(const uint64_t* off, uint64_t n) {
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; i++) bad |= off[i + 1] < off[i];
    return bad == 0;
}

// A grow-only device block. A failed grow leaves it empty (p null, cap 0), never a stale capacity over
// a null pointer: the next grow of any size allocates again.
struct PvDevBuf {
    uint8_t* p = nullptr;
    uint64_t cap = 0;  // bytes

    int grow(uint64_t want) {
        if (want <= cap) return PV_OK;
        release();  // hipFree synchronises: no launch still reads the old block
        PV_HIP(hipMalloc((void**)&p, want), PV_ERR_ALLOC);
        cap = want;
        return PV_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// The same in pinned host memory; `flags` as for hipHostMalloc.
struct PvPinnedBuf {
    uint8_t* p = nullptr;
    uint64_t cap = 0;  // bytes

    int grow(uint64_t want, unsigned flags) {
        if (want <= cap) return PV_OK;
        release();
        PV_HIP(hipHostMalloc((void**)&p, want, flags), PV_ERR_ALLOC);
        cap = want;
        return PV_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// The hand-over of a workspace between caller streams: every use ends by recording `ev` on its stream,
// and a use on a DIFFERENT stream first waits for it, so two batches enqueued on two streams never
// share the workspace at the same time.
struct PvHandover {
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;

    int ensure() {  // the event exists from the first use on
        if (!ev) PV_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming), PV_ERR_NO_DEVICE);
        return PV_OK;
    }
    // `waiter` waits for the last use unless that was on `user`.
    int wait(hipStream_t waiter, hipStream_t user) {
        if (int rc = ensure()) return rc;
        if (last && last != user) PV_HIP(hipStreamWaitEvent(waiter, ev, 0), PV_ERR_LAUNCH);
        return PV_OK;
    }
    int begin(hipStream_t s) { return wait(s, s); }
    int end(hipStream_t s) {
        if (int rc = ensure()) return rc;
        PV_HIP(hipEventRecord(ev, s), PV_ERR_LAUNCH);
        last = s;
        return PV_OK;
    }
    // `s` is being destroyed.
    void forget(hipStream_t s) {
        if (last == s) last = nullptr;
    }
    void destroy() {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
        last = nullptr;
    }
};

// Offsets of a staging block's sections, each 256-byte aligned and at least 256 bytes; `at` is the
// block's size so far.
struct PvLayout {
    uint64_t at = 0;
    uint64_t add(uint64_t bytes) {
        const uint64_t o = at;
        at += pv_up256(bytes ? bytes : 1);
        return o;
    }
};

#endif  // PV_WORKSPACE_H
