// What every device workspace of libplenum_verify.so is made of (host code): the early-return macro,
// grow-only device and pinned buffers, the owner of a set of resources created once, the event hand-over
// between caller streams, the 256-byte staging layout, and the AUTO / HOST / DEVICE path choice. The
// staged call of a host-buffer entry built on them, PvStage, is in stage.h. Callers serialise use of a
// workspace on its own mutex.
#ifndef PV_WORKSPACE_H
#define PV_WORKSPACE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/plenum_verify.h"

// Records `msg` as the calling thread's pv_last_error() and returns `code`.
int pv_fail(int code, const std::string& msg);

#define PV_HIP(call, code)                                                                             \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return pv_fail(code, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// A kernel launch and its check: a launch the runtime refuses returns PV_ERR_LAUNCH from the caller.
#define PV_LAUNCH(k, ...)                         \
    do {                                          \
        hipLaunchKernelGGL(k, __VA_ARGS__);       \
        PV_HIP(hipGetLastError(), PV_ERR_LAUNCH); \
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

// The owner of a set of resources created once and released together (the engine context, its key
// cache): each call creates one resource into the caller's plain field and remembers it, so release is
// one call that cannot forget an entry. A failed creation leaves the field null and records nothing.
// No destructor: an owner inside a global must not call a runtime that may be gone at process exit.
struct PvOwner {
    std::vector<void*> devs, pins;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;

    template <class T>
    int dev(T*& p, uint64_t bytes) {
        void* q = nullptr;
        p = nullptr;
        PV_HIP(hipMalloc(&q, bytes), PV_ERR_ALLOC);
        devs.push_back(q);
        p = static_cast<T*>(q);
        return PV_OK;
    }
    template <class T>
    int pinned(T*& p, uint64_t bytes, unsigned flags) {
        void* q = nullptr;
        p = nullptr;
        PV_HIP(hipHostMalloc(&q, bytes, flags), PV_ERR_ALLOC);
        pins.push_back(q);
        p = static_cast<T*>(q);
        return PV_OK;
    }
    int stream(hipStream_t& s, unsigned flags) {
        hipStream_t q = s = nullptr;
        PV_HIP(hipStreamCreateWithFlags(&q, flags), PV_ERR_NO_DEVICE);
        streams.push_back(s = q);
        return PV_OK;
    }
    int stream(hipStream_t& s, unsigned flags, int priority) {
        hipStream_t q = s = nullptr;
        PV_HIP(hipStreamCreateWithPriority(&q, flags, priority), PV_ERR_NO_DEVICE);
        streams.push_back(s = q);
        return PV_OK;
    }
    int event(hipEvent_t& e, unsigned flags) {
        hipEvent_t q = e = nullptr;
        PV_HIP(hipEventCreateWithFlags(&q, flags), PV_ERR_NO_DEVICE);
        events.push_back(e = q);
        return PV_OK;
    }
    // Frees the recorded device block `p` now (the half of an optional pair whose other half failed).
    void drop(void* p) {
        for (size_t i = devs.size(); i-- > 0;)
            if (devs[i] == p) {
                (void)hipFree(p);
                devs.erase(devs.begin() + i);
                return;
            }
    }
    // Each kind newest first. The device blocks go first: hipFree synchronises, so no stream or event
    // is destroyed under work that is still running.
    void release_all() {
        while (!devs.empty()) (void)hipFree(devs.back()), devs.pop_back();
        while (!pins.empty()) (void)hipHostFree(pins.back()), pins.pop_back();
        while (!events.empty()) (void)hipEventDestroy(events.back()), events.pop_back();
        while (!streams.empty()) (void)hipStreamDestroy(streams.back()), streams.pop_back();
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
    // One use on `s`: the hand-over begun, `body` run, and the hand-over ended also after a failure
    // (whatever did get enqueued is covered). The first error is returned.
    template <class F>
    int run(hipStream_t s, F&& body) {
        if (int rc = begin(s)) return rc;
        const int rc = body();
        const int rc2 = end(s);
        return rc ? rc : rc2;
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

// The path of a host-buffer entry `who` under a PV_MERKLE_* / PV_TRIE_* mode (both AUTO 0, HOST 1,
// DEVICE 2): PV_ERR_NO_DEVICE for a forced device path without a device, else PV_OK with *device set
// (forced, or AUTO with `work` at or above `auto_min`).
inline int pv_choose_path(int mode, bool have_dev, uint64_t work, uint64_t auto_min, const char* who, bool* device) {
    static_assert(PV_MERKLE_AUTO == PV_TRIE_AUTO && PV_MERKLE_DEVICE == PV_TRIE_DEVICE, "one set of mode values");
    if (mode == PV_TRIE_DEVICE && !have_dev)
        return pv_fail(PV_ERR_NO_DEVICE, std::string(who) + ": the device path is forced and no device is initialised");
    *device = have_dev && (mode == PV_TRIE_DEVICE || (mode == PV_TRIE_AUTO && work >= auto_min));
    return PV_OK;
}

#endif  // PV_WORKSPACE_H
