// A stand-in for <hip/hip_runtime.h> that lets workspace_check.cpp compile csrc/workspace.h with g++ and
// no GPU: allocations over malloc, events and streams as small integers, copies as memcpy between those
// blocks, a log of every runtime call, a switch that makes the k-th creation from now on (a block, a stream
// or an event) fail and one of its own for the k-th copy or synchronisation.
#ifndef STUB_HIP_RUNTIME_H
#define STUB_HIP_RUNTIME_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorLaunchFailure = 719 };
inline const char* hipGetErrorString(hipError_t e) {
    return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory (stub)" : "launch failure (stub)";
}
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };

typedef struct StubEvent* hipEvent_t;    // never dereferenced: (hipEvent_t)id
typedef struct StubStream* hipStream_t;  // the same
constexpr unsigned hipHostMallocDefault = 0, hipHostMallocPortable = 1, hipEventDisableTiming = 2;
constexpr unsigned hipStreamNonBlocking = 1, hipEventReleaseToDevice = 0x40000000;

struct StubCall {
    std::string name;  // "hipMalloc", "hipStreamWaitEvent", ...
    uintptr_t a, b;    // bytes and flags / stream and event / the pointer freed / the handle made and its flags /
                       // a copy's destination and bytes / the stream synchronised
    int c = 0;         // the priority of a stream made with one / a copy's kind
};
struct StubState {
    std::vector<StubCall> log;
    int fail_in = 0;       // > 0: the fail_in-th creation from now fails
    int fail_call_in = 0;  // > 0: the fail_call_in-th copy or synchronisation from now fails (and copies nothing)
    uint64_t dev_allocs = 0, dev_frees = 0, host_allocs = 0, host_frees = 0, events = 0, events_destroyed = 0;
    uint64_t streams = 0, streams_destroyed = 0;
};
inline StubState& stub() {
    static StubState s;
    return s;
}
inline bool stub_fails() { return stub().fail_in > 0 && --stub().fail_in == 0; }
inline hipError_t stub_alloc(const char* name, void** p, size_t bytes, unsigned flags, uint64_t& count) {
    stub().log.push_back({name, bytes, flags});
    if (stub_fails()) return hipErrorOutOfMemory;
    *p = malloc(bytes);
    count++;
    return hipSuccess;
}
inline hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc("hipMalloc", p, bytes, 0, stub().dev_allocs); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
    return stub_alloc("hipHostMalloc", p, bytes, flags, stub().host_allocs);
}
inline hipError_t hipFree(void* p) {
    stub().log.push_back({"hipFree", (uintptr_t)p, 0});
    stub().dev_frees++;
    free(p);
    return hipSuccess;
}
inline hipError_t hipHostFree(void* p) {
    stub().log.push_back({"hipHostFree", (uintptr_t)p, 0});
    stub().host_frees++;
    free(p);
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    if (stub_fails()) {
        stub().log.push_back({"hipEventCreateWithFlags", 0, flags});
        return hipErrorOutOfMemory;
    }
    *e = (hipEvent_t)(uintptr_t)(++stub().events);
    stub().log.push_back({"hipEventCreateWithFlags", (uintptr_t)*e, flags});
    return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
    stub().log.push_back({"hipEventDestroy", (uintptr_t)e, 0});
    stub().events_destroyed++;
    return hipSuccess;
}
inline hipError_t stub_stream(const char* name, hipStream_t* s, unsigned flags, int priority) {
    if (stub_fails()) {
        stub().log.push_back({name, 0, flags, priority});
        return hipErrorOutOfMemory;
    }
    *s = (hipStream_t)(uintptr_t)(0x1000 + ++stub().streams);
    stub().log.push_back({name, (uintptr_t)*s, flags, priority});
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    return stub_stream("hipStreamCreateWithFlags", s, flags, 0);
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority) {
    return stub_stream("hipStreamCreateWithPriority", s, flags, priority);
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
    stub().log.push_back({"hipStreamDestroy", (uintptr_t)s, 0});
    stub().streams_destroyed++;
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    stub().log.push_back({"hipEventRecord", (uintptr_t)s, (uintptr_t)e});
    return hipSuccess;
}
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    stub().log.push_back({"hipStreamWaitEvent", (uintptr_t)s, (uintptr_t)e});
    return hipSuccess;
}
inline bool stub_call_fails() { return stub().fail_call_in > 0 && --stub().fail_call_in == 0; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    stub().log.push_back({"hipMemcpyAsync", (uintptr_t)dst, bytes, (int)kind});
    if (stub_call_fails()) return hipErrorLaunchFailure;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t s) {
    stub().log.push_back({"hipStreamSynchronize", (uintptr_t)s, 0});
    return stub_call_fails() ? hipErrorLaunchFailure : hipSuccess;
}

#endif  // STUB_HIP_RUNTIME_H
