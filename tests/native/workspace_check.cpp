// csrc/workspace.h compiled with g++ against the stub runtime in stub_hip/ (no GPU): the grow-only buffers
// leave themselves empty after a failed allocation, the hand-over issues exactly the waits it should, the
// staging layout never overlaps. Prints one JSON object of named checks; tests/test_workspace_host.py
// builds this with -fsanitize=address,undefined and asserts on it.
#include <stdio.h>

#include <string>
#include <vector>

#include "../../indy-plenum_amd/csrc/workspace.h"

static std::string g_last_error;
int pv_fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

static std::string g_json;
static void put(const char* group, const char* name, bool ok) {
    g_json += std::string(g_json.empty() ? "" : ", ") + "\"" + group + "." + name + "\": " + (ok ? "true" : "false");
}

static size_t calls() { return stub().log.size(); }
// the calls named `name` logged from position `from` on
static std::vector<StubCall> since(size_t from, const char* name) {
    std::vector<StubCall> v;
    for (size_t i = from; i < stub().log.size(); i++)
        if (stub().log[i].name == name) v.push_back(stub().log[i]);
    return v;
}

template <class Buf, class Grow>
static void check_buffer(const char* group, const char* alloc_name, Grow grow) {
    Buf b;
    put(group, "starts_empty", b.p == nullptr && b.cap == 0);
    put(group, "first_grow", grow(b, 1000) == PV_OK && b.p != nullptr && b.cap == 1000);
    b.p[0] = 1;
    b.p[999] = 2;  // the block is really that large (AddressSanitizer watches)
    size_t at = calls();
    const uint8_t* before = b.p;
    put(group, "grow_within_cap_is_no_call", grow(b, 1000) == PV_OK && grow(b, 1) == PV_OK && grow(b, 0) == PV_OK &&
                                                 calls() == at && b.p == before && b.cap == 1000);
    put(group, "typed_accessor", (void*)b.template as<uint64_t>() == (void*)b.p);
    put(group, "regrow", grow(b, 5000) == PV_OK && b.cap == 5000 && since(at, alloc_name).size() == 1);
    b.p[4999] = 3;
    // the allocation of a larger block fails: empty, not the old capacity over a null pointer
    stub().fail_in = 1;
    g_last_error.clear();
    put(group, "failed_grow_returns_alloc_error", grow(b, 9000) == PV_ERR_ALLOC && !g_last_error.empty());
    put(group, "failed_grow_leaves_empty", b.p == nullptr && b.cap == 0);
    // any size allocates again, one below the old capacity included
    at = calls();
    put(group, "smaller_grow_after_failure_allocates",
        grow(b, 100) == PV_OK && b.p != nullptr && b.cap == 100 && since(at, alloc_name).size() == 1);
    b.p[99] = 4;
    b.release();
    put(group, "release_empties", b.p == nullptr && b.cap == 0);
    at = calls();
    b.release();
    put(group, "second_release_is_no_call", calls() == at && b.p == nullptr && b.cap == 0);
    put(group, "grow_after_release", grow(b, 64) == PV_OK && b.cap == 64);
    b.release();
}

int main() {
    check_buffer<PvDevBuf>("dev", "hipMalloc", [](PvDevBuf& b, uint64_t want) { return b.grow(want); });
    check_buffer<PvPinnedBuf>("pinned", "hipHostMalloc",
                              [](PvPinnedBuf& b, uint64_t want) { return b.grow(want, hipHostMallocPortable); });
    put("dev", "allocs_equal_frees", stub().dev_allocs == stub().dev_frees && stub().dev_allocs == 4);
    put("pinned", "allocs_equal_frees", stub().host_allocs == stub().host_frees && stub().host_allocs == 4);
    put("dev", "call_counts", since(0, "hipMalloc").size() == 5 && since(0, "hipFree").size() == 4);
    {
        bool portable = true;
        for (const StubCall& c : since(0, "hipHostMalloc")) portable = portable && c.b == hipHostMallocPortable;
        PvPinnedBuf b;
        const size_t at = calls();
        (void)b.grow(10, hipHostMallocDefault);
        const std::vector<StubCall> c = since(at, "hipHostMalloc");
        put("pinned", "flags_passed_through", portable && c.size() == 1 && c[0].a == 10 && c[0].b == hipHostMallocDefault);
        b.release();
    }
    {
        const hipStream_t A = (hipStream_t)0x10, B = (hipStream_t)0x20, C = (hipStream_t)0x30, X = (hipStream_t)0x40;
        PvHandover h;
        size_t at = calls();
        bool ok = h.begin(A) == PV_OK;
        std::vector<StubCall> made = since(at, "hipEventCreateWithFlags");
        put("hand", "first_begin_creates_event_without_timing",
            ok && h.ev != nullptr && made.size() == 1 && made[0].b == hipEventDisableTiming);
        put("hand", "first_begin_no_wait", since(at, "hipStreamWaitEvent").empty());
        at = calls();
        ok = h.end(A) == PV_OK;
        std::vector<StubCall> rec = since(at, "hipEventRecord");
        put("hand", "end_records_on_its_stream",
            ok && h.last == A && rec.size() == 1 && rec[0].a == (uintptr_t)A && rec[0].b == (uintptr_t)h.ev);
        at = calls();
        put("hand", "same_stream_no_wait", h.begin(A) == PV_OK && calls() == at);
        at = calls();
        ok = h.begin(B) == PV_OK;
        std::vector<StubCall> w = since(at, "hipStreamWaitEvent");
        put("hand", "other_stream_one_wait_on_it",
            ok && calls() == at + 1 && w.size() == 1 && w[0].a == (uintptr_t)B && w[0].b == (uintptr_t)h.ev);
        (void)h.end(B);
        at = calls();
        put("hand", "wait_compares_user_not_waiter", h.wait(C, B) == PV_OK && calls() == at);
        ok = h.wait(C, A) == PV_OK;
        w = since(at, "hipStreamWaitEvent");
        put("hand", "wait_two_streams_waits_on_waiter", ok && w.size() == 1 && w[0].a == (uintptr_t)C && w[0].b == (uintptr_t)h.ev);
        h.forget(X);
        put("hand", "forget_other_stream_changes_nothing", h.last == B && h.ev != nullptr);
        at = calls();
        (void)h.begin(A);
        put("hand", "still_waits_after_forgetting_another", since(at, "hipStreamWaitEvent").size() == 1);
        h.forget(B);
        at = calls();
        put("hand", "forget_last_then_no_wait", h.last == nullptr && h.begin(A) == PV_OK && calls() == at);
        (void)h.end(A);
        const hipEvent_t old = h.ev;
        at = calls();
        h.destroy();
        std::vector<StubCall> d = since(at, "hipEventDestroy");
        put("hand", "destroy", h.ev == nullptr && h.last == nullptr && d.size() == 1 && d[0].a == (uintptr_t)old);
        at = calls();
        h.destroy();
        put("hand", "second_destroy_is_no_call", calls() == at);
        ok = h.begin(B) == PV_OK;
        put("hand", "begin_after_destroy_recreates_event",
            ok && h.ev != nullptr && since(at, "hipEventCreateWithFlags").size() == 1 && since(at, "hipStreamWaitEvent").empty());
        h.destroy();
        // a record with no begin before it (the key cache's put) creates the event as well
        at = calls();
        ok = h.end(A) == PV_OK;
        put("hand", "end_first_creates_event", ok && since(at, "hipEventCreateWithFlags").size() == 1 && h.last == A);
        h.destroy();
        put("hand", "events_all_destroyed", stub().events == stub().events_destroyed);
    }
    {
        const uint64_t sizes[] = {0, 1, 255, 256, 257};
        PvLayout l;
        bool aligned = true, increasing = true, disjoint = true;
        uint64_t prev_end = 0;
        int64_t prev = -1;
        for (int round = 0; round < 2; round++)
            for (uint64_t sz : sizes) {
                const uint64_t o = l.add(sz);
                aligned = aligned && o % 256 == 0 && l.at % 256 == 0;
                increasing = increasing && (int64_t)o > prev;
                disjoint = disjoint && o >= prev_end && o + sz <= l.at;
                prev = (int64_t)o;
                prev_end = o + (sz ? sz : 1);
            }
        put("layout", "multiples_of_256", aligned);
        put("layout", "strictly_increasing", increasing);
        put("layout", "never_overlap", disjoint);
        put("layout", "total", l.at == 2 * (256 + 256 + 256 + 256 + 512));
        put("layout", "up256", pv_up256(0) == 0 && pv_up256(1) == 256 && pv_up256(256) == 256 && pv_up256(257) == 512);
    }
    {
        const uint64_t one[] = {7}, equal[] = {3, 3, 3, 3}, inc[] = {0, 1, 5, 5, 9}, first[] = {4, 3, 5, 6, 7},
                       last[] = {0, 1, 2, 3, 2};
        put("monotone", "empty", pv_offsets_monotone(one, 0));
        put("monotone", "equal", pv_offsets_monotone(equal, 3));
        put("monotone", "increasing", pv_offsets_monotone(inc, 4));
        put("monotone", "decrease_at_first_pair", !pv_offsets_monotone(first, 4));
        put("monotone", "decrease_at_last_pair", !pv_offsets_monotone(last, 4));
        put("monotone", "prefix_before_the_decrease", pv_offsets_monotone(last, 3));
    }
    printf("{%s}\n", g_json.c_str());
    return 0;
}
