// csrc/workspace.h and csrc/stage.h compiled with g++ against the stub runtime in stub_hip/ (no GPU): the grow-only buffers
// leave themselves empty after a failed allocation, the hand-over issues exactly the waits it should, the
// staging layout never overlaps, the owner releases exactly what it created however far creation got, a
// staged call (PvStage) lays out, rebases, copies and recovers from every failing step in both its modes,
// and the path choice answers its whole table.
// Prints one JSON object of named checks; tests/test_workspace_host.py builds this with
// -fsanitize=address,undefined and asserts on it.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../indy-plenum_amd/csrc/stage.h"
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

// What an engine context creates through its owner, in miniature and interleaved as there: 3 streams (one
// with a priority), 4 events, 6 device blocks, 2 pinned blocks. rc[i] is creation i's return code.
struct OwnerSet {
    static constexpr int N = 15;
    static constexpr unsigned EVF = hipEventDisableTiming | hipEventReleaseToDevice;
    hipStream_t s[3] = {};
    hipEvent_t e[4] = {};
    uint32_t* d[6] = {};
    uint8_t* h[2] = {};
    int rc[N] = {};

    void create(PvOwner& o) {
        int i = 0;
        rc[i++] = o.stream(s[0], hipStreamNonBlocking);
        rc[i++] = o.stream(s[1], hipStreamNonBlocking);
        rc[i++] = o.event(e[0], EVF);
        rc[i++] = o.event(e[1], EVF);
        rc[i++] = o.stream(s[2], hipStreamNonBlocking, -1);
        rc[i++] = o.event(e[2], hipEventDisableTiming);
        for (int j = 0; j < 3; j++) rc[i++] = o.dev(d[j], 400 * (j + 1));
        rc[i++] = o.pinned(h[0], 64, hipHostMallocPortable);
        for (int j = 3; j < 6; j++) rc[i++] = o.dev(d[j], 400 * (j + 1));
        rc[i++] = o.pinned(h[1], 128, hipHostMallocDefault);
        rc[i++] = o.event(e[3], 0);
    }
    // creation i's out-parameter is null
    bool null_at(int i) const {
        const bool null[N] = {!s[0], !s[1], !e[0], !e[1], !s[2], !e[2], !d[0], !d[1], !d[2], !h[0],
                              !d[3], !d[4], !d[5], !h[1], !e[3]};
        return null[i];
    }
    static bool is_block(int i) { return i >= 6 && i <= 13; }
};

static bool stub_balanced() {
    const StubState& t = stub();
    return t.dev_allocs == t.dev_frees && t.host_allocs == t.host_frees && t.events == t.events_destroyed &&
           t.streams == t.streams_destroyed;
}
static bool owner_empty(const PvOwner& o) {
    return o.devs.empty() && o.pins.empty() && o.streams.empty() && o.events.empty();
}

static void check_owner() {
    PvOwner o;
    {
        OwnerSet a;
        size_t at = calls();
        a.create(o);
        bool ok = true;
        for (int i = 0; i < OwnerSet::N; i++) ok = ok && a.rc[i] == PV_OK && !a.null_at(i);
        put("owner", "creates_all_non_null", ok && o.devs.size() == 6 && o.pins.size() == 2 && o.streams.size() == 3 &&
                                                 o.events.size() == 4 && calls() == at + OwnerSet::N);
        for (int j = 0; j < 6; j++) a.d[j][0] = a.d[j][100 * (j + 1) - 1] = 7;  // really that large
        a.h[0][63] = a.h[1][127] = 7;
        std::vector<StubCall> m = since(at, "hipMalloc"), hm = since(at, "hipHostMalloc");
        ok = m.size() == 6 && hm.size() == 2;
        for (size_t j = 0; ok && j < 6; j++) ok = m[j].a == 400 * (j + 1);
        put("owner", "sizes_and_pinned_flags_unchanged", ok && hm[0].a == 64 && hm[0].b == hipHostMallocPortable &&
                                                             hm[1].a == 128 && hm[1].b == hipHostMallocDefault);
        std::vector<StubCall> sf = since(at, "hipStreamCreateWithFlags"), sp = since(at, "hipStreamCreateWithPriority"),
                              ev = since(at, "hipEventCreateWithFlags");
        put("owner", "stream_flags_and_priority_unchanged",
            sf.size() == 2 && sf[0].a == (uintptr_t)a.s[0] && sf[1].a == (uintptr_t)a.s[1] &&
                sf[0].b == hipStreamNonBlocking && sf[1].b == hipStreamNonBlocking && sp.size() == 1 &&
                sp[0].a == (uintptr_t)a.s[2] && sp[0].b == hipStreamNonBlocking && sp[0].c == -1);
        put("owner", "event_flags_unchanged", ev.size() == 4 && ev[0].b == OwnerSet::EVF && ev[1].b == OwnerSet::EVF &&
                                                  ev[2].b == hipEventDisableTiming && ev[3].b == 0);
        at = calls();
        o.release_all();
        put("owner", "release_all_balances_every_kind", stub_balanced() && owner_empty(o) && calls() == at + OwnerSet::N);
        std::vector<StubCall> f = since(at, "hipFree"), hf = since(at, "hipHostFree"), sd = since(at, "hipStreamDestroy"),
                              ed = since(at, "hipEventDestroy");
        ok = f.size() == 6 && hf.size() == 2 && sd.size() == 3 && ed.size() == 4;
        for (size_t j = 0; ok && j < 6; j++) ok = f[j].a == (uintptr_t)a.d[5 - j];
        for (size_t j = 0; ok && j < 2; j++) ok = hf[j].a == (uintptr_t)a.h[1 - j];
        for (size_t j = 0; ok && j < 3; j++) ok = sd[j].a == (uintptr_t)a.s[2 - j];
        for (size_t j = 0; ok && j < 4; j++) ok = ed[j].a == (uintptr_t)a.e[3 - j];
        put("owner", "releases_newest_first", ok);
        at = calls();
        o.release_all();
        put("owner", "second_release_all_is_no_call", calls() == at && owner_empty(o));
    }
    {  // the emptied owner is used again
        OwnerSet a;
        a.create(o);
        bool ok = true;
        for (int i = 0; i < OwnerSet::N; i++) ok = ok && a.rc[i] == PV_OK && !a.null_at(i);
        o.release_all();
        put("owner", "used_again_after_release_all", ok && stub_balanced() && owner_empty(o));
    }
    {
        OwnerSet a;
        a.create(o);
        size_t at = calls();
        o.drop(a.d[2]);
        std::vector<StubCall> f = since(at, "hipFree");
        put("owner", "drop_frees_that_block_once",
            calls() == at + 1 && f.size() == 1 && f[0].a == (uintptr_t)a.d[2] && o.devs.size() == 5);
        at = calls();
        int local = 0;
        o.drop(&local);
        o.drop(nullptr);
        o.drop(a.d[2]);  // forgotten: not freed a second time (AddressSanitizer watches)
        put("owner", "drop_of_unknown_pointer_is_no_call", calls() == at && o.devs.size() == 5);
        at = calls();
        o.release_all();
        bool again = false;
        for (const StubCall& c : since(at, "hipFree")) again = again || c.a == (uintptr_t)a.d[2];
        put("owner", "release_all_skips_dropped_block", !again && since(at, "hipFree").size() == 5 && stub_balanced());
    }
    {  // a half-built context: creation k fails, the rest is made, one release_all leaves nothing behind
        bool code = true, null = true, rest = true, named = true, balanced = true, recorded = true;
        for (int k = 0; k < OwnerSet::N; k++) {
            OwnerSet a;
            stub().fail_in = k + 1;
            g_last_error.clear();
            a.create(o);
            code = code && a.rc[k] == (OwnerSet::is_block(k) ? PV_ERR_ALLOC : PV_ERR_NO_DEVICE);
            null = null && a.null_at(k);
            for (int i = 0; i < OwnerSet::N; i++) rest = rest && (i == k || (a.rc[i] == PV_OK && !a.null_at(i)));
            named = named && g_last_error.find("hip") == 0 && g_last_error.find("out of memory (stub)") != std::string::npos;
            recorded = recorded && o.devs.size() + o.pins.size() + o.streams.size() + o.events.size() == OwnerSet::N - 1;
            o.release_all();
            balanced = balanced && stub_balanced() && owner_empty(o) && stub().fail_in == 0;
        }
        put("owner", "failed_creation_returns_its_error_code", code);
        put("owner", "failed_creation_leaves_null", null);
        put("owner", "failed_creation_names_call_and_error", named);
        put("owner", "creations_around_a_failure_succeed", rest);
        put("owner", "failed_creation_is_not_recorded", recorded);
        put("owner", "release_all_after_any_failure_balances", balanced);
    }
    {  // an optional pair (the key cache's wide rows and their scratch): kept only if both exist
        OwnerSet a;
        a.create(o);
        const size_t before = o.devs.size();
        const uint64_t allocs = stub().dev_allocs, frees = stub().dev_frees;
        uint32_t *first = nullptr, *second = (uint32_t*)&a;
        bool ok = o.dev(first, 4096) == PV_OK && first != nullptr;
        stub().fail_in = 1;
        ok = ok && o.dev(second, 4096) == PV_ERR_ALLOC && second == nullptr;
        o.drop(first);
        put("owner", "optional_pair_leaves_count_as_before",
            ok && o.devs.size() == before && stub().dev_allocs == allocs + 1 && stub().dev_frees == frees + 1);
        o.release_all();
        put("owner", "all_released_at_the_end", stub_balanced() && owner_empty(o));
    }
}

// One use of a stage as a host-buffer entry makes it, sizes scaled by k: a blob with 37 bytes in front
// and offsets that start there, a lent array, an empty section, an arena that goes up and comes back, three
// outputs (one without a dst, one whose tail is only reserved), a stand-in for the kernels in between.
static const hipStream_t STAGE_STREAM = (hipStream_t)0x50;
struct StageUse {
    bool layout = false, rebased = false, caller_array_untouched = false, slack = false, empty = false, inputs = false,
         outs = false, inout = false, lent = false;
    size_t up = 0, down = 0, syncs = 0, want_up = 0, want_down = 0;
    bool good() const {
        return layout && rebased && caller_array_untouched && slack && empty && inputs && outs && inout && lent &&
               up == want_up && down == want_down && syncs == 1;
    }
};
static int stage_use(PvStage& st, bool pinned, uint64_t k, StageUse* r) {
    *r = StageUse();
    const uint64_t nb = 53 * k;
    std::vector<uint8_t> blob(37 + nb);  // exactly: a copy that takes the slack along reads past its end
    for (size_t i = 0; i < blob.size(); i++) blob[i] = (uint8_t)(7 * i + 1);
    const std::vector<uint64_t> off = {37, 40, 40, 37 + nb}, off_before = off;
    std::vector<uint8_t> arena(300 * k), arena_out(300 * k, 0), dst1(70 * k, 0), dst3(16, 0xAA);
    for (size_t i = 0; i < arena.size(); i++) arena[i] = (uint8_t)(3 * i);
    const std::vector<uint8_t> arena_before = arena;
    if (int rc = st.reset(STAGE_STREAM, pinned)) return rc;
    int i_lent;
    uint64_t* lent = st.in_u64(5, &i_lent);
    for (uint64_t j = 0; j < 5; j++) lent[j] = 1000 + j;
    const int i_off = st.in_offsets(off.data(), 3);
    for (int j = 0; j < 20; j++) (void)st.in_offsets(off.data(), 3);  // the stage's own arrays grow in number
    const int i_empty = st.in(nullptr, 0), i_blob = st.in(blob.data() + 37, nb, 200),
              i_arena = st.inout(arena.data(), arena_out.data(), arena.size()), o1 = st.out(dst1.data(), dst1.size()),
              o2 = st.out(nullptr, 33), o3 = st.out(dst3.data(), 9, 7), o_empty = st.out(nullptr, 0);
    r->lent = true;
    for (uint64_t j = 0; j < 5; j++) r->lent = r->lent && lent[j] == 1000 + j;  // still there (AddressSanitizer watches)
    r->want_up = pinned ? 1 : 24;  // lent, 21 offset arrays, blob, arena; nothing for the empty section
    r->want_down = pinned ? 1 : 3;  // arena, dst1, dst3
    const size_t at = calls();
    if (int rc = st.upload()) return rc;

    struct Span {
        uint8_t* p;
        uint64_t bytes;  // reserved
        bool out;
    };
    const Span spans[] = {{st.dev<uint8_t>(i_lent), 40, false},     {st.dev<uint8_t>(i_off), 32, false},
                          {st.dev<uint8_t>(i_empty), 1, false},     {st.dev<uint8_t>(i_blob), nb + 200, false},
                          {st.dev<uint8_t>(i_arena), 300 * k, false}, {st.dev<uint8_t>(o1), 70 * k, true},
                          {st.dev<uint8_t>(o2), 33, true},          {st.dev<uint8_t>(o3), 16, true},
                          {st.dev<uint8_t>(o_empty), 1, true}};
    r->layout = st.dev<uint8_t>(-1) == nullptr;
    for (const Span& a : spans) {
        const PvDevBuf& blk = a.out && !pinned ? st.d_out : st.d_in;
        r->layout = r->layout && a.p != nullptr && (uintptr_t)(a.p - blk.p) % 256 == 0 && a.p >= blk.p &&
                    a.p + a.bytes <= blk.p + blk.cap;
        for (const Span& b : spans) r->layout = r->layout && (&a == &b || a.p + a.bytes <= b.p || b.p + b.bytes <= a.p);
    }
    r->empty = st.dev<uint8_t>(i_empty) != nullptr && st.dev<uint8_t>(o_empty) != nullptr;
    const uint64_t* d_off = st.dev<const uint64_t>(i_off);
    r->rebased = d_off[0] == 0 && d_off[1] == 3 && d_off[2] == 3 && d_off[3] == nb;
    r->caller_array_untouched = off == off_before;
    r->inputs = memcmp(st.dev<uint8_t>(i_blob), blob.data() + 37, nb) == 0 && memcmp(st.dev<uint8_t>(i_lent), lent, 40) == 0;
    r->slack = true;  // reserved: the span check above; not copied: the copy into the blob's section has its bytes alone
    for (const StubCall& c : since(at, "hipMemcpyAsync"))
        if (!pinned && c.a == (uintptr_t)st.dev<uint8_t>(i_blob)) r->slack = c.b == nb;
    // the kernels
    for (uint64_t i = 0; i < 70 * k; i++) st.dev<uint8_t>(o1)[i] = (uint8_t)(5 * i + 2);
    memset(st.dev<uint8_t>(o2), 0x33, 33);
    memset(st.dev<uint8_t>(o3), 0x44, 16);  // whole words, of which dst3 takes 9 bytes
    for (uint64_t i = 0; i < 300 * k; i++) st.dev<uint8_t>(i_arena)[i] += 1;
    if (int rc = st.download()) return rc;

    r->outs = true;
    for (uint64_t i = 0; i < 70 * k; i++) r->outs = r->outs && dst1[i] == (uint8_t)(5 * i + 2);
    for (int i = 0; i < 16; i++) r->outs = r->outs && dst3[i] == (i < 9 ? 0x44 : 0xAA);
    r->inout = arena == arena_before;
    for (uint64_t i = 0; i < 300 * k; i++) r->inout = r->inout && arena_out[i] == (uint8_t)(arena[i] + 1);
    for (const StubCall& c : since(at, "hipMemcpyAsync")) (c.c == hipMemcpyHostToDevice ? r->up : r->down)++;
    r->syncs = since(at, "hipStreamSynchronize").size();
    return PV_OK;
}

// the first synchronisation logged from `from` on comes before the first copy
static bool sync_comes_first(size_t from) {
    for (size_t i = from; i < stub().log.size(); i++) {
        if (stub().log[i].name == "hipStreamSynchronize") return stub().log[i].a == (uintptr_t)STAGE_STREAM;
        if (stub().log[i].name == "hipMemcpyAsync") return false;
    }
    return false;
}

static void check_stage(bool pinned) {
    const std::string m = pinned ? "pinned_" : "caller_";
    auto say = [&](const char* name, bool ok) { put("stage", (m + name).c_str(), ok); };
    StageUse r;
    size_t allocs = 0, steps = 0;  // what one use of a fresh stage creates, and its copies and synchronisation
    {
        PvStage st;
        const size_t at = calls();
        const int rc = stage_use(st, pinned, 2, &r);
        allocs = since(at, "hipMalloc").size() + since(at, "hipHostMalloc").size();
        steps = since(at, "hipMemcpyAsync").size() + since(at, "hipStreamSynchronize").size();
        say("use_succeeds", rc == PV_OK && allocs == 2 && since(at, "hipHostMalloc").size() == (pinned ? 1u : 0u));
        say("sections_aligned_disjoint_in_their_blocks", r.layout);
        say("empty_section_has_a_pointer_and_no_copy", r.empty && r.up == r.want_up);
        say("offsets_arrive_rebased", r.rebased && r.inputs);
        say("callers_offsets_untouched", r.caller_array_untouched);
        say("slack_reserved_not_copied", r.slack);
        say("outputs_arrive_and_null_dst_is_skipped", r.outs);
        say("inout_round_trips", r.inout);
        say("lent_array_survives_later_sections", r.lent);
        say("copy_count", r.up == r.want_up && r.down == r.want_down);
        say("one_synchronise", r.syncs == 1);
        // chunk after chunk: a larger one grows the blocks, then a smaller and an equal one allocate nothing
        size_t at2 = calls();
        bool ok = stage_use(st, pinned, 5, &r) == PV_OK && r.good();
        ok = ok && since(at2, "hipMalloc").size() + since(at2, "hipHostMalloc").size() == 2;
        at2 = calls();
        ok = ok && stage_use(st, pinned, 1, &r) == PV_OK && r.good() && stage_use(st, pinned, 5, &r) == PV_OK && r.good();
        say("reset_reuses_blocks_that_fit", ok && since(at2, "hipMalloc").empty() && since(at2, "hipHostMalloc").empty() &&
                                                since(at2, "hipFree").empty() && since(at2, "hipHostFree").empty());
        // the other mode on the same stage
        say("mode_can_change_between_uses", stage_use(st, !pinned, 3, &r) == PV_OK && r.good());
        st.release();
        say("release_frees_every_block", stub().dev_allocs == stub().dev_frees && stub().host_allocs == stub().host_frees);
    }
    bool code = true, next = true, synced = true;
    for (size_t k = 1; k <= allocs; k++) {  // each grow
        PvStage st;
        stub().fail_in = (int)k;
        g_last_error.clear();
        code = code && stage_use(st, pinned, 2, &r) == PV_ERR_ALLOC && !g_last_error.empty() && stub().fail_in == 0;
        const size_t at = calls();
        next = next && stage_use(st, pinned, 2, &r) == PV_OK && r.good();
        synced = synced && sync_comes_first(at);
        st.release();
    }
    say("failed_grow_returns_alloc_error", code);
    say("use_after_failed_grow_succeeds", next);
    say("use_after_failed_grow_synchronises_first", synced);
    code = next = synced = true;
    for (size_t k = 1; k <= steps; k++) {  // each copy, the synchronisation
        PvStage st;
        stub().fail_call_in = (int)k;
        g_last_error.clear();
        code = code && stage_use(st, pinned, 2, &r) == PV_ERR_LAUNCH && !g_last_error.empty() && stub().fail_call_in == 0;
        const size_t at = calls();
        next = next && stage_use(st, pinned, 2, &r) == PV_OK && r.good();
        synced = synced && sync_comes_first(at);
        st.release();
    }
    say("failed_copy_or_synchronise_returns_launch_error", code && steps == (pinned ? 3u : 28u));
    say("use_after_failed_copy_succeeds", next);
    say("use_after_failed_copy_synchronises_first", synced);
    say("all_released_at_the_end", stub().dev_allocs == stub().dev_frees && stub().host_allocs == stub().host_frees);
}

// mode x have-device x work {0, below, at the threshold}
static void check_path_choice() {
    bool code = true, choice = true, text = true, untouched = true;
    const uint64_t works[] = {0, 351, 352};
    for (int mode = 0; mode < 3; mode++)
        for (int have = 0; have < 2; have++)
            for (uint64_t work : works) {
                bool device = true;
                g_last_error.clear();
                const int rc = pv_choose_path(mode, have != 0, work, 352, "pv_some_entry", &device);
                const bool forced_without = mode == PV_TRIE_DEVICE && !have;
                code = code && rc == (forced_without ? PV_ERR_NO_DEVICE : PV_OK);
                if (forced_without) {
                    text = text && g_last_error == "pv_some_entry: the device path is forced and no device is initialised";
                    untouched = untouched && device;
                } else {
                    const bool want = have && (mode == PV_TRIE_DEVICE || (mode == PV_TRIE_AUTO && work >= 352));
                    choice = choice && device == want && g_last_error.empty();
                }
            }
    put("stage", "path_forced_device_without_device_is_an_error", code);
    put("stage", "path_error_text", text && untouched);
    put("stage", "path_choice_table", choice);
    put("stage", "path_modes_are_0_1_2", PV_MERKLE_AUTO == 0 && PV_MERKLE_HOST == 1 && PV_MERKLE_DEVICE == 2 &&
                                             PV_TRIE_AUTO == 0 && PV_TRIE_HOST == 1 && PV_TRIE_DEVICE == 2);
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
        // run: the body's error comes back and the hand-over is ended all the same
        at = calls();
        ok = h.run(B, [] { return (int)PV_ERR_ARG; }) == PV_ERR_ARG;
        put("hand", "run_ends_after_a_failed_body", ok && since(at, "hipEventRecord").size() == 1 && h.last == B);
        put("hand", "run_returns_ok", h.run(B, [] { return (int)PV_OK; }) == PV_OK);
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
    check_owner();
    check_stage(false);
    check_stage(true);
    check_path_choice();
    printf("{%s}\n", g_json.c_str());
    return 0;
}
