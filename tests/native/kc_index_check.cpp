// CPU check of the key cache's host index (csrc/kc_index.h, the header the library compiles) together with
// the device's own lookup (csrc/keycache.h: pv_kc_hash and pv_kc_lookup, compiled for the host by emptying
// the function attributes). Prints one JSON object for tests/test_kc_index.py:
//   s1 .. s7   small scenarios whose expected outcome the Python file states by hand
//   random     per capacity, 2,000 seeded random operations (assign with duplicates and present keys, fold,
//              rollback of the last assign, clear); after each one the operation's inputs and results, the LRU,
//              the free list, and the invariants checked here: every slot free or in the LRU exactly once,
//              one index entry per LRU node, slot_key agreeing with the index, and -- through fill_htab and
//              pv_kc_lookup -- every indexed key found at its slot and stamped, every other key not found
// A key is named by a small id; key_of(id) spreads it over the 32 bytes.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
struct uint4 {
    uint32_t x, y, z, w;
};
#include "../../indy-plenum_amd/csrc/kc_index.h"
#include "../../indy-plenum_amd/csrc/keycache.h"

using pvhost::KcIndex;

static void key_of(uint32_t id, uint8_t out[32]) {
    uint32_t A[8];
    A[0] = id;
    for (int q = 1; q < 8; q++) A[q] = (id + 1) * 0x85EBCA6Bu + q * 0xC2B2AE35u;
    memcpy(out, A, 32);
}
static uint32_t id_of(const void* key) {
    uint32_t id;
    memcpy(&id, key, 4);
    return id;
}
static std::vector<uint8_t> keys_of(const std::vector<uint32_t>& ids) {
    std::vector<uint8_t> pk(32 * ids.size() + 1);  // + 1: never a null pointer
    for (size_t i = 0; i < ids.size(); i++) key_of(ids[i], pk.data() + 32 * i);
    return pk;
}
static std::vector<uint32_t> range(uint32_t a, uint32_t b) {
    std::vector<uint32_t> v;
    for (uint32_t i = a; i < b; i++) v.push_back(i);
    return v;
}

static std::string g_out;
static void emit(const std::string& s) { g_out += s; }
template <class V, class F>
static std::string list(const V& v, F f) {
    std::string s = "[";
    bool first = true;
    for (const auto& x : v) {
        s += (first ? "" : ", ") + f(x);
        first = false;
    }
    return s + "]";
}
static std::string nums(const std::vector<uint32_t>& v) {
    return list(v, [](uint32_t x) { return std::to_string(x); });
}
static std::string ids(const std::vector<std::string>& v) {
    return list(v, [](const std::string& k) { return std::to_string(id_of(k.data())); });
}

// "lru": [[slot, key id], ...] most recent first, "free": [...] in order (handed out from the back), "size"
static std::string state(const KcIndex& x) {
    return "\"lru\": " + list(x.lru(), [&](uint32_t s) {
               return "[" + std::to_string(s) + ", " + std::to_string(id_of(x.slot_key()[s].data())) + "]";
           }) + ", \"free\": " + nums(x.free_slots()) + ", \"size\": " + std::to_string(x.size()) +
           ", \"capacity\": " + std::to_string(x.capacity());
}

// every batch of a put at `kcap`: [[f0, next, m, [key ids], [slots]], ...]; bytes_ok: the packed keys are the
// fresh keys' 32 bytes
static std::string packs(const KcIndex::Assigned& a, uint32_t kcap, bool& bytes_ok) {
    std::string s = "[";
    std::vector<uint8_t> bpk(32ull * kcap);
    std::vector<uint32_t> bslot(kcap);
    for (size_t f0 = 0; f0 < a.fresh.size();) {
        uint32_t m = 12345;
        const size_t next = KcIndex::pack(a, f0, kcap, bpk.data(), bslot.data(), m);
        std::vector<uint32_t> pid, ps;
        for (uint32_t j = 0; j < m && j < kcap; j++) {
            uint8_t want[32];
            key_of(id_of(bpk.data() + 32 * j), want);
            if (memcmp(want, bpk.data() + 32 * j, 32) != 0) bytes_ok = false;
            pid.push_back(id_of(bpk.data() + 32 * j));
            ps.push_back(bslot[j]);
        }
        s += std::string(f0 ? ", " : "") + "[" + std::to_string(f0) + ", " + std::to_string(next) + ", " +
             std::to_string(m) + ", " + nums(pid) + ", " + nums(ps) + "]";
        if (next <= f0) break;  // no progress: reported as it is, the Python side fails on it
        f0 = next;
    }
    return s + "]";
}
static std::string assigned(const KcIndex::Assigned& a) {
    return "\"fresh\": " + ids(a.fresh) + ", \"fresh_slot\": " + nums(a.fresh_slot) + ", \"touched\": " +
           nums(a.touched) + ", \"evicted\": " + ids(a.evicted);
}

// The device's side of a cache of `cap` slots over host arrays: keys[] as the scatter kernel leaves it (a
// built key's bytes at its slot, stale bytes elsewhere), the hash table sized as pv_key_cache_configure sizes it.
struct DeviceSide {
    uint32_t cap, hmask, seed, epoch = 1;
    std::vector<uint32_t> keys, htab, stamp;
    DeviceSide(uint32_t cap_, uint32_t seed_) : cap(cap_), seed(seed_ | 1u), keys(8ull * cap_, 0xA5A5A5A5u), stamp(cap_, 0) {
        uint32_t H = 2;
        while (H < 2 * cap) H <<= 1;
        hmask = H - 1;
        htab.assign(H, 0);
    }
    void built(const KcIndex::Assigned& a) {
        for (size_t f = 0; f < a.fresh.size(); f++)
            if (a.fresh_slot[f] != PV_KC_EMPTY) memcpy(&keys[8ull * a.fresh_slot[f]], a.fresh[f].data(), 32);
    }
    // fill_htab, then pv_kc_lookup of every key id below `universe`
    bool lookups_agree(const KcIndex& x, uint32_t universe) {
        x.fill_htab(htab.data(), hmask, seed);
        PvKeyCacheView v{htab.data(), keys.data(), nullptr, nullptr, hmask, seed};
        v.stamp = stamp.data();
        v.epoch = ++epoch;
        std::vector<uint32_t> slot_of_id(universe, PV_KC_EMPTY);
        for (uint32_t s : x.lru()) {
            const uint32_t id = id_of(x.slot_key()[s].data());
            if (id < universe) slot_of_id[id] = s;
        }
        bool ok = true;
        for (uint32_t id = 0; id < universe; id++) {
            uint8_t pk[32];
            uint32_t A[8];
            key_of(id, pk);
            memcpy(A, pk, 32);
            const uint32_t s = pv_kc_lookup(v, A);
            ok = ok && x.contains(pk) == (slot_of_id[id] != PV_KC_EMPTY) && s == slot_of_id[id];
            if (s != PV_KC_EMPTY) ok = ok && s < cap && stamp[s] == epoch;
        }
        return ok;
    }
};

// each slot free or in the LRU, never both, exactly once; index size == LRU length; slot_key agrees with the index
static bool invariants(const KcIndex& x) {
    std::vector<int> seen(x.capacity(), 0);
    for (uint32_t s : x.free_slots()) {
        if (s >= x.capacity()) return false;
        seen[s]++;
    }
    for (uint32_t s : x.lru()) {
        if (s >= x.capacity()) return false;
        seen[s]++;
        if (x.slot_key()[s].size() != 32 || !x.contains(reinterpret_cast<const uint8_t*>(x.slot_key()[s].data()))) return false;
    }
    for (int c : seen)
        if (c != 1) return false;
    // distinct keys over the LRU, as many as the index holds: the index is exactly the LRU's keys
    for (auto a = x.lru().begin(); a != x.lru().end(); ++a)
        for (auto b = std::next(a); b != x.lru().end(); ++b)
            if (x.slot_key()[*a] == x.slot_key()[*b]) return false;
    return x.size() == x.lru().size() && x.slot_key().size() == x.capacity();
}

static std::string checks(const KcIndex& x, DeviceSide& d, uint32_t universe) {
    return std::string("\"invariants\": ") + (invariants(x) ? "true" : "false") + ", \"lookups\": " +
           (d.lookups_agree(x, universe) ? "true" : "false");
}

static KcIndex::Assigned put(KcIndex& x, DeviceSide& d, const std::vector<uint32_t>& key_ids) {
    KcIndex::Assigned a = x.assign(keys_of(key_ids).data(), key_ids.size());
    d.built(a);
    return a;
}

static void scenarios() {
    bool bytes_ok = true;
    {  // s1, s2, s3: 40 keys into 16 slots in one put; 4 old keys; duplicates after a clear
        KcIndex x;
        DeviceSide d(16, 0x1234567);
        x.configure(16);
        emit("\"s0\": {" + state(x) + ", " + checks(x, d, 48) + "}, ");
        KcIndex::Assigned a = put(x, d, range(0, 40));
        emit("\"s1\": {" + assigned(a) + ", \"packs\": " + packs(a, 16, bytes_ok) + ", " + state(x) + ", " + checks(x, d, 48) + "}, ");
        a = put(x, d, range(0, 4));
        emit("\"s2\": {" + assigned(a) + ", " + state(x) + ", " + checks(x, d, 48) + "}, ");
        x.clear();
        emit("\"s3_cleared\": {" + state(x) + ", \"needs_fold_20\": " + (x.needs_fold(20) ? "true" : "false") + ", " +
             checks(x, d, 48) + "}, ");
        std::vector<uint32_t> twice = range(0, 10), again = range(0, 10);
        twice.insert(twice.end(), again.begin(), again.end());
        a = put(x, d, twice);
        emit("\"s3\": {" + assigned(a) + ", " + state(x) + ", \"needs_fold_6\": " + (x.needs_fold(6) ? "true" : "false") +
             ", \"needs_fold_7\": " + (x.needs_fold(7) ? "true" : "false") + ", " + checks(x, d, 48) + "}, ");
    }
    {  // s4: put 16, assign 8 more, roll back, put 11
        KcIndex x;
        DeviceSide d(16, 0x89ABCDE);
        x.configure(16);
        put(x, d, range(0, 16));
        KcIndex::Assigned a = put(x, d, range(16, 24));
        x.rollback(a.touched);
        emit("\"s4_rolled_back\": {" + assigned(a) + ", " + state(x) + ", " + checks(x, d, 48) + "}, ");
        a = put(x, d, range(24, 35));
        emit("\"s4_put_11\": {" + assigned(a) + ", " + state(x) + ", " + checks(x, d, 48) + "}, ");
    }
    {  // s5: a slot assigned more than once in the put that is rolled back
        KcIndex x;
        DeviceSide d(2, 0x55);
        x.configure(2);
        KcIndex::Assigned a = put(x, d, range(0, 5));
        emit("\"s5_assigned\": {" + assigned(a) + ", " + state(x) + ", " + checks(x, d, 8) + "}, ");
        x.rollback(a.touched);
        emit("\"s5_rolled_back\": {" + state(x) + ", " + checks(x, d, 8) + "}, ");
        a = put(x, d, range(5, 7));
        emit("\"s5_put_2\": {" + assigned(a) + ", " + state(x) + ", " + checks(x, d, 8) + "}, ");
    }
    {  // s6: folds at capacity 4, each from the state "keys 0..3 put in order"
        struct Fold {
            const char* name;
            uint32_t epoch;
            uint32_t stamps[4];
        };
        const Fold folds[] = {
            {"only_slot_0_newer", 10, {11, 10, 9, 5}},  // equal to the epoch, one below it (wraps negative), older
            {"equal_ages", 10, {12, 12, 10, 10}},
            {"largest_age_most_recent", 10, {13, 11, 12, 10}},
            {"half_range_ahead", 10, {10, 10u + 0x7FFFFFFFu, 10u + 0x80000000u, 10}},  // 2^31 - 1 ahead: taken; 2^31: not
            {"epoch_wrapped", 0xFFFFFFF0u, {0xFFFFFFEFu, 5, 0xFFFFFFF0u, 0xFFFFFFF8u}},
        };
        emit("\"s6\": {");
        for (const Fold& f : folds) {
            KcIndex x;
            DeviceSide d(4, 0x77);
            x.configure(4);
            put(x, d, range(0, 4));
            x.fold(f.stamps, f.epoch);
            emit(std::string("\"") + f.name + "\": {" + state(x) + ", " + checks(x, d, 12));
            KcIndex::Assigned a = put(x, d, range(4, 8));  // four evictions: the whole LRU from its tail
            emit(", \"evicted_next\": " + ids(a.evicted) + "}, ");
        }
        emit("\"folds\": " + std::to_string(sizeof(folds) / sizeof(folds[0])) + "}, ");
    }
    {  // s7: packing at kcap 5 with holes at the batch boundaries and a last batch of holes only
        KcIndex::Assigned a;
        const uint32_t E = PV_KC_EMPTY;
        const uint32_t slots[] = {E, 10, 11, 12, 13, 14, E, E, 15, 16, 17, 18, 19, E, 20, 21, 22, 23, 24, E, E};
        for (uint32_t i = 0; i < sizeof(slots) / sizeof(slots[0]); i++) {
            uint8_t pk[32];
            key_of(100 + i, pk);
            a.fresh.emplace_back(reinterpret_cast<const char*>(pk), 32);
            a.fresh_slot.push_back(slots[i]);
        }
        emit("\"s7\": {\"packs\": " + packs(a, 5, bytes_ok) + "}, ");
    }
    emit(std::string("\"pack_bytes_ok\": ") + (bytes_ok ? "true" : "false") + ", ");
}

static void random_ops(uint32_t cap, uint32_t nops, bool last) {
    std::mt19937 r(1000 + cap);
    auto below = [&](uint32_t n) { return (uint32_t)(r() % n); };
    const uint32_t universe = 4 * cap + 4, kcap = cap >= 10 ? 5 : cap >= 2 ? cap / 2 : 1;  // several batches per put
    KcIndex x;
    DeviceSide d(cap, r());
    x.configure(cap);
    KcIndex::Assigned last_put;
    bool can_roll_back = false, bytes_ok = true;
    emit("{\"cap\": " + std::to_string(cap) + ", \"kcap\": " + std::to_string(kcap) + ", \"ops\": [");
    for (uint32_t op = 0; op < nops; op++) {
        const uint32_t what = below(100);
        emit(op ? ", {" : "{");
        if (what < 15 && can_roll_back) {
            x.rollback(last_put.touched);
            can_roll_back = false;
            emit("\"op\": \"rollback\", ");
        } else if (what < 20) {
            x.clear();
            can_roll_back = false;
            emit("\"op\": \"clear\", ");
        } else if (what < 45) {
            static const uint32_t epochs[] = {1, 1000, 0x7FFFFFFEu, 0x80000001u, 0xFFFFFFFEu};
            static const uint32_t deltas[] = {0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0, 1, 2, 3, 0x7FFFFFFFu, 0x80000000u};
            const uint32_t epoch = epochs[below(5)] + below(3);
            std::vector<uint32_t> st(cap);
            for (auto& s : st) s = below(8) ? epoch + deltas[below(9)] : (uint32_t)r();
            x.fold(st.data(), epoch);
            can_roll_back = false;
            emit("\"op\": \"fold\", \"epoch\": " + std::to_string(epoch) + ", \"stamps\": " + nums(st) + ", ");
        } else {
            const uint32_t n = below(3 * cap + 1);
            std::vector<uint32_t> key_ids(n);
            for (auto& k : key_ids) k = below(universe);
            const bool nf = x.needs_fold(n);
            last_put = put(x, d, key_ids);
            can_roll_back = true;
            emit("\"op\": \"assign\", \"keys\": " + nums(key_ids) + ", \"needs_fold\": " + (nf ? "true" : "false") + ", " +
                 assigned(last_put) + ", \"packs\": " + packs(last_put, kcap, bytes_ok) + ", ");
        }
        emit(state(x) + ", " + checks(x, d, universe) + "}");
    }
    emit(std::string("], \"pack_bytes_ok\": ") + (bytes_ok ? "true" : "false") + "}" + (last ? "" : ", "));
}

int main() {
    emit("{");
    scenarios();
    emit("\"random\": [");
    const uint32_t caps[] = {1, 2, 7, 64};
    for (int i = 0; i < 4; i++) random_ops(caps[i], 2000, i == 3);
    emit("]}");
    fwrite(g_out.data(), 1, g_out.size(), stdout);
    printf("\n");
    return 0;
}
