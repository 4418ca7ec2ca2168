// Host index of the node-side key cache (keycache.h): which slot holds which key, the LRU over the
// occupied slots and the free list. Host only and without a runtime call, so tests/native/
// kc_index_check.cpp runs it on a CPU; pv_keycache.hip and kc_build_tables (pv_engine.hip) do the copies
// and launches around it. The device's view of the same state is the open-addressing table fill_htab
// writes and pv_kc_lookup (keycache.h) reads.
//
// Invariants: a slot is either in the free list or in the LRU, exactly once; the index has one entry
// per LRU node; slot_key[s] is the key of an occupied slot s (of a free one: empty after a rollback or
// a clear, else the key that last held it).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <list>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "keycache.h"  // PV_KC_EMPTY, pv_kc_hash

#pragma GCC visibility push(hidden)  // internal to libplenum_verify.so
namespace pvhost {

class KcIndex {
   public:
    // What one put changed: the keys that were not present with the slots they got (PV_KC_EMPTY: evicted
    // again by a later key of the same call, nothing to build), every slot handed out, in order, and the
    // keys that left.
    struct Assigned {
        std::vector<std::string> fresh;
        std::vector<uint32_t> fresh_slot, touched;
        std::vector<std::string> evicted;
    };

    // `cap` slots, all free, handed out in ascending order from 0 (the cache's wide rows belong to the
    // lowest slots).
    void configure(uint32_t cap) {
        reset();
        slot_key_.assign(cap, std::string());
        for (uint32_t i = cap; i-- > 0;) free_slots_.push_back(i);
    }
    // Drops every key; the capacity stays.
    void clear() {
        index_.clear();
        lru_.clear();
        free_slots_.clear();
        for (uint32_t i = capacity(); i-- > 0;) free_slots_.push_back(i);
        for (auto& sk : slot_key_) sk.clear();
    }
    // Capacity 0.
    void reset() {
        index_.clear();
        lru_.clear();
        slot_key_.clear();
        free_slots_.clear();
    }

    uint32_t size() const { return (uint32_t)index_.size(); }
    bool empty() const { return index_.empty(); }
    uint32_t capacity() const { return (uint32_t)slot_key_.size(); }
    bool contains(const uint8_t pk[32]) const {
        return index_.count(std::string(reinterpret_cast<const char*>(pk), 32)) != 0;
    }

    // A put of n keys (duplicates included) may evict: the launches' reads are to be folded in first.
    bool needs_fold(uint64_t n) const { return free_slots_.size() < n && !lru_.empty(); }

    // Slots for the keys of one put (n x 32 bytes; at most capacity() of them stay: the last distinct
    // ones of the call win). A key already present becomes the most recent one.
    Assigned assign(const uint8_t* pks, uint64_t n) {
        Assigned a;
        for (uint64_t i = 0; i < n; i++) {
            std::string key(reinterpret_cast<const char*>(pks + 32 * i), 32);
            auto it = index_.find(key);
            if (it != index_.end()) {  // refresh
                lru_.splice(lru_.begin(), lru_, it->second);
                continue;
            }
            uint32_t slot;
            if (!free_slots_.empty()) {
                slot = free_slots_.back();
                free_slots_.pop_back();
            } else {  // evict the least recently used key
                slot = lru_.back();
                lru_.pop_back();
                index_.erase(slot_key_[slot]);
                a.evicted.push_back(slot_key_[slot]);
                for (size_t f = 0; f < a.fresh.size(); f++)
                    if (a.fresh_slot[f] == slot) a.fresh_slot[f] = PV_KC_EMPTY;  // evicted before it was built
            }
            lru_.push_front(slot);
            index_[key] = lru_.begin();
            slot_key_[slot] = key;
            a.fresh.push_back(key);
            a.fresh_slot.push_back(slot);
            a.touched.push_back(slot);
        }
        return a;
    }

    // Undoes a put whose tables were not all built: every slot it handed out (its new key's table may
    // be unbuilt, and its evicted key's table may already be overwritten) leaves the index and goes to
    // the back of the free list, once; the keys the put did not touch keep their slots.
    void rollback(const std::vector<uint32_t>& touched) {
        std::vector<char> seen(capacity(), 0);
        for (uint32_t slot : touched) {
            if (seen[slot]) continue;
            seen[slot] = 1;
            auto it = index_.find(slot_key_[slot]);
            if (it != index_.end() && *it->second == slot) {
                lru_.erase(it->second);
                index_.erase(it);
            }
            slot_key_[slot].clear();
            free_slots_.push_back(slot);
        }
    }

    // LRU refresh on use: the slots whose stamp (stamps[capacity()], the epoch of the last launch that
    // read the slot) is newer than fold_epoch move to the front, least recently read first; slots read
    // by the same launch keep their order.
    void fold(const uint32_t* stamps, uint32_t fold_epoch) {
        std::vector<std::pair<uint32_t, uint32_t>> used;  // (age of the stamp past the fold, slot), LRU order
        for (auto it = lru_.rbegin(); it != lru_.rend(); ++it) {
            const uint32_t age = stamps[*it] - fold_epoch;
            if ((int32_t)age > 0) used.emplace_back(age, *it);
        }
        std::stable_sort(used.begin(), used.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (const auto& u : used) {
            auto it = index_.find(slot_key_[u.second]);
            if (it != index_.end() && *it->second == u.second) lru_.splice(lru_.begin(), lru_, it->second);
        }
    }

    // The open-addressing table of the indexed keys' slots, h[hmask + 1], as pv_kc_lookup probes it.
    void fill_htab(uint32_t* h, uint32_t hmask, uint32_t seed) const {
        std::fill(h, h + (size_t)hmask + 1, PV_KC_EMPTY);
        for (auto& e : index_) {
            uint32_t A[8];
            memcpy(A, e.first.data(), 32);
            uint32_t p = pv_kc_hash(A, seed) & hmask;
            while (h[p] != PV_KC_EMPTY) p = (p + 1) & hmask;
            h[p] = *e.second;
        }
    }

    // One build batch of a put: from position f0 of a.fresh, up to kcap keys that still hold a slot go
    // to bpk [kcap][32] / bslot [kcap]. Returns the position the next batch starts at; m: keys packed.
    static size_t pack(const Assigned& a, size_t f0, uint32_t kcap, uint8_t* bpk, uint32_t* bslot, uint32_t& m) {
        m = 0;
        size_t f = f0;
        for (; f < a.fresh.size() && m < kcap; f++) {
            if (a.fresh_slot[f] == PV_KC_EMPTY) continue;
            memcpy(bpk + 32ull * m, a.fresh[f].data(), 32);
            bslot[m++] = a.fresh_slot[f];
        }
        return f;
    }

    // read-only, for the checks
    const std::list<uint32_t>& lru() const { return lru_; }                 // slots, most recent first
    const std::vector<std::string>& slot_key() const { return slot_key_; }
    const std::vector<uint32_t>& free_slots() const { return free_slots_; }  // handed out from the back

   private:
    std::unordered_map<std::string, std::list<uint32_t>::iterator> index_;  // key bytes -> LRU node
    std::list<uint32_t> lru_;
    std::vector<std::string> slot_key_;
    std::vector<uint32_t> free_slots_;
};

}  // namespace pvhost
#pragma GCC visibility pop
