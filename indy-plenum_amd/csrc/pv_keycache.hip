// libplenum_verify: the host side of the node-side key cache (keycache.h; pv_key_cache_* in
// include/plenum_verify.h). Allocation and release of the device arrays, the put with its rollback, the
// LRU refresh from the launches' stamps, the hash-table upload and the view the launches read the cache
// through. The slot bookkeeping is pvhost::KcIndex (kc_index.h); here are the copies, the
// synchronisation and the error handling around it. No kernel is defined here: a put's tables are built by
// kc_build_tables (pv_engine.hip) with the kernels of kern_tables.h and kern_wide.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "kc_index.h"
#include "keycache.h"
#include "pv_ctx.h"
#include "../../include/plenum_verify.h"

namespace {

// Rebuild the open-addressing table from the index and upload it (stream-ordered). hbuf: pinned
// room for hmask + 1 words whose copy the caller lets run asynchronously; nullptr = a local buffer
// and a synchronous upload.
int kc_upload_htab(hipStream_t s, uint32_t* hbuf = nullptr) {
    auto& k = g_ctx.kc;
    std::vector<uint32_t> local;
    uint32_t* h = hbuf;
    if (!h) {
        local.resize((size_t)k.hmask + 1);
        h = local.data();
    }
    k.index.fill_htab(h, k.hmask, k.seed);
    PV_HIP(hipMemcpyAsync(k.d_htab, h, ((size_t)k.hmask + 1) * 4, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
    if (!hbuf) PV_HIP(hipStreamSynchronize(s), PV_ERR_LAUNCH);  // h is a local buffer
    return PV_OK;
}

// LRU refresh on use: the slots that launches read since the last fold (d_stamp newer than
// fold_epoch) move to the front of the LRU, least recently read first, so eviction takes the least
// recently USED keys rather than the least recently put. Only the engine stream is waited for: a
// launch still running on another stream may stamp a slot after the copy, with an epoch no newer than
// the new fold_epoch, so that read is not folded later either.
int kc_fold_hits() {
    auto& k = g_ctx.kc;
    if (!k.d_stamp || k.cap == 0) return PV_OK;
    std::vector<uint32_t> st(k.cap);
    PV_HIP(hipMemcpyAsync(st.data(), k.d_stamp, (uint64_t)k.cap * 4, hipMemcpyDeviceToHost, g_ctx.stream), PV_ERR_LAUNCH);
    PV_HIP(hipStreamSynchronize(g_ctx.stream), PV_ERR_LAUNCH);
    k.index.fold(st.data(), k.fold_epoch);
    k.fold_epoch = k.epoch;
    return PV_OK;
}

}  // namespace

// Empties the key cache. enabled, auto_min, the admission counters, seed and ev_async survive: a
// reconfigure keeps them.
void kc_free() {
    auto& k = g_ctx.kc;
    if (k.async_pending && k.ev_async) (void)hipEventSynchronize(k.ev_async);  // the put reads h_async
    k.async_pending = false;
    k.own.release_all();
    k.d_htab = k.d_keys = k.d_flags = k.d_put_slot = k.d_wscr = k.d_stamp = nullptr;
    k.d_tab = k.d_ntab = k.d_wtab = nullptr;
    k.d_put_pk = k.h_async = nullptr;
    k.wcap = 0;
    k.h_async_cap = 0;
    k.cap = k.hmask = 0;
    k.broken = false;
    k.seen.reset();
    k.epoch = k.fold_epoch = 1;
    k.index.reset();
}

PvKeyCacheView kc_view() {
    auto& k = g_ctx.kc;
    PvKeyCacheView v{k.d_htab, k.d_keys, k.d_flags, k.d_tab, 0u, k.seed, k.d_wtab, k.wcap};
    if (k.enabled && !k.broken && k.cap > 0 && !k.index.empty()) {
        v.hmask = k.hmask;
        v.stamp = k.d_stamp;
        v.epoch = ++k.epoch;
    }
    return v;
}

// pv_key_cache_put under g_mu. async (automatic admission): at most kcap new keys, nothing waited
// for (pinned staging; the hash-table upload and the hand-over event are stream-ordered after the build).
int kc_put_locked(const uint8_t* pks, uint64_t n, bool async) {
    auto& k = g_ctx.kc;
    if (async) {
        if (k.async_pending) PV_HIP(hipEventSynchronize(k.ev_async), PV_ERR_LAUNCH);  // h_async is free again
        k.async_pending = false;
    }
    // slots for the new keys (at most cap of them: the last cap distinct keys of the call win).
    // The device hash table still holds the state before this call until kc_upload_htab below.
    if (k.index.needs_fold(n)) {
        const int rc = kc_fold_hits();  // evictions ahead: take the launches' reads into account
        if (rc != PV_OK) return rc;
    }
    const pvhost::KcIndex::Assigned put = k.index.assign(pks, n);
    for (const std::string& key : put.evicted) k.seen.forget(reinterpret_cast<const uint8_t*>(key.data()));  // re-admissible
    int rc = kc_build_tables(put, async);
    if (rc != PV_OK) {
        // roll back to a state in which every indexed key's table is built (KcIndex::rollback). Then
        // the device hash table is re-uploaded; if even that fails, the cache is switched off
        // (kc_view() reports it empty) until configure / clear.
        const std::string err = g_err;
        k.index.rollback(put.touched);
        (void)hipStreamSynchronize(g_ctx.stream);
        if (kc_upload_htab(g_ctx.stream) != PV_OK) k.broken = true;
        g_err = err;
        return rc;
    }
    g_ctx.last_keyed = false;
    if (async) {
        rc = kc_upload_htab(g_ctx.stream, reinterpret_cast<uint32_t*>(k.h_async + (uint64_t)g_ctx.kw.kcap * 36));
        if (rc == PV_OK) {
            PV_HIP(hipEventRecord(k.ev_async, g_ctx.stream), PV_ERR_LAUNCH);
            k.async_pending = true;
        }
    } else {
        rc = kc_upload_htab(g_ctx.stream);
    }
    if (int rc2 = g_ctx.hand.end(g_ctx.stream)) return rc2;
    k.broken = rc != PV_OK;  // a complete upload also repairs an earlier failed one
    return rc;
}

extern "C" {

int pv_key_cache_configure(uint32_t capacity) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_key_cache_configure: call pv_init first");
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);  // no launch may still read the old tables
    kc_free();
    if (capacity == 0) return PV_OK;
    if (capacity > (1u << 20)) return fail(PV_ERR_ARG, "pv_key_cache_configure: capacity above 2^20 keys");
    auto& k = g_ctx.kc;
    uint32_t H = 2;
    while (H < 2 * capacity) H <<= 1;
    const uint64_t per = (uint64_t)PV_COMB_POS * PV_COMB_ENT * 160;  // bytes per key table
    const uint64_t kcap = g_ctx.kw.kcap, async_bytes = kcap * 36 + (uint64_t)H * 4;
    auto make = [&]() -> int {
        if (int rc = k.own.dev(k.d_tab, per * capacity)) return rc;
        if (int rc = k.own.dev(k.d_keys, (uint64_t)capacity * 32)) return rc;
        if (int rc = k.own.dev(k.d_flags, (uint64_t)capacity * 4)) return rc;
        if (int rc = k.own.dev(k.d_htab, (uint64_t)H * 4)) return rc;
        if (int rc = k.own.dev(k.d_stamp, (uint64_t)capacity * 4)) return rc;
        PV_HIP(hipMemset(k.d_stamp, 0, (uint64_t)capacity * 4), PV_ERR_ALLOC);
        if (int rc = k.own.dev(k.d_put_pk, kcap * 32)) return rc;
        if (int rc = k.own.dev(k.d_put_slot, kcap * 4)) return rc;
        if (int rc = k.own.pinned(k.h_async, async_bytes, hipHostMallocDefault)) return rc;
        // the context's, not the cache's: made on the first configure, kept across every later one
        if (!k.ev_async) return g_ctx.own.event(k.ev_async, hipEventDisableTiming);
        return PV_OK;
    };
    if (int rc = make()) {
        kc_free();
        return rc;
    }
    k.h_async_cap = async_bytes;
    // the affine rows (660 KB per key): optional -- without them cached keys use the cached-form rows
    static const bool affine = env_int("PV_KC_AFFINE", 1) != 0;
    if (affine && k.own.dev(k.d_ntab, per * capacity) != PV_OK) (void)hipGetLastError();
    // the wide rows (67 MB per key) for the first min(capacity, PV_KC_WIDE_KEYS) slots: optional, and
    // kept only together with their scratch
    {
        const uint32_t want = std::min<uint32_t>(capacity, (uint32_t)std::max(0, env_int("PV_KC_WIDE_KEYS", PV_KC_WIDE_KEYS)));
        const uint64_t per_w = (uint64_t)PV_KW_POS * PV_KW_ENT * 128;
        if (want > 0 && k.own.dev(k.d_wtab, per_w * want) == PV_OK &&
            k.own.dev(k.d_wscr, (uint64_t)PV_KW_GROUP * PV_KW_POS * PV_KW_ENT * 40) == PV_OK) {
            k.wcap = want;
        } else {
            (void)hipGetLastError();
            k.own.drop(k.d_wtab);
            k.d_wtab = nullptr;
            k.wcap = 0;
        }
    }
    k.cap = capacity;
    k.hmask = H - 1;
    k.seed = (uint32_t)std::random_device{}() | 1u;
    k.index.configure(capacity);
    return kc_upload_htab(g_ctx.stream);
}

int pv_key_cache_put(const uint8_t* pks, uint64_t n) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto& k = g_ctx.kc;
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_key_cache_put: call pv_init first");
    if (k.cap == 0) return fail(PV_ERR_NOT_INIT, "pv_key_cache_put: cache not configured");
    if (n > 0 && !pks) return fail(PV_ERR_ARG, "pv_key_cache_put: null pointer");
    return kc_put_locked(pks, n, false);
}

int pv_key_cache_auto(uint32_t min_seen) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_key_cache_auto: call pv_init first");
    if (min_seen > 254) return fail(PV_ERR_ARG, "pv_key_cache_auto: min_seen above 254");
    g_ctx.kc.auto_min = min_seen;
    g_ctx.kc.seen.reset();
    return PV_OK;
}

int pv_key_cache_auto_stats(uint64_t* admitted, uint64_t* failed) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (admitted) *admitted = g_ctx.kc.auto_admitted;
    if (failed) *failed = g_ctx.kc.auto_failed;
    return PV_OK;
}

int pv_key_cache_clear(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto& k = g_ctx.kc;
    if (k.cap == 0) return PV_OK;
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    k.index.clear();
    k.seen.reset();  // every key may be admitted again
    const int rc = kc_upload_htab(g_ctx.stream);
    k.broken = rc != PV_OK;
    return rc;
}

int pv_key_cache_enable(int enable) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_ctx.kc.enabled = enable != 0;
    return PV_OK;
}

int pv_key_cache_stats(uint32_t* size, uint32_t* capacity) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (size) *size = g_ctx.kc.index.size();
    if (capacity) *capacity = g_ctx.kc.cap;
    return PV_OK;
}

int pv_key_cache_contains(const uint8_t* pk) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!pk) return 0;
    return g_ctx.kc.index.contains(pk) ? 1 : 0;
}

}  // extern "C"
