// libplenum_verify: the host-buffer entries of the verification engine. pv_verify_batch (zero-copy form
// for small calls, else stage_and_launch: pinned staging, the sub-batch H2D pipeline on the copy stream),
// the pinned-memory registry and cache (pv_host_*), the copy workers, the host-side key-repeat hint,
// automatic key-cache admission after a batch, and the ordered copies (pv_memcpy_*, pv_dev_alloc). No
// kernel is defined here: everything is enqueued through pv_engine.hip's launch() and pv_latency.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "copy_pool.h"
#include "kc_admit.h"
#include "keycache.h"
#include "pv_ctx.h"
#include "../../include/plenum_verify.h"
#include "../../include/plenum_verify_test.h"

// Zero-copy verdict bytes start at 0xFF and each workgroup's last store sets its byte: the host spins
// on them instead of the runtime's completion wait (a kernel fault surfaces at the next call's
// synchronisation); bounded at 50 ms, then false and the caller waits on the stream.
// Exported under this name although no header declares it (the one-file engine defined it inside an
// open extern "C" block): kept so that the library's dynamic symbols stay what they were.
extern "C" bool pv_spin_verdict_bytes(const uint8_t* vb, uint64_t n) {
    const auto t0 = std::chrono::steady_clock::now();
    volatile const uint8_t* vv = vb;
    uint64_t i = 0;
    while (i < n) {
        if (vv[i] != 0xFFu) {
            i++;
            continue;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) return false;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return true;
}

namespace {

// Host-side copy workers (copy_pool.h): one pool per device context, so the per-device workers of
// pv_verify_batch_multi_gpu stage their shards at the same time; pinned host ranges the library owns
// or registered (pv_host_alloc / pv_host_register), whose bytes the host-buffer entry DMAs directly.
pvhost::PinnedRegistry g_pinned_alloc, g_pinned_reg;
// freed pv_host_alloc blocks kept for reuse (copy_pool.h PinnedCache), up to PV_PINNED_CACHE_MB (4 GB)
pvhost::PinnedCache& pinned_cache() {
    static pvhost::PinnedCache* c = [] {
        const char* e = getenv("PV_PINNED_CACHE_MB");
        return new pvhost::PinnedCache((e && *e ? strtoull(e, nullptr, 10) : 4096ull) << 20);
    }();
    return *c;
}
void pinned_release(const std::vector<pvhost::PinnedCache::Block>& v) {
    for (const auto& b : v) (void)hipHostFree(b.p);
}
bool pv_is_pinned(const void* p, uint64_t bytes) {
    return g_pinned_alloc.contains(p, bytes) || g_pinned_reg.contains(p, bytes);
}
pvhost::CopyPool& cur_pool() {
    static const unsigned ndev = (unsigned)std::max(1, pv_device_count());
    return pvhost::copy_pool_for<PV_MAX_DEV>(pv_cur_dev(), ndev);
}

int ensure_stage(uint64_t host_bytes, uint64_t dev_bytes) {
    if (host_bytes)
        if (int rc = g_ctx.h_stage.grow(std::max<uint64_t>(host_bytes, 1 << 20), hipHostMallocPortable)) return rc;
    return dev_bytes ? g_ctx.d_stage.grow(std::max<uint64_t>(dev_bytes, 1 << 20)) : PV_OK;
}

// Move the request blob host -> pinned staging -> HBM. One host thread copies ~10 GB/s, so the blob is
// cut into pieces (256 KB - 4 MB) that the copy pool stages in parallel; with `dma`, each piece's DMA
// (hipMemcpyAsync from pinned memory) is enqueued as soon as it is staged, so the PCIe transfer of
// earlier pieces overlaps the staging of later ones (the pieces are disjoint: their order on the
// stream does not matter, and the kernels launched on the same stream afterwards see every piece).
static int pv_stage_to_device(uint8_t* d_dst, uint8_t* h_stage, const uint8_t* src, uint64_t bytes, hipStream_t s,
                              bool dma) {
    const uint64_t piece = std::min<uint64_t>(4ull << 20, std::max<uint64_t>(256ull << 10, bytes / 16));
    const unsigned k = (unsigned)((bytes + piece - 1) / piece);
    std::atomic<int> err{0};
    cur_pool().run(k, [&](unsigned i) {
        const uint64_t o = (uint64_t)i * piece, e = std::min(bytes, o + piece);
        memcpy(h_stage + o, src + o, e - o);
        if (dma && hipMemcpyAsync(d_dst + o, h_stage + o, e - o, hipMemcpyHostToDevice, s) != hipSuccess) err = 1;
    });
    return err.load() ? fail(PV_ERR_LAUNCH, "hipMemcpyAsync (request blob) failed") : PV_OK;
}

#ifndef PV_KC_AUTO_MAX_BATCH
#define PV_KC_AUTO_MAX_BATCH 4096  // automatic admission counts every key of host batches up to this size (a sample above)
#endif
// Automatic admission: count the VERIFIED appearances of this batch's keys (idx: the sampled requests,
// or null for all n; pre: each one's entry located by kc_auto_locate while the kernels ran, or -1); the
// keys reaching auto_min appearances in the window are returned, at most kcap of them. The verdicts are
// vb[i] & 1 (zero-copy verdict bytes) or bit i of hver (verdict words).
static void kc_auto_count(const uint8_t* pk, const uint64_t* idx, uint64_t n, const int32_t* pre, uint64_t gen,
                          const uint8_t* vb, const uint64_t* hver, std::vector<uint8_t>& admit) {
    auto& k = g_ctx.kc;
    for (uint64_t j = 0; j < n; j++) {
        const uint64_t i = idx ? idx[j] : j;
        const bool ok = vb ? (vb[i] & 1u) != 0 : ((hver[i >> 6] >> (i & 63)) & 1u) != 0;
        if (!ok) continue;  // a key is never counted on the strength of a failing signature
        const auto o = pre && pre[j] >= 0 && k.seen.generation() == gen ? k.seen.bump_at(pre[j], k.auto_min)
                                                                         : k.seen.count(pk + 32 * i, k.auto_min);
        if (o == pvhost::AdmitTable::ADMIT) {
            admit.insert(admit.end(), pk + 32 * i, pk + 32 * i + 32);
            if (admit.size() >= 32ull * g_ctx.kw.kcap) break;
        }
    }
}
// The counting side's read-only lookups, run while the batch's kernels run (the verdicts decide later
// which of them count).
static void kc_auto_locate(const uint8_t* pk, const uint64_t* idx, uint64_t n, std::vector<int32_t>& pre) {
    pre.resize(n);
    for (uint64_t j = 0; j < n; j++) pre[j] = g_ctx.kc.seen.find(pk + 32 * (idx ? idx[j] : j));
}

// AUTO between the latency path and the keyed path for a host batch of PV_KEYED_HINT_MIN..
// PV_LATENCY_MAX requests: the device cannot count keys before the path is chosen, the host can
// (~10 us for 4,096 keys). With >= 3 requests per key on average (and at most PV_ALLCOMB_KEYS keys:
// every key a comb key, sparse fill) the keyed path is faster -- MI355X, 1,024 signers, PCIe
// included (profiles/r02/latency_vs_keyed_crossover.txt): 3,072 requests 0.64 vs 0.71 ms, 4,096
// 0.65 vs 0.92; at 2 requests per key (2,048) the latency path still wins (0.58 vs 0.61). Keys in
// the node-side key cache make the latency path faster still: no hint while the cache holds keys.
static bool pv_keyed_hint(const uint8_t* pk, uint64_t n) {
    if (g_ctx.path != PV_PATH_AUTO || n < PV_KEYED_HINT_MIN || n > PV_LATENCY_MAX) return false;
    if (g_ctx.kc.enabled && !g_ctx.kc.index.empty()) return false;
    // distinct keys by open addressing on the keys' first 16 bytes (a heuristic: a rare collision
    // only miscounts, the verdicts do not depend on the path)
    constexpr uint32_t H = 16384;  // > 2 x PV_LATENCY_MAX
    static_assert(H >= 2 * PV_LATENCY_MAX, "hint table too small");
    static thread_local std::vector<uint64_t> tab;
    tab.assign(2 * H, 0);
    uint64_t distinct = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t a, b;
        memcpy(&a, pk + 32 * i, 8);
        memcpy(&b, pk + 32 * i + 8, 8);
        a |= 1;  // (0, 0) marks an empty entry
        uint32_t h = (uint32_t)((a * 0x9E3779B97F4A7C15ull) >> 50) & (H - 1);
        while (tab[2 * h] && !(tab[2 * h] == a && tab[2 * h + 1] == b)) h = (h + 1) & (H - 1);
        if (!tab[2 * h]) {
            tab[2 * h] = a;
            tab[2 * h + 1] = b;
            distinct++;
        }
    }
    return distinct <= PV_ALLCOMB_KEYS && 3 * distinct <= n;
}

// Requests per sub-batch of the pipelined host-buffer form (a multiple of 64; env PV_PIPE_SUB overrides
// it for A/Bs). Sub-batch j's H2D runs on the copy stream while sub-batch j-1's kernels run, so a large
// host batch costs about its PCIe time plus the last sub-batch's kernels instead of their sum.
#ifndef PV_PIPE_SUB
#define PV_PIPE_SUB 262144
#endif
#ifndef PV_PIPE_END_DEFAULT
#define PV_PIPE_END_DEFAULT (PV_PIPE_SUB / 2)
#endif
static constexpr uint64_t PV_PIPE_MAX = 64;                // sub-batches per call (copy events)
static constexpr uint64_t PV_PIPE_MIN_BLOB = 8ull << 20;   // smaller blobs: one piece
static uint64_t pipe_sub() {
    static const uint64_t v = [] {
        const char* e = getenv("PV_PIPE_SUB");
        const uint64_t x = e && *e ? strtoull(e, nullptr, 10) : (uint64_t)PV_PIPE_SUB;
        return std::max<uint64_t>(8192, x / 64 * 64);
    }();
    return v;
}

// The shared-table store of the pipelined host path (on first use; a failed allocation is not retried:
// the sub-batches then build their own tables, same verdicts).
static int ensure_xtab() {
    auto& x = g_ctx.xt;
    if (x.tab) return PV_OK;
    if (x.failed) return PV_ERR_ALLOC;
    PvOwner& own = g_ctx.own;
    if (own.dev(x.htab, PV_XT_HASH * 4) || own.dev(x.keys, PV_XT_KEYS * 32) || own.dev(x.flags, PV_XT_KEYS * 4) ||
        own.dev(x.tab, (uint64_t)PV_XT_KEYS * PV_COMB_POS * PV_COMB_ENT * 160)) {
        (void)hipGetLastError();
        own.drop(x.flags);  // whichever of them exist; x.tab, the last, failed
        own.drop(x.keys);
        own.drop(x.htab);
        x.htab = x.keys = x.flags = nullptr;
        x.failed = true;
        return PV_ERR_ALLOC;
    }
    return PV_OK;
}

// Automatic key-cache admission after a host-buffer batch whose verdicts are the last thing enqueued on
// `s`. Waits for the verdicts first (vb: zero-copy verdict bytes, spun on; else the verdict words hver
// copied back on `s`), then counts the keys of the requests that VERIFIED -- a request with a failing
// signature never counts towards its key's admission, so senders without a valid signature cannot make
// the node build tables or evict its signers (plenum/server/client_authn.py:84-118: every signature is
// untrusted input). The admitted keys' tables are built right behind the batch on the engine stream;
// the call does not wait for the build (the next launch is stream-ordered after it).
int kc_auto_after_batch(const uint8_t* pk, uint64_t n, hipStream_t s, const uint8_t* vb, const uint64_t* hver) {
    auto& k = g_ctx.kc;
    const bool on = k.auto_min > 0 && k.cap > 0 && k.enabled && !k.broken;
    // the requests counted: all of a batch of <= 4,096, else a sample of one request from each block of
    // ceil(n / 4,096), at a hashed position in the block (a fixed stride would alias with periodic
    // signer orders); their table entries are located while the kernels still run
    std::vector<uint64_t> sample;
    std::vector<int32_t> pre;
    uint64_t gen = 0;
    if (on) {
        if (n > PV_KC_AUTO_MAX_BATCH) {
            const uint64_t stride = (n + PV_KC_AUTO_MAX_BATCH - 1) / PV_KC_AUTO_MAX_BATCH;
            sample.reserve(n / stride + 1);
            for (uint64_t b = 0, t = 0; b < n; b += stride, t++)
                sample.push_back(b + ((t * 0x9E3779B97F4A7C15ull) >> 40) % std::min(stride, n - b));
        }
        gen = k.seen.generation();
        kc_auto_locate(pk, sample.empty() ? nullptr : sample.data(), sample.empty() ? n : sample.size(), pre);
    }
    if (!(vb && pv_spin_verdict_bytes(vb, n))) PV_HIP(hipStreamSynchronize(s), PV_ERR_LAUNCH);
    if (!on) return PV_OK;
    std::vector<uint8_t> admit;
    kc_auto_count(pk, sample.empty() ? nullptr : sample.data(), sample.empty() ? n : sample.size(), pre.data(), gen,
                  vb, hver, admit);
    if (admit.empty()) return PV_OK;
    const std::string err = g_err;
    if (kc_put_locked(admit.data(), admit.size() / 32, true) == PV_OK) {
        k.auto_admitted += admit.size() / 32;
    } else {
        k.auto_failed += admit.size() / 32;  // the verdicts stand; the keys stay uncached and re-admissible
        for (size_t j = 0; j < admit.size(); j += 32) k.seen.forget(admit.data() + j);
        g_err = err;
    }
    return PV_OK;
}

// A copy ordered after every launch enqueued so far on the primary context, whatever stream the caller
// gave it: the library stream first waits for the last launch's completion event, then copies; the
// call returns once the copy is done. (A plain null-stream hipMemcpy is not ordered after the
// library's non-blocking streams: a D2H could read verdict words before the launch wrote them, an H2D
// could overwrite inputs a running launch still reads.)
int ordered_copy(void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind) {
    if (bytes == 0) return PV_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) {
        PV_HIP(hipMemcpy(dst, src, bytes, kind), PV_ERR_LAUNCH);
        return PV_OK;
    }
    hipStream_t s = g_ctx.stream;
    if (int rc = g_ctx.hand.begin(s)) return rc;
    PV_HIP(hipMemcpyAsync(dst, src, bytes, kind, s), PV_ERR_LAUNCH);
    PV_HIP(hipStreamSynchronize(s), PV_ERR_LAUNCH);
    return PV_OK;
}

}  // namespace

// What the engine's other translation units call (declared in pv_ctx.h).

void pinned_cache_drain() { pinned_release(pinned_cache().drain()); }

// sm_off[0..n] non-decreasing (the host-buffer entries refuse anything else before touching the
// device); large batches are checked in slices on the calling context's copy workers.
bool offsets_nondecreasing(const uint64_t* off, uint64_t n) {
    if (n < (1u << 17)) return pv_offsets_monotone(off, n);
    pvhost::CopyPool& pool = cur_pool();
    const unsigned k = std::max(1u, pool.threads());
    std::atomic<bool> good{true};
    pool.run(k, [&](unsigned t) {
        const uint64_t a = n * t / k, b = n * (t + 1) / k;
        if (!pv_offsets_monotone(off + a, b - a)) good = false;
    });
    return good.load();
}

// The copy form of a host-buffer batch on the calling thread's context: moves the keys, offsets and
// records to the device staging area and enqueues the verification on the context's stream. d_out:
// where the verdict words go (nullptr = the staging area's own verdict section); *dver / *hver receive
// the device verdict section and a pinned buffer for the caller's copy back.
//   * small batches (blob < 8 MB, no input in pinned memory): one host copy into pinned staging in the
//     device layout, one DMA, the kernels (the quota sizes: fewest packets on the path);
//   * otherwise, in sub-batches of pipe_sub() requests: the copy workers stage sub-batch j's pageable
//     inputs (inputs inside pv_host_alloc / pv_host_register memory are not copied: the DMA reads them
//     where they are), its H2D goes on the copy stream, and its kernels on the engine stream after an
//     event -- so PCIe, host staging and kernels of consecutive sub-batches overlap.
// Staging layout (host and device, 256-B aligned sections): [pk n*32][off (n+1) u64][verdict][blob +
// PV_BLOB_SLACK]. A failure after DMAs were enqueued returns only after both streams drained, so no copy
// still reads the caller's or the staging buffers.
int stage_and_launch(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk, uint64_t* d_out,
                            uint64_t** dver_out, uint64_t** hver_out) {
    Ctx& c = g_ctx;
    c.last_zero_copy = false;
    auto up = [](uint64_t x) { return (x + 255) & ~255ull; };
    const uint64_t pk_bytes = up(n * 32), off_bytes = up((n + 1) * 8), vwords = (n + 63) / 64;
    const uint64_t v_bytes = up(vwords * 8);
    const uint64_t base = sm_off[0], blob = sm_off[n] - base;
    const uint64_t total = pk_bytes + off_bytes + v_bytes + blob + PV_BLOB_SLACK;
    const bool pin_sm = pv_is_pinned(sm + base, blob), pin_pk = pv_is_pinned(pk, 32 * n);
    const bool pin_off = base == 0 && pv_is_pinned(sm_off, 8 * (n + 1));
    const bool any_pin = pin_sm || pin_pk || pin_off, all_pin = pin_sm && pin_pk && pin_off;
    const uint64_t sub = pipe_sub();
    // sub-batch bounds (64-aligned). The call ends one sub-batch's kernels after the last H2D, and
    // the first sub-batch's kernels (which also build the shared tables) start only after the first
    // H2D, so with >= 2 full sub-batches the first and the last are half-size
    // (profiles/r05/host_path: 1M requests, 0.5 + 3 x 1 + 0.5 of 262,144)
    std::vector<uint64_t> bnd{0};
    static const bool halves = env_int("PV_PIPE_HALF_ENDS", 1) != 0;
    // first / last piece size (env PV_PIPE_END, A/B): half a sub-batch by default. Smaller ends are slower
    // (1M arena: 116.8-119.1 M/s at 131,072, 113.6-114.1 at 65,536, 110.4-112.7 at 32,768; profiles/r06/
    // host_path/ab_pipe_end.txt): the copies are the critical path and a sub-batch's kernels beside a DMA
    // take longer than a small last piece's copy, so the last FULL piece's kernels become the tail
    static const uint64_t end_req = (uint64_t)std::max(8192, env_int("PV_PIPE_END", (int)(PV_PIPE_END_DEFAULT)));
    if (blob >= PV_PIPE_MIN_BLOB && halves && n >= 3 * sub) {
        const uint64_t h = std::min<uint64_t>(end_req, sub) / 64 * 64;
        const uint64_t mid = n - 2 * h;
        const uint64_t k = std::min<uint64_t>(PV_PIPE_MAX - 2, std::max<uint64_t>(1, (mid + sub / 2) / sub));
        bnd.push_back(h);
        for (uint64_t j = 1; j < k; j++) bnd.push_back(h + (mid * j / k) / 64 * 64);
        bnd.push_back((n - h) & ~63ull);  // every bound a whole verdict word (n itself need not be)
    } else if (blob >= PV_PIPE_MIN_BLOB) {
        const uint64_t k = std::min<uint64_t>(PV_PIPE_MAX, std::max<uint64_t>(1, n / sub));
        for (uint64_t j = 1; j < k; j++) bnd.push_back((n * j / k) & ~63ull);
    }
    bnd.push_back(n);
    const uint64_t np = bnd.size() - 1;
    hipStream_t s = c.stream;
    int rc = ensure_stage(all_pin ? 0 : total, total);
    if (rc) return rc;
    uint8_t* h = c.h_stage.p;
    uint8_t* d = c.d_stage.p;
    uint64_t* dver = reinterpret_cast<uint64_t*>(d + pk_bytes + off_bytes);
    uint8_t* dblob = d + pk_bytes + off_bytes + v_bytes;
    auto finish_piece = [&](uint64_t lo, uint64_t hi) -> int {
        c.verdict_zeroed = d_out == nullptr;
        c.keyed_hint = pv_keyed_hint(pk + 32 * lo, hi - lo);
        c.hint_set = true;
        const int r = launch(dblob, reinterpret_cast<const uint64_t*>(d + pk_bytes) + lo, hi - lo, d + 32 * lo,
                             (d_out ? d_out : dver) + lo / 64, s);
        c.verdict_zeroed = false;
        c.keyed_hint = false;
        c.hint_set = false;
        return r;
    };
    if (np == 1 && !any_pin) {
        // the quota sizes: everything in the device layout in pinned staging, one DMA
        uint64_t* hoff = reinterpret_cast<uint64_t*>(h + pk_bytes);
        const unsigned k = n >= (1u << 16) ? 8u : 1u;
        cur_pool().run(k, [&](unsigned t) {
            const uint64_t a = n * t / k, b = n * (t + 1) / k;
            memcpy(h + 32 * a, pk + 32 * a, 32 * (b - a));
            for (uint64_t i = a; i < b; i++) hoff[i] = sm_off[i] - base;
        });
        hoff[n] = sm_off[n] - base;
        uint8_t* hblob = h + pk_bytes + off_bytes + v_bytes;
        memset(h + pk_bytes + off_bytes, 0, v_bytes);  // the verdict words travel zeroed
        memset(hblob + blob, 0, PV_BLOB_SLACK);
        if (c.inject_stage > 0) {
            c.inject_stage--;
            return fail(PV_ERR_ALLOC, "stage_and_launch: injected staging failure (pv_test_inject)");
        }
        if (blob < (256ull << 10)) {
            memcpy(hblob, sm + base, blob);
        } else {
            rc = pv_stage_to_device(dblob, hblob, sm + base, blob, s, false);
            if (rc) return rc;
        }
        PV_HIP(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
        if ((rc = finish_piece(0, n))) return rc;
        *dver_out = dver;
        *hver_out = reinterpret_cast<uint64_t*>(h + pk_bytes + off_bytes);
        return PV_OK;
    }
    if ((rc = c.h_ver.grow(std::max<uint64_t>(v_bytes, 64 << 10), hipHostMallocPortable))) return rc;
    while (c.ev_copy.size() < np) {
        hipEvent_t e;
        if ((rc = c.own.event(e, hipEventDisableTiming))) return rc;
        c.ev_copy.push_back(e);
    }
    hipStream_t cs = c.cstream;
    const uint8_t* spk = pin_pk ? pk : h;
    const uint64_t* soff = pin_off ? sm_off : reinterpret_cast<const uint64_t*>(h + pk_bytes);
    const uint8_t* sblob = pin_sm ? sm + base : h + pk_bytes + off_bytes + v_bytes;
    uint64_t* hoff = reinterpret_cast<uint64_t*>(h + pk_bytes);
    uint8_t* hblob = h + pk_bytes + off_bytes + v_bytes;
    uint64_t* doff = reinterpret_cast<uint64_t*>(d + pk_bytes);
    // the copy stream starts after everything enqueued so far (the previous users of the staging area)
    PV_HIP(hipEventRecord(c.ev_cstart, s), PV_ERR_LAUNCH);
    PV_HIP(hipStreamWaitEvent(cs, c.ev_cstart, 0), PV_ERR_LAUNCH);
    if ((rc = c.hand.wait(cs, s))) return rc;
    // sub-batch j = requests [lo(j), lo(j + 1))
    auto lo_of = [&](uint64_t j) -> uint64_t { return bnd[std::min<uint64_t>(j, np)]; };
    pvhost::CopyPool& pool = cur_pool();
    // sub-batch j's pageable inputs into pinned staging (copy workers), its H2D on the copy stream, then
    // ev_copy[j]
    auto stage_copy = [&](uint64_t j) -> int {
        const uint64_t lo = lo_of(j), hi = lo_of(j + 1);
        const uint64_t b0 = sm_off[lo] - base, b1 = sm_off[hi] - base;
        if (!all_pin) {  // this sub-batch's pageable inputs into pinned staging, on the copy workers
            const unsigned k = std::max(1u, std::min(pool.threads(), (unsigned)((b1 - b0) >> 22)));
            pool.run(k, [&](unsigned t) {
                const uint64_t a = lo + (hi - lo) * t / k, b = lo + (hi - lo) * (t + 1) / k;
                if (!pin_pk) memcpy(h + 32 * a, pk + 32 * a, 32 * (b - a));
                if (!pin_off)
                    for (uint64_t i = a; i < b; i++) hoff[i] = sm_off[i] - base;
                if (!pin_sm) memcpy(hblob + (sm_off[a] - base), sm + sm_off[a], sm_off[b] - sm_off[a]);
            });
            if (!pin_off) hoff[hi] = sm_off[hi] - base;
        }
        PV_HIP(hipMemcpyAsync(d + 32 * lo, spk + 32 * lo, 32 * (hi - lo), hipMemcpyHostToDevice, cs), PV_ERR_LAUNCH);
        PV_HIP(hipMemcpyAsync(doff + lo, soff + lo, 8 * (hi - lo + 1), hipMemcpyHostToDevice, cs), PV_ERR_LAUNCH);
        if (b1 > b0)
            PV_HIP(hipMemcpyAsync(dblob + b0, sblob + b0, b1 - b0, hipMemcpyHostToDevice, cs), PV_ERR_LAUNCH);
        PV_HIP(hipEventRecord(c.ev_copy[j], cs), PV_ERR_LAUNCH);
        return PV_OK;
    };
    // PV_PIPE_TRACE=1 (development): timing events after each sub-batch's copies and kernels, printed to
    // stderr relative to the call's first event -- the untraced pipeline timeline
    static const bool ptrace = env_int("PV_PIPE_TRACE", 0) != 0;
    static const int lookahead = env_int("PV_PIPE_LOOKAHEAD", 1);
    std::vector<hipEvent_t> tev;
    auto tmark = [&](hipStream_t st) {
        if (!ptrace) return;
        hipEvent_t e;
        if (hipEventCreate(&e) == hipSuccess) {
            (void)hipEventRecord(e, st);
            tev.push_back(e);
        }
    };
    // the sub-batches share one set of comb tables: sub-batch 0 builds the tables of its comb keys that
    // the node-side key cache does not hold, the later ones read the cache's for cached keys and the
    // shared store's for the rest (pv_key_cache_probe_kernel's two views)
    static const bool share_env = env_int("PV_PIPE_SHARE", 1) != 0;
    const bool share = share_env && np > 1 && (c.path == PV_PATH_AUTO || c.path == PV_PATH_COMB) &&
                       ensure_xtab() == PV_OK;
    auto run = [&]() -> int {
        tmark(cs);
        if (share) PV_HIP(hipMemsetAsync(c.xt.htab, 0xFF, PV_XT_HASH * 4, s), PV_ERR_LAUNCH);
        if (!d_out) PV_HIP(hipMemsetAsync(dver, 0, vwords * 8, s), PV_ERR_LAUNCH);  // the latency path ORs bits
        PV_HIP(hipMemsetAsync(dblob + blob, 0, PV_BLOB_SLACK, cs), PV_ERR_LAUNCH);
        int r = stage_copy(0);
        tmark(cs);
        // sub-batch j + 1's copies are enqueued BEFORE sub-batch j's kernels: should the copy stream share a
        // hardware queue with one of the engine's streams, no copy waits behind kernels enqueued before it
        for (uint64_t j = 0; j < np && r == PV_OK; j++) {
            if (lookahead && j + 1 < np) {
                if ((r = stage_copy(j + 1)) != PV_OK) break;
                tmark(cs);
            }
            if (c.inject_stage > 0 && j == std::min<uint64_t>(1, np - 1)) {  // sub-batch 0's kernels in flight
                c.inject_stage--;
                return fail(PV_ERR_ALLOC, "stage_and_launch: injected staging failure (pv_test_inject)");
            }
            PV_HIP(hipStreamWaitEvent(s, c.ev_copy[j], 0), PV_ERR_LAUNCH);
            c.xt_fill = share && j == 0;
            c.xt_use = share && j > 0;
            r = finish_piece(lo_of(j), lo_of(j + 1));
            c.xt_fill = c.xt_use = false;
            tmark(s);
            if (!lookahead && r == PV_OK && j + 1 < np) {
                if ((r = stage_copy(j + 1)) != PV_OK) break;
                tmark(cs);
            }
        }
        return r;
    };
    if ((rc = run()) != PV_OK) {
        (void)hipStreamSynchronize(cs);  // no DMA may still read the caller's or the staging buffers
        (void)hipStreamSynchronize(s);
        return rc;
    }
    if (ptrace && !tev.empty()) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(cs);
        std::string line = "pv_pipe: n " + std::to_string(n) + " pieces " + std::to_string(np) + " us:";
        for (size_t i = 1; i < tev.size(); i++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, tev[0], tev[i]);
            line += " " + std::to_string((int)(ms * 1000));
        }
        fprintf(stderr, "%s\n", line.c_str());
        for (hipEvent_t e : tev) (void)hipEventDestroy(e);
    }
    *dver_out = dver;
    *hver_out = c.h_ver.as<uint64_t>();
    return PV_OK;
}

extern "C" {

int pv_verify_batch(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk,
                    uint8_t* verdict_bits) {
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_verify_batch: call pv_init first");
    if (n == 0) return PV_OK;
    if (!sm || !sm_off || !pk || !verdict_bits) return fail(PV_ERR_ARG, "null pointer");
    if (!offsets_nondecreasing(sm_off, n)) return fail(PV_ERR_ARG, "sm_off must be non-decreasing");
    std::lock_guard<std::mutex> lk(g_mu);
    {
        // a small call that takes the latency path (plan_batch, chunk_plan.h: the choice launch_chunks makes
        // for a host-buffer call, which sets the hint it counted; the cache's state is not read then) and
        // whose records fit a 2 KB slot: the kernel reads the pinned staging slots over PCIe and stores one
        // verdict byte per request back -- no copy kernels around it
        uint64_t maxlen = 0;
        for (uint64_t i = 0; i < n && n <= PV_ZC_MAX_REQ; i++) maxlen = std::max(maxlen, sm_off[i + 1] - sm_off[i]);
        const uint64_t stride = (4ull * PV_ZC_REC_WORD + maxlen + PV_ZC_SLACK + 63) & ~63ull;
        if (!g_ctx.timing && n <= PV_ZC_MAX_REQ && stride <= PV_ZC_MAX_STRIDE &&
            pvhost::plan_batch({g_ctx.path, n, true, pv_keyed_hint(pk, n), false}).latency) {
            int rc = ensure_stage(n * stride, 0);
            if (rc) return rc;
            uint8_t* vb = g_ctx.h_zc_verdict;  // coherent pinned memory, read while the kernel runs
            uint8_t* slots = g_ctx.h_stage.p;
            memset(vb, 0xFF, n);  // pending: the host spins on these bytes instead of a stream sync
            auto fill_at = [&](uint8_t* base, uint64_t a, uint64_t b) {
                for (uint64_t i = a; i < b; i++) {
                    uint8_t* sl = base + i * stride;
                    const uint64_t len = sm_off[i + 1] - sm_off[i];
                    const uint32_t hdr[PV_ZC_PK_WORD] = {(uint32_t)len, 0u, 0u, 0u};
                    memcpy(sl, hdr, sizeof(hdr));
                    memcpy(sl + 4 * PV_ZC_PK_WORD, pk + 32 * i, 32);
                    memcpy(sl + 4 * PV_ZC_REC_WORD, sm + sm_off[i], len);
                    memset(sl + 4 * PV_ZC_REC_WORD + len, 0, stride - 4 * PV_ZC_REC_WORD - len);
                }
            };
            const bool one = n == 1 && stride <= sizeof(PvZcOne);  // the slot goes in the kernel arguments
            PvZcOne one_slot;
            if (one) {
                fill_at(reinterpret_cast<uint8_t*>(one_slot.w), 0, 1);
            } else if (n * stride < (128u << 10)) {
                fill_at(slots, 0, n);
            } else {  // node-quota sizes: the slots are written by the copy pool's threads
                const unsigned k = 8;
                cur_pool().run(k, [&](unsigned t) { fill_at(slots, n * t / k, n * (t + 1) / k); });
            }
            hipStream_t s = g_ctx.stream;
            if ((rc = g_ctx.hand.begin(s))) return rc;
            g_ctx.last_latency = true;
            g_ctx.last_keyed = false;
            g_ctx.last_dev_choice = false;
            g_ctx.last_zero_copy = true;
            rc = one ? pv_latency_launch_zc_one(one_slot, (uint32_t)stride, g_ctx.d_bcomb, kc_view(), vb, s)
                     : pv_latency_launch_zc(slots, (uint32_t)stride, n, g_ctx.d_bcomb, kc_view(), vb, s);
            if (int rc2 = g_ctx.hand.end(s)) return rc2;
            if (rc) {
                (void)hipStreamSynchronize(s);
                return rc;
            }
            rc = kc_auto_after_batch(pk, n, s, vb, nullptr);  // returns once the verdict bytes are written
            if (rc) return rc;
            memset(verdict_bits, 0, (n + 7) / 8);
            for (uint64_t i = 0; i < n; i++) verdict_bits[i >> 3] |= (uint8_t)((vb[i] & 1u) << (i & 7));
            return PV_OK;
        }
    }
    uint64_t *dver = nullptr, *hver = nullptr;
    int rc = stage_and_launch(sm, sm_off, n, pk, nullptr, &dver, &hver);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(hver, dver, (n + 63) / 64 * 8, hipMemcpyDeviceToHost, g_ctx.stream), PV_ERR_LAUNCH);
    rc = kc_auto_after_batch(pk, n, g_ctx.stream, nullptr, hver);
    if (rc) return rc;
    memcpy(verdict_bits, hver, (n + 7) / 8);  // little-endian words, LSB-first bits
    return PV_OK;
}

int pv_host_alloc(void** p, uint64_t bytes) {
    if (!p) return fail(PV_ERR_ARG, "pv_host_alloc: null pointer");
    *p = nullptr;
    bytes = std::max<uint64_t>(bytes, 64);
    pvhost::PinnedCache::Block b = pinned_cache().take(bytes);  // a block an earlier pv_host_free released
    if (!b.p) {
        b.bytes = bytes;
        if (hipHostMalloc(&b.p, bytes, hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            pinned_release(pinned_cache().drain());  // the cached blocks back to the system, then once more
            PV_HIP(hipHostMalloc(&b.p, bytes, hipHostMallocPortable), PV_ERR_ALLOC);
        }
    }
    g_pinned_alloc.add(b.p, b.bytes);
    *p = b.p;
    return PV_OK;
}
int pv_host_free(void* p) {
    if (!p) return PV_OK;
    const uint64_t bytes = g_pinned_alloc.size_of(p);
    if (!bytes || !g_pinned_alloc.remove(p)) return fail(PV_ERR_ARG, "pv_host_free: not a pv_host_alloc block");
    pinned_release(pinned_cache().put(p, bytes));  // kept pinned for the next allocation of a similar size
    return PV_OK;
}
int pv_host_register(void* p, uint64_t bytes) {
    if (!p || bytes == 0) return fail(PV_ERR_ARG, "pv_host_register: empty range");
    PV_HIP(hipHostRegister(p, bytes, hipHostRegisterPortable), PV_ERR_ALLOC);
    g_pinned_reg.add(p, bytes);
    return PV_OK;
}
int pv_host_unregister(void* p) {
    if (!p || g_pinned_reg.size_of(p) == 0) return fail(PV_ERR_ARG, "pv_host_unregister: not a registered range");
    // the runtime first: if it refuses, the registry still describes what is pinned
    PV_HIP(hipHostUnregister(p), PV_ERR_ALLOC);
    (void)g_pinned_reg.remove(p);
    return PV_OK;
}
int pv_host_is_pinned(const void* p, uint64_t bytes) { return pv_is_pinned(p, bytes) ? 1 : 0; }

int pv_test_inject(int what, int device, int count) {
    const char* on = getenv("PV_ENABLE_TEST_HOOKS");
    if (!on || strcmp(on, "1") != 0) return fail(PV_ERR_ARG, "pv_test_inject: test hooks are disabled (PV_ENABLE_TEST_HOOKS=1)");
    if (what != PV_INJECT_STAGE) return fail(PV_ERR_ARG, "pv_test_inject: unknown fault");
    if (device < 0 || device >= PV_MAX_DEV || count < 0) return fail(PV_ERR_ARG, "pv_test_inject: bad device / count");
    std::lock_guard<std::mutex> lk(g_mus[device]);
    g_ctxs[device].inject_stage = count;
    return PV_OK;
}

int pv_dev_alloc(void** p, uint64_t bytes) {
    PV_HIP(hipMalloc(p, std::max<uint64_t>(bytes, 16)), PV_ERR_ALLOC);
    return PV_OK;
}
int pv_dev_free(void* p) {
    PV_HIP(hipFree(p), PV_ERR_ALLOC);
    return PV_OK;
}

int pv_memcpy_h2d(void* dst, const void* src, uint64_t bytes) { return ordered_copy(dst, src, bytes, hipMemcpyHostToDevice); }
int pv_memcpy_d2h(void* dst, const void* src, uint64_t bytes) { return ordered_copy(dst, src, bytes, hipMemcpyDeviceToHost); }
int pv_last_zero_copy(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_ctx.last_zero_copy ? 1 : 0;
}

}  // extern "C"
