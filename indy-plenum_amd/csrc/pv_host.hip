// libplenum_verify: the host-buffer entries of the verification engine. pv_verify_batch reads: validate,
// lock, the zero-copy form if the gate says so (verify_zero_copy), otherwise stage_and_launch, copy back,
// admit. stage_and_launch plans the call (host_plan.h: layout, sub-batch bounds, form), sizes the staging
// and runs one of two straight-line forms: stage_one_dma (one host copy, one DMA, the kernels) or
// stage_pipelined (per sub-batch: pinned staging, H2D on the copy stream, kernels on the engine stream).
// What depends on numbers alone is decided in host_plan.h and kc_admit.h and tested on a CPU; this file
// reads the facts and enqueues. The environment is read in three places: PV_PINNED_CACHE_MB, PV_PIPE_SUB,
// PV_ENABLE_TEST_HOOKS. Also here: the pinned-memory registry and cache (pv_host_*), the copy workers,
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
#include "host_plan.h"
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
    return pvhost::few_distinct_keys(pk, n);
}

// Requests per sub-batch of the pipelined form: the environment's PV_PIPE_SUB, read once, else the default.
static uint64_t pipe_sub() {
    static const uint64_t v = [] {
        const char* e = getenv("PV_PIPE_SUB");
        return pvhost::pipe_sub_of(e && *e ? strtoull(e, nullptr, 10) : (uint64_t)PV_PIPE_SUB);
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
    // the requests counted: all of a batch of <= 4,096, else a sample (kc_admit.h admit_sample); their
    // table entries are located while the kernels still run
    std::vector<uint64_t> sample;
    std::vector<int32_t> pre;
    uint64_t gen = 0;
    if (on) {
        sample = pvhost::admit_sample(n, PV_KC_AUTO_MAX_BATCH);
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

namespace {

// One staged call: the caller's pointers, the layout and the plan (host_plan.h), and the sections of the
// host and device staging areas they resolve to.
struct HostCall {
    const uint8_t* sm;
    const uint64_t* sm_off;
    uint64_t n;
    const uint8_t* pk;
    uint64_t* d_out;      // where the verdict words go (nullptr: dver)
    uint64_t base, blob;  // sm_off[0], and the records' bytes from there
    pvhost::HostLayout lay;
    pvhost::CallPlan plan;
    uint8_t *h, *d;  // host (pinned) and device staging
    uint64_t *hoff, *doff, *dver;
    uint8_t *hblob, *dblob;
};

// Requests [lo, hi) of the call, staged on the device, enqueued on the engine stream.
int launch_piece(const HostCall& k, uint64_t lo, uint64_t hi) {
    Ctx& c = g_ctx;
    c.verdict_zeroed = k.d_out == nullptr;
    c.keyed_hint = pv_keyed_hint(k.pk + 32 * lo, hi - lo);
    c.hint_set = true;
    const int r = launch(k.dblob, k.doff + lo, hi - lo, k.d + 32 * lo, (k.d_out ? k.d_out : k.dver) + lo / 64, c.stream);
    c.verdict_zeroed = false;
    c.keyed_hint = false;
    c.hint_set = false;
    return r;
}

int injected_failure() {
    g_ctx.inject_stage--;
    return fail(PV_ERR_ALLOC, "stage_and_launch: injected staging failure (pv_test_inject)");
}

// The quota sizes: everything in the device layout in pinned staging, one DMA, the kernels.
int stage_one_dma(const HostCall& k, uint64_t** dver_out, uint64_t** hver_out) {
    Ctx& c = g_ctx;
    hipStream_t s = c.stream;
    const uint64_t n = k.n;
    const unsigned w = n >= (1u << 16) ? 8u : 1u;
    cur_pool().run(w, [&](unsigned t) {
        const uint64_t a = n * t / w, b = n * (t + 1) / w;
        memcpy(k.h + 32 * a, k.pk + 32 * a, 32 * (b - a));
        for (uint64_t i = a; i < b; i++) k.hoff[i] = k.sm_off[i] - k.base;
    });
    k.hoff[n] = k.sm_off[n] - k.base;
    memset(k.h + k.lay.ver, 0, k.lay.ver_bytes);  // the verdict words travel zeroed
    memset(k.hblob + k.blob, 0, PV_BLOB_SLACK);
    if (c.inject_stage > 0) return injected_failure();
    if (k.blob < (256ull << 10)) {
        memcpy(k.hblob, k.sm + k.base, k.blob);
    } else if (int rc = pv_stage_to_device(k.dblob, k.hblob, k.sm + k.base, k.blob, s, false)) {
        return rc;
    }
    PV_HIP(hipMemcpyAsync(k.d, k.h, k.lay.total, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
    if (int rc = launch_piece(k, 0, n)) return rc;
    *dver_out = k.dver;
    *hver_out = reinterpret_cast<uint64_t*>(k.h + k.lay.ver);
    return PV_OK;
}

// Sub-batch j's pageable inputs into pinned staging (copy workers), its H2D on the copy stream, then
// ev_copy[j].
int copy_piece(const HostCall& k, uint64_t j) {
    Ctx& c = g_ctx;
    hipStream_t cs = c.cstream;
    const pvhost::CallPlan& p = k.plan;
    const uint64_t lo = p.bnd[j], hi = p.bnd[j + 1];
    const uint64_t b0 = k.sm_off[lo] - k.base, b1 = k.sm_off[hi] - k.base;
    if (!p.all_pin) {
        pvhost::CopyPool& pool = cur_pool();
        const unsigned w = std::max(1u, std::min(pool.threads(), (unsigned)((b1 - b0) >> 22)));
        pool.run(w, [&](unsigned t) {
            const uint64_t a = lo + (hi - lo) * t / w, b = lo + (hi - lo) * (t + 1) / w;
            if (!p.pin_pk) memcpy(k.h + 32 * a, k.pk + 32 * a, 32 * (b - a));
            if (!p.pin_off)
                for (uint64_t i = a; i < b; i++) k.hoff[i] = k.sm_off[i] - k.base;
            if (!p.pin_sm) memcpy(k.hblob + (k.sm_off[a] - k.base), k.sm + k.sm_off[a], k.sm_off[b] - k.sm_off[a]);
        });
        if (!p.pin_off) k.hoff[hi] = k.sm_off[hi] - k.base;
    }
    // an input in pinned memory is DMA'd where it is, the others from pinned staging
    const uint8_t* spk = p.pin_pk ? k.pk : k.h;
    const uint64_t* soff = p.pin_off ? k.sm_off : k.hoff;
    const uint8_t* sblob = p.pin_sm ? k.sm + k.base : k.hblob;
    PV_HIP(hipMemcpyAsync(k.d + 32 * lo, spk + 32 * lo, 32 * (hi - lo), hipMemcpyHostToDevice, cs), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpyAsync(k.doff + lo, soff + lo, 8 * (hi - lo + 1), hipMemcpyHostToDevice, cs), PV_ERR_LAUNCH);
    if (b1 > b0) PV_HIP(hipMemcpyAsync(k.dblob + b0, sblob + b0, b1 - b0, hipMemcpyHostToDevice, cs), PV_ERR_LAUNCH);
    PV_HIP(hipEventRecord(c.ev_copy[j], cs), PV_ERR_LAUNCH);
    return PV_OK;
}

// The pipeline's enqueues: the copies on the copy stream, each sub-batch's kernels on the engine stream
// behind its copies' event. `share`: the sub-batches share one set of comb tables (CallPlan::may_share).
int enqueue_pipeline(const HostCall& k, bool share) {
    Ctx& c = g_ctx;
    hipStream_t s = c.stream, cs = c.cstream;
    const pvhost::CallPlan& p = k.plan;
    if (share) PV_HIP(hipMemsetAsync(c.xt.htab, 0xFF, PV_XT_HASH * 4, s), PV_ERR_LAUNCH);
    if (!k.d_out) PV_HIP(hipMemsetAsync(k.dver, 0, k.lay.vwords * 8, s), PV_ERR_LAUNCH);  // the latency path ORs bits
    PV_HIP(hipMemsetAsync(k.dblob + k.blob, 0, PV_BLOB_SLACK, cs), PV_ERR_LAUNCH);
    if (int rc = copy_piece(k, 0)) return rc;
    for (uint64_t j = 0; j < p.np; j++) {
        // sub-batch j + 1's copies are enqueued BEFORE sub-batch j's kernels: should the copy stream share a
        // hardware queue with one of the engine's streams, no copy waits behind kernels enqueued before it
        // (the other order is never faster: profiles/r05/host_path/ab_prio_lookahead.txt)
        if (j + 1 < p.np)
            if (int rc = copy_piece(k, j + 1)) return rc;
        if (c.inject_stage > 0 && j == p.inject_at) return injected_failure();
        PV_HIP(hipStreamWaitEvent(s, c.ev_copy[j], 0), PV_ERR_LAUNCH);
        c.xt_fill = share && j == 0;
        c.xt_use = share && j > 0;
        const int rc = launch_piece(k, p.bnd[j], p.bnd[j + 1]);
        c.xt_fill = c.xt_use = false;
        if (rc) return rc;
    }
    return PV_OK;
}

// Everything else, in the plan's sub-batches, so that PCIe, host staging and kernels of consecutive
// sub-batches overlap. How the copies and kernels interleave is seen in a kernel and memory-copy trace
// (profiles/r05/host_path/overlap.txt).
int stage_pipelined(const HostCall& k, uint64_t** dver_out, uint64_t** hver_out) {
    Ctx& c = g_ctx;
    hipStream_t s = c.stream, cs = c.cstream;
    if (int rc = c.h_ver.grow(std::max<uint64_t>(k.lay.ver_bytes, 64 << 10), hipHostMallocPortable)) return rc;
    while (c.ev_copy.size() < k.plan.np) {
        hipEvent_t e;
        if (int rc = c.own.event(e, hipEventDisableTiming)) return rc;
        c.ev_copy.push_back(e);
    }
    // the copy stream starts after everything enqueued so far (the previous users of the staging area)
    PV_HIP(hipEventRecord(c.ev_cstart, s), PV_ERR_LAUNCH);
    PV_HIP(hipStreamWaitEvent(cs, c.ev_cstart, 0), PV_ERR_LAUNCH);
    if (int rc = c.hand.wait(cs, s)) return rc;
    const bool share = k.plan.may_share && ensure_xtab() == PV_OK;
    if (int rc = enqueue_pipeline(k, share)) {
        (void)hipStreamSynchronize(cs);  // no DMA may still read the caller's or the staging buffers
        (void)hipStreamSynchronize(s);
        return rc;
    }
    *dver_out = k.dver;
    *hver_out = c.h_ver.as<uint64_t>();
    return PV_OK;
}

// The zero-copy form of a small call that takes the latency path and whose records fit a 2 KB slot: the
// kernel reads the pinned staging slots over PCIe and stores one verdict byte per request back -- no copy
// kernels around it.
int verify_zero_copy(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk, uint64_t stride,
                     uint8_t* verdict_bits) {
    int rc = ensure_stage(n * stride, 0);
    if (rc) return rc;
    uint8_t* vb = g_ctx.h_zc_verdict;  // coherent pinned memory, read while the kernel runs
    uint8_t* slots = g_ctx.h_stage.p;
    memset(vb, 0xFF, n);  // pending: the host spins on these bytes instead of a stream sync
    const bool one = n == 1 && stride <= sizeof(PvZcOne);  // the slot goes in the kernel arguments
    PvZcOne one_slot;
    if (one) {
        pvhost::zc_fill_slots(reinterpret_cast<uint8_t*>(one_slot.w), stride, sm, sm_off, pk, 0, 1);
    } else if (n * stride < (128u << 10)) {
        pvhost::zc_fill_slots(slots, stride, sm, sm_off, pk, 0, n);
    } else {  // node-quota sizes: the slots are written by the copy pool's threads
        const unsigned w = 8;
        cur_pool().run(w, [&](unsigned t) {
            pvhost::zc_fill_slots(slots, stride, sm, sm_off, pk, n * t / w, n * (t + 1) / w);
        });
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

}  // namespace

// The copy form of a host-buffer batch on the calling thread's context: moves the keys, offsets and
// records to the device staging area and enqueues the verification on the context's stream. d_out:
// where the verdict words go (nullptr = the staging area's own verdict section); *dver / *hver receive
// the device verdict section and a pinned buffer for the caller's copy back. Three steps: plan the call
// (host_plan.h: the layout, the sub-batch bounds, the form), size the staging, run the form. A failure
// after DMAs were enqueued returns only after both streams drained, so no copy still reads the caller's
// or the staging buffers.
int stage_and_launch(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk, uint64_t* d_out,
                     uint64_t** dver_out, uint64_t** hver_out) {
    Ctx& c = g_ctx;
    c.last_zero_copy = false;
    HostCall k{sm, sm_off, n, pk, d_out, sm_off[0], sm_off[n] - sm_off[0]};
    k.lay = pvhost::plan_layout(n, k.blob);
    k.plan = pvhost::plan_call(pvhost::plan_pieces(n, k.blob, pipe_sub(), pvhost::pipe_end_req()),
                               pv_is_pinned(sm + k.base, k.blob), pv_is_pinned(pk, 32 * n),
                               k.base == 0 && pv_is_pinned(sm_off, 8 * (n + 1)), c.path, k.lay.total);
    if (int rc = ensure_stage(k.plan.host_bytes, k.lay.total)) return rc;
    k.h = c.h_stage.p;
    k.d = c.d_stage.p;
    k.hoff = reinterpret_cast<uint64_t*>(k.h + k.lay.off);
    k.doff = reinterpret_cast<uint64_t*>(k.d + k.lay.off);
    k.dver = reinterpret_cast<uint64_t*>(k.d + k.lay.ver);
    k.hblob = k.h + k.lay.blob;
    k.dblob = k.d + k.lay.blob;
    return k.plan.form == pvhost::ONE_DMA ? stage_one_dma(k, dver_out, hver_out)
                                          : stage_pipelined(k, dver_out, hver_out);
}

extern "C" {

int pv_verify_batch(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk,
                    uint8_t* verdict_bits) {
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_verify_batch: call pv_init first");
    if (n == 0) return PV_OK;
    if (!sm || !sm_off || !pk || !verdict_bits) return fail(PV_ERR_ARG, "null pointer");
    if (!offsets_nondecreasing(sm_off, n)) return fail(PV_ERR_ARG, "sm_off must be non-decreasing");
    std::lock_guard<std::mutex> lk(g_mu);
    // the zero-copy gate: the call takes the latency path (plan_batch, chunk_plan.h: the choice launch_chunks
    // makes for a host-buffer call, which sets the hint it counted; the cache's state is not read then) and
    // its longest record fits a slot
    uint64_t maxlen = 0;
    for (uint64_t i = 0; i < n && n <= PV_ZC_MAX_REQ; i++) maxlen = std::max(maxlen, sm_off[i + 1] - sm_off[i]);
    const uint64_t stride = pvhost::zc_stride(maxlen);
    if (!g_ctx.timing && n <= PV_ZC_MAX_REQ && stride <= PV_ZC_MAX_STRIDE &&
        pvhost::plan_batch({g_ctx.path, n, true, pv_keyed_hint(pk, n), false}).latency)
        return verify_zero_copy(sm, sm_off, n, pk, stride, verdict_bits);
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
