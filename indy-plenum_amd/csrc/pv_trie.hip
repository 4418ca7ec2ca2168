// The hashing half of the batched state-trie update on the GPU: SHA3-256 (keccak.h) of every new node,
// one lane per node, depth by depth. The structural half (trie_host.cpp) lays every node's RLP out in an
// arena with a 32-byte hole per hashed child; a node's lane absorbs its record, then stores the digest
// into its parent's hole and into the output hash array. A depth's nodes only need the depths below, so:
//   pv_sha3_batch_kernel  one launch per depth, deepest first, while that depth and everything above it
//                         hold more than TR_TAIL_MAX nodes;
//   pv_sha3_tail_kernel   one workgroup for all remaining depths in a single launch, a fence and a
//                         barrier between depths (as pv_merkle_upper_kernel for the upper Merkle
//                         levels): a long, thin top of the trie costs no launches.
// and pv_sha3_blob_kernel, the primitive on its own: records in a blob plus offsets, at any alignment.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/plenum_verify.h"
#include "keccak.h"
#include "pv_internal.h"
#include "trie_host.h"

namespace {

constexpr int TR_BLOCK = 256;
constexpr uint64_t TR_TAIL_MAX = 256;  // records the single-workgroup tail takes: one per lane

__device__ __forceinline__ void tr_hash_record(uint8_t* arena, const PvTrieRec& r, uint64_t* out) {
    uint64_t d[4];
    sha3_256(d, r.len, PvKeccakWords(arena + r.off, r.len));
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = d[k];
    if (r.hole != PV_TRIE_NO_HOLE) {  // the hole lies at any byte offset of the parent's record
        uint8_t* h = arena + r.hole;
#pragma unroll
        for (int k = 0; k < 32; k++) h[k] = (uint8_t)(d[k >> 3] >> (8 * (k & 7)));
    }
}

// records [first, first + count): one depth
__global__ __launch_bounds__(TR_BLOCK) void pv_sha3_batch_kernel(uint8_t* arena, const PvTrieRec* __restrict__ recs,
                                                                 uint32_t first, uint32_t count, uint64_t* hashes) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= count) return;
    tr_hash_record(arena, recs[first + i], hashes + 4 * (uint64_t)(first + i));
}

// records [first, n): every remaining depth, one workgroup
__global__ __launch_bounds__(TR_BLOCK) void pv_sha3_tail_kernel(uint8_t* arena, const PvTrieRec* __restrict__ recs,
                                                                uint32_t first, uint32_t n, uint64_t* hashes) {
    for (uint32_t i0 = first; i0 < n;) {
        const uint32_t i1 = recs[i0].next;  // uniform
        for (uint32_t i = i0 + threadIdx.x; i < i1; i += TR_BLOCK) tr_hash_record(arena, recs[i], hashes + 4 * (uint64_t)i);
        __threadfence();  // the next depth reads this depth's digests
        __syncthreads();
        i0 = i1;
    }
}

__global__ __launch_bounds__(TR_BLOCK) void pv_sha3_blob_kernel(const uint8_t* __restrict__ data,
                                                                const uint64_t* __restrict__ off, uint64_t n,
                                                                uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], len = off[i + 1] - a;
    uint64_t d[4];
    sha3_256(d, len, PvKeccakWords(data + a, len));
#pragma unroll
    for (int k = 0; k < 4; k++) out[4 * i + k] = d[k];
}

// --------------------------------------------------------------------------------------------- host

#define TR_HIP(call, code)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) return pv_fail(code, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The trie code's own workspace: allocated on first use (an engine that never touches a trie holds
// nothing), freed by pv_shutdown, handed over between caller streams by an event as the Merkle
// workspace is. Launches are serialised on g_tr_mu.
struct TrWork {
    uint8_t* d_in = nullptr;  // the arena and its records, or a blob and its offsets
    uint64_t d_in_cap = 0;
    uint8_t* d_out = nullptr;  // digests
    uint64_t d_out_cap = 0;
    hipEvent_t ev_done = nullptr;
    hipStream_t last_stream = nullptr;
};
TrWork g_tr;
std::mutex g_tr_mu;
int g_tr_path = PV_TRIE_AUTO;

uint64_t tr_up(uint64_t x) { return (x + 255) & ~255ull; }

int tr_grow(uint8_t*& p, uint64_t& cap, uint64_t want) {
    if (want <= cap) return PV_OK;
    if (p) (void)hipFree(p);  // synchronises: no launch still reads the old block
    p = nullptr;
    cap = 0;
    TR_HIP(hipMalloc((void**)&p, want), PV_ERR_ALLOC);
    cap = want;
    return PV_OK;
}
int tr_begin(hipStream_t stream) {
    if (!g_tr.ev_done) TR_HIP(hipEventCreateWithFlags(&g_tr.ev_done, hipEventDisableTiming), PV_ERR_NO_DEVICE);
    if (g_tr.last_stream && g_tr.last_stream != stream) TR_HIP(hipStreamWaitEvent(stream, g_tr.ev_done, 0), PV_ERR_LAUNCH);
    return PV_OK;
}
int tr_end(hipStream_t stream) {
    TR_HIP(hipEventRecord(g_tr.ev_done, stream), PV_ERR_LAUNCH);
    g_tr.last_stream = stream;
    return PV_OK;
}

bool tr_monotone(const uint64_t* o, uint64_t k) {
    for (uint64_t i = 0; i < k; i++)
        if (o[i + 1] < o[i]) return false;
    return true;
}

// The launches for nr records on device buffers. Caller holds g_tr_mu.
int tr_enqueue(uint8_t* d_arena, const PvTrieRec* d_recs, const PvTrieRec* recs, uint64_t nr, uint64_t* d_hashes,
               hipStream_t st, uint64_t* launches, uint64_t* tail_records) {
    for (uint64_t i0 = 0; i0 < nr;) {
        if (nr - i0 <= TR_TAIL_MAX) {
            hipLaunchKernelGGL(pv_sha3_tail_kernel, dim3(1), dim3(TR_BLOCK), 0, st, d_arena, d_recs, (uint32_t)i0,
                               (uint32_t)nr, d_hashes);
            TR_HIP(hipGetLastError(), PV_ERR_LAUNCH);
            ++*launches;
            *tail_records = nr - i0;
            break;
        }
        const uint64_t i1 = recs[i0].next, count = i1 - i0;
        hipLaunchKernelGGL(pv_sha3_batch_kernel, dim3((unsigned)((count + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0, st,
                           d_arena, d_recs, (uint32_t)i0, (uint32_t)count, d_hashes);
        TR_HIP(hipGetLastError(), PV_ERR_LAUNCH);
        ++*launches;
        i0 = i1;
    }
    return PV_OK;
}

// arena and records staged whole, hashed, copied back: arena -> blob, digests -> hashes
int tr_device_hash(PvTriePlan& plan, uint8_t* blob, uint8_t* hashes, uint64_t* launches, uint64_t* tail_records) {
    const hipStream_t st = pv_engine_stream();
    int rc = tr_begin(st);
    if (rc) return rc;
    auto run = [&]() -> int {
        const uint64_t nr = plan.recs.size(), i_recs = tr_up(plan.arena_bytes);
        int rc;
        if ((rc = tr_grow(g_tr.d_in, g_tr.d_in_cap, i_recs + tr_up(nr * sizeof(PvTrieRec)))) ||
            (rc = tr_grow(g_tr.d_out, g_tr.d_out_cap, tr_up(32 * nr))))
            return rc;
        TR_HIP(hipMemcpyAsync(g_tr.d_in, plan.arena.data(), plan.arena_bytes, hipMemcpyHostToDevice, st), PV_ERR_LAUNCH);
        TR_HIP(hipMemcpyAsync(g_tr.d_in + i_recs, plan.recs.data(), nr * sizeof(PvTrieRec), hipMemcpyHostToDevice, st),
               PV_ERR_LAUNCH);
        if ((rc = tr_enqueue(g_tr.d_in, reinterpret_cast<const PvTrieRec*>(g_tr.d_in + i_recs), plan.recs.data(), nr,
                             reinterpret_cast<uint64_t*>(g_tr.d_out), st, launches, tail_records)))
            return rc;
        TR_HIP(hipMemcpyAsync(blob, g_tr.d_in, plan.arena_bytes, hipMemcpyDeviceToHost, st), PV_ERR_LAUNCH);
        TR_HIP(hipMemcpyAsync(hashes, g_tr.d_out, 32 * nr, hipMemcpyDeviceToHost, st), PV_ERR_LAUNCH);
        TR_HIP(hipStreamSynchronize(st), PV_ERR_LAUNCH);
        return PV_OK;
    };
    rc = run();
    const int rc2 = tr_end(st);
    return rc ? rc : rc2;
}

// PV_OK with *device set, or PV_ERR_NO_DEVICE for a forced device path without a device. Caller holds g_tr_mu.
int tr_choose(uint64_t work, const char* who, bool* device) {
    const bool have_dev = pv_engine_stream() != nullptr;
    if (g_tr_path == PV_TRIE_DEVICE && !have_dev)
        return pv_fail(PV_ERR_NO_DEVICE, std::string(who) + ": the device path is forced and no device is initialised");
    *device = work > 0 && have_dev && (g_tr_path == PV_TRIE_DEVICE || (g_tr_path == PV_TRIE_AUTO && work >= PV_TRIE_AUTO_MIN));
    return PV_OK;
}

}  // namespace

void pv_trie_forget_stream(void* stream) {
    std::lock_guard<std::mutex> lk(g_tr_mu);
    if (g_tr.last_stream == (hipStream_t)stream) g_tr.last_stream = nullptr;
}

void pv_trie_shutdown() {
    std::lock_guard<std::mutex> lk(g_tr_mu);
    for (void* p : {(void*)g_tr.d_in, (void*)g_tr.d_out})
        if (p) (void)hipFree(p);
    if (g_tr.ev_done) (void)hipEventDestroy(g_tr.ev_done);
    g_tr = TrWork();
}

extern "C" {

int pv_trie_path(int mode) {
    std::lock_guard<std::mutex> lk(g_tr_mu);
    if (mode != PV_TRIE_AUTO && mode != PV_TRIE_HOST && mode != PV_TRIE_DEVICE)
        return pv_fail(PV_ERR_ARG, "pv_trie_path: unknown mode");
    g_tr_path = mode;
    return PV_OK;
}

int pv_sha3_256_batch(const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* out) {
    if (n == 0) return PV_OK;
    if (!off || !out) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: null pointer");
    if (!tr_monotone(off, n)) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: offsets must be non-decreasing");
    if (!data && off[n] != off[0]) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: null data");
    if (n >> 31) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: more than 2^31 - 1 records");
    std::unique_lock<std::mutex> lk(g_tr_mu);
    bool device;
    int rc = tr_choose(n, "pv_sha3_256_batch", &device);
    if (rc) return rc;
    if (!device) {
        lk.unlock();  // the host path shares no workspace
        pv_sha3_host_batch(data, off, n, out);
        return PV_OK;
    }
    const hipStream_t st = pv_engine_stream();
    if ((rc = tr_begin(st))) return rc;
    auto run = [&]() -> int {
        // staged whole: [offsets, rebased][data, to a whole word]
        const uint64_t base = off[0], bytes = off[n] - base, i_data = tr_up(8 * (n + 1));
        int rc;
        if ((rc = tr_grow(g_tr.d_in, g_tr.d_in_cap, i_data + tr_up(bytes + 8))) ||
            (rc = tr_grow(g_tr.d_out, g_tr.d_out_cap, tr_up(32 * n))))
            return rc;
        std::vector<uint64_t> rebased(n + 1);
        for (uint64_t i = 0; i <= n; i++) rebased[i] = off[i] - base;
        TR_HIP(hipMemcpyAsync(g_tr.d_in, rebased.data(), 8 * (n + 1), hipMemcpyHostToDevice, st), PV_ERR_LAUNCH);
        if (bytes) TR_HIP(hipMemcpyAsync(g_tr.d_in + i_data, data + base, bytes, hipMemcpyHostToDevice, st), PV_ERR_LAUNCH);
        hipLaunchKernelGGL(pv_sha3_blob_kernel, dim3((unsigned)((n + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0, st,
                           g_tr.d_in + i_data, reinterpret_cast<const uint64_t*>(g_tr.d_in), n,
                           reinterpret_cast<uint64_t*>(g_tr.d_out));
        TR_HIP(hipGetLastError(), PV_ERR_LAUNCH);
        TR_HIP(hipMemcpyAsync(out, g_tr.d_out, 32 * n, hipMemcpyDeviceToHost, st), PV_ERR_LAUNCH);
        TR_HIP(hipStreamSynchronize(st), PV_ERR_LAUNCH);
        return PV_OK;
    };
    rc = run();
    const int rc2 = tr_end(st);
    return rc ? rc : rc2;
}

int pv_sha3_256_batch_device(const uint8_t* d_data, const uint64_t* d_off, uint64_t n, uint8_t* d_out, void* stream) {
    if (!pv_engine_stream()) return pv_fail(PV_ERR_NOT_INIT, "pv_sha3_256_batch_device: call pv_init first");
    if (n == 0) return PV_OK;
    if (!d_data || !d_off || !d_out) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch_device: null pointer");
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch_device: d_out must be 8-byte aligned");
    if (n >> 31) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch_device: more than 2^31 - 1 records");
    hipLaunchKernelGGL(pv_sha3_blob_kernel, dim3((unsigned)((n + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0,
                       stream ? (hipStream_t)stream : pv_engine_stream(), d_data, d_off, n, reinterpret_cast<uint64_t*>(d_out));
    TR_HIP(hipGetLastError(), PV_ERR_LAUNCH);
    return PV_OK;
}

int pv_trie_update_batch(const uint8_t* root, const uint8_t* known_hash, const uint8_t* known_blob,
                         const uint64_t* known_off, uint64_t n_known, const uint8_t* key_blob, const uint64_t* key_off,
                         const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, PvTrieOut* out) {
    if (!root || !out || !out->root) return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: null root or output struct");
    out->n_nodes = out->blob_bytes = out->n_missing = out->launches = out->tail_records = 0;
    if (n == 0) {
        memcpy(out->root, root, 32);
        return PV_OK;
    }
    if (!key_off || !val_off || !val_blob) return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: null keys or values");
    if (!tr_monotone(key_off, n) || !tr_monotone(val_off, n))
        return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: offsets must be non-decreasing");
    if (!key_blob && key_off[n] != key_off[0]) return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: null key blob");
    if (n_known && (!known_hash || !known_blob || !known_off || !tr_monotone(known_off, n_known)))
        return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: known nodes need hashes, a blob and non-decreasing offsets");
    if ((out->node_cap && (!out->node_hash || !out->node_off || !out->node_len)) || (out->blob_cap && !out->node_blob) ||
        (out->missing_cap && !out->missing))
        return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: a capacity without its array");
    {
        std::lock_guard<std::mutex> lk(g_tr_mu);
        if (g_tr_path == PV_TRIE_DEVICE && !pv_engine_stream())
            return pv_fail(PV_ERR_NO_DEVICE, "pv_trie_update_batch: the device path is forced and no device is initialised");
    }
    const PvTrieIn in{root, known_hash, known_blob, known_off, n_known, key_blob, key_off, val_blob, val_off, n};
    PvTriePlan plan;
    std::string err;
    int rc = pv_trie_host_build(in, &plan, &err);
    if (rc == PV_TRIE_NEED_NODES) {
        out->n_missing = plan.missing.size() / 32;
        if (out->missing_cap) memcpy(out->missing, plan.missing.data(), 32 * std::min(out->n_missing, out->missing_cap));
        return rc;
    }
    if (rc) return pv_fail(rc, "pv_trie_update_batch: " + err);
    const uint64_t nr = plan.recs.size();
    out->n_nodes = nr;
    out->blob_bytes = plan.arena_bytes;
    if (nr == 0) {  // nothing to set
        memcpy(out->root, root, 32);
        return PV_OK;
    }
    if (nr > out->node_cap || plan.arena_bytes > out->blob_cap) return PV_TRIE_NEED_SPACE;
    std::unique_lock<std::mutex> lk(g_tr_mu);
    bool device;
    if ((rc = tr_choose(nr, "pv_trie_update_batch", &device))) return rc;
    if (device) {
        if ((rc = tr_device_hash(plan, out->node_blob, out->node_hash, &out->launches, &out->tail_records))) return rc;
    } else {
        lk.unlock();  // the host path shares no workspace; it hashes in the plan's own (aligned) arena
        pv_trie_host_hash(reinterpret_cast<uint8_t*>(plan.arena.data()), plan.recs.data(), nr, out->node_hash);
        memcpy(out->node_blob, plan.arena.data(), plan.arena_bytes);
    }
    for (uint64_t i = 0; i < nr; i++) {
        out->node_off[i] = plan.recs[i].off;
        out->node_len[i] = plan.recs[i].len;
    }
    memcpy(out->root, out->node_hash + 32 * (nr - 1), 32);  // the root is the last record
    return PV_OK;
}

}  // extern "C"
