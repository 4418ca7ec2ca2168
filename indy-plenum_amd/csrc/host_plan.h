// What a host-buffer verification call (pv_verify_batch, a shard of pv_verify_batch_multi_gpu) decides from
// numbers alone, before it touches the device: the staging layout, the sub-batch bounds, which of the two
// staging forms the call takes and what follows from that, the key-repeat answer behind AUTO's host-side
// hint, and the slot format of the zero-copy form. Host only and without a runtime call, so
// tests/native/host_plan_check.cpp runs every function on a CPU; pv_host.hip gathers the facts (what is
// pinned, the path, PV_PIPE_SUB), asks here and enqueues what the plan names. The sampled requests of
// automatic admission are in kc_admit.h, next to the table they feed.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "chunk_plan.h"   // PV_PATH_*, PV_ALLCOMB_KEYS, PV_LATENCY_MAX
#include "pv_internal.h"  // PV_ZC_*; with workspace.h: PvLayout

// Requests per sub-batch of the pipelined form (a multiple of 64; the environment's PV_PIPE_SUB, read once
// per process, overrides it). Sub-batch j's H2D runs on the copy stream while sub-batch j-1's kernels run,
// so a large host batch costs about its PCIe time plus the last sub-batch's kernels instead of their sum.
#ifndef PV_PIPE_SUB
#define PV_PIPE_SUB 262144
#endif
// Requests of the first and of the last sub-batch of a call of >= 3 sub-batches: half a sub-batch. Smaller
// ends are slower (1M arena: 116.8-119.1 M/s at 131,072, 113.6-114.1 at 65,536, 110.4-112.7 at 32,768;
// profiles/r06/host_path/ab_pipe_end.txt): the copies are the critical path and a sub-batch's kernels
// beside a DMA take longer than a small last piece's copy, so the last FULL piece's kernels become the tail.
#ifndef PV_PIPE_END_DEFAULT
#define PV_PIPE_END_DEFAULT (PV_PIPE_SUB / 2)
#endif
#ifndef PV_KC_AUTO_MAX_BATCH
#define PV_KC_AUTO_MAX_BATCH 4096  // automatic admission counts every key of host batches up to this size (a sample above)
#endif
static constexpr uint64_t PV_PIPE_MAX = 64;               // sub-batches per call (copy events)
static constexpr uint64_t PV_PIPE_MIN_BLOB = 8ull << 20;  // smaller blobs: one piece

#pragma GCC visibility push(hidden)  // internal to libplenum_verify.so
namespace pvhost {

// The sub-batch size a process runs with: `x` requests as asked for, a multiple of 64 and at least 8,192.
inline uint64_t pipe_sub_of(uint64_t x) { return std::max<uint64_t>(8192, x / 64 * 64); }
// The first / last piece size handed to plan_pieces.
inline uint64_t pipe_end_req() { return (uint64_t)std::max(8192, (int)(PV_PIPE_END_DEFAULT)); }

// Staging layout of n >= 1 requests, the same on the host and on the device, in 256-byte aligned sections:
// [pk n*32][off (n+1) u64][verdict words][blob + PV_BLOB_SLACK]. The last section is not padded.
struct HostLayout {
    uint64_t pk, off, ver, blob;  // section offsets
    uint64_t vwords;              // verdict words, (n + 63) / 64
    uint64_t ver_bytes;           // the verdict section's size
    uint64_t total;
};
inline HostLayout plan_layout(uint64_t n, uint64_t blob_bytes) {
    HostLayout h;
    PvLayout l;
    h.vwords = (n + 63) / 64;
    h.pk = l.add(n * 32);
    h.off = l.add((n + 1) * 8);
    h.ver = l.add(h.vwords * 8);
    h.blob = l.at;
    h.ver_bytes = h.blob - h.ver;
    h.total = h.blob + blob_bytes + PV_BLOB_SLACK;
    return h;
}

// Sub-batch bounds (64-aligned; sub-batch j = requests [bnd[j], bnd[j + 1])) of a call of n requests whose
// records take blob_bytes, for sub-batches of `sub` requests. A blob below PV_PIPE_MIN_BLOB is one piece.
// The call ends one sub-batch's kernels after the last H2D, and the first sub-batch's kernels (which also
// build the shared tables) start only after the first H2D, so from three sub-batches on the first and the
// last are end_req requests, half a sub-batch (profiles/r05/host_path/ab_half_ends.txt: 1M requests as
// 0.5 + 3 x 1 + 0.5 of 262,144, no slower than four equal pieces); below that, n / sub equal pieces.
inline std::vector<uint64_t> plan_pieces(uint64_t n, uint64_t blob_bytes, uint64_t sub, uint64_t end_req) {
    std::vector<uint64_t> bnd{0};
    if (blob_bytes >= PV_PIPE_MIN_BLOB && n >= 3 * sub) {
        const uint64_t h = std::min<uint64_t>(end_req, sub) / 64 * 64;
        const uint64_t mid = n - 2 * h;
        const uint64_t k = std::min<uint64_t>(PV_PIPE_MAX - 2, std::max<uint64_t>(1, (mid + sub / 2) / sub));
        bnd.push_back(h);
        for (uint64_t j = 1; j < k; j++) bnd.push_back(h + (mid * j / k) / 64 * 64);
        bnd.push_back((n - h) & ~63ull);  // every bound a whole verdict word (n itself need not be)
    } else if (blob_bytes >= PV_PIPE_MIN_BLOB) {
        const uint64_t k = std::min<uint64_t>(PV_PIPE_MAX, std::max<uint64_t>(1, n / sub));
        for (uint64_t j = 1; j < k; j++) bnd.push_back((n * j / k) & ~63ull);
    }
    bnd.push_back(n);
    return bnd;
}

// The two forms of a staged call:
//   ONE_DMA    one piece and no input in pinned memory (the quota sizes): one host copy into pinned staging
//              in the device layout, one DMA, the kernels -- fewest packets on the path;
//   PIPELINED  otherwise: per sub-batch, the pageable inputs into pinned staging on the copy workers (inputs
//              in pinned memory are DMA'd where they are), the H2D on the copy stream, the kernels on the
//              engine stream after an event.
enum Form : int { ONE_DMA = 0, PIPELINED = 1 };
struct CallPlan {
    std::vector<uint64_t> bnd;  // plan_pieces
    uint64_t np;                // pieces, bnd.size() - 1
    bool pin_sm, pin_pk, pin_off, all_pin;
    Form form;
    uint64_t host_bytes;  // pinned staging the call needs: none when every input is pinned already
    // the sub-batches may share one set of comb tables: sub-batch 0 builds the tables of its comb keys that
    // the node-side key cache does not hold, the later ones read the cache's for cached keys and the shared
    // store's for the rest. Without it every sub-batch rebuilds every signer's table: 9.53 against 9.19 ms
    // per 1M-request arena call, 12.5 against 10.0 at 131,072 per sub-batch (the host-fed path).
    // The caller still has to get the store (ensure_xtab).
    bool may_share;
    uint64_t inject_at;  // the piece before whose kernels an injected staging failure fires
};
inline CallPlan plan_call(std::vector<uint64_t> bnd, bool pin_sm, bool pin_pk, bool pin_off, int path,
                          uint64_t total_bytes) {
    CallPlan p;
    p.np = bnd.size() - 1;
    p.bnd = std::move(bnd);
    p.pin_sm = pin_sm;
    p.pin_pk = pin_pk;
    p.pin_off = pin_off;
    p.all_pin = pin_sm && pin_pk && pin_off;
    p.form = p.np == 1 && !(pin_sm || pin_pk || pin_off) ? ONE_DMA : PIPELINED;
    p.host_bytes = p.all_pin ? 0 : total_bytes;
    p.may_share = p.np > 1 && (path == PV_PATH_AUTO || path == PV_PATH_COMB);
    p.inject_at = std::min<uint64_t>(1, p.np - 1);  // sub-batch 0's kernels in flight, where there are two
    return p;
}

// Few distinct keys among pk[0..n): at most PV_ALLCOMB_KEYS, and >= 3 requests per key on average. Counted
// by open addressing on the keys' first 16 bytes (a heuristic: a rare collision only miscounts, the
// verdicts do not depend on the path), ~10 us for 4,096 keys. n <= 8,192: the table is never full.
inline bool few_distinct_keys(const uint8_t* pk, uint64_t n) {
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

// The zero-copy form's slots (pv_internal.h: word 0 the record's length, the key from word PV_ZC_PK_WORD,
// the record from word PV_ZC_REC_WORD, zeros to the end of the slot, at least PV_ZC_SLACK of them). The
// stride for a longest record of maxlen bytes; the call takes the form only if it is <= PV_ZC_MAX_STRIDE.
inline uint64_t zc_stride(uint64_t maxlen) { return (4ull * PV_ZC_REC_WORD + maxlen + PV_ZC_SLACK + 63) & ~63ull; }
// Slots [a, b) of the call written at slots + i * stride.
inline void zc_fill_slots(uint8_t* slots, uint64_t stride, const uint8_t* sm, const uint64_t* sm_off,
                          const uint8_t* pk, uint64_t a, uint64_t b) {
    for (uint64_t i = a; i < b; i++) {
        uint8_t* sl = slots + i * stride;
        const uint64_t len = sm_off[i + 1] - sm_off[i];
        const uint32_t hdr[PV_ZC_PK_WORD] = {(uint32_t)len, 0u, 0u, 0u};
        memcpy(sl, hdr, sizeof(hdr));
        memcpy(sl + 4 * PV_ZC_PK_WORD, pk + 32 * i, 32);
        memcpy(sl + 4 * PV_ZC_REC_WORD, sm + sm_off[i], len);
        memset(sl + 4 * PV_ZC_REC_WORD + len, 0, stride - 4 * PV_ZC_REC_WORD - len);
    }
}

}  // namespace pvhost
#pragma GCC visibility pop
