// Key stage of the throughput path: the dedup of a chunk's keys (seed, insert, assign), the key-cache and
// directory probe, the scan that splits the keys between the paths and hands out table slots, the scatter to
// slot order, the publish kernels and the unpermute of the verdicts. launch_key_stage enqueues the dedup, probe,
// scan and scatter, launch_epilogue the unpermute and publish kernels (pv_engine.hip). pv_engine.hip alone
// includes this header: its non-template __global__ functions have external linkage, so a second includer
// would define them twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk_plan.h"
#include "keycache.h"
#include "kern_access.h"
#include "pv_engine_dev.h"
#include "verify_core.h"

// requests per key, on average, up to which an all-comb chunk fills sparsely (chunk_plan.h PV_SPARSE_CHUNK has the A/B)
#ifndef PV_SPARSE_PER_KEY
#define PV_SPARSE_PER_KEY 16
#endif
// Per-key request counters of the dedup are split PV_RANK_SUB ways (sub-table = the request's
// workgroup index mod PV_RANK_SUB), so the ~1,000 requests of a hot key queue on PV_RANK_SUB
// device-scope atomics instead of one; the assign kernel turns the sub-counts into offsets.
#ifndef PV_RANK_SUB
#define PV_RANK_SUB 8
#endif
static_assert((PV_RANK_SUB & (PV_RANK_SUB - 1)) == 0, "PV_RANK_SUB must be a power of two");

// ------------------------------------------------------------------ keyed comb path (comb.h)

__device__ __forceinline__ uint32_t pv_key_hash(const uint32_t A[8], uint32_t seed) {
    uint32_t h = seed;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        h = (h ^ A[q]) * 0x9E3779B1u;
        h ^= h >> 15;
    }
    return h;
}

// The insert kernel's workgroup (chunk_plan.h PV_INS_*) counts its requests' keys in an LDS table:
static constexpr uint32_t PV_INS_LT = 4096;  // LDS table entries (more distinct keys: direct atomics)
__device__ __forceinline__ uint32_t pv_rank_sub(uint32_t i) {
    return (i / PV_INS_REQS) & (PV_RANK_SUB - 1u);
}

// The key's slot of request i (open addressing; the key is inserted if new).
__device__ __forceinline__ uint32_t pv_key_slot(const uint8_t* __restrict__ pk, const KeyWork& kw, uint32_t i) {
    uint32_t A[8];
    pv_load_pk(A, pk, i);
    uint32_t h = pv_key_hash(A, kw.seed) & kw.hmask;
    for (uint32_t probe = 0; probe <= kw.hmask; probe++) {  // the table is >= 2x the chunk: never full
        // a plain (L2-cached) read first: once a key is in, its other requests find it without an
        // atomic (the atomics of one key's requests all queue on one slot). A stale PV_EMPTY only sends
        // the request to the CAS, which returns the slot's current value; a slot never changes once
        // set within the kernel
        uint32_t cur = kw.slot[h];
        if (cur == PV_EMPTY) cur = atomicCAS(&kw.slot[h], PV_EMPTY, i);
        if (cur == PV_EMPTY) break;
        uint32_t B[8];
        pv_load_pk(B, pk, cur);
        if (pv_words_equal(A, B)) break;
        h = (h + 1) & kw.hmask;
    }
    return h;
}

// Dedup 1/2: every request's key slot as above (req_key[i]), then its rank among the key's requests
// = the workgroup's base for the key (one device atomic per distinct key of the workgroup) + its rank
// inside the workgroup (an LDS atomic).
__global__ __launch_bounds__(PV_INS_THREADS) void pv_key_insert_lds_kernel(const uint8_t* __restrict__ pk, uint64_t n,
                                                                          KeyWork kw) {
    __shared__ uint32_t lkey[PV_INS_LT], lcnt[PV_INS_LT];
    const uint32_t t = threadIdx.x;
    const uint32_t g = blockIdx.x * PV_INS_THREADS + t;
    // the chunk's split counters start at 0 (the assign kernel, next on the stream, counts keys into
    // them); done here instead of a separate hipMemsetAsync (~11 us of dispatch + gap per chunk)
    if (g < PV_SPLIT_WORDS) kw.nkeys[g] = 0u;
    if (g < PV_NSEG) kw.nkeys[PV_SEG_BASE + g * PV_SEG_STRIDE] = 0u;
    for (uint32_t e = t; e < PV_INS_LT; e += PV_INS_THREADS) {
        lkey[e] = PV_EMPTY;
        lcnt[e] = 0u;
    }
    __syncthreads();
    const uint32_t i0 = blockIdx.x * PV_INS_REQS;
    uint32_t* cnt = kw.slot_cnt + (uint64_t)((blockIdx.x & (PV_RANK_SUB - 1u))) * (kw.hmask + 1ull);
    uint32_t es[PV_INS_PER_THREAD], lr[PV_INS_PER_THREAD];
#pragma unroll
    for (uint32_t u = 0; u < PV_INS_PER_THREAD; u++) {
        const uint32_t i = i0 + u * PV_INS_THREADS + t;
        es[u] = PV_EMPTY;
        if (i >= n) continue;
        const uint32_t h = pv_key_slot(pk, kw, i);
        kw.req_key[i] = h;
        uint32_t e = (h * 2654435761u) >> (32 - 12);  // log2(PV_INS_LT)
        for (int probe = 0; probe < 64; probe++) {
            const uint32_t cur = atomicCAS(&lkey[e], PV_EMPTY, h);
            if (cur == PV_EMPTY || cur == h) {
                es[u] = e;
                break;
            }
            e = (e + 1) & (PV_INS_LT - 1u);
        }
        if (es[u] != PV_EMPTY) lr[u] = atomicAdd(&lcnt[e], 1u);
        else lr[u] = atomicAdd(&cnt[h], 1u);  // LDS table crowded: this request counts itself
    }
    __syncthreads();
    for (uint32_t e = t; e < PV_INS_LT; e += PV_INS_THREADS) {
        const uint32_t h = lkey[e];
        if (h != PV_EMPTY) lcnt[e] = atomicAdd(&cnt[h], lcnt[e]);  // count -> the workgroup's base
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < PV_INS_PER_THREAD; u++) {
        const uint32_t i = i0 + u * PV_INS_THREADS + t;
        if (i >= n) continue;
        kw.req_rank[i] = es[u] != PV_EMPTY ? lcnt[es[u]] + lr[u] : lr[u];
    }
}

// Dedup 0/2: the first requests of the chunk claim their keys' slots before the full insert, so a
// frequent key is already in the table when its other requests arrive: the full insert then finds
// it with a plain read instead of hundreds of its requests racing a compare-and-swap on one slot.
__global__ __launch_bounds__(PV_BLOCK) void pv_key_seed_kernel(const uint8_t* __restrict__ pk, uint64_t n,
                                                                KeyWork kw) {
    const uint32_t i = blockIdx.x * PV_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t A[8];
    pv_load_pk(A, pk, i);
    uint32_t h = pv_key_hash(A, kw.seed) & kw.hmask;
    for (uint32_t probe = 0; probe <= kw.hmask; probe++) {
        uint32_t cur = __hip_atomic_load(&kw.slot[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == PV_EMPTY) cur = atomicCAS(&kw.slot[h], PV_EMPTY, i);
        if (cur == PV_EMPTY) return;
        uint32_t B[8];
        pv_load_pk(B, pk, cur);
        if (pv_words_equal(A, B)) return;
        h = (h + 1) & kw.hmask;
    }
}

// Dedup 2/2: the owner request of each occupied slot takes a key id and records its key's request
// count. One atomic per wave that owns keys, on one of PV_NSEG counters (the wave's index mod
// PV_NSEG): same-address atomics serialise (~7 ns each), and with one counter a chunk of 7k distinct
// keys spent ~50 us in them (config 3), against ~11 us at 1,024 keys. Ids are segment-major
// (s * seg_cap + rank in segment s: a segment holds at most seg_cap requests, so it never
// overflows); the scan kernel walks the segments in order.
__global__ __launch_bounds__(PV_BLOCK) void pv_key_assign_kernel(uint64_t n, KeyWork kw) {
    const uint32_t i = blockIdx.x * PV_BLOCK + threadIdx.x;
    const uint32_t s = i < n ? kw.req_key[i] : 0u;
    const bool own = i < n && kw.slot[s] == i;
    const uint64_t owners = __ballot(own);
    if (owners == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = (i >> 6) & (PV_NSEG - 1u);
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)owners) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&kw.nkeys[PV_SEG_BASE + seg * PV_SEG_STRIDE], (uint32_t)__popcll(owners));
    base = __shfl(base, (int)leader);
    if (!own) return;
    const uint32_t id = seg * kw.seg_cap + base + (uint32_t)__popcll(owners & ((1ull << lane) - 1ull));
    kw.slot_id[s] = id;
    kw.key_owner[id] = i;
    // sub-counts -> offsets (zero counts stay zero: no request reads them); all loads before the stores
    uint32_t v[PV_RANK_SUB];
    const uint64_t H = kw.hmask + 1ull;
#pragma unroll
    for (int u = 0; u < PV_RANK_SUB; u++) v[u] = kw.slot_cnt[u * H + s];
    uint32_t total = 0;
#pragma unroll
    for (int u = 0; u < PV_RANK_SUB; u++) {
        if (v[u]) kw.slot_cnt[u * H + s] = total;
        total += v[u];
    }
    kw.key_count[id] = total;
}

// Dedup 2b (only when the node-side key cache holds keys): every distinct key id looks its key up
// in the cache (keycache.h); key_cslot[id] = its cache slot or PV_EMPTY. xt (hmask != 0 only for a
// later sub-batch of a pipelined host call): a key the cache misses is looked up in the call's shared
// table store next, a hit there giving its slot | PV_CSLOT_XT. dir (hmask != 0 while table reuse is
// on): a key both miss is looked up in the resident-table directory last, a hit there giving its
// ctab slot | PV_CSLOT_DIR; such a hit says where the table is and nothing about the key's path.
__global__ __launch_bounds__(PV_BLOCK) void pv_key_cache_probe_kernel(const uint8_t* __restrict__ pk, KeyWork kw,
                                                                       PvKeyCacheView kc, PvKeyCacheView xt,
                                                                       PvKeyCacheView dir) {
    const uint32_t id = blockIdx.x * PV_BLOCK + threadIdx.x;  // grid: PV_NSEG * seg_cap ids
    const uint32_t seg = id / kw.seg_cap;
    if (seg >= PV_NSEG || id - seg * kw.seg_cap >= kw.nkeys[PV_SEG_BASE + seg * PV_SEG_STRIDE]) return;
    uint32_t A[8];
    pv_load_pk(A, pk, kw.key_owner[id]);
    uint32_t s = pv_kc_lookup(kc, A);
    if (s == PV_KC_EMPTY && xt.hmask) {
        const uint32_t x = pv_kc_lookup(xt, A);
        if (x != PV_KC_EMPTY) s = x | PV_CSLOT_XT;
    }
    if (s == PV_KC_EMPTY && dir.hmask) {
        const uint32_t x = pv_kc_lookup(dir, A);
        if (x != PV_KC_EMPTY) s = x | PV_CSLOT_DIR;
    }
    kw.key_cslot[id] = s;
}

// Lists the tables a dense chunk built (comb keys without a cslot: the allocator gave each a ctab slot
// above the directory's count) in the resident-table directory: key bytes and libsodium flag, then the
// slot into the hash; the count moves up to what the scan computed. Runs on the main stream after the
// chunk's comb kernel, so the tables are whole. A slot at or above the capacity stays unlisted.
__global__ __launch_bounds__(PV_BLOCK) void pv_dir_publish_kernel(const uint8_t* __restrict__ pk, KeyWork kw) {
    const uint32_t j = blockIdx.x * PV_BLOCK + threadIdx.x;
    if (kw.nkeys[PV_SPLIT_LAT]) return;
    if (j == 0) kw.dir_cnt[0] = kw.dir_cnt[1];
    if (j >= kw.nkeys[PV_SPLIT_COMB_KEYS] || kw.comb_cslot[j] != PV_EMPTY) return;
    const uint32_t s = kw.comb_tslot[j];
    if (s >= kw.dir_cap) return;
    uint32_t A[8];
    pv_load_pk(A, pk, kw.key_owner[kw.comb_key[j]]);
#pragma unroll
    for (int q = 0; q < 8; q++) kw.dir_keys[8 * s + q] = A[q];
    kw.dir_flags[s] = kw.key_flag[j] & PV_KF_OK;  // a table this chunk built: cached form, PV_KF_AFF and PV_KF_HIT clear
    __threadfence();  // the key bytes before the hash entry that names them
    constexpr uint32_t hmask = PV_DIR_HASH - 1;
    uint32_t h = pv_kc_hash(A, kw.seed) & hmask;
    for (uint32_t probe = 0; probe <= hmask; probe++) {  // distinct keys, PV_DIR_HASH >= 2 x entries
        if (atomicCAS(&kw.dir_htab[h], PV_KC_EMPTY, s) == PV_KC_EMPTY) return;
        h = (h + 1) & hmask;
    }
}

// Tables shared by the sub-batches of one pipelined host call (stage_and_launch): sub-batch 0 builds
// its comb keys' tables straight into the call's table store (kw.ctab points there), then this kernel
// publishes them as a key-cache view -- comb index j = slot j: its key's bytes and libsodium flag, and j
// inserted into the view's open-addressing hash table (cleared before the call) -- so the later
// sub-batches find those keys with the cache probe and read the tables instead of rebuilding them.
__global__ __launch_bounds__(PV_BLOCK) void pv_xtab_publish_kernel(const uint8_t* __restrict__ pk, KeyWork kw,
                                                                    uint32_t* __restrict__ htab, uint32_t hmask,
                                                                    uint32_t seed, uint32_t* __restrict__ keys,
                                                                    uint32_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * PV_BLOCK + threadIdx.x;
    if (j >= kw.nkeys[PV_SPLIT_COMB_KEYS] || kw.comb_cslot[j] != PV_EMPTY) return;
    uint32_t A[8];
    pv_load_pk(A, pk, kw.key_owner[kw.comb_key[j]]);
#pragma unroll
    for (int q = 0; q < 8; q++) keys[8 * j + q] = A[q];
    flags[j] = kw.key_flag[j] & PV_KF_OK;
    __threadfence();  // the key bytes before the hash entry that names them
    uint32_t h = pv_kc_hash(A, seed) & hmask;
    for (uint32_t probe = 0; probe <= hmask; probe++) {  // distinct keys, hmask + 1 >= 2 x entries
        if (atomicCAS(&htab[h], PV_KC_EMPTY, j) == PV_KC_EMPTY) return;
        h = (h + 1) & hmask;
    }
}

// Exclusive prefix sum of one value per thread over a 1024-thread workgroup; *total = the sum.
static constexpr uint32_t PV_SCAN_THREADS = 1024;  // pv_key_scan_kernel's block
// Wave scans by shuffles, then the 16 wave totals (two barriers instead of Hillis-Steele's twenty).
// Written for 64-lane waves and exactly 16 of them (the 1,024-thread pv_key_scan_kernel).
#if defined(__AMDGCN_WAVEFRONT_SIZE) && __AMDGCN_WAVEFRONT_SIZE != 64
#error "pv_block_scan assumes wave64 (gfx950)"
#endif
__device__ uint32_t pv_block_scan(uint32_t v, uint32_t* part, uint32_t* total) {
    static_assert(PV_SCAN_THREADS == 16 * 64, "16 wave64 totals");
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint32_t x = v;  // inclusive scan within the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads();  // every thread is done with the previous scan's results
    if (lane == 63) part[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t u = 0; u < 16; u++) {
        const uint32_t pw = part[u];
        before += u < w ? pw : 0u;
        all += pw;
    }
    *total = all;
    return before + x - v;
}

// Sort 2/3 (one workgroup): split the keys between the paths and give each key its slot range.
// Comb keys (>= min_req requests, the first kcap of them in id order) take slots [0, CS) in id
// order, every other key's requests the slots [CS, n). Threads own contiguous id ranges; three
// passes over key_count: comb index, slot totals, cursors.
static constexpr uint32_t PV_SCAN_REG = 16;  // key counts a scan thread keeps in registers
// launched with exactly PV_SCAN_THREADS threads (pv_block_scan's 16 wave totals)
__global__ __launch_bounds__(1024) void pv_key_scan_kernel(KeyWork kw, const uint32_t* __restrict__ kc_flags) {
    __shared__ uint32_t part[1024];
    // the key ids are segment-major (pv_key_assign_kernel): v-th key in segment order = id vid(v)
    uint32_t pre[PV_NSEG + 1];
    pre[0] = 0;
#pragma unroll
    for (uint32_t g = 0; g < PV_NSEG; g++) pre[g + 1] = pre[g] + kw.nkeys[PV_SEG_BASE + g * PV_SEG_STRIDE];
    const uint32_t nk = pre[PV_NSEG];
    auto vid = [&](uint32_t v) -> uint32_t {
        uint32_t id = v;
#pragma unroll
        for (uint32_t g = 1; g < PV_NSEG; g++)
            if (v >= pre[g]) id = v - pre[g] + g * kw.seg_cap;
        return id;
    };
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nk + 1023) / 1024;
    const uint32_t lo = min(t * per, nk), hi = min(lo + per, nk);
    // a key in the node-side cache costs no table build: it is a comb candidate at any count; a
    // medium chunk with few distinct keys makes every key a comb key (PV_ALLCOMB_*)
    const bool all_comb = nk <= PV_ALLCOMB_KEYS && kw.chunk_n <= PV_ALLCOMB_CHUNK;
    auto is_cand = [&](uint32_t id, uint32_t c) {
        return all_comb || c >= kw.min_req || (kw.kc_on && pv_cslot_cached(kw.key_cslot[id]));
    };
    // up to 16k keys every count is loaded once, all loads in flight together (three dependent
    // passes of L2 reads took ~18 us at 7k keys); above that the passes re-read
    const bool reg = per <= PV_SCAN_REG;
    uint32_t cr[PV_SCAN_REG];
#pragma unroll
    for (uint32_t u = 0; u < PV_SCAN_REG; u++) cr[u] = reg && lo + u < hi ? kw.key_count[vid(lo + u)] : 0u;
    auto count = [&](uint32_t v, uint32_t id) -> uint32_t {
        if (!reg) return kw.key_count[id];
        uint32_t c = 0;
#pragma unroll
        for (uint32_t u = 0; u < PV_SCAN_REG; u++) c = v - lo == u ? cr[u] : c;
        return c;
    };
    uint32_t cand = 0;
    for (uint32_t v = lo; v < hi; v++) {
        const uint32_t id = vid(v);
        cand += is_cand(id, count(v, id)) ? 1u : 0u;
    }
    uint32_t ncand;
    const uint32_t jbase = pv_block_scan(cand, part, &ncand);
    // nm / nh: this thread's comb keys with no table anywhere / with a resident one (directory hit)
    uint32_t cs = 0, ss = 0, nm = 0, nh = 0;
    for (uint32_t v = lo, j = jbase; v < hi; v++) {
        const uint32_t id = vid(v);
        const uint32_t c = count(v, id);
        if (is_cand(id, c) && j++ < kw.kcap) {
            cs += c;
            if (kw.dir_on) {
                const uint32_t cslot = kw.key_cslot[id];
                nm += cslot == PV_EMPTY ? 1u : 0u;
                nh += cslot != PV_EMPTY && (cslot & PV_CSLOT_DIR) ? 1u : 0u;
            }
        } else {
            ss += c;
        }
    }
    uint32_t ctotal, stotal;
    uint32_t cc = pv_block_scan(cs, part, &ctotal);
    uint32_t sc = ctotal + pv_block_scan(ss, part, &stotal);
    const bool lat = kw.lat_choice && !(nk <= PV_ALLCOMB_KEYS && 3u * nk <= kw.chunk_n);
    // Slot allocator of the resident-table directory: miss number r builds into ctab slot count + r,
    // above every listed slot. When the misses do not fit (a dense chunk: below the capacity, its
    // tables get listed; any other: in the buffer, they are scratch) the chunk resets the directory:
    // every comb key without a cached table is a miss and they take slots 0, 1, ...
    uint32_t tnext = 0;  // this thread's next slot
    bool dir_reset = false;
    uint32_t wbase = 0;  // wide pool: the first free slot; this chunk's q-th queued table takes slot wbase + q
    if (kw.dir_on) {
        wbase = kw.wide_cnt[1];  // pool slots in use: read by every thread before the scans' barriers, written after
        if (t == 0) kw.aff_cnt[0] = kw.wide_cnt[0] = 0;  // the queues below fill after the scans' barriers
        const uint32_t have = kw.dir_cnt[0];  // read by every thread before the scans' barriers, written after
        uint32_t M, D;
        const uint32_t mb = pv_block_scan(nm, part, &M);
        const uint32_t hb = pv_block_scan(nh, part, &D);
        dir_reset = !lat && have + M > (kw.dir_pub ? kw.dir_cap : kw.kcap);
        tnext = dir_reset ? mb + hb : have + mb;
        if (dir_reset)
            for (uint32_t h = t; h < PV_DIR_HASH; h += PV_SCAN_THREADS) kw.dir_htab[h] = PV_KC_EMPTY;
        if (t == 0) {
            const uint32_t built = dir_reset ? M + D : M;
            const uint32_t base = dir_reset ? 0u : have;
            kw.dir_cnt[0] = base;
            if (dir_reset) kw.wide_cnt[1] = 0;  // the wide pool empties with the directory (a reset chunk hits nothing)
            kw.dir_cnt[1] = kw.dir_pub && !lat ? min(base + built, kw.dir_cap) : base;
            if (!lat) {
                kw.dir_stat[0] += dir_reset ? 0u : D;
                kw.dir_stat[1] += built;
            }
            kw.dir_stat[2] += dir_reset ? 1u : 0u;
        }
    }
    // tables this chunk may queue for widening: the queue's length and what the pool has left
    const uint32_t wroom = dir_reset || kw.wide_cap <= wbase ? 0u : min(PV_WIDE_CAP, kw.wide_cap - wbase);
    uint32_t na = 0, nw = 0;  // this thread's directory hits whose rows are affine / that are read wide
    for (uint32_t v = lo, j = jbase; v < hi; v++) {
        const uint32_t id = vid(v);
        const uint32_t c = count(v, id);
        const bool cand_id = is_cand(id, c);
        if (cand_id && j < kw.kcap) {
            uint32_t cslot = kw.kc_on ? kw.key_cslot[id] : PV_EMPTY;
            uint32_t tslot = j;  // no directory: comb index j builds into ctab[j]
            if (kw.dir_on) {
                const bool hit = cslot != PV_EMPTY && (cslot & PV_CSLOT_DIR);
                if (hit && dir_reset) cslot = PV_EMPTY;  // rebuilt below the reset count
                if (cslot == PV_EMPTY) tslot = tnext++;
                else if (hit) tslot = cslot & ~PV_CSLOT_DIR;
            }
            kw.key_cid[id] = j;
            kw.comb_key[j] = id;
            kw.comb_cslot[j] = cslot;
            kw.comb_tslot[j] = tslot;
            uint32_t wslot = PV_EMPTY;  // the pool slot of a resident table read from its wide rows
            // a cached or resident key's libsodium checks ran when its table was built (the chain skips it)
            if (cslot != PV_EMPTY) {
                const uint32_t f = (cslot & PV_CSLOT_DIR)  ? kw.dir_flags[tslot]
                                   : (cslot & PV_CSLOT_XT) ? kw.xt_flags[cslot & ~PV_CSLOT_XT]
                                                           : kc_flags[cslot];
                kw.key_flag[j] = f;  // a directory hit: every bit, the comb kernels read PV_KF_AFF rows as affine
                if ((cslot & PV_CSLOT_DIR) && !lat) {
                    na += f & PV_KF_AFF ? 1u : 0u;
                    // a dense chunk's hit on a checked key's cached-form table: the first is remembered in the
                    // slot (this thread alone handles the key), the second queues it: converted behind the
                    // chunk's comb kernels
                    if (kw.aff_conv && (f & (PV_KF_OK | PV_KF_AFF)) == PV_KF_OK) {
                        if (!(f & PV_KF_HIT)) {
                            kw.dir_flags[tslot] = f | PV_KF_HIT;
                        } else {
                            const uint32_t q = atomicAdd(&kw.aff_cnt[0], 1u);
                            if (q < PV_AFF_CAP) kw.aff_list[q] = tslot;
                        }
                    }
                }
                if ((cslot & PV_CSLOT_DIR) && kw.wide_cap) {
                    if (f & PV_KF_WIDE) {
                        wslot = kw.dir_wslot[tslot];
                        if (!lat) nw++;
                    } else if (kw.wide_conv && !lat && (f & (PV_KF_OK | PV_KF_AFF)) == (PV_KF_OK | PV_KF_AFF)) {
                        // a dense chunk's hit on affine rows -- the table's third dense hit: queued while the
                        // queue and the pool have room (thread 0 settles both counts below); the chunk itself
                        // reads the affine rows, pv_dir_widen_kernel builds the wide ones behind it
                        const uint32_t q = atomicAdd(&kw.wide_cnt[0], 1u);
                        if (q < wroom) {
                            kw.wide_list[2 * q] = tslot;
                            kw.wide_list[2 * q + 1] = wbase + q;
                        }
                    }
                }
            }
            kw.comb_wslot[j] = wslot;
            kw.key_cursor[id] = cc;
            cc += c;
        } else {
            kw.key_cid[id] = PV_EMPTY;
            kw.key_cursor[id] = sc;
            sc += c;
        }
        if (cand_id) j++;
    }
    if (na) atomicAdd(&kw.dir_stat[4], (unsigned long long)na);
    if (nw) atomicAdd(&kw.dir_stat[6], (unsigned long long)nw);
    if (kw.wide_conv) {  // uniform: the queue is complete once every thread is here
        __syncthreads();
        if (t == 0 && !dir_reset) {
            const uint32_t queued = min(atomicAdd(&kw.wide_cnt[0], 0u), wroom);
            kw.wide_cnt[0] = queued;  // what pv_dir_widen_kernel builds: entries [0, queued) are all filled
            kw.wide_cnt[1] = wbase + queued;
        }
    }
    if (t == 0) {
        kw.nkeys[PV_SPLIT_KEYS] = nk;  // distinct keys (pv_last_path)
        // AUTO's device-side choice for a 2,049..4,096-request batch of pv_verify_batch_device: the
        // rule pv_keyed_hint applies on the host (>= 3 requests per key, every key a comb key) now
        // that the dedup has counted the keys; otherwise the latency kernel runs after this chunk
        kw.nkeys[PV_SPLIT_LAT] = lat ? 1u : 0u;
        kw.nkeys[PV_SPLIT_COMB_KEYS] = min(ncand, kw.kcap);
        kw.nkeys[PV_SPLIT_SLOTS] = ctotal;
        kw.nkeys[PV_SPLIT_SPARSE] =
            !kw.dense_only && all_comb && kw.chunk_n <= PV_SPARSE_CHUNK && kw.chunk_n <= PV_SPARSE_PER_KEY * nk ? 1u : 0u;
    }
}

// Sort 3/3: each request takes its key's first slot + its rank among the key's requests.
__global__ __launch_bounds__(PV_BLOCK) void pv_key_scatter_kernel(uint64_t n, KeyWork kw) {
    const uint32_t i = blockIdx.x * PV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = kw.req_key[i];
    const uint32_t id = kw.slot_id[h];
    const uint32_t sub_off = kw.slot_cnt[pv_rank_sub(i) * (kw.hmask + 1ull) + h];
    const uint32_t pos = kw.key_cursor[id] + sub_off + kw.req_rank[i];
    kw.slot_req[pos] = i;
    kw.req_pos[i] = pos;
    kw.skey[pos] = kw.key_cid[id];
}

// Slot verdict bits back to request order: one ballot per 64 requests.
__global__ __launch_bounds__(PV_BLOCK) void pv_unpermute_kernel(uint64_t n, KeyWork kw, uint64_t* __restrict__ verdict,
                                                                 Gate gate) {
    if (!gate.keyed()) return;
    const bool lat = gate.off();  // handed to the latency path: zero words for its OR, clean up
    const uint32_t r = blockIdx.x * PV_BLOCK + threadIdx.x;
    bool ok = false;
    if (r < n) {
        const uint32_t s = kw.req_pos[r];
        ok = !lat && ((kw.sverdict[s >> 6] >> (s & 63)) & 1);
        // leave the key hash table empty for the next keyed chunk (instead of a 16 MB memset there):
        // every occupied slot is some request's slot
        const uint32_t h = kw.req_key[r];
        kw.slot[h] = PV_EMPTY;
        kw.slot_cnt[pv_rank_sub(r) * (kw.hmask + 1ull) + h] = 0u;
    }
    const uint64_t bits = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && r < n) verdict[r >> 6] = bits;
}
