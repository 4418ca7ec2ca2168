// What a launch decides on the host before it enqueues anything: the path of a batch (latency, device
// choice, or the throughput paths), and per chunk the path (keyed or Straus), the views a key is looked
// up in, the KeyWork scalars, the launch shape and grids, the follow-up kernels, and the clears the dirty
// flags force. Pure functions over structs of scalars and bools, host only and without a runtime call, so
// tests/native/chunk_plan_check.cpp runs them on a CPU; launch_chunks / launch_chunk (pv_engine.hip) gather
// the facts from the context, apply the plan to the KeyWork and enqueue what it names. The thresholds the
// rules read are defined here, each once, with what was measured for them (pv_engine_dev.h includes this
// file: the kernels, in the kern_*.h headers of pv_engine.hip, read the same constants). The #ifndef ones are tuning knobs that microbench/
// build_variants.sh varies with -D.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/plenum_verify.h"  // PV_PATH_*

static constexpr int PV_BLOCK = 256;
static constexpr uint32_t PV_KEY_CAP = 16384;     // distinct keys the comb tables hold (10.8 GB)
// AUTO: chunks above the latency path's range go keyed (dedup, then comb keys / Straus side). At
// medium sizes (4k-256k requests) the Straus side's one-lane latency (~0.9 ms) is paid by the whole
// launch as soon as it has any request, so a chunk with few distinct keys makes EVERY key a comb
// key (PV_ALLCOMB_*): tools/latency_probe.py on MI355X, 1,024 signers, device time per call --
// 10k requests 0.77 ms all-comb vs 0.91 Straus, 32k 0.76 vs 0.95 (and 1.02 split at >= 48 requests
// per key); bounded so the fill never exceeds 2,048 keys' tables (~0.5 ms).
static constexpr uint64_t PV_KEYED_MIN = 4097;
static constexpr uint32_t PV_ALLCOMB_KEYS = 2048;
static constexpr uint32_t PV_XT_KEYS = 2048;      // tables shared by a pipelined call's sub-batches (1.35 GB)
#ifndef PV_LATENCY_MAX
#define PV_LATENCY_MAX 4096  // AUTO: batches up to this size take the latency path (pv_latency.hip)
#endif
// AUTO picks latency vs keyed by key repeats from this size up to PV_LATENCY_MAX (pv_keyed_hint on
// the host, the dedup's lat_choice on the device)
#ifndef PV_KEYED_HINT_MIN
#define PV_KEYED_HINT_MIN 2049
#endif
static constexpr uint32_t PV_NSEG = 8;         // key-id segments (pv_key_assign_kernel)
// A key takes the comb path when it carries at least this many requests of the chunk (KeyWork::min_req;
// the per-key table costs about as much as ~50 requests save)
#ifndef PV_COMB_MIN_REQ
#define PV_COMB_MIN_REQ 48
#endif
// An all-comb chunk of at most PV_SPARSE_CHUNK requests and at most PV_SPARSE_PER_KEY requests per key
// on average builds only the table entries its digits use (comb.h pv_comb_fill_sparse; the need
// masks are set by pv_comb_prep_req_kernel). A/B on MI355X (1,024 signers, device time,
// profiles/r02/ab_sparse_fill.txt): 6k requests 0.71 -> 0.54 ms, 10k 0.70 -> 0.56; at 32 requests
// per key the per-position thread's serial additions outlast the parallel full fill (32k 0.69 ->
// 0.72, 64k 0.74 -> 0.89), hence the per-key bound.
#ifndef PV_SPARSE_CHUNK
#define PV_SPARSE_CHUNK 65536
#endif
// Chunks above PV_FUSED_MIN_REQ requests run [S]B and [k](-A) in one kernel (pv_comb_ab_kernel). Below
// that the two-kernel form stays: a small chunk's [S]B kernel is a latency-bound chain of 10 dependent
// HBM lookups that the split form hides beside the table fill, while the fused kernel would add it
// after the fill (4,096-32,768-request calls were 0.08-0.12 ms slower fused).
#ifndef PV_FUSED_MIN_REQ
#define PV_FUSED_MIN_REQ 262144
#endif
// Dedup contention (1,024 signers x ~1,000 requests each per 1M chunk). Kernel times on MI355X
// (rocprofv3, profiles/r02/ab_dedup_seed.txt): insert + assign 143 us with one atomic counter per
// key and an atomic first read; 95 us with the seed pre-pass; 92 with a plain first read; 85 us
// (+ 8 us seed) with the counters split 8 ways (16: 86, 32: 87 -- the assign kernel's sums grow).
#ifndef PV_KEY_SEED
#define PV_KEY_SEED 4096  // requests of a keyed chunk whose keys are inserted first (pv_key_seed_kernel)
#endif
// Workgroups per CU of the Straus side stream's kernels in a keyed chunk (ChunkPlan::side_grid)
#ifndef PV_SIDE_GRID_PER_CU
#define PV_SIDE_GRID_PER_CU 2
#endif
#ifndef PV_LP_CHAIN_BLOCKS
#define PV_LP_CHAIN_BLOCKS 2048  // waves of the limb-parallel key chain (one key each at a time)
#endif
// Requests per lane of the encode kernel: B = 16 (two groups of 8 under one inversion, verify_core.h) for
// chunks of >= PV_ENC16_MIN requests, else PV_ENC_SMALL_B = 8. With each lane's own inversion chain 16
// won at 1M requests (0.185-0.190 ms against 0.191-0.198 for 2,048 waves of 8, profiles/r05/
// ab_encode_prefetch.txt); with the wave's limb-parallel inversion 8 wins everywhere (0.145-0.148 vs
// 0.159-0.161 ms at 1M, 4 per lane 0.185-0.191: profiles/r06/ab/ab_encode_batch.txt), so 16 is off.
#ifndef PV_ENC_SMALL_B
#define PV_ENC_SMALL_B 8
#endif
#ifndef PV_ENC16_MIN
#define PV_ENC16_MIN 0xffffffffu
#endif
// The insert kernel's workgroup takes PV_INS_REQS consecutive requests, counts their keys in an LDS
// table and makes ONE device atomic per (key, workgroup) for the whole group's ranks (per-request
// atomics on the keys' counters were ~56 of the kernel's ~74 us at 1M requests). The sub-table of
// request i's per-key counter is its insert-workgroup index mod PV_RANK_SUB.
static constexpr uint32_t PV_INS_THREADS = 1024, PV_INS_PER_THREAD = 4;
static constexpr uint32_t PV_INS_REQS = PV_INS_THREADS * PV_INS_PER_THREAD;
// fill work items per key: comb.h's PV_COMB_POS * PV_COMB_BLOCKS (pv_engine.hip asserts the product)
static constexpr uint32_t PV_FILL_ITEMS_PER_KEY = 256;

#pragma GCC visibility push(hidden)  // internal to libplenum_verify.so
namespace pvhost {

// workgroups of PV_BLOCK threads, one thread per item
inline unsigned block_grid(uint64_t items) { return (unsigned)((items + PV_BLOCK - 1) / PV_BLOCK); }
// waves of the key chain for `keys` comb keys, and the workgroups of the fill that follows it (a chunk's
// key stream, and the table build of a key-cache put)
inline unsigned chain_blocks(uint32_t keys) { return std::min<uint32_t>(keys, PV_LP_CHAIN_BLOCKS); }
inline unsigned fill_grid(uint32_t keys) {
    const uint64_t items = (uint64_t)keys * PV_FILL_ITEMS_PER_KEY;
    return (unsigned)std::min<uint64_t>((items + PV_BLOCK - 1) / PV_BLOCK, 4096);
}

// ------------------------------------------------------------------------------------------ batch

struct BatchFacts {
    int path;         // PV_PATH_* as set by pv_set_path
    uint64_t n;       // requests of the whole launch
    bool hint_set;    // a host-buffer call counted the keys itself: no device-side choice
    bool keyed_hint;  // ... and found few distinct keys (pv_keyed_hint)
    bool kc_active;   // the node-side key cache holds keys and is consulted (kc_view().hmask != 0)
};
struct BatchPlan {
    bool latency;     // every chunk is one latency-path launch
    bool dev_choice;  // the keyed kernels run and their scan picks latency vs keyed on the device
};

// small batches: one wave pair per request (pv_latency.hip); forced LATENCY takes it at any size.
// Between PV_KEYED_HINT_MIN and PV_LATENCY_MAX requests AUTO picks by key repeats: the host-buffer
// call counted the keys (keyed_hint, hint_set); a device-buffer call lets the dedup kernels count
// them and decide on the device (dev_choice: the keyed kernels exit at once and the latency kernel
// runs when the scan picks latency; no host round trip). A non-empty key cache keeps the latency
// path there (cached keys make it faster still).
// The zero-copy gate of pv_verify_batch asks the same question for a host-buffer call before anything is
// staged: hint_set with the hint it has just computed.
inline BatchPlan plan_batch(const BatchFacts& f) {
    BatchPlan p;
    p.dev_choice = f.path == PV_PATH_AUTO && !f.hint_set && !f.kc_active &&
                   f.n >= PV_KEYED_HINT_MIN && f.n <= PV_LATENCY_MAX;
    p.latency = f.path == PV_PATH_LATENCY ||
                (f.path == PV_PATH_AUTO && f.n <= PV_LATENCY_MAX && !f.keyed_hint && !p.dev_choice);
    return p;
}

// ------------------------------------------------------------------------------------------ chunk

// Where the chunk's probe kernel looks a key up before the resident-table directory (which dir_on adds).
enum Lookup : uint32_t {
    LOOKUP_NONE = 0,          // nowhere: every comb key's table is built (or resident)
    LOOKUP_NODE = 1,          // the node-side key cache
    LOOKUP_NODE_THEN_XT = 2,  // the node cache first, then the call's shared store for the keys it misses
    LOOKUP_XT_ONLY = 3,       // the shared store is the only view (in the node cache's place: no affine or
                              // wide rows of the cache are read)
};

struct ChunkFacts {
    uint64_t m;        // requests of this chunk (>= 1)
    int path;          // PV_PATH_*
    bool keyed_hint;   // as in BatchFacts
    bool node_kc;      // the node-side key cache is active (kc_view().hmask != 0)
    uint32_t kc_wcap;  // its slots that have radix-65536 rows
    bool xt_use;       // a later sub-batch of a pipelined host call: the call's shared tables are looked up
    bool xt_fill;      // sub-batch 0 of one: its tables go to the shared store
    bool dir_on;       // the resident-table directory is on (pv_table_reuse)
    uint32_t dir_cap;  // slots it may list
    bool aff_on;       // pv_table_affine
    uint32_t wide_cap;   // configured capacity of the wide pool in tables (pv_table_wide; 0: off)
    uint64_t wide_have;  // tables the pool holds now (after this chunk's allocation attempt, if any)
    uint32_t kcap;     // comb keys the workspace holds
    int cus;           // compute units of the device
    bool slots_dirty;  // the key hash table / need masks may hold entries
    bool dir_dirty;    // the directory may be stale
};

struct ChunkPlan {
    bool keyed;  // dedup, comb keys and a Straus side; else every request on the Straus path (no key kernel)
    Lookup lookup;
    // KeyWork scalars (pv_engine_dev.h)
    uint32_t min_req, kc_on, kc_wcap, dir_on, dir_cap, dir_pub, aff_conv, wide_cap, wide_conv, chunk_n, seg_cap,
        lat_choice, dense_only, kcap;
    // launch shape of a keyed chunk
    bool dir_use;      // the chunk goes through the directory (KeyWork::dir_on as a bool)
    bool direct_fill;  // the fill follows the chain on the key stream; else fill and sparse fill on the fill stream
    bool fused;        // pv_comb_ab_kernel; else pv_comb_b_kernel, then pv_comb_a_kernel
    uint64_t seed_reqs;  // requests of the seed pre-pass, 0: no seed launch
    bool enc16;        // pv_encode_kernel<16>, else <PV_ENC_SMALL_B>
    unsigned req_grid, ins_grid, probe_grid, chain_blocks, fill_grid, side_grid, enc_grid, pub_grid;
    // what the dirty flags force before a keyed chunk, and the kernels that run or not
    bool clear_slots, clear_dir, mark_dir_dirty;
    bool run_probe, run_xtab_publish, run_dir_publish, run_affine, run_widen, run_dev_latency;
};

// The chunk's key-cache view is the node cache's, or the shared store's where that is the only view.
inline bool chunk_kc_active(const ChunkFacts& f) { return f.node_kc || f.xt_use; }

// Path split (measured round-1 costs on MI355X): a key's comb table costs ~0.47 us of device
// time (chain + 4,128-entry fill) and then saves ~10 ns per request against the Straus
// path (~3 vs ~13 ns), so AUTO gives a table to keys with >= PV_COMB_MIN_REQ requests in
// the chunk and verifies every other request on the Straus path in the same launch. The
// split is computed on the device by the dedup/sort kernels (Gate); nothing synchronises.
// Chunks below PV_KEYED_MIN (the latency path's range; only the tail chunk of a large
// batch can be that small) skip dedup and go Straus. A key in the node-side key cache has
// its comb table already built: its requests take the comb path at any count.
inline bool chunk_keyed(const BatchPlan& b, const ChunkFacts& f) {
    return f.path == PV_PATH_COMB ||
           (f.path == PV_PATH_AUTO && (f.m >= PV_KEYED_MIN || f.keyed_hint || b.dev_choice || chunk_kc_active(f)));
}
// Table reuse: the chunk's keys are looked up in the resident-table directory as well, and the
// scan's allocator keeps what it builds off the listed slots. It decides where a table is read
// from and nothing else: kc_active, keyed and the scan's candidate rule do not see it. Sub-batch 0
// of a pipelined host call builds into the call's store, not into ctab: it stays outside.
inline bool chunk_dir_use(const ChunkFacts& f) { return f.dir_on && !f.xt_fill; }
// a dense chunk (direct_fill): its tables are whole and pv_dir_publish_kernel lists them
inline bool chunk_dir_pub(const ChunkFacts& f) { return chunk_dir_use(f) && f.m > PV_SPARSE_CHUNK; }

// Wide rows: the pool is allocated by the first dense chunk that can widen a table -- the fourth since
// pv_init at the earliest (build, first hit, affine rows, then this) -- and not at pv_init. When the
// allocation fails the feature turns itself off (wide_failed) and says so once through the error string.
// A pool that has to grow (pv_table_wide) is replaced: that call marked the directory dirty already.
// The engine attempts the allocation between this and plan_chunk, which sees the pool as it is afterwards.
struct WideTrigger {
    bool attempt;    // allocate the pool (and its builder's scratch) now
    uint32_t dense;  // Ctx::wide_dense from here on
};
inline WideTrigger plan_wide_pool(bool keyed, bool dir_pub, bool wide_failed, uint64_t pool_bytes, uint64_t want_bytes,
                                  uint32_t dense) {
    WideTrigger t{false, dense};
    if (keyed && dir_pub && !wide_failed && pool_bytes < want_bytes) t.attempt = ++t.dense >= 4;
    return t;
}

inline ChunkPlan plan_chunk(const BatchPlan& b, const ChunkFacts& f) {
    ChunkPlan p;
    const uint64_t m = f.m;
    if (f.xt_use)  // a later sub-batch of a pipelined host call: the call's shared tables
        p.lookup = f.node_kc ? LOOKUP_NODE_THEN_XT : LOOKUP_XT_ONLY;
    else
        p.lookup = f.node_kc ? LOOKUP_NODE : LOOKUP_NONE;
    const bool kc_active = chunk_kc_active(f);
    p.keyed = chunk_keyed(b, f);
    p.min_req = f.path == PV_PATH_COMB ? 1u : (uint32_t)PV_COMB_MIN_REQ;
    p.dir_use = chunk_dir_use(f);
    p.kc_on = kc_active || p.dir_use ? 1u : 0u;
    p.kc_wcap = p.lookup == LOOKUP_XT_ONLY ? 0u : f.kc_wcap;  // the shared store has no wide rows
    p.dir_on = p.dir_use ? 1u : 0u;
    p.dir_cap = f.dir_cap;
    p.dir_pub = chunk_dir_pub(f) ? 1u : 0u;
    p.aff_conv = p.dir_pub && f.aff_on ? 1u : 0u;
    p.wide_cap = p.dir_use ? (uint32_t)std::min<uint64_t>(f.wide_cap, f.wide_have) : 0u;
    p.wide_conv = p.dir_pub && p.wide_cap ? 1u : 0u;
    p.chunk_n = (uint32_t)m;
    // a key-id segment holds the owners among its waves (every PV_NSEG-th wave of the chunk)
    p.seg_cap = (uint32_t)((((m + 63) / 64) + PV_NSEG - 1) / PV_NSEG * 64);
    p.lat_choice = b.dev_choice ? 1u : 0u;
    // sub-batch 0 of a pipelined host call: its tables go to the shared store, whole
    p.kcap = f.xt_fill ? std::min<uint32_t>(f.kcap, PV_XT_KEYS) : f.kcap;
    p.dense_only = f.xt_fill ? 1u : 0u;
    // a chunk above PV_SPARSE_CHUNK never fills sparsely: its fill follows the chain on kstream
    p.direct_fill = m > PV_SPARSE_CHUNK;
    p.fused = m > PV_FUSED_MIN_REQ;
    // small chunks: no contention worth a launch
    p.seed_reqs = PV_KEY_SEED > 0 && m > 16ull * PV_KEY_SEED ? std::min<uint64_t>(m, PV_KEY_SEED) : 0;
    p.enc16 = m >= PV_ENC16_MIN;
    p.req_grid = block_grid(m);
    p.ins_grid = (unsigned)((m + PV_INS_REQS - 1) / PV_INS_REQS);
    p.probe_grid = (PV_NSEG * p.seg_cap + PV_BLOCK - 1) / PV_BLOCK;
    // p.kcap: comb keys a chunk can hold (launch grids of the key stream)
    p.chain_blocks = chain_blocks(p.kcap);
    p.fill_grid = fill_grid(p.kcap);
    // The Straus-path slots of a split chunk run on their own stream beside the comb kernels; their blocks
    // are dispatched from the END of the slot range and blocks of comb slots exit at once, so a small grid
    // strides over them.
    p.side_grid = std::min<unsigned>(p.req_grid, std::max(1u, (unsigned)(PV_SIDE_GRID_PER_CU * std::max(1, f.cus))));
    p.enc_grid = p.enc16 ? (unsigned)((m + PV_BLOCK * 16 - 1) / (PV_BLOCK * 16))
                         : (unsigned)((m + PV_BLOCK * PV_ENC_SMALL_B - 1) / (PV_BLOCK * PV_ENC_SMALL_B));
    p.pub_grid = (p.kcap + PV_BLOCK - 1) / PV_BLOCK;
    // the hash table and need masks are left empty by the previous keyed chunk (unpermute and
    // sparse fill kernels); after an enqueue failure they may not be, and are cleared first.
    // The directory likewise: emptied when it may be stale, stale until the chunk is enqueued
    // whole. A chunk outside it builds into ctab[j], over whatever is listed.
    p.clear_slots = p.keyed && f.slots_dirty;
    p.clear_dir = p.keyed && p.dir_use && f.dir_dirty;
    p.mark_dir_dirty = p.keyed && !f.xt_fill;
    p.run_probe = p.keyed && (kc_active || p.dir_use);
    p.run_xtab_publish = p.keyed && f.xt_fill;  // this chunk's tables for the call's later sub-batches
    p.run_dir_publish = p.keyed && p.dir_pub;  // list this chunk's tables for what follows
    p.run_affine = p.keyed && p.aff_conv;      // the listed tables this chunk hit: affine rows
    p.run_widen = p.keyed && p.wide_conv;       // the affine tables this chunk hit: radix-2^11 rows
    p.run_dev_latency = p.keyed && b.dev_choice;  // runs only when the scan picked latency
    return p;
}

}  // namespace pvhost
#pragma GCC visibility pop
