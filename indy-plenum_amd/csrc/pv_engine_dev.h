// Device-visible types of the verification engine that more than one translation unit names, and the
// constants they use: pv_engine.hip (the verification kernels' unit, the device context's launches),
// pv_sign.hip (the signing kernels) and pv_ctx.h (Ctx holds a Work and a KeyWork). What only the
// verification kernels use is in the kern_*.h headers that pv_engine.hip alone includes: Soa and DevDigits
// in kern_access.h, DevATab in kern_straus.h, the staged comb loops' accessors in kern_comb.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "chunk_plan.h"  // PV_BLOCK, PV_KEY_CAP and the thresholds the launch rules read
#include "comb.h"
#include "lp25519.h"

// Dynamic LDS requested by every pv_comb_prep_req_kernel workgroup, unused: it caps the kernel's residency
// so that the key chain, launched beside it on the key stream, finds a wave slot on every SIMD at
// once instead of waiting for prep workgroups to retire (env PV_PREP_LDS_PAD overrides at pv_init).
// 41,984 B: 3 workgroups per CU (126 KB of the 160 KB), 3 prep waves per SIMD leave the chain's wave a
// slot from the start -- A/B (profiles/r04/ab_pad.txt): chain 0.40 -> 0.31 ms in-step, comb kernel
// starts 0.83 -> 0.79 ms, step -2 %; 54 KB (2 per CU) slows the prep more than it helps
#ifndef PV_PREP_LDS_PAD
#define PV_PREP_LDS_PAD 41984
#endif
static constexpr uint64_t PV_CHUNK = 1ull << 20;  // requests per launch sequence (workspace ~1.8 GB)
static constexpr uint32_t PV_ALLCOMB_CHUNK = 262144;  // the all-comb rule of chunk_plan.h PV_ALLCOMB_KEYS: chunks up to this size
static constexpr uint32_t PV_XT_HASH = 4096;      // their hash table (>= 2 x keys)
static constexpr uint32_t PV_DIR_HASH = 2 * PV_KEY_CAP;  // hash words of the resident-table directory (KeyWork::dir_*)
// Slots the directory lists by default: the rest of ctab is scratch for the tables of a chunk that lists
// nothing (at most PV_SPARSE_CHUNK requests). Such a chunk has at most PV_ALLCOMB_KEYS comb keys under
// AUTO (all-comb, or PV_SPARSE_CHUNK / PV_COMB_MIN_REQ of them, or keys whose tables exist already). Only
// forced PV_PATH_COMB (every key a comb key) can bring more misses than fit, and then resets the directory.
static constexpr uint32_t PV_DIR_DEFAULT_CAP = PV_KEY_CAP - PV_ALLCOMB_KEYS;
// Radix of the wide fixed-base comb chosen at pv_init: PV_BC2_W (24: 10.7 GB of HBM) or, when that
// allocation fails (or PV_FORCE_BCOMB16 is set), W = 16 over the radix-65536 comb T_B the latency
// path already holds (the same layout and digits: comb.h). Kernels that recode or read S's digits
// are instantiated for both.
template <int W>
struct Bc2 {
    static constexpr int POS = (253 + W - 1) / W;
    static constexpr uint32_t ENT = (1u << (W - 1)) + 1u;
};
static_assert(Bc2<16>::ENT == PV_BCOMB_ENT && Bc2<16>::POS == PV_BCOMB_POS, "W = 16 is the radix-65536 comb");

// Request bytes at an arbitrary byte offset: aligned dword loads + v_alignbyte_b32 funnel shifts.
struct DevMsg {
    const uint32_t* ap;  // rec rounded down to 4 bytes
    uint32_t sh;         // rec & 3
    __device__ __forceinline__ uint32_t dw(uint64_t i) const {
        return __builtin_amdgcn_alignbyte(ap[i + 1], ap[i], sh);
    }
    // little-endian bytes [8q, 8q + 8) of the record
    __device__ __forceinline__ uint64_t operator()(uint64_t q) const {
        return ((uint64_t)dw(2 * q + 1) << 32) | dw(2 * q);
    }
};

// Per-request intermediate state between the kernels (SoA, coalesced per wave):
//   atab  [n / 64][18][64][10] uint4        Straus path: cached [j](+-A) and [j](-R'), j = 0..8 (DevATab)
//   digits[PV_DIGIT_ROWS][n] uint32          see DevDigits
//   flags [n] uint32                        1 = every libsodium pre-check passed
//   q     [40][n] uint32                    projective Q = (X, Y, Z) from the msm kernel (rows 0..29);
//                                           the comb path's [S]B half parks an extended point here
struct Work {
    uint4* atab;
    uint32_t* digits;
    uint32_t* flags;
    uint32_t* q;
    uint4* qb;        // not read by any kernel (kept: dropping it moves the kernel-argument layout)
    uint64_t stride;  // chunk capacity (requests)
    uint4* aos;       // per REQUEST comb-prep results, PrepAos<W>::Q uint4 each (pv_comb_prep_req_kernel)
};

// How a chunk's requests are split between the two arithmetic paths, decided ON THE DEVICE by the
// dedup/sort kernels (no host round trip). split == nullptr: the Straus path was forced (or the
// chunk is too small for dedup to pay) -- no key kernels ran and slot == request. Otherwise the
// requests are in key-sorted slot order, the first split[PV_SPLIT_SLOTS] slots belong to keys
// that take the comb path and the remaining slots take the Straus path (request = slot_req[slot]).
static constexpr int PV_SPLIT_KEYS = 0;        // distinct keys in the chunk
static constexpr int PV_SPLIT_COMB_KEYS = 1;   // keys given a comb table
static constexpr int PV_SPLIT_SLOTS = 2;       // requests (slots) of those keys
static constexpr int PV_SPLIT_SPARSE = 3;      // 1: the comb tables are filled sparsely (small chunk)
static constexpr int PV_SPLIT_LAT = 4;         // 1: the dedup chose the latency path for this chunk
static constexpr uint32_t PV_SPLIT_WORDS = 8;  // counters cleared per keyed chunk
// segment g's id counter: word PV_SEG_BASE + g * PV_SEG_STRIDE of the split buffer, one counter per
// 1 KB so that the segments' atomics land on different memory channels (same-line counters
// serialise like one)
#ifndef PV_SEG_STRIDE
#define PV_SEG_STRIDE 256
#endif
static constexpr uint32_t PV_SEG_BASE = 256;
static constexpr uint32_t PV_SPLIT_ALLOC_WORDS = PV_SEG_BASE + PV_NSEG * PV_SEG_STRIDE;
struct Gate {
    const uint32_t* split;
    const uint32_t* slot_req;
    __device__ __forceinline__ bool keyed() const { return split != nullptr; }
    // the dedup handed this chunk to the latency path (pv_key_scan_kernel, lat_choice): every
    // kernel of the throughput paths exits at once, the unpermute kernel only cleans up
    __device__ __forceinline__ bool off() const { return split != nullptr && split[PV_SPLIT_LAT] != 0u; }
    // Straus-path kernels loop over 256-slot tiles t = blockIdx.x, blockIdx.x + gridDim.x, ...;
    // split, the tiles are taken from the END of the slot range (where the Straus slots are) and a
    // small grid strides over them, so the first tile with no Straus slot ends the loop and no
    // flood of empty workgroups competes with the comb kernels for CUs.
    __device__ __forceinline__ uint32_t stile(uint32_t t, uint32_t ntiles) const { return split ? ntiles - 1 - t : t; }
    __device__ __forceinline__ uint32_t ncomb() const { return split ? split[PV_SPLIT_SLOTS] : 0u; }
    // request of a Straus-path slot
    __device__ __forceinline__ uint32_t req(uint32_t i) const { return split ? slot_req[i] : i; }
};

// Keyed workspace (comb.h). The hash table maps a 32-byte key to the index of the first request
// that carried it; slot_id gives the dense key id of an owned slot (ids < chunk size).
//   slot     [H] u32   owner request index, PV_EMPTY = free
//   slot_id  [H] u32   dense key id of an owned slot
//   slot_cnt [PV_RANK_SUB][H]  requests carrying the key per sub-table (request workgroup mod
//            PV_RANK_SUB); the assign kernel replaces each nonzero count by its offset in the key
//   req_key  [stride]  the request's hash slot;         req_rank [stride] its rank in its sub-table
//   nkeys    [3]       PV_SPLIT_* counters (see Gate)
//   key_owner[stride]  a request carrying key id
//   key_cid  [stride]  comb index of key id (PV_EMPTY: its requests take the Straus path)
//   comb_key [kcap]    key id of comb index j;  key_flag [kcap]  libsodium key checks passed
//   bases    [kcap][32][4][10] uint4 [256^i](-A) and its [16], [32], [64] multiples, extended
//   ctab     [kcap][32][129][10] uint4  T_A, cached form
//   key_cslot [stride] / comb_cslot [kcap]  node-side key cache slot of a key id / comb index: a key
//            in the cache is a comb key whatever its request count, its T_A is the cache's table
//            and the key stream (chain, fill) skips it
//   comb_tslot [kcap]  slot of kw.ctab that holds (or will hold) the table of comb index j when it is
//            not read from a cache: the allocator in pv_key_scan_kernel hands them out
// Resident-table directory: the tables a dense chunk builds stay in ctab and are listed here, so a
// later chunk that carries the same key reads its table instead of building it again. Nothing of it
// lives on the host but an on/off flag, the capacity and a dirty bit.
//   dir_htab [PV_DIR_HASH] open-addressing hash of listed slots (pv_kc_lookup with kw.seed: a hit
//            compares the full 32-byte key), dir_keys [kcap][8], dir_flags [kcap]: bit 0 (PV_KF_OK) the
//            libsodium key checks passed, bit 1 (PV_KF_AFF) the slot's rows are affine, bit 2 (PV_KF_HIT)
//            a dense chunk has read the slot once already (both below), bit 3 (PV_KF_WIDE) the slot has
//            radix-2^11 rows in the wide pool (further below)
//   dir_cnt  [2]  count: slots [0, count) are listed, nothing above them is; and the count the
//            chunk's publish kernel stores once its tables are built and listed
//   dir_stat [PV_DIR_STATS]  u64 hits, built, resets, tables converted to affine rows, tables read in affine
//            form (wide reads included: they are affine rows of the same table), tables widened, tables read wide
// Affine rows: a dense chunk (dir_pub) that hits a listed table whose key passed the checks marks the
// slot PV_KF_HIT; the next dense chunk that hits it -- the table's second hit: converting 1,024 tables
// costs as much as ten warm 1M-request chunks save, so a table that comes back once is left alone --
// queues the slot in aff_list; pv_dir_affine_kernel converts those tables in place behind the chunk's comb kernels
// (comb.h pv_comb_row_to_affine_inplace) and sets PV_KF_AFF, and every later chunk reads them in affine
// form. The scan copies dir_flags into key_flag for a hit; key_flag of a key the chunk
// builds comes from the chain kernel and has bit 0 only. PV_KF_AFF and PV_KF_HIT are cleared wherever a
// slot is rebuilt, because a rebuilt slot is listed again only by pv_dir_publish_kernel, which stores bit 0
// alone: after a reset by the scan, after dir_dirty emptied the directory (a control call, an enqueue
// failure, a key-cache put that ran over the directory), and for the tables built above the count.
//   aff_list [PV_AFF_CAP] slots queued by this chunk's scan;  aff_cnt [1] how many it queued (may exceed
//            the cap: the rest wait for their next hit);  aff_scr  the conversion's parked Z2 products
// Wide rows: a dense chunk that hits a listed table with PV_KF_OK and PV_KF_AFF but not PV_KF_WIDE -- the
// table's third dense hit -- queues it in wide_list with a slot of the wide pool (wide_cnt[1], a bump
// counter reset wherever dir_cnt is), at most PV_WIDE_CAP tables per chunk and while the pool has room;
// pv_dir_widen_kernel builds the table's radix-2^11 rows (comb.h PV_KR_*) into that slot behind the chunk's
// kernels, stores dir_wslot and sets PV_KF_WIDE. Every later keyed chunk that hits the table reads [k](-A)
// from the wide rows; the radix-256 table stays where it is (the bases' source, the latency path's table).
// PV_KF_WIDE follows PV_KF_AFF's discipline: cleared by pv_dir_publish_kernel for every rebuilt slot.
//   comb_wslot [kcap] written by the scan for every comb index: the pool slot, or PV_EMPTY. The prep, digits
//            and comb kernels decide a request's form from it and never from key_flag, whose upper bits
//            are not settled before ev_tables_ready for a key the chunk builds.
// A key takes the comb path when it carries >= min_req requests of the chunk (the per-key table
// costs about as much as ~50 requests save; 1 when the comb path is forced) and fewer than kcap
// keys came before it; the rest -- singletons such as the adversarial keys of config 3 -- take the
// Straus path in the same launch.
// Key-sorted processing order ("slots"): after dedup the requests of each key occupy a contiguous
// range of slots, comb keys first, so consecutive lanes and waves read the same key's table rows
// (L2-resident) instead of 1,024 keys' tables at random:
//   key_count[stride], key_cursor[stride]  requests per key id, then the key's first slot
//   slot_req [stride]                   slot -> request index;  req_pos [stride] request -> slot
//   skey     [stride]                   slot -> comb index;     sverdict [stride / 64] slot verdicts
struct KeyWork {
    uint32_t* slot;
    uint32_t* slot_id;
    uint32_t* slot_cnt;
    uint32_t* req_key;
    uint32_t* req_rank;
    uint32_t* nkeys;
    uint32_t* key_owner;
    uint32_t* key_cid;
    uint32_t* comb_key;
    uint32_t* key_flag;
    uint4* bases;
    uint4* ctab;
    uint32_t* key_count;
    uint32_t* key_cursor;
    uint32_t* slot_req;
    uint32_t* req_pos;
    uint32_t* skey;
    uint64_t* sverdict;
    uint32_t* key_cslot;   // [stride] node-side key cache slot of key id (PV_EMPTY: not cached)
    uint32_t* comb_cslot;  // [kcap] the same per comb index: its table is read from the cache
    uint32_t* comb_tslot;  // [kcap] ctab slot of comb index j (a table this chunk builds, or a resident one)
    uint32_t* dir_htab;    // the resident-table directory (above)
    uint32_t* dir_keys;
    uint32_t* dir_flags;
    uint32_t* dir_cnt;
    unsigned long long* dir_stat;
    uint32_t* aff_list;    // affine-row conversion queue (above)
    uint32_t* aff_cnt;
    uint32_t* aff_scr;
    uint32_t* need;        // [PV_ALLCOMB_KEYS][32][5] needed |digit| bits per (comb index, position)
    const uint4* kc_tab;   // the cache's tables [cap][32][129][10] (keycache.h)
    const uint4* kc_ntab;  // the same divided by Z [cap][32][129][10] (comb.h pv_comb_row_to_affine), or null
    const uint4* kc_wtab;  // radix-65536 rows of slots < kc_wcap [kc_wcap][16][32897][8] (comb.h PV_KW_*), or null
    uint32_t kc_wcap;
    // a later sub-batch of a pipelined host call with a non-empty node cache: the keys the node cache
    // misses are looked up in the call's shared store too; a hit there is slot | PV_CSLOT_XT
    const uint32_t* xt_flags;
    const uint4* xt_tab;
    uint32_t hmask;
    uint32_t kcap;
    uint32_t seed;
    uint32_t min_req;
    uint32_t kc_on;    // this launch consults the key cache (pv_key_cache_probe_kernel ran)
    uint32_t chunk_n;  // requests in this chunk
    uint32_t lat_choice;  // the scan picks latency vs keyed for this chunk (AUTO, device-buffer call)
    uint32_t seg_cap;     // key ids of segment s are s * seg_cap + [0, its counter)
    uint32_t dense_only;  // never fill sparsely (the tables outlive the chunk: pv_xtab_publish_kernel)
    uint32_t dir_on;      // this chunk goes through the directory (probe, slot allocator)
    uint32_t dir_cap;     // slots the directory may list (<= kcap)
    uint32_t dir_pub;     // a dense chunk: its tables are whole and pv_dir_publish_kernel lists them
    uint32_t aff_conv;    // a dense chunk with pv_table_affine on: its scan queues hit tables for conversion
    // wide rows of resident tables (above); every pointer is null until the pool exists
    uint4* wide_tab;       // [wide_cap][PV_KR_POS][PV_KR_ENT][8]
    uint32_t* wide_scr;    // [PV_WIDE_GRID][PV_KR_RUN][10][PV_WIDE_THREADS] Z products of the runs in flight
    uint32_t* wide_list;   // [PV_WIDE_CAP][2] (ctab slot, pool slot) queued by this chunk's scan
    uint32_t* wide_cnt;    // [2] entries queued by this chunk; pool slots handed out (the bump counter)
    uint32_t* dir_wslot;   // [kcap] pool slot of a directory slot whose dir_flags has PV_KF_WIDE
    uint32_t* comb_wslot;  // [kcap] pool slot of comb index j, PV_EMPTY unless its table is read wide
    uint32_t wide_cap;     // pool slots (0: the feature is off for this chunk)
    uint32_t wide_conv;    // a dense chunk with the pool in place: its scan queues affine tables for widening
};
static constexpr uint32_t PV_KF_OK = 1u;   // key_flag / dir_flags: libsodium's key checks passed
static constexpr uint32_t PV_KF_AFF = 2u;  // the table's rows are affine (a directory hit only)
static constexpr uint32_t PV_KF_HIT = 4u;  // a dense chunk has hit the table before: its next dense hit converts it
static constexpr uint32_t PV_DIR_STATS = 7;
static constexpr uint32_t PV_KF_WIDE = 8u; // the table has radix-2^11 rows in the wide pool (dir_wslot)
static constexpr uint32_t PV_AFF_CAP = 1024;  // tables one chunk converts (aff_scr: 165 KB each, 173 MB)
static constexpr uint32_t PV_WIDE_CAP = 1024;       // tables one chunk widens
static constexpr uint32_t PV_WIDE_DEFAULT = 2048;   // slots of the wide pool (3.0 MB each, 6.2 GB)
static constexpr uint32_t PV_WIDE_THREADS = 384;    // pv_dir_widen_kernel: one run per thread, 23 x 16 = 368 used
static constexpr uint32_t PV_WIDE_GRID = 512;       // its workgroups, each with 0.98 MB of scratch (503 MB)
static_assert(PV_KR_POS * PV_KR_RUNS <= PV_WIDE_THREADS, "one thread per run of a table");
#ifndef PV_KC_WIDE_KEYS
#define PV_KC_WIDE_KEYS 1024  // key-cache slots that get radix-65536 rows (67 MB each)
#endif
static constexpr uint32_t PV_KW_GROUP = 64;  // keys per wide build launch of a key-cache put (scratch: 1.35 GB)
static constexpr uint32_t PV_EMPTY = 0xFFFFFFFFu;
static constexpr uint32_t PV_CSLOT_XT = 0x40000000u;  // cache slot in the call's shared store (KeyWork::xt_*)
static constexpr uint32_t PV_CSLOT_DIR = 0x20000000u;  // slot of kw.ctab listed in the resident-table directory
// a key id's / comb index's cslot names a table of the node cache or the call store (never a directory hit)
__host__ __device__ __forceinline__ bool pv_cslot_cached(uint32_t cslot) {
    return cslot != PV_EMPTY && !(cslot & PV_CSLOT_DIR);
}

// LDS-DMA staging of one table entry per lane (comb.h, the staged comb loops). An entry of Q uint4 is
// fetched by Q global_load_lds_dwordx4, each writing 1 KiB = 16 B x 64 lanes of the wave's staging
// area, laid out [q][lane] so that reading it back is one conflict-free ds_read_b128 per q.
// pv_glds16_row: Q pieces of 16 B from g[0..Q) to l[q * 64 + lane] (a wave's [q][lane] staging area). The
// instruction's immediate offset (16 q) applies to BOTH the global and the LDS address, so the LDS
// base of piece q is moved back by the same 16 q bytes (M0 is set per instruction anyway): all Q
// loads then share ONE 64-bit global address instead of Q 64-bit adds per staged entry.
template <int Q, int q = 0>
__device__ __forceinline__ void pv_glds16_row(const uint4* g, uint4* l) {
    if constexpr (q < Q) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                         (__attribute__((address_space(3))) void*)(l + q * 64 - q), 16, 16 * q, 0);
        pv_glds16_row<Q, q + 1>(g, l);
    }
}
// the LDS reads of the previous staged entry must be complete before its buffer is refilled
__device__ __forceinline__ void pv_lds_reads_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Wide fixed-base comb rows (comb.h PV_BC2_*): row j = entries 0..PV_BC2_ENT-1 of [d 2^(W j)] B,
// 8 uint4 each, LDS-staged like DevCombStage; 64-bit entry index (the table is ~10.7 GB at W = 24).
template <uint32_t ENT>
struct DevB2Stage {
    const uint4* base;
    uint4* lds;
    uint32_t lane;
    __device__ __forceinline__ void stage(int j, int d) const {
        const uint4* e = base + ((uint64_t)j * ENT + (uint32_t)d) * (PV_BCOMB_STRIDE / 4);
        pv_lds_reads_done();
        pv_glds16_row<PV_BCOMB_STRIDE / 4>(e, lds);
    }
    __device__ __forceinline__ void staged(int part, uint32_t w[20]) const {
#pragma unroll
        for (int q = 0; q < (part ? 3 : 5); q++) {
            const uint4 v = lds[(5 * part + q) * 64 + lane];
            const int lim = part ? 10 : 20;
            if (4 * q < lim) w[4 * q] = v.x;
            if (4 * q + 1 < lim) w[4 * q + 1] = v.y;
            if (4 * q + 2 < lim) w[4 * q + 2] = v.z;
            if (4 * q + 3 < lim) w[4 * q + 3] = v.w;
        }
    }
};

// The encode's one inversion per lane done by the whole wave: the 64 lanes' products are multiplied
// pairwise across lanes (xor partners 32, 16, 8, 4, 2) down to two products, one per lane residue mod 2,
// which are inverted at once in limb-parallel form (lp_invert<true>: rows 0, 1 the two products, repeated
// in rows 2, 3, and five column terms per lane, a shorter dependent chain per product), and the inverses
// walked back down the same tree (one product per level). Where every lane ran its own ~27k-instruction
// exponentiation chain (the chain's latency was most of the kernel's time), the wave now runs ~265
// limb-parallel products. Every lane of the wave must be active (pv_encode_kernel: all lanes run the batch).
__device__ __forceinline__ void pv_shfl_xor_fe(fe& o, const fe& a, int m) {
#pragma unroll
    for (int k = 0; k < 10; k++) o.v[k] = __shfl_xor(a.v[k], m);
}
struct PvWaveInvert {
    __device__ void operator()(fe& x) const {
#if LP_DEVICE
        constexpr int LV = 5;         // tree levels
        constexpr uint32_t RES = 1u;  // lane residue a row's product covers
        const uint32_t lane = threadIdx.x & 63u;
        constexpr int M[5] = {32, 16, 8, 4, 2};
        fe p[LV + 1], q;
        p[0] = x;
#pragma unroll
        for (int i = 0; i < LV; i++) {
            pv_shfl_xor_fe(q, p[i], M[i]);
            fe_mul(p[i + 1], p[i], q);
        }
        const LpLane c = LpLane::make();
        const int src = (int)((lane >> 4) & RES);
        fe inv;
        // row r (lanes 16 r + k) gets limb k of lane (r & RES)'s product
        uint32_t z = 0;
#pragma unroll
        for (int k = 0; k < 10; k++) {
            const uint32_t t = __shfl(p[LV].v[k], src);
            z = (lane & 15u) == (uint32_t)k ? t : z;
        }
        const lu zi = lp_invert<true>(c, lu(z));
#pragma unroll
        for (int k = 0; k < 10; k++) inv.v[k] = __shfl(static_cast<uint32_t>(zi), (int)(16u * (lane & RES)) + k);
#pragma unroll
        for (int i = LV - 1; i >= 0; i--) {
            pv_shfl_xor_fe(q, p[i], M[i]);
            fe_mul(inv, inv, q);
        }
        x = inv;
#else
        fe_invert(x, x);
#endif
    }
};
