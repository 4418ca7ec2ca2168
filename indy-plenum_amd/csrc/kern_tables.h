// Table stage of the throughput path: a comb key's bases (the limb-parallel chain) and its table rows (dense
// and sparse fill), the key cache's scatter and affine rows, the resident tables' conversion to affine rows.
// launch_key_stage enqueues the chain and the dense fill, launch_comb_stage the sparse fill, launch_epilogue
// pv_dir_affine_kernel and kc_build_tables the chain, the fill and the pv_kc_* kernels (pv_engine.hip).
// pv_engine.hip alone includes this header: its non-template __global__ functions have external linkage, so
// a second includer would define them twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "comb.h"
#include "kern_access.h"
#include "lp25519.h"
#include "pv_engine_dev.h"
#include "verify_core.h"

#ifndef PV_FILL_MINBLOCKS
#define PV_FILL_MINBLOCKS 2
#endif

struct DevBases {
    uint4* b;  // [32][PV_COMB_PTS][10]: per position P_i, [16] P_i, [32] P_i, [64] P_i (extended)
    __device__ __forceinline__ void store(int i, int m, const ge_p3& p) const {
        uint32_t w[40];
        ge_p3_store_words(w, p);
        uint4* e = b + (i * PV_COMB_PTS + m) * 10;
        pv_quads_store<10>([&](int q) -> uint4& { return e[q]; }, w);
    }
    __device__ __forceinline__ void load(int i, int m, ge_p3& p) const {
        const uint4* e = b + (i * PV_COMB_PTS + m) * 10;
        uint32_t w[40];
        pv_quads_load<10>(w, [&](int q) { return e[q]; });
        ge_p3_load_words(p, w);
    }
};
struct DevBasePts {  // the points of one position, for pv_comb_fill_block
    DevBases bs;
    int i;
    __device__ __forceinline__ void load(int m, ge_p3& p) const { bs.load(i, m, p); }
};

// One position's row of a key's comb table: entries d = 0..128, 10 uint4 (160 B) each.
struct DevCombRow {
    uint4* r;
    __device__ __forceinline__ void store(int d, const ge_cached& c) const {
        uint32_t w[40];
        ge_cached_store_words(w, c);
        pv_quads_store<10>([&](int q) -> uint4& { return r[d * 10 + q]; }, w);
    }
    __device__ __forceinline__ void load(int d, ge_cached& c) const {
        uint32_t w[40];
        pv_quads_load<10>(w, [&](int q) { return r[d * 10 + q]; });
        ge_cached_load_words(c, w);
    }
    __device__ __forceinline__ void load_half(int d, int h, uint32_t w[20]) const {
        pv_quads_load<5>(w, [&](int q) { return r[d * 10 + 5 * h + q]; });
    }
};

#if LP_DEVICE
// Positions [lo, hi) of one key's chain. Part 0 decompresses -A and writes the key flag; a later part
// resumes from P_lo, which the previous part stored as slot 0 of position lo.
__device__ __forceinline__ void pv_key_chain_lp(const uint8_t* __restrict__ pk, const KeyWork& kw, uint32_t id,
                                                const LpLane& c, const LpConsts& K, int lo, int hi) {
    uint32_t* b = reinterpret_cast<uint32_t*>(kw.bases + (uint64_t)id * PV_COMB_POS * PV_COMB_PTS * 10);
    const uint32_t w = 10u * (threadIdx.x >> 4) + (threadIdx.x & 15u);  // word of [X, Y, Z, T] x 10 limbs
    const bool limb = (threadIdx.x & 15u) < 10u;
    auto store = [&](int i, int m, const lu& P) {
        const lu R = lp_carry1(c, P);  // LR -> limb < 2^w + 19: the per-lane code's reduced bound
        if (limb) b[(i * PV_COMB_PTS + m) * 40 + w] = R;
    };
    lu P;
    if (lo == 0) {
        uint32_t A[8];
        pv_load_pk(A, pk, kw.key_owner[kw.comb_key[id]]);
        lu sw[8];
#pragma unroll
        for (int q = 0; q < 8; q++) sw[q] = A[q];
        const LpDecomp dec = lp_decompress_ar(c, K, sw);
        const bool ok = pv_ge_is_canonical(A) && !pv_has_small_order(A) && dec.ok_a;
        if (threadIdx.x == 0) kw.key_flag[id] = ok ? 1u : 0u;
        P = lp_ext_from_xy(c, K, dec.X, dec.Y, 0);
    } else {
        P = lp_load_ext40(c, b + lo * PV_COMB_PTS * 40);
    }
    P = lp_comb_chain_part(c, P, lo, hi, store);
    if (hi < PV_COMB_POS) store(hi, 0, P);  // P_hi: where the next part resumes
}
#endif

// Limb-parallel key chain (lp25519.h): ONE wave per key, every field element over a 16-lane row and
// the four squarings / products of a doubling in the four rows at once: the chain of 254 dependent
// doublings is the only long dependency of the comb path and runs on very few keys, so its LATENCY,
// not its work, is what the batch waits for. Blocks stride over the keys (a batch with
// more keys than blocks runs them in turn), so the launch needs no host-side key count and no gated
// companion kernel: a gated launch is not free on a saturated chip, its blocks wait ~0.2 ms for
// dispatch slots (rocprofv3, profiles/r02/prof_a). Outputs: key_flag and the bases [256^i](-A) with
// their [16], [32], [64] multiples, carried to reduced limbs. The launcher runs all 32 positions in one
// launch (lo = 0, hi = 32).
__global__ __launch_bounds__(64) void pv_key_chain_lp_kernel(const uint8_t* __restrict__ pk, KeyWork kw, Gate gate,
                                                              int lo, int hi) {
#if LP_DEVICE
    if (!gate.keyed() || gate.off()) return;
    const uint32_t nk = kw.nkeys[PV_SPLIT_COMB_KEYS];
    if (blockIdx.x >= nk) return;
    // the chain is the keyed path's long serial dependency and shares SIMDs with the per-request prep
    // kernel: its waves take issue priority
    __builtin_amdgcn_s_setprio(3);
    const LpLane c = LpLane::make();
    const LpConsts K = LpConsts::make(c);
    for (uint32_t id = blockIdx.x; id < nk; id += gridDim.x)
        if (kw.comb_cslot[id] == PV_EMPTY) pv_key_chain_lp(pk, kw, id, c, K, lo, hi);  // cached or resident: table ready
#endif
}

// Per (key, position in [lo, hi), block of 16 entries): the comb table rows. Grid-stride over
// nkeys * (hi - lo) * 8 items.
__global__ __launch_bounds__(PV_BLOCK, PV_FILL_MINBLOCKS) void pv_key_fill_kernel(KeyWork kw, Gate gate, int lo,
                                                                                  int hi) {
    if (!gate.keyed() || gate.off() || kw.nkeys[PV_SPLIT_SPARSE]) return;
    const uint32_t np = (uint32_t)(hi - lo);
    const uint32_t items = kw.nkeys[PV_SPLIT_COMB_KEYS] * np * PV_COMB_BLOCKS;
    for (uint32_t it = blockIdx.x * PV_BLOCK + threadIdx.x; it < items; it += gridDim.x * PV_BLOCK) {
        const uint32_t id = it / (np * PV_COMB_BLOCKS);
        if (kw.comb_cslot[id] != PV_EMPTY) continue;  // the key's table is in a cache or resident in ctab
        const int pos = lo + (int)((it / PV_COMB_BLOCKS) % np);
        const int b = it % PV_COMB_BLOCKS;
        const DevBasePts pts{DevBases{kw.bases + (uint64_t)id * PV_COMB_POS * PV_COMB_PTS * 10}, pos};
        const uint64_t ts = kw.comb_tslot[id];
        pv_comb_fill_block(DevCombRow{kw.ctab + (ts * PV_COMB_POS + pos) * PV_COMB_ENT * 10}, pts, b);
    }
}

// Sparse variant for small chunks (PV_SPLIT_SPARSE): one thread per (comb key, position), only the
// entries the chunk's digits use (pv_comb_fill_sparse). Runs on the main stream after
// pv_comb_prep_req_kernel (need masks) and the key chain (bases). Sparse chunks have <= PV_ALLCOMB_KEYS
// comb keys: the grid covers that many.
struct DevNeed {
    const uint32_t* p;  // the position's 5 mask words (registers of the caller)
    __device__ __forceinline__ uint32_t word(int w) const { return p[w]; }
};
__global__ __launch_bounds__(PV_BLOCK) void pv_key_fill_sparse_kernel(KeyWork kw, Gate gate) {
    if (!gate.keyed() || gate.off() || !kw.nkeys[PV_SPLIT_SPARSE]) return;
    const uint32_t it = blockIdx.x * PV_BLOCK + threadIdx.x;
    const uint32_t id = it / PV_COMB_POS;
    const int pos = (int)(it % PV_COMB_POS);
    if (id >= kw.nkeys[PV_SPLIT_COMB_KEYS]) return;
    uint32_t* nd = kw.need + ((uint64_t)id * PV_COMB_POS + pos) * 5;
    uint32_t m[5];
#pragma unroll
    for (int w = 0; w < 5; w++) {  // read and clear: the masks start empty for the next sparse chunk
        m[w] = nd[w];
        nd[w] = 0u;
    }
    if (kw.comb_cslot[id] != PV_EMPTY) return;
    const DevBasePts pts{DevBases{kw.bases + (uint64_t)id * PV_COMB_POS * PV_COMB_PTS * 10}, pos};
    const uint64_t ts = kw.comb_tslot[id];
    pv_comb_fill_sparse(DevCombRow{kw.ctab + (ts * PV_COMB_POS + pos) * PV_COMB_ENT * 10}, pts, DevNeed{m});
}

// Key cache fill: comb index j of a put batch (tables built in the workspace by the chain / fill
// kernels) -> cache slot slots[j]: its 660 KB table, its key words and its libsodium key-check flag.
__global__ __launch_bounds__(PV_BLOCK) void pv_kc_scatter_kernel(const uint4* __restrict__ ctab,
                                                                  const uint32_t* __restrict__ key_flag,
                                                                  const uint8_t* __restrict__ pk,
                                                                  const uint32_t* __restrict__ slots, uint32_t m,
                                                                  uint4* __restrict__ tab, uint32_t* __restrict__ flags,
                                                                  uint32_t* __restrict__ keys) {
    constexpr uint32_t per = PV_COMB_POS * PV_COMB_ENT * 10;  // uint4 per key table
    const uint32_t j = blockIdx.y;
    if (j >= m) return;
    const uint64_t dst = (uint64_t)slots[j] * per, src = (uint64_t)j * per;
    for (uint32_t t = blockIdx.x * PV_BLOCK + threadIdx.x; t < per; t += gridDim.x * PV_BLOCK)
        tab[dst + t] = ctab[src + t];
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        keys[8 * slots[j] + threadIdx.x] = reinterpret_cast<const uint32_t*>(pk)[8 * j + threadIdx.x];
        if (threadIdx.x == 0) flags[slots[j]] = key_flag[j] & PV_KF_OK;
    }
}

// Key cache fill, second part: the affine rows of every slot just filled (one thread per (slot, position):
// pv_comb_row_to_affine over the 129 cached-form entries, one inversion).
struct DevCachedRowSrc {
    const uint4* r;  // [129][10]
    __device__ __forceinline__ void load(int d, ge_cached& c) const {
        uint32_t w[40];
        pv_quads_load<10>(w, [&](int q) { return r[d * 10 + q]; });
        ge_cached_load_words(c, w);
    }
};
struct DevAffineRowDst {
    uint4* r;  // [129][10]
    __device__ __forceinline__ uint32_t* e(int d) const { return reinterpret_cast<uint32_t*>(r + d * 10); }
};
__global__ __launch_bounds__(64) void pv_kc_affine_kernel(const uint4* __restrict__ tab,
                                                          const uint32_t* __restrict__ slots, uint32_t m,
                                                          uint4* __restrict__ atab) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= m * PV_COMB_POS) return;
    const uint64_t slot = slots[t / PV_COMB_POS], pos = t % PV_COMB_POS;
    pv_comb_row_to_affine(DevCachedRowSrc{tab + (slot * PV_COMB_POS + pos) * PV_COMB_ENT * 10},
                          DevAffineRowDst{atab + (slot * PV_COMB_POS + pos) * PV_COMB_ENT * 10});
}

// Resident tables to affine rows, in place (comb.h pv_comb_row_to_affine_inplace): the slots this
// chunk's scan queued (aff_list, aff_cnt: device-side, so the launch is fixed -- PV_AFF_CAP workgroups,
// each leaving at once when its index is past the count, as the chain's do for resident keys). One
// workgroup per table, one thread per (position, segment of 33 entries); the parked products go to
// aff_scr [workgroup][33][10][128], one word per thread and step, coalesced. Runs on the main stream
// after every kernel of the chunk that reads ctab and before any of the next chunk, so no reader sees
// a table half converted; PV_KF_AFF is set once the whole table is written (fence, barrier, flag), the
// order pv_dir_publish_kernel keeps between a key's bytes and its hash entry.
struct DevAffineRow {
    uint4* r;  // [129][10]
    __device__ __forceinline__ void load(int d, ge_cached& c) const { DevCachedRowSrc{r}.load(d, c); }
    __device__ __forceinline__ void load_z2(int d, fe& z) const {
        const uint4 a = r[d * 10 + 5], b = r[d * 10 + 6], c = r[d * 10 + 7];
        const uint32_t w[10] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y};
#pragma unroll
        for (int q = 0; q < 10; q++) z.v[q] = w[q];
    }
    __device__ __forceinline__ void store_affine(int d, const fe& ypx, const fe& ymx, const fe& xy2d) const {
        uint4* e = r + d * 10;
        e[0] = make_uint4(ypx.v[0], ypx.v[1], ypx.v[2], ypx.v[3]);
        e[1] = make_uint4(ypx.v[4], ypx.v[5], ypx.v[6], ypx.v[7]);
        e[2] = make_uint4(ypx.v[8], ypx.v[9], ymx.v[0], ymx.v[1]);
        e[3] = make_uint4(ymx.v[2], ymx.v[3], ymx.v[4], ymx.v[5]);
        e[4] = make_uint4(ymx.v[6], ymx.v[7], ymx.v[8], ymx.v[9]);
        e[5] = make_uint4(0u, 0u, 0u, 0u);
        e[6] = make_uint4(0u, 0u, 0u, 0u);
        e[7] = make_uint4(0u, 0u, xy2d.v[0], xy2d.v[1]);
        e[8] = make_uint4(xy2d.v[2], xy2d.v[3], xy2d.v[4], xy2d.v[5]);
        e[9] = make_uint4(xy2d.v[6], xy2d.v[7], xy2d.v[8], xy2d.v[9]);
    }
};
static constexpr uint32_t PV_AFF_THREADS = PV_COMB_POS * PV_AFF_SEGS;  // 128: one table per workgroup
struct DevAffineScr {
    uint32_t* z;  // this thread's column of [33][10][PV_AFF_THREADS]
    __device__ __forceinline__ void store(int k, const fe& f) const {
#pragma unroll
        for (int q = 0; q < 10; q++) z[(uint32_t)(k * 10 + q) * PV_AFF_THREADS] = f.v[q];
    }
    __device__ __forceinline__ void load(int k, fe& f) const {
#pragma unroll
        for (int q = 0; q < 10; q++) f.v[q] = z[(uint32_t)(k * 10 + q) * PV_AFF_THREADS];
    }
};
__global__ __launch_bounds__(PV_AFF_THREADS) void pv_dir_affine_kernel(KeyWork kw) {
    // a chunk that took the latency choice or reset the directory queued nothing
    if (blockIdx.x >= min(kw.aff_cnt[0], PV_AFF_CAP)) return;
    const uint64_t slot = kw.aff_list[blockIdx.x];  // < dir_cnt <= kcap: a listed slot the scan read from the hash
    const uint32_t pos = threadIdx.x / PV_AFF_SEGS, seg = threadIdx.x % PV_AFF_SEGS;
    const int d0 = (int)seg * PV_AFF_SEG, d1 = min(d0 + PV_AFF_SEG, PV_COMB_ENT);
    pv_comb_row_to_affine_inplace(
        DevAffineRow{kw.ctab + (slot * PV_COMB_POS + pos) * PV_COMB_ENT * 10},
        DevAffineScr{kw.aff_scr + (uint64_t)blockIdx.x * PV_AFF_SEG * 10 * PV_AFF_THREADS + threadIdx.x}, d0, d1);
    __threadfence();  // the rows before the bit that says they are affine
    __syncthreads();
    if (threadIdx.x == 0) {
        kw.dir_flags[slot] |= PV_KF_AFF;
        atomicAdd(&kw.dir_stat[3], 1ull);
    }
}

// Key cache put: the workspace set up for m keys given in order (d_put_pk[j] is comb index j's key):
// identity key ids, no cached table, split counters {m keys, m comb keys, everything else 0}.
__global__ __launch_bounds__(PV_BLOCK) void pv_kc_put_prep_kernel(KeyWork kw, uint32_t m) {
    const uint32_t j = blockIdx.x * PV_BLOCK + threadIdx.x;
    if (j < PV_SPLIT_WORDS) kw.nkeys[j] = (j == PV_SPLIT_KEYS || j == PV_SPLIT_COMB_KEYS) ? m : 0u;
    if (j < m) {
        kw.comb_key[j] = j;
        kw.key_owner[j] = j;
        kw.comb_cslot[j] = PV_EMPTY;
        kw.comb_tslot[j] = j;
    }
}
