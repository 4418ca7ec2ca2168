// Comb stage of the throughput path: per request of a comb key the prep (in request order) and the gather of
// its digits into slot order, then [S]B from the wide fixed-base rows and [k](-A) from the key's table, as
// two kernels or fused. launch_comb_stage (pv_engine.hip) enqueues them. The clock probe of the diagnostic
// build (PV_CLOCK_PROBE) lives beside pv_comb_ab_kernel, which stamps it. pv_engine.hip alone includes this
// header: its non-template __global__ functions have external linkage, so a second includer would define
// them twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "comb.h"
#include "kern_access.h"
#include "pv_engine_dev.h"
#include "verify_core.h"

#ifndef PV_COMB_A_MINBLOCKS
#define PV_COMB_A_MINBLOCKS 3
#endif

// Per request on the comb path: signature checks, k, radix-256 digits of k, radix-2^W digits of S. It
// runs in REQUEST order: the 64 lanes of a wave read 64 CONSECUTIVE records, ~23 KB of contiguous blob,
// so the lines that straddle two lanes' records or two SHA-512 blocks of one record are reused within
// the wave's own burst (slot order gave every lane a record at a random place in the blob). The
// per-request results (digits, the signature-check flag) go to a per-request AoS record, written
// coalesced; pv_comb_digits_kernel then gathers them into the slot-ordered rows the comb kernel reads.
// The key's own checks (key_flag) are written by the chain kernel on the key stream, which runs
// concurrently with this kernel: the comb kernels fold them into flags[slot].
template <int W>
struct PrepAos {  // uint4 per request: ek[8], fb[POS], flag, the digit words 8..11 of a key read wide, padding
    static constexpr int KR = 8 + Bc2<W>::POS + 1;  // first of those words
    static constexpr int WORDS = KR + (PV_KR_WORDS - 8);
    static constexpr int Q = (WORDS + 3) / 4;
};
static constexpr int PV_PREP_AOS_QMAX = 8;  // the largest PrepAos<W>::Q (W = 16: 29 words)
static_assert(PrepAos<16>::Q <= PV_PREP_AOS_QMAX && PrepAos<PV_BC2_W>::Q <= PV_PREP_AOS_QMAX, "AoS record size");
template <int W>
__global__ __launch_bounds__(PV_BLOCK, 2) void pv_comb_prep_req_kernel(const uint8_t* __restrict__ sm,
                                                                        const uint64_t* __restrict__ off, uint64_t n,
                                                                        const uint8_t* __restrict__ pk, Work wk,
                                                                        KeyWork kw, Gate gate) {
    if (!gate.keyed() || gate.off()) return;
    const uint32_t r = blockIdx.x * PV_BLOCK + threadIdx.x;  // request
    if (r >= n) return;
    const uint32_t i = kw.req_pos[r];  // its slot
    if (i >= gate.ncomb()) return;     // a Straus-path request (its prep runs on the side stream)
    const uint64_t o0 = off[r], o1 = off[r + 1];
    const uint64_t smlen = o1 - o0;
    const uint64_t raddr = reinterpret_cast<uint64_t>(sm + o0);
    const DevMsg mw{reinterpret_cast<const uint32_t*>(raddr & ~3ull), (uint32_t)(raddr & 3)};
    pv_sig_words in;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        in.R[q] = mw.dw(q);
        in.S[q] = mw.dw(8 + q);
    }
    pv_load_pk(in.A, pk, r);
    const bool ok = pv_sig_ok(in, smlen);
    uint32_t k[8];
    pv_hash_k(k, in, smlen, mw);
    constexpr int P = Bc2<W>::POS;
    uint32_t w[4 * PrepAos<W>::Q];
    const bool wide = kw.comb_wslot[kw.skey[i]] != PV_EMPTY;  // the scan's word, not key_flag (pv_engine_dev.h)
    if (wide) {
        uint32_t d[PV_KR_WORDS];
        sc_recode_w_packed<PV_KR_W, PV_KR_POS>(d, k);
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = d[q];
#pragma unroll
        for (int q = 8; q < PV_KR_WORDS; q++) w[PrepAos<W>::KR - 8 + q] = d[q];
    } else {
        sc_recode256(w, k);
#pragma unroll
        for (int q = 8; q < PV_KR_WORDS; q++) w[PrepAos<W>::KR - 8 + q] = 0u;
    }
    int32_t fb[P];
    sc_recode_w<W, P>(fb, in.S);
#pragma unroll
    for (int j = 0; j < P; j++) w[8 + j] = (uint32_t)fb[j];
    w[8 + P] = ok ? 1u : 0u;
#pragma unroll
    for (int j = PrepAos<W>::WORDS; j < 4 * PrepAos<W>::Q; j++) w[j] = 0u;
    uint4* o = wk.aos + (uint64_t)r * PrepAos<W>::Q;
#pragma unroll
    for (int q = 0; q < PrepAos<W>::Q; q++)  // a piece that holds nothing but the wide digit words: wide keys only
        if (4 * q < PrepAos<W>::KR || wide) o[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    if (kw.nkeys[PV_SPLIT_SPARSE] && !wide) {  // small chunk: record which entries of each row this request uses
        uint32_t* nd = kw.need + (uint64_t)kw.skey[i] * PV_COMB_POS * 5;
#pragma unroll
        for (int pos = 0; pos < PV_COMB_POS; pos++) {
            const int e = pv_byte(w[pos >> 2], pos);
            const uint32_t d = (uint32_t)(e < 0 ? -e : e);
            atomicOr(nd + pos * 5 + (d >> 5), 1u << (d & 31));
        }
    }
}

// Slot order: every comb slot's digit rows and flag from its request's AoS record (80-112 contiguous
// bytes per lane), written as the coalesced rows pv_comb_ab_kernel / pv_comb_a_kernel and the encode read.
template <int W>
__global__ __launch_bounds__(PV_BLOCK) void pv_comb_digits_kernel(Work wk, KeyWork kw, Gate gate) {
    if (!gate.keyed() || gate.off()) return;
    const uint32_t i = blockIdx.x * PV_BLOCK + threadIdx.x;  // slot
    if (i >= gate.ncomb()) return;
    const uint4* a = wk.aos + (uint64_t)kw.slot_req[i] * PrepAos<W>::Q;
    uint32_t w[4 * PrepAos<W>::Q];
    const bool wide = kw.comb_wslot[kw.skey[i]] != PV_EMPTY;  // as the prep kernel decided
#pragma unroll
    for (int q = 0; q < PrepAos<W>::Q; q++) {
        const uint4 v = 4 * q < PrepAos<W>::KR || wide ? a[q] : make_uint4(0u, 0u, 0u, 0u);
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
    const Soa ds(wk.digits, PV_DIGIT_ROWS, wk.stride);
#pragma unroll
    for (int q = 0; q < 8 + Bc2<W>::POS; q++) ds.st(q, i, w[q]);
#pragma unroll
    for (int q = 8; q < PV_KR_WORDS; q++)
        if (wide) ds.st(PV_KR_ROW - 8 + q, i, w[PrepAos<W>::KR - 8 + q]);
    wk.flags[i] = w[8 + Bc2<W>::POS];
}

// The niels loop of a comb slot over the wide fixed-base rows and, when the slot's key has wide rows
// (kpos != 0), over those too: positions kpos.. are the fixed base's (row j - kpos), 0..kpos-1 the key's --
// a cached key's 16 radix-65536 rows (comb.h PV_KW_*) or a resident table's 23 radix-2^11 rows (PV_KR_*),
// per lane. Same entry format, same LDS staging as DevB2Stage.
struct DevKeyWide {
    const uint4* rows;  // [kpos][entries][8], or null
    int kpos;           // PV_KW_POS, PV_KR_POS, or 0: the key has no wide rows
    __device__ __forceinline__ uint32_t ent() const { return kpos == PV_KR_POS ? PV_KR_ENT : PV_KW_ENT; }
};
template <uint32_t ENT>
struct DevBWStage {
    const uint4* base;  // T_B2
    DevKeyWide key;
    uint4* lds;
    uint32_t lane;
    __device__ __forceinline__ void stage(int j, int d) const {
        const uint4* e = j < key.kpos
                             ? key.rows + ((uint64_t)j * key.ent() + (uint32_t)d) * (PV_BCOMB_STRIDE / 4)
                             : base + ((uint64_t)(j - key.kpos) * ENT + (uint32_t)d) * (PV_BCOMB_STRIDE / 4);
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
// The wide rows of slot i's key: a resident table's (comb_wslot, written by the scan for every comb index),
// else a cached key's; kpos = 0 when it has neither.
__device__ __forceinline__ DevKeyWide pv_key_wide(const KeyWork& kw, uint32_t i) {
    const uint32_t j = kw.skey[i];
    const uint32_t ws = kw.comb_wslot[j];
    if (ws != PV_EMPTY)
        return DevKeyWide{kw.wide_tab + (uint64_t)ws * PV_KR_POS * PV_KR_ENT * (PV_BCOMB_STRIDE / 4), PV_KR_POS};
    if (kw.kc_wtab) {
        const uint32_t cslot = kw.comb_cslot[j];
        if (cslot < kw.kc_wcap)
            return DevKeyWide{kw.kc_wtab + (uint64_t)cslot * PV_KW_POS * PV_KW_ENT * (PV_BCOMB_STRIDE / 4), PV_KW_POS};
    }
    return DevKeyWide{nullptr, 0};
}
// [S]B, plus [k](-A) when the key has wide rows: the niels loop over 11 (+ 16 or 23) positions (comb.h
// pv_comb_b_acc_w). Digit word j >> 1 holds digit j of either wide form.
template <int W>
__device__ __forceinline__ void pv_comb_bw_acc(ge_p3& acc, const uint4* bcomb, const DevKeyWide& key,
                                               const DevDigits& dig, uint4* stg_wave) {
    constexpr int P = Bc2<W>::POS;
    pv_comb_b_acc_w<P>(
        acc, DevBWStage<Bc2<W>::ENT>{bcomb, key, stg_wave, threadIdx.x & 63u},
        [&](int j) {
            if (j < key.kpos) {
                const uint32_t w = dig.kr(j >> 1);
                return key.kpos == PV_KR_POS ? pv_kr_digit(w, j) : pv_kw_digit(w, j);
            }
            return dig.fb(j - key.kpos);
        },
        P + key.kpos);
}
// A slot whose [k](-A) was added in the niels loop: projective Q to q rows 0..29 and the key's flag.
__device__ __forceinline__ void pv_comb_store_q(const Work& wk, const KeyWork& kw, uint32_t i, const ge_p3& acc) {
    if ((kw.key_flag[kw.skey[i]] & PV_KF_OK) == 0) wk.flags[i] = 0;
    const Soa qs(wk.q, 40, wk.stride);
#pragma unroll
    for (int q = 0; q < 10; q++) {
        qs.st(q, i, acc.X.v[q]);
        qs.st(10 + q, i, acc.Y.v[q]);
        qs.st(20 + q, i, acc.Z.v[q]);
    }
}

// Per request on the comb path, first half: acc = [S]B from the wide fixed-base comb (PV_BC2_POS
// positions: one entry conversion + PV_BC2_POS - 1 additions). Needs no per-key data, so it runs on
// the main stream while the key stream builds the tables. acc (extended, 40 words) goes to q rows
// 0..39.
// A slot whose key has wide cached rows gets [k](-A) here too (16 more niels additions): pv_comb_a_kernel
// then only copies its flag.
template <int W>
__global__ __launch_bounds__(PV_BLOCK, 2) void pv_comb_b_kernel(uint64_t n, Work wk, KeyWork kw,
                                                                 const uint4* __restrict__ bcomb, Gate gate) {
    if (!gate.keyed() || gate.off()) return;
    const uint32_t i = blockIdx.x * PV_BLOCK + threadIdx.x;  // slot
    if (i >= gate.ncomb()) return;
    const DevDigits dig{wk.digits, (uint32_t)wk.stride, i};
    ge_p3 acc;
    __shared__ uint4 stg[PV_BLOCK / 64][PV_BCOMB_STRIDE / 4][64];
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    pv_comb_bw_acc<W>(acc, bcomb, pv_key_wide(kw, i), dig, &stg[wv][0][0]);
    const Soa qs(wk.q, 40, wk.stride);
#pragma unroll
    for (int q = 0; q < 10; q++) {
        qs.st(q, i, acc.X.v[q]);
        qs.st(10 + q, i, acc.Y.v[q]);
        qs.st(20 + q, i, acc.Z.v[q]);
        qs.st(30 + q, i, acc.T.v[q]);
    }
}

struct DevCombStage {  // per-key comb table rows, entries of 10 uint4
    const uint4* key;  // the key's table [32][129][10]
    uint4* lds;        // this wave's [10][64] staging area
    uint32_t lane;
    bool aff;          // affine rows (the key cache's pv_comb_row_to_affine form): rows 5, 6 not fetched
    __device__ __forceinline__ void stage(int i, int d) const {
        const uint4* e = key + ((uint32_t)i * PV_COMB_ENT + (uint32_t)d) * 10;
        pv_lds_reads_done();
        pv_glds16_row10_skip56(e, lds, aff);
    }
    __device__ __forceinline__ bool affine() const { return aff; }
    __device__ __forceinline__ void staged(int h, uint32_t w[20]) const {
        pv_quads_load<5>(w, [&](int q) { return lds[(5 * h + q) * 64 + lane]; });
    }
};

// XCD-aware block order. Workgroups are dealt round-robin over the 8 XCDs (block b runs on the XCD
// of b % 8; MI355X_MICROARCH.md, workgroup dispatch), each XCD with its own 4 MB L2. Slot order is
// key-sorted, so mapping the blocks of XCD x to ONE contiguous range of slots keeps a key's table
// rows in one L2 instead of fetching them into all eight. A bijection on [0, gridDim.x).
__device__ __forceinline__ uint32_t pv_xcd_block() {
    const uint32_t nb = gridDim.x, b = blockIdx.x;
    const uint32_t q = nb >> 3, r = nb & 7, x = b & 7, k = b >> 3;
    return x < r ? x * (q + 1) + k : r * (q + 1) + (x - r) * q + k;
}

// Second half: Q = acc + [k](-A) from the key's comb table (32 additions, no doublings), projective
// Q to q rows 0..29; the key's own libsodium checks are folded into flags[i] here.
__device__ __forceinline__ void pv_comb_a_from(const Work& wk, const KeyWork& kw, uint32_t i, const ge_p3& acc,
                                               uint4* stg_wave) {
    const uint32_t id = kw.skey[i];  // comb index
    const uint32_t cslot = kw.comb_cslot[id];
    const bool cached = pv_cslot_cached(cslot);  // else in kw.ctab: built by this chunk, or resident
    const bool xt = cached && (cslot & PV_CSLOT_XT);
    const uint4* ktab = !cached ? kw.ctab + (uint64_t)kw.comb_tslot[id] * PV_COMB_POS * PV_COMB_ENT * 10
                        : xt    ? kw.xt_tab + (uint64_t)(cslot & ~PV_CSLOT_XT) * PV_COMB_POS * PV_COMB_ENT * 10
                                : kw.kc_tab + (uint64_t)cslot * PV_COMB_POS * PV_COMB_ENT * 10;
    const Soa qs(wk.q, 40, wk.stride);
    const DevDigits dig{wk.digits, (uint32_t)wk.stride, i};
    fe X, Y, Z;
    // a cached key with affine rows: additions without the Z1 Z2 product (comb.h pv_comb_row_to_affine)
    // so has a resident table that pv_dir_affine_kernel converted in place (PV_KF_AFF from the directory)
    const uint32_t kf = kw.key_flag[id];
    const bool kc_aff = cached && !xt && kw.kc_ntab;
    const bool aff = kc_aff || (!cached && (kf & PV_KF_AFF));
    if (kc_aff) ktab = kw.kc_ntab + (uint64_t)cslot * PV_COMB_POS * PV_COMB_ENT * 10;
    pv_comb_a_xyz_staged(X, Y, Z, acc, DevCombStage{ktab, stg_wave, threadIdx.x & 63u, aff}, dig);
    if ((kf & PV_KF_OK) == 0) wk.flags[i] = 0;
#pragma unroll
    for (int q = 0; q < 10; q++) {
        qs.st(q, i, X.v[q]);
        qs.st(10 + q, i, Y.v[q]);
        qs.st(20 + q, i, Z.v[q]);
    }
}

// comb_a after a separate pv_comb_b_kernel: acc = [S]B from q rows 0..39.
__device__ __forceinline__ void pv_comb_a_slot(const Work& wk, const KeyWork& kw, uint32_t i, uint4* stg_wave) {
    const Soa qs(wk.q, 40, wk.stride);
    ge_p3 acc;
#pragma unroll
    for (int q = 0; q < 10; q++) {
        acc.X.v[q] = qs.ld(q, i);
        acc.Y.v[q] = qs.ld(10 + q, i);
        acc.Z.v[q] = qs.ld(20 + q, i);
        acc.T.v[q] = qs.ld(30 + q, i);
    }
    pv_comb_a_from(wk, kw, i, acc, stg_wave);
}

__global__ __launch_bounds__(PV_BLOCK, PV_COMB_A_MINBLOCKS) void pv_comb_a_kernel(uint64_t n, Work wk, KeyWork kw,
                                                                               Gate gate) {
    if (!gate.keyed() || gate.off()) return;
    const uint32_t i = pv_xcd_block() * PV_BLOCK + threadIdx.x;  // slot
    if (i >= gate.ncomb()) return;
    if (pv_key_wide(kw, i).kpos) {  // pv_comb_b_kernel added [k](-A) from the key's wide rows: Q is in q rows 0..29
        if ((kw.key_flag[kw.skey[i]] & PV_KF_OK) == 0) wk.flags[i] = 0;
        return;
    }
    __shared__ uint4 stg[PV_BLOCK / 64][10][64];
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    pv_comb_a_slot(wk, kw, i, &stg[wv][0][0]);
}

// [S]B and [k](-A) of a comb slot in ONE kernel: the 10 niels additions from the wide
// fixed-base comb (random 128 B entries in HBM, LDS-staged one addition ahead in the first 8 rows of
// the wave's staging area) run inside the issue-bound comb kernel, where the other waves of the SIMD
// cover their fetch latency, instead of as a latency-bound kernel of their own between comb_prep and
// the per-key tables; and acc never round-trips through q. The kernel then starts as soon as the
// per-key tables are built. The launcher takes it for chunks above PV_FUSED_MIN_REQ requests
// (chunk_plan.h has why the two-kernel form stays below that).
// Diagnostic build only (PV_CLOCK_PROBE=1, tools/clock_probe.py; MI355X_MICROARCH "DVFS give-back"
// item 6): wave 0 of every comb_ab workgroup stamps the shader clock (s_memtime) and the 100 MHz
// constant clock (s_memrealtime) at entry and exit into a buffer of its own, which no other code reads;
// the in-kernel clock is the median over workgroups of delta-memtime / delta-realtime x 100 MHz. The
// product build compiles no stamp.
#ifndef PV_CLOCK_PROBE
#define PV_CLOCK_PROBE 0
#endif
#if PV_CLOCK_PROBE
static constexpr uint32_t PV_CLOCK_SLOTS = 16384;  // workgroups stamped (block index mod this)
__device__ uint64_t pv_clock_stamps[PV_CLOCK_SLOTS * 4];
__device__ __forceinline__ void pv_clock_stamp(uint64_t& t, uint64_t& r) {
    __builtin_amdgcn_sched_barrier(0);
    t = __builtin_amdgcn_s_memtime();
    r = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) alone
    __builtin_amdgcn_sched_barrier(0);
}
#endif

template <int W>
__global__ __launch_bounds__(PV_BLOCK, PV_COMB_A_MINBLOCKS) void pv_comb_ab_kernel(uint64_t n, Work wk, KeyWork kw,
                                                                                const uint4* __restrict__ bcomb,
                                                                                Gate gate) {
    if (!gate.keyed() || gate.off()) return;
    const uint32_t i = pv_xcd_block() * PV_BLOCK + threadIdx.x;  // slot
    if (i >= gate.ncomb()) return;
#if PV_CLOCK_PROBE
    uint64_t t0 = 0, r0 = 0;
    pv_clock_stamp(t0, r0);
#endif
    __shared__ uint4 stg[PV_BLOCK / 64][10][64];
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const DevDigits dig{wk.digits, (uint32_t)wk.stride, i};
    ge_p3 acc;
    const DevKeyWide wkey = pv_key_wide(kw, i);
    pv_comb_bw_acc<W>(acc, bcomb, wkey, dig, &stg[wv][0][0]);
    if (wkey.kpos)  // [k](-A) came from the key's wide rows in the same loop
        pv_comb_store_q(wk, kw, i, acc);
    else
        pv_comb_a_from(wk, kw, i, acc, &stg[wv][0][0]);
#if PV_CLOCK_PROBE
    uint64_t t1 = 0, r1 = 0;
    pv_clock_stamp(t1, r1);
    if (threadIdx.x == 0) {
        uint64_t* o = pv_clock_stamps + 4ull * (blockIdx.x % PV_CLOCK_SLOTS);
        o[0] = t0;
        o[1] = t1;
        o[2] = r0;
        o[3] = r1;
    }
#endif
}
