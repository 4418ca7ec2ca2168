// libplenum_verify: MI355X batch Ed25519 verification engine: the verification kernels, the device
// context (pv_ctx.h Ctx: lifecycle, launch, control and statistics entries), the table build of a
// key-cache put and the device-buffer entry. The rest of the engine lives beside it: signing in
// pv_sign.hip, the host-buffer entries in pv_host.hip, the key cache's host side in pv_keycache.hip, RCCL
// and in-process multi-GPU in pv_multi.hip, the latency path in pv_latency.hip; the device types they
// share are pv_engine_dev.h. What a launch decides on the host (path, lookup views, KeyWork scalars, launch
// shape, grids) is chunk_plan.h, with the thresholds those rules read; launch_chunk applies it.
//
// One lane per request, 256-thread workgroups, two workgroups per CU (2 waves/SIMD: measured
// v_mad_u64_u32 throughput saturates at >= 2 waves/SIMD, profiles/r01_isa_rates.jsonl). The grid is
// a fixed number of workgroups that stride over the batch, so the per-lane HBM table of [j](-A)
// (9 cached points x 160 B) is sized by resident lanes, not by the batch.
//
// Replaces (per request) stp_core/crypto/nacl_wrappers.py:108 libnacl.crypto_sign_open(sm, pk);
// see include/plenum_verify.h for the ABI contract and verify_core.h for the arithmetic.
//
// The #ifndef switches in this file are numeric tuning constants (microbench/build_variants.sh varies
// them) and diagnostic builds. The kernel forms, priorities and stream layouts that lost their A/B are
// not in the source any more: DESIGN.md, "Variants tried and retired", has each one's result.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <atomic>
#include <random>
#include <functional>
#include <thread>
#include <string>
#include <vector>

#include "btable.h"
#include "comb.h"
#include "keycache.h"
#include "lp25519.h"
#include "verify_core.h"
#include "pv_engine_dev.h"
#include "pv_ctx.h"
#include "pv_internal.h"
#include "../../include/plenum_verify.h"
#include "../../include/plenum_verify_test.h"

#ifndef PV_COMB_A_MINBLOCKS
#define PV_COMB_A_MINBLOCKS 3
#endif
#ifndef PV_FILL_MINBLOCKS
#define PV_FILL_MINBLOCKS 2
#endif
#ifndef PV_MSM_MINBLOCKS
// workgroups per CU the msm kernel's register budget is sized for (3: <= 168 VGPRs, 3 waves/SIMD)
#define PV_MSM_MINBLOCKS 3
#endif
#ifndef PV_PREP_MINBLOCKS
#define PV_PREP_MINBLOCKS 2  // Straus prep (decompression + SHA-512 + recoding)
#endif
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

// ---------------------------------------------------------------------------------------- device

// [rows][S] u32 structure-of-arrays buffer through a buffer resource: every access is one
// buffer_load/store_dword with the lane's 32-bit byte offset in a VGPR and the row offset in an
// SGPR (soffset), so rows cost no per-lane address registers (global_load addressing kept 40 live
// 64-bit addresses for a 40-row point).
struct Soa {
    __amdgpu_buffer_rsrc_t r;
    uint32_t S4;  // row stride in bytes
    __device__ __forceinline__ Soa(uint32_t* base, uint64_t rows, uint64_t S)
        : r(__builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)(rows * S * 4 < 0x7fffffffull ? rows * S * 4 : 0x7fffffffull),
                                              0x00020000)),
          S4((uint32_t)(S * 4)) {}
    __device__ __forceinline__ uint32_t ld(uint32_t row, uint32_t i) const {
        return __builtin_amdgcn_raw_buffer_load_b32(r, i * 4, row * S4, 0);
    }
    __device__ __forceinline__ void st(uint32_t row, uint32_t i, uint32_t v) const {
        __builtin_amdgcn_raw_buffer_store_b32(v, r, i * 4, row * S4, 0);
    }
};

// Per-lane cached table of [j](-A) in HBM. Indices are 32-bit (chunk <= 2^20 slots, 90 quads per
// slot < 2^32) so each access is a uniform 64-bit base plus one per-lane 32-bit offset instead of ten
// live 64-bit addresses. Layout [slot][entry][quad] uint4 -- the lanes of a wave pick different entries
// (their own digits), so each lane reads its own contiguous 160 B entry (two 128 B lines) instead of a
// 16 B piece of a line shared with lanes that want other entries.
// The Straus path is half-size (sc25519.h sc_halfsize, verify_core.h pv_straus_ar_xyz): k = k1 / k2
// (mod 8L) with |k1|, k2 ~ 2^128, so the per-request loop runs ~33 windows of both scalars against two
// tables ([j](+-A) and [j](-R')) instead of 64 windows of k against one.
static constexpr uint32_t PV_ATAB_ENT = 18u;  // table entries per slot (9 of each table)
struct DevATab {
    uint4* base;
    uint32_t slot;
    uint32_t t0 = 0;  // first entry of this table in the slot (the R table starts at 9)
    __device__ __forceinline__ uint4& at(int j, int q) const {
        // [slot / 64][entry][slot % 64][quad]: a lane's entry is 160 contiguous bytes, and one wave's
        // ten stores of an entry cover 10 KB contiguously (full lines reach HBM)
        return base[(((slot >> 6) * PV_ATAB_ENT + t0 + (uint32_t)j) * 64u + (slot & 63u)) * 10u + (uint32_t)q];
    }
    __device__ __forceinline__ void store(int j, const uint32_t w[40]) const {
#pragma unroll
        for (int q = 0; q < 10; q++) at(j, q) = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
    __device__ __forceinline__ void store_p3(int j, const ge_p3& p) const {
        uint32_t w[40];
#pragma unroll
        for (int q = 0; q < 10; q++) {
            w[q] = p.X.v[q];
            w[10 + q] = p.Y.v[q];
            w[20 + q] = p.Z.v[q];
            w[30 + q] = p.T.v[q];
        }
        store(j, w);
    }
    __device__ __forceinline__ void load_p3(int j, ge_p3& p) const {
        uint32_t w[40];
        load(j, w);
#pragma unroll
        for (int q = 0; q < 10; q++) {
            p.X.v[q] = w[q];
            p.Y.v[q] = w[10 + q];
            p.Z.v[q] = w[20 + q];
            p.T.v[q] = w[30 + q];
        }
    }
    __device__ __forceinline__ void load_half(int j, int h, uint32_t w[20]) const {
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const uint4 v = at(j, 5 * h + q);
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
    }
    __device__ __forceinline__ void load(int j, uint32_t w[40]) const {
        load_half(j, 0, w);
        load_half(j, 1, w + 20);
    }
};

// Digit rows, one coalesced load each time a loop enters a new group of windows. Rows 0..7: |k1|
// (Straus path, radix 16) or k (comb path, radix 256); rows 8..: the signed radix-2^W digits of k2 S
// (Straus) or S (comb) for the wide fixed-base comb.
// Straus path: rows PV_K2_ROW.. hold k2's radix-16 digits, row PV_NW_ROW the lane's window count
static constexpr int PV_K2_ROW = 8 + (Bc2<16>::POS > PV_BC2_POS ? Bc2<16>::POS : PV_BC2_POS);
static constexpr int PV_NW_ROW = PV_K2_ROW + 8;
// comb path, a key read from its radix-2^11 rows (comb.h PV_KR_*): the 23 digits of k, two per word, in
// rows 0..7 (in place of the radix-256 digits) and PV_KR_ROW .. PV_KR_ROW + 3
static constexpr int PV_KR_ROW = PV_NW_ROW + 1;
static constexpr int PV_DIGIT_ROWS = PV_KR_ROW + (PV_KR_WORDS - 8);
struct DevDigits {
    Soa d;
    uint32_t slot;
    __device__ __forceinline__ DevDigits(uint32_t* base, uint32_t stride, uint32_t slot_)
        : d(base, PV_DIGIT_ROWS, stride), slot(slot_) {}
    __device__ __forceinline__ uint32_t ek(int q) const { return d.ld(q, slot); }
    __device__ __forceinline__ uint32_t kr(int q) const { return d.ld(q < 8 ? q : PV_KR_ROW - 8 + q, slot); }
    __device__ __forceinline__ uint32_t ek2(int q) const { return d.ld(PV_K2_ROW + q, slot); }
    __device__ __forceinline__ uint32_t nw() const { return d.ld(PV_NW_ROW, slot); }
    __device__ __forceinline__ int fb(int j) const { return (int)d.ld(8 + j, slot); }
};

// A 10-piece entry whose pieces 5 and 6 (words 20..27) are skipped on lanes with `skip` (affine comb rows:
// their Z2 words are not read). Lanes that skip leave those pieces of their staging column stale.
__device__ __forceinline__ void pv_glds16_row10_skip56(const uint4* g, uint4* l, bool skip) {
    pv_glds16_row<5>(g, l);
    if (!skip) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                         (__attribute__((address_space(3))) void*)(l + 5 * 64 - 5), 16, 16 * 5, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                         (__attribute__((address_space(3))) void*)(l + 6 * 64 - 6), 16, 16 * 6, 0);
    }
    pv_glds16_row<10, 7>(g, l);
}

__device__ __forceinline__ void pv_load_pk(uint32_t A[8], const uint8_t* pk, uint32_t i) {
    const uint4* p4 = reinterpret_cast<const uint4*>(pk + 32 * (uint64_t)i);
    const uint4 a0 = p4[0], a1 = p4[1];
    A[0] = a0.x; A[1] = a0.y; A[2] = a0.z; A[3] = a0.w;
    A[4] = a1.x; A[5] = a1.y; A[6] = a1.z; A[7] = a1.w;
}

// Straus path, per slot i (request r): the signature checks, k = SHA-512(R||A||M) mod L, A's checks
// and decompression; -A for the table kernel.
__device__ __forceinline__ void pv_prep_slot(const uint8_t* __restrict__ sm, const uint64_t* __restrict__ off,
                                             const uint8_t* __restrict__ pk, const Work& wk, uint32_t i, uint32_t r) {
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
    const uint4* pk4 = reinterpret_cast<const uint4*>(pk + 32 * (uint64_t)r);
    const uint4 a0 = pk4[0], a1 = pk4[1];
    in.A[0] = a0.x; in.A[1] = a0.y; in.A[2] = a0.z; in.A[3] = a0.w;
    in.A[4] = a1.x; in.A[5] = a1.y; in.A[6] = a1.z; in.A[7] = a1.w;
    // pv_prepare_half over three kernels: here the signature checks, k (to rows 0..7 for
    // pv_split_kernel), A's checks and -A (table entry 1); the split of k and the digits in
    // pv_split_kernel; the sign of k1 on -A, R's checks, -R' and both tables in pv_table_kernel
    bool ok = pv_sig_ok(in, smlen);
    const Soa ds(wk.digits, PV_DIGIT_ROWS, wk.stride);
    {
        uint32_t k[8];
        pv_hash_k(k, in, smlen, mw);
#pragma unroll
        for (int q = 0; q < 8; q++) ds.st(q, (uint32_t)i, k[q]);
    }
    {
        ge_p3 negA;
        ok &= pv_key_ok_negate(negA, in.A);
        const DevATab at{wk.atab, (uint32_t)i};
        at.store_p3(1, negA);
    }
    wk.flags[i] = ok ? 1u : 0u;
}

// Kernel 1 (Straus path): pv_prep_slot over the Straus slots. Its two instantiations are the same code
// (the wide comb's digits are written by pv_split_kernel); both names are launched.
template <int W>
__global__ __launch_bounds__(PV_BLOCK, PV_PREP_MINBLOCKS) void pv_prep_kernel(const uint8_t* __restrict__ sm,
                                                               const uint64_t* __restrict__ off, uint64_t n,
                                                               const uint8_t* __restrict__ pk, Work wk, Gate gate) {
    if (gate.off()) return;
    const uint32_t nc = gate.ncomb(), ntiles = (uint32_t)((n + PV_BLOCK - 1) / PV_BLOCK);
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t sb = gate.stile(t, ntiles);
        if ((sb + 1) * PV_BLOCK <= nc) break;  // this and every later tile: comb-path slots
        const uint32_t i = sb * PV_BLOCK + threadIdx.x;  // slot
        if (i < n && i >= nc) pv_prep_slot(sm, off, pk, wk, i, gate.req(i));
    }
}

// Kernel 1a (half-size path): the split k = k1 / k2 (mod 8L) of each Straus slot's k (rows 0..7, from
// pv_prep_kernel), s2 = k2 S mod L; writes the digits of |k1| (rows 0..7), k2 (PV_K2_ROW..), the window
// count and k1's sign (row PV_NW_ROW: nw | neg << 8) and the wide-comb digits of s2 (rows 8..). Its own
// kernel: few registers, so the latency of the Euclid steps is hidden by occupancy.
template <int W>
__global__ __launch_bounds__(PV_BLOCK) void pv_split_kernel(const uint8_t* __restrict__ sm,
                                                            const uint64_t* __restrict__ off, uint64_t n, Work wk,
                                                            Gate gate) {
    if (gate.off()) return;
    const uint32_t nc = gate.ncomb(), ntiles = (uint32_t)((n + PV_BLOCK - 1) / PV_BLOCK);
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t sb = gate.stile(t, ntiles);
        if ((sb + 1) * PV_BLOCK <= nc) break;
        const uint32_t i = sb * PV_BLOCK + threadIdx.x;  // slot
        if (i >= n || i < nc) continue;
        const Soa ds(wk.digits, PV_DIGIT_ROWS, wk.stride);
        uint32_t k[8], S[8];
#pragma unroll
        for (int q = 0; q < 8; q++) k[q] = ds.ld(q, i);
        {
            const uint64_t raddr = reinterpret_cast<uint64_t>(sm + off[gate.req(i)]);
            const DevMsg mw{reinterpret_cast<const uint32_t*>(raddr & ~3ull), (uint32_t)(raddr & 3)};
#pragma unroll
            for (int q = 0; q < 8; q++) S[q] = mw.dw(8 + q);
        }
        pv_halfk hk;
        sc_halfsize(hk, k);
        uint32_t s2[8];
        sc_mul<5>(s2, hk.k2, S);
        int32_t fb[Bc2<W>::POS];
        sc_recode_w<W, Bc2<W>::POS>(fb, s2);
#pragma unroll
        for (int j = 0; j < Bc2<W>::POS; j++) ds.st(8 + j, i, (uint32_t)fb[j]);
        uint32_t e1[8], e2[8];
        sc_recode16(e1, hk.k1);
        sc_recode16(e2, hk.k2);
        const int nw1 = sc_nwin16(e1), nw2 = sc_nwin16(e2);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            ds.st(q, i, e1[q]);
            ds.st(PV_K2_ROW + q, i, e2[q]);
        }
        ds.st(PV_NW_ROW, i, (uint32_t)(nw1 > nw2 ? nw1 : nw2) | (hk.neg ? 0x100u : 0u));
    }
}

// Kernel 1b: decompression and checks of R, the cached tables [j](+-A) (entries 0..8, from -A in
// entry 1) and [j](-R') (entries 9..17).
#ifndef PV_TABLE_MINBLOCKS
#define PV_TABLE_MINBLOCKS 2  // waves per SIMD (256 VGPRs; 3 spills 264 B)
#endif
__global__ __launch_bounds__(PV_BLOCK, PV_TABLE_MINBLOCKS) void pv_table_kernel(const uint8_t* __restrict__ sm,
                                                                const uint64_t* __restrict__ off, uint64_t n,
                                                                const uint8_t* __restrict__ pk, Work wk, Gate gate) {
    if (gate.off()) return;
    const uint32_t nc = gate.ncomb(), ntiles = (uint32_t)((n + PV_BLOCK - 1) / PV_BLOCK);
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t sb = gate.stile(t, ntiles);
        if ((sb + 1) * PV_BLOCK <= nc) break;
        const uint32_t i = sb * PV_BLOCK + threadIdx.x;  // slot
        if (i >= n || i < nc) continue;
        // [j](+-A) from -A (entry 1, pv_prep_kernel) and k1's sign (pv_split_kernel), then R's
        // canonical-decoding rule and [j](-R')
        const uint32_t r = gate.req(i);
        const uint64_t raddr = reinterpret_cast<uint64_t>(sm + off[r]);
        const DevMsg mw{reinterpret_cast<const uint32_t*>(raddr & ~3ull), (uint32_t)(raddr & 3)};
        {
            DevATab at{wk.atab, i};
            ge_p3 PA;
            at.load_p3(1, PA);
            ge_p3_cneg(PA, (Soa(wk.digits, PV_DIGIT_ROWS, wk.stride).ld(PV_NW_ROW, i) & 0x100u) != 0);  // +-A
            pv_build_a_table(at, PA);
        }
        bool ok;
        {
            uint32_t R[8];
#pragma unroll
            for (int q = 0; q < 8; q++) R[q] = mw.dw(q);
            ge_p3 negR;
            ok = pv_r_decode_negate(negR, R);
            DevATab rt{wk.atab, i, 9u};
            pv_build_a_table(rt, negR);
        }
        if (!ok) wk.flags[i] = 0u;
    }
}

// Kernel 2: Q = [k2 S]B + [k1](+-A) + [k2](-R') by the regular-window Straus loop over both half-size
// scalars. [k2 S]B is added inside the loop's epilogue (the wide comb's niels additions straight into
// the loop's point, entries LDS-staged one addition ahead), and each 256-slot tile's lanes are
// regrouped by window count first (below). btab_g is not read.
static constexpr int PV_MSM_SORT_CLS = 8;
template <int W>
__global__ __launch_bounds__(PV_BLOCK, PV_MSM_MINBLOCKS) void pv_msm_kernel(const uint8_t* __restrict__ sm,
                                                              const uint64_t* __restrict__ off, uint64_t n,
                                                              const uint32_t* __restrict__ btab_g, Work wk,
                                                              const uint4* __restrict__ bcomb, Gate gate) {
    if (gate.off()) return;
    const uint32_t nc = gate.ncomb(), ntiles = (uint32_t)((n + PV_BLOCK - 1) / PV_BLOCK);
    // nothing for this block (or no Straus slot at all): leave before the LDS fill
    if (blockIdx.x >= ntiles || nc >= n || (gate.stile(blockIdx.x, ntiles) + 1) * PV_BLOCK <= nc) return;
    __shared__ uint32_t s_wcnt[PV_BLOCK / 64][PV_MSM_SORT_CLS];
    __shared__ uint16_t s_perm[PV_BLOCK];
    __shared__ uint4 stgb[PV_BLOCK / 64][PV_BCOMB_STRIDE / 4][64];
    uint4* stgb_wave = &stgb[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)][0][0];
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t sb = gate.stile(t, ntiles);
        if ((sb + 1) * PV_BLOCK <= nc) break;
        const uint32_t i0 = sb * PV_BLOCK + threadIdx.x;  // slot
        // the tile's lanes regrouped by their window count (a stable counting sort: lanes with no Straus
        // slot first, then counts <= 30, 31, ..., >= 36), so a wave runs the largest count of lanes that
        // need about as many: 33.1 windows per wave on average at random scalars instead of 33.9
        // (lane mean 32.7). Block-uniform: every thread of the block takes the same tiles.
        uint32_t src = threadIdx.x;
        {
            int cls = 0;
            if (i0 < n && i0 >= nc) {
                const int w = (int)(DevDigits{wk.digits, (uint32_t)wk.stride, i0}.nw() & 0xFFu);
                cls = 1 + min(max(w - 30, 0), PV_MSM_SORT_CLS - 2);
            }
            const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63u;
            const uint64_t below = (1ull << ln) - 1ull;
            uint32_t rank = 0;
            for (int c = 0; c < PV_MSM_SORT_CLS; c++) {
                const uint64_t m = __ballot(cls == c);
                if (c == cls) rank = (uint32_t)__popcll(m & below);
                if (ln == 0) s_wcnt[wv][c] = (uint32_t)__popcll(m);
            }
            __syncthreads();
            uint32_t base = 0;
            for (int c = 0; c < PV_MSM_SORT_CLS; c++)
                for (int w2 = 0; w2 < PV_BLOCK / 64; w2++)
                    if (c < cls || (c == cls && w2 < (int)wv)) base += s_wcnt[w2][c];
            s_perm[base + rank] = (uint16_t)threadIdx.x;
            __syncthreads();
            src = s_perm[threadIdx.x];
            __syncthreads();  // the next tile rewrites s_wcnt and s_perm
        }
        const uint32_t is = sb * PV_BLOCK + src;
        const bool active = is < n && is >= nc;
        const uint32_t i = active ? is : (uint32_t)n - 1;  // n - 1 >= nc here: a Straus slot
        const DevATab at{wk.atab, i};
        const DevDigits dig{wk.digits, (uint32_t)wk.stride, i};
        const Soa qs(wk.q, 40, wk.stride);
        fe X, Y, Z;
        // the wave's window count: its lanes' maximum (a lane's digits above its own count are 0)
        int nw = (int)(dig.nw() & 0xFFu);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nw = max(nw, __shfl_xor(nw, m));
        nw = __builtin_amdgcn_readfirstlane(nw);
        const DevATab rt{wk.atab, i, 9u};
        pv_straus_ar_xyz_addb(X, Y, Z, at, rt, dig, nw, [&](ge_p3& acc) {  // + [k2 S]B from the wide comb
            pv_comb_b_add_w<Bc2<W>::POS>(acc, DevB2Stage<Bc2<W>::ENT>{bcomb, stgb_wave, threadIdx.x & 63u},
                                         [&](int j) { return dig.fb(j); });
        });
        if (active) {
#pragma unroll
            for (int q = 0; q < 10; q++) {
                qs.st(q, i, X.v[q]);
                qs.st(10 + q, i, Y.v[q]);
                qs.st(20 + q, i, Z.v[q]);
            }
        }
    }
}

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

struct DevBases {
    uint4* b;  // [32][PV_COMB_PTS][10]: per position P_i, [16] P_i, [32] P_i, [64] P_i (extended)
    __device__ __forceinline__ void store(int i, int m, const ge_p3& p) const {
        uint32_t w[40];
#pragma unroll
        for (int q = 0; q < 10; q++) {
            w[q] = p.X.v[q];
            w[10 + q] = p.Y.v[q];
            w[20 + q] = p.Z.v[q];
            w[30 + q] = p.T.v[q];
        }
        uint4* e = b + (i * PV_COMB_PTS + m) * 10;
#pragma unroll
        for (int q = 0; q < 10; q++) e[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
    __device__ __forceinline__ void load(int i, int m, ge_p3& p) const {
        const uint4* e = b + (i * PV_COMB_PTS + m) * 10;
        uint32_t w[40];
#pragma unroll
        for (int q = 0; q < 10; q++) {
            const uint4 v = e[q];
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int q = 0; q < 10; q++) {
            p.X.v[q] = w[q];
            p.Y.v[q] = w[10 + q];
            p.Z.v[q] = w[20 + q];
            p.T.v[q] = w[30 + q];
        }
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
#pragma unroll
        for (int q = 0; q < 10; q++) r[d * 10 + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
    __device__ __forceinline__ void load(int d, ge_cached& c) const {
        uint32_t w[40];
#pragma unroll
        for (int q = 0; q < 10; q++) {
            const uint4 v = r[d * 10 + q];
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
        ge_cached_load_words(c, w);
    }
    __device__ __forceinline__ void load_half(int d, int h, uint32_t w[20]) const {
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const uint4 v = r[d * 10 + 5 * h + q];
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
    }
};

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
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const uint4 v = lds[(5 * h + q) * 64 + lane];
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
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
#pragma unroll
        for (int q = 0; q < 10; q++) {
            const uint4 v = r[d * 10 + q];
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
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

// Wide fixed-base comb build (pv_init): each thread makes PV_BC2_RUN consecutive entries d0.. of one
// row (base point P = [2^(W j)] B): start [d0] P by double-and-add, then P-steps, the projective
// points parked in the entries themselves and the running product of their Z in `scratch`; one
// inversion per run (Montgomery's trick) gives every entry's affine niels form (canonical limbs).
static constexpr uint32_t PV_BC2_RUN = 64;
struct PvPoint40 {
    uint32_t w[40];  // X, Y, Z, T limbs
};
struct DevBc2Row {  // one row of the wide comb, 32 words per entry
    uint32_t* r;
    __device__ __forceinline__ uint32_t* e(uint32_t d) const { return r + (uint64_t)d * PV_BCOMB_STRIDE; }
};
struct DevBc2Scratch {  // running Z products, 10 words per entry
    uint32_t* z;
    __device__ __forceinline__ void store(uint32_t d, const fe& f) const {
#pragma unroll
        for (int q = 0; q < 10; q++) z[(uint64_t)d * 10 + q] = f.v[q];
    }
    __device__ __forceinline__ void load(uint32_t d, fe& f) const {
#pragma unroll
        for (int q = 0; q < 10; q++) f.v[q] = z[(uint64_t)d * 10 + q];
    }
};
__global__ __launch_bounds__(PV_BLOCK) void pv_bc2_build_kernel(uint4* __restrict__ row, uint32_t ent, PvPoint40 base,
                                                                uint32_t* __restrict__ scratch) {
    const uint32_t d0 = (blockIdx.x * PV_BLOCK + threadIdx.x) * PV_BC2_RUN;
    if (d0 >= ent) return;
    ge_p3 P;
#pragma unroll
    for (int q = 0; q < 10; q++) {
        P.X.v[q] = base.w[q];
        P.Y.v[q] = base.w[10 + q];
        P.Z.v[q] = base.w[20 + q];
        P.T.v[q] = base.w[30 + q];
    }
    pv_bc2_build_run(DevBc2Row{reinterpret_cast<uint32_t*>(row)}, DevBc2Scratch{scratch}, P, d0,
                     min(PV_BC2_RUN, ent - d0));
}

// Key cache fill, third part: the radix-65536 rows of the slots below wcap (comb.h PV_KW_*), keys
// [j0, j0 + g) of the put batch: one thread per run of PV_BC2_RUN entries of one row, the row's base
// [65536^q](-A) = the chain's P_{2q}; pv_bc2_build_run (double-and-add start, P-steps, one inversion
// per run) writes affine niels entries, the Z products in scratch.
static constexpr uint32_t PV_KW_RUNS = (PV_KW_ENT + PV_BC2_RUN - 1) / PV_BC2_RUN;  // runs per row
__global__ __launch_bounds__(PV_BLOCK) void pv_kc_wide_kernel(KeyWork kw, const uint32_t* __restrict__ slots,
                                                              uint32_t j0, uint32_t g, uint32_t wcap,
                                                              uint4* __restrict__ wtab, uint32_t* __restrict__ scr) {
    const uint32_t t = blockIdx.x * PV_BLOCK + threadIdx.x;
    const uint32_t per_key = PV_KW_POS * PV_KW_RUNS;
    if (t >= g * per_key) return;
    const uint32_t jj = t / per_key, q = (t % per_key) / PV_KW_RUNS, r = t % PV_KW_RUNS;
    const uint32_t j = j0 + jj, slot = slots[j];
    if (slot >= wcap) return;
    ge_p3 P;
    DevBases{kw.bases + (uint64_t)j * PV_COMB_POS * PV_COMB_PTS * 10}.load(2 * q, 0, P);
    const uint32_t d0 = r * PV_BC2_RUN;
    pv_bc2_build_run(DevBc2Row{reinterpret_cast<uint32_t*>(wtab + ((uint64_t)slot * PV_KW_POS + q) * PV_KW_ENT * 8)},
                     DevBc2Scratch{scr + ((uint64_t)jj * PV_KW_POS + q) * PV_KW_ENT * 10}, P, d0,
                     min(PV_BC2_RUN, PV_KW_ENT - d0));
}

// Resident tables to radix-2^11 rows (comb.h PV_KR_*): the tables this chunk's scan queued (wide_list,
// wide_cnt[0]: device-side, so the launch is fixed -- PV_WIDE_GRID workgroups that stride over the queue
// and leave at once when it is empty). One workgroup per table at a time, one thread per (position, run of
// 64 entries): the position's base from the table's affine radix-256 row (pv_kr_base), then
// pv_kr_build_run straight into the pool slot; the runs' Z products go to the workgroup's own scratch
// [64][10][PV_WIDE_THREADS], one word per thread and step, coalesced, so the scratch is sized by the grid
// and not by the queue. Runs on the main stream behind pv_dir_affine_kernel: after every kernel of the
// chunk that reads the pool or ctab, before any of the next chunk. dir_wslot and PV_KF_WIDE are stored once
// the whole table is written (fence, barrier, flag), as pv_dir_affine_kernel does.
struct DevWideScr {
    uint32_t* z;  // this thread's column of [PV_KR_RUN][10][PV_WIDE_THREADS]
    __device__ __forceinline__ void store(uint32_t d, const fe& f) const {
        const uint32_t k = (d - 1u) % PV_KR_RUN;
#pragma unroll
        for (int q = 0; q < 10; q++) z[(k * 10 + q) * PV_WIDE_THREADS] = f.v[q];
    }
    __device__ __forceinline__ void load(uint32_t d, fe& f) const {
        const uint32_t k = (d - 1u) % PV_KR_RUN;
#pragma unroll
        for (int q = 0; q < 10; q++) f.v[q] = z[(k * 10 + q) * PV_WIDE_THREADS];
    }
};
__global__ __launch_bounds__(PV_WIDE_THREADS) void pv_dir_widen_kernel(KeyWork kw) {
    // a chunk that took the latency choice or reset the directory queued nothing
    const uint32_t cnt = min(kw.wide_cnt[0], PV_WIDE_CAP);  // settled by the scan: every entry below it is filled
    const uint32_t pos = threadIdx.x / PV_KR_RUNS, run = threadIdx.x % PV_KR_RUNS;
    for (uint32_t u = blockIdx.x; u < cnt; u += gridDim.x) {
        const uint64_t slot = kw.wide_list[2 * u];  // < dir_cnt <= kcap: a listed slot the scan read from the hash
        const uint64_t ws = kw.wide_list[2 * u + 1];
        if (slot >= kw.kcap || ws >= kw.wide_cap) continue;  // never: the scan's bounds (uniform over the workgroup)
        if (pos < (uint32_t)PV_KR_POS) {
            const uint4* e = kw.ctab + ((slot * PV_COMB_POS + pv_kr_base_row(pos)) * PV_COMB_ENT + pv_kr_base_ent(pos)) * 10;
            uint32_t w[40];
#pragma unroll
            for (int q = 0; q < 10; q++) {
                const uint4 v = e[q];
                w[4 * q] = v.x;
                w[4 * q + 1] = v.y;
                w[4 * q + 2] = v.z;
                w[4 * q + 3] = v.w;
            }
            ge_p3 P;
            pv_kr_base(P, w, true);  // the scan queues tables with PV_KF_AFF only
            pv_kr_build_run(
                DevBc2Row{reinterpret_cast<uint32_t*>(kw.wide_tab + (ws * PV_KR_POS + pos) * PV_KR_ENT * (PV_BCOMB_STRIDE / 4))},
                DevWideScr{kw.wide_scr + (uint64_t)blockIdx.x * PV_KR_RUN * 10 * PV_WIDE_THREADS + threadIdx.x}, P, run);
        }
        __threadfence();  // the rows before the bit that says they exist
        __syncthreads();
        if (threadIdx.x == 0) {
            kw.dir_wslot[slot] = (uint32_t)ws;
            kw.dir_flags[slot] |= PV_KF_WIDE;
            atomicAdd(&kw.dir_stat[5], 1ull);
        }
    }
}

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

// Kernel 3: encode Q for B requests per lane with one shared inversion, compare with R, one __ballot
// per request group. Wave w covers requests [64 B w, 64 B (w + 1)): lane l handles 64 B w + l + 64 t,
// t = 0..B-1, so every load is coalesced and group t's ballot is verdict word B w + t. Points are
// re-read from q rather than held. B is 16 or PV_ENC_SMALL_B = 8 (chunk_plan.h PV_ENC16_MIN has the A/Bs).
template <int B>
struct DevEncSrc {
    Soa q;
    uint32_t w, l;
    uint64_t n;
    __device__ __forceinline__ uint32_t req(int t) const {
        const uint32_t r = w * (64u * B) + l + 64 * t;
        return r < n ? r : 0;
    }
    __device__ __forceinline__ void z(int t, fe& o) const {
        const uint32_t r = req(t);
#pragma unroll
        for (int k = 0; k < 10; k++) o.v[k] = q.ld(20 + k, r);
    }
    __device__ __forceinline__ void xy(int t, fe& x, fe& y) const {
        const uint32_t r = req(t);
#pragma unroll
        for (int k = 0; k < 10; k++) {
            x.v[k] = q.ld(k, r);
            y.v[k] = q.ld(10 + k, r);
        }
    }
};
template <int B>
struct DevEncSink {
    const uint8_t* sm;
    const uint64_t* off;
    uint64_t* verdict;
    const uint32_t* slot_req;  // comb path: slot -> request (verdict words are then slot-ordered)
    uint32_t w, l;
    uint64_t n;
    __device__ __forceinline__ void operator()(int t, const uint32_t enc[8], bool use) const {
        const uint32_t r = w * (64u * B) + l + 64 * t;
        const uint32_t rr0 = r < n ? r : 0;
        const uint32_t rr = slot_req ? slot_req[rr0] : rr0;
        const uint64_t raddr = reinterpret_cast<uint64_t>(sm + off[rr]);
        const DevMsg mw{reinterpret_cast<const uint32_t*>(raddr & ~3ull), (uint32_t)(raddr & 3)};
        uint32_t R[8];
#pragma unroll
        for (int q = 0; q < 8; q++) R[q] = mw.dw(q);
        const bool ok = use && pv_words_equal(enc, R);
        const uint64_t bits = __ballot(ok);
        const uint32_t r0 = w * (64u * B) + 64 * t;
        if (l == 0 && r0 < n) verdict[r0 >> 6] = bits;
    }
};

template <int B>
__global__ __launch_bounds__(PV_BLOCK, 2) void pv_encode_kernel(const uint8_t* __restrict__ sm,
                                                                 const uint64_t* __restrict__ off, uint64_t n,
                                                                 Work wk, uint64_t* __restrict__ verdict,
                                                                 KeyWork kw, Gate gate) {
    if (gate.off()) return;
    const bool comb = gate.keyed();  // slot order
    const uint32_t g = blockIdx.x * PV_BLOCK + threadIdx.x;
    const uint32_t w = g >> 6, l = g & 63;
    const DevEncSrc<B> src{Soa(wk.q, 40, wk.stride), w, l, n};
    bool use[B];
#pragma unroll
    for (int t = 0; t < B; t++) {
        const uint32_t r = w * (64u * B) + l + 64 * t;
        use[t] = r < n && wk.flags[r < n ? r : 0] != 0;
    }
    pv_encode_batch_stream_b<B>(src, use, DevEncSink<B>{sm, off, comb ? kw.sverdict : verdict,
                                                        comb ? kw.slot_req : nullptr, w, l, n}, PvWaveInvert{});
}

// ------------------------------------------------------------------------------------------ host

// The device contexts and the calling thread's error string (pv_ctx.h).
Ctx g_ctxs[PV_MAX_DEV];
std::mutex g_mus[PV_MAX_DEV];
std::atomic<int> g_primary{-1};
thread_local int t_dev = -1;
thread_local std::string g_err;

namespace {

int ensure_events(int count) {
    while ((int)g_ctx.ev.size() < count) {
        hipEvent_t e;
        if (int rc = g_ctx.own.event(e, hipEventDefault)) return rc;
        g_ctx.ev.push_back(e);
    }
    return PV_OK;
}

static_assert(PV_FILL_ITEMS_PER_KEY == PV_COMB_POS * PV_COMB_BLOCKS, "chunk_plan.h: fill work items per key");
// bytes of one table's radix-2^11 rows in the wide pool
constexpr uint64_t PV_WIDE_TABLE_BYTES = (uint64_t)PV_KR_POS * PV_KR_ENT * PV_BCOMB_STRIDE * 4;

// One chunk's launch sequence: what its stages share. Every decision is in `p` (chunk_plan.h); the stages
// below enqueue what it names, record and wait on events, and keep the dirty flags in step with the enqueues.
struct ChunkLaunch {
    const pvhost::ChunkPlan& p;
    const KeyWork& kw;  // the context's, with the plan applied (apply_plan)
    Gate gate;
    const uint8_t* d_sm;
    const uint64_t* d_off;  // the chunk's first offset
    uint64_t m;
    const uint8_t* d_pk;  // the chunk's first key
    uint64_t* d_verdict;  // the chunk's first verdict word
    hipStream_t stream;
    hipEvent_t* e;  // the chunk's PV_NSTAGES + 1 timing events, or null
    int mark(int k) const {
        if (e) PV_HIP(hipEventRecord(e[k], stream), PV_ERR_LAUNCH);
        return PV_OK;
    }
};

// The plan's scalars into the chunk's KeyWork, and the pointers its lookup arrangement names: kcv / xtv are
// the probe's first and second view, kc_flags the flags of the first.
void apply_plan(const pvhost::ChunkPlan& p, KeyWork& kw, PvKeyCacheView& kcv, PvKeyCacheView& xtv,
                const uint32_t*& kc_flags) {
    const PvKeyCacheView xv{g_ctx.xt.htab, g_ctx.xt.keys, g_ctx.xt.flags, g_ctx.xt.tab, PV_XT_HASH - 1, g_ctx.kw.seed};
    const bool xt_only = p.lookup == pvhost::LOOKUP_XT_ONLY, xt_second = p.lookup == pvhost::LOOKUP_NODE_THEN_XT;
    xtv = xt_second ? xv : PvKeyCacheView{nullptr, nullptr, nullptr, nullptr, 0u, 0u};
    if (xt_only) kcv = xv;
    kc_flags = xt_only ? g_ctx.xt.flags : g_ctx.kc.d_flags;
    kw.kc_tab = xt_only ? g_ctx.xt.tab : g_ctx.kc.d_tab;
    kw.kc_ntab = xt_only ? nullptr : g_ctx.kc.d_ntab;
    kw.kc_wtab = xt_only ? nullptr : g_ctx.kc.d_wtab;
    kw.xt_flags = xt_second ? g_ctx.xt.flags : nullptr;
    kw.xt_tab = xt_second ? g_ctx.xt.tab : nullptr;
    kw.wide_tab = g_ctx.d_wide.as<uint4>();
    kw.wide_scr = g_ctx.d_wide_scr.as<uint32_t>();
    if (p.dense_only) kw.ctab = g_ctx.xt.tab;  // sub-batch 0 of a pipelined host call builds into the shared store
    kw.min_req = p.min_req;
    kw.kc_on = p.kc_on;
    kw.kc_wcap = p.kc_wcap;
    kw.dir_on = p.dir_on;
    kw.dir_cap = p.dir_cap;
    kw.dir_pub = p.dir_pub;
    kw.aff_conv = p.aff_conv;
    kw.wide_cap = p.wide_cap;
    kw.wide_conv = p.wide_conv;
    kw.chunk_n = p.chunk_n;
    kw.seg_cap = p.seg_cap;
    kw.lat_choice = p.lat_choice;
    kw.dense_only = p.dense_only;
    kw.kcap = p.kcap;
}

// The wide pool's allocation, when plan_wide_pool asks for it. A failure turns the feature off and is
// reported once through the error string; the chunk goes on without wide rows.
void wide_pool_attempt(uint64_t wide_want) {
    if (g_ctx.d_wide.grow(wide_want) != PV_OK ||
        g_ctx.d_wide_scr.grow((uint64_t)PV_WIDE_GRID * PV_KR_RUN * 10 * PV_WIDE_THREADS * 4) != PV_OK) {
        (void)hipGetLastError();  // clear the failed allocation's sticky error
        g_ctx.d_wide.release();
        g_ctx.d_wide_scr.release();
        g_ctx.wide_failed = true;
        (void)fail(PV_ERR_ALLOC, "wide rows of resident tables: no memory for the pool, the feature is off");
    }
}

// Key stage of a keyed chunk: the clears the dirty flags force, dedup (seed, insert, assign), the probe of
// the lookup views, the scan, the scatter on the main stream and the chain and fill on the key stream.
int launch_key_stage(const ChunkLaunch& L, const PvKeyCacheView& kcv, const PvKeyCacheView& xtv,
                     const uint32_t* kc_flags) {
    const pvhost::ChunkPlan& p = L.p;
    const KeyWork& kw = L.kw;
    hipStream_t stream = L.stream;
    if (p.clear_slots) {
        PV_HIP(hipMemsetAsync(kw.slot, 0xFF, (uint64_t)(kw.hmask + 1) * 4, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.slot_cnt, 0, (uint64_t)(kw.hmask + 1) * 4 * PV_RANK_SUB, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.need, 0, (uint64_t)PV_ALLCOMB_KEYS * PV_COMB_POS * 5 * 4, stream), PV_ERR_LAUNCH);
    }
    g_ctx.slots_dirty = true;  // until this chunk's unpermute kernel is enqueued
    if (p.clear_dir) {
        PV_HIP(hipMemsetAsync(kw.dir_htab, 0xFF, (uint64_t)PV_DIR_HASH * 4, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.dir_cnt, 0, 2 * 4, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.wide_cnt, 0, 2 * 4, stream), PV_ERR_LAUNCH);  // the pool empties with it
    }
    if (p.mark_dir_dirty) g_ctx.dir_dirty = true;  // until the chunk is enqueued whole
    // kw.nkeys is cleared by pv_key_insert_lds_kernel (m >= 1 here: the grid has a thread 0)
    if (p.seed_reqs) {
        PV_LAUNCH(pv_key_seed_kernel, dim3(pvhost::block_grid(p.seed_reqs)), dim3(PV_BLOCK), 0, stream, L.d_pk,
                  p.seed_reqs, kw);
    }
    PV_LAUNCH(pv_key_insert_lds_kernel, dim3(p.ins_grid), dim3(PV_INS_THREADS), 0, stream, L.d_pk, L.m, kw);
    PV_LAUNCH(pv_key_assign_kernel, dim3(p.req_grid), dim3(PV_BLOCK), 0, stream, L.m, kw);
    if (p.run_probe) {
        PvKeyCacheView dirv{kw.dir_htab, kw.dir_keys, kw.dir_flags, kw.ctab, p.dir_use ? PV_DIR_HASH - 1 : 0u, kw.seed};
        PV_LAUNCH(pv_key_cache_probe_kernel, dim3(p.probe_grid), dim3(PV_BLOCK), 0, stream, L.d_pk, kw, kcv, xtv, dirv);
    }
    // key-sorted slot order: comb keys' requests first, then the Straus requests
    PV_LAUNCH(pv_key_scan_kernel, dim3(1), dim3(PV_SCAN_THREADS), 0, stream, kw, kc_flags);
    // the per-key chain (few, long-latency lanes) and the table fill run on kstream, overlapped
    // with the scatter and the per-request prep on the main stream: the chain needs only the
    // scan's comb-key list (comb_key, comb_cslot), so kstream forks before the scatter
    PV_HIP(hipEventRecord(g_ctx.ev_scan_done, stream), PV_ERR_LAUNCH);
    PV_HIP(hipStreamWaitEvent(g_ctx.kstream, g_ctx.ev_scan_done, 0), PV_ERR_LAUNCH);
    PV_LAUNCH(pv_key_scatter_kernel, dim3(p.req_grid), dim3(PV_BLOCK), 0, stream, L.m, kw);
    PV_HIP(hipEventRecord(g_ctx.ev_keys_ready, stream), PV_ERR_LAUNCH);
    // one chain launch over all positions, then the fill. direct_fill: back to back on kstream
    // and the tables-ready event right after the fill (no event hop to fstream, no gated
    // sparse-fill launch in the dependency chain of the comb kernel). Otherwise the fill runs on
    // fstream, where the sparse fill follows it (launch_comb_stage).
    hipStream_t fs = p.direct_fill ? g_ctx.kstream : g_ctx.fstream;
    PV_LAUNCH(pv_key_chain_lp_kernel, dim3(p.chain_blocks), dim3(64), 0, g_ctx.kstream, L.d_pk, kw, L.gate, 0,
              PV_COMB_POS);
    if (!p.direct_fill) {
        PV_HIP(hipEventRecord(g_ctx.ev_chain, g_ctx.kstream), PV_ERR_LAUNCH);
        PV_HIP(hipStreamWaitEvent(fs, g_ctx.ev_chain, 0), PV_ERR_LAUNCH);
    }
    PV_LAUNCH(pv_key_fill_kernel, dim3(p.fill_grid), dim3(PV_BLOCK), 0, fs, kw, L.gate, 0, PV_COMB_POS);
    if (p.direct_fill) PV_HIP(hipEventRecord(g_ctx.ev_tables_ready, g_ctx.kstream), PV_ERR_LAUNCH);
    return PV_OK;
}

// The Straus-path slots of a split chunk (keys without a table: usually a few thousand one-off requests)
// run on their own stream beside the comb kernels: their waves take ~1 ms from start to end however few
// they are, which on the main stream would delay the whole comb path. Their blocks are dispatched from
// the END of the slot range (where the Straus slots are), and blocks of comb slots exit at once.
int launch_straus_side(const ChunkLaunch& L) {
    hipStream_t ss = g_ctx.sstream;
    const dim3 grid(L.p.side_grid), block(PV_BLOCK);
    PV_HIP(hipStreamWaitEvent(ss, g_ctx.ev_keys_ready, 0), PV_ERR_LAUNCH);
    PV_LAUNCH_BC2(pv_prep_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    PV_LAUNCH_BC2(pv_split_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, g_ctx.work, L.gate);
    PV_LAUNCH(pv_table_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    PV_LAUNCH_BC2(pv_msm_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, g_ctx.d_btab, g_ctx.work, g_ctx.d_bc2,
                  L.gate);
    PV_HIP(hipEventRecord(g_ctx.ev_straus_done, ss), PV_ERR_LAUNCH);
    return PV_OK;
}

// Comb stage of a keyed chunk on the main stream: the per-request prep and digits while the key stream
// builds the tables, then [S]B + [k](-A) once they are ready, then the join with the Straus side.
int launch_comb_stage(const ChunkLaunch& L) {
    const pvhost::ChunkPlan& p = L.p;
    const KeyWork& kw = L.kw;
    hipStream_t stream = L.stream;
    const dim3 grid(p.req_grid), block(PV_BLOCK);
    int rc;
    PV_LAUNCH_BC2(pv_comb_prep_req_kernel, grid, block, g_ctx.prep_lds_pad, stream, L.d_sm, L.d_off, L.m, L.d_pk,
                  g_ctx.work, kw, L.gate);
    if (!p.direct_fill) {
        // a small chunk's sparse table fill (needs the chain's bases and the need masks comb_prep
        // writes) runs on fstream after the full fill; for a large chunk it exits at once
        PV_HIP(hipEventRecord(g_ctx.ev_prep_done, stream), PV_ERR_LAUNCH);
        PV_HIP(hipStreamWaitEvent(g_ctx.fstream, g_ctx.ev_prep_done, 0), PV_ERR_LAUNCH);
        PV_LAUNCH(pv_key_fill_sparse_kernel, dim3(PV_ALLCOMB_KEYS * PV_COMB_POS / PV_BLOCK), block, 0, g_ctx.fstream,
                  kw, L.gate);
        PV_HIP(hipEventRecord(g_ctx.ev_tables_ready, g_ctx.fstream), PV_ERR_LAUNCH);
    }
    // the per-request results to slot-ordered rows, while the key stream finishes the tables
    PV_LAUNCH_BC2(pv_comb_digits_kernel, grid, block, 0, stream, g_ctx.work, kw, L.gate);
    if ((rc = L.mark(PV_STAGE_TABLE))) return rc;
    if (!p.fused)  // [S]B while the key stream finishes the tables, then join
        PV_LAUNCH_BC2(pv_comb_b_kernel, grid, block, 0, stream, L.m, g_ctx.work, kw, g_ctx.d_bc2, L.gate);
    PV_HIP(hipStreamWaitEvent(stream, g_ctx.ev_tables_ready, 0), PV_ERR_LAUNCH);
    if ((rc = L.mark(PV_STAGE_MSM))) return rc;
    if (p.fused)  // [S]B + [k](-A) in one kernel as soon as the tables are built
        PV_LAUNCH_BC2(pv_comb_ab_kernel, grid, block, 0, stream, L.m, g_ctx.work, kw, g_ctx.d_bc2, L.gate);
    else
        PV_LAUNCH(pv_comb_a_kernel, grid, block, 0, stream, L.m, g_ctx.work, kw, L.gate);
    PV_HIP(hipStreamWaitEvent(stream, g_ctx.ev_straus_done, 0), PV_ERR_LAUNCH);
    return PV_OK;
}

// A chunk with no key kernels: every request on the Straus path, on the main stream.
int launch_straus_only(const ChunkLaunch& L) {
    hipStream_t stream = L.stream;
    const dim3 grid(L.p.req_grid), block(PV_BLOCK);
    int rc;
    PV_LAUNCH_BC2(pv_prep_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    PV_LAUNCH_BC2(pv_split_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, g_ctx.work, L.gate);
    if ((rc = L.mark(PV_STAGE_TABLE))) return rc;
    PV_LAUNCH(pv_table_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    if ((rc = L.mark(PV_STAGE_MSM))) return rc;
    PV_LAUNCH_BC2(pv_msm_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, g_ctx.d_btab, g_ctx.work, g_ctx.d_bc2,
                  L.gate);
    return PV_OK;
}

// Epilogue: the encode; for a keyed chunk the verdicts back to request order, the publishes and conversions
// for the chunks that follow, and the latency launch of a device-side choice.
int launch_epilogue(const ChunkLaunch& L) {
    const pvhost::ChunkPlan& p = L.p;
    const KeyWork& kw = L.kw;
    hipStream_t stream = L.stream;
    if (p.enc16)
        PV_LAUNCH(pv_encode_kernel<16>, dim3(p.enc_grid), dim3(PV_BLOCK), 0, stream, L.d_sm, L.d_off, L.m, g_ctx.work,
                  L.d_verdict, kw, L.gate);
    else
        PV_LAUNCH(pv_encode_kernel<PV_ENC_SMALL_B>, dim3(p.enc_grid), dim3(PV_BLOCK), 0, stream, L.d_sm, L.d_off, L.m,
                  g_ctx.work, L.d_verdict, kw, L.gate);
    if (!p.keyed) return PV_OK;
    PV_LAUNCH(pv_unpermute_kernel, dim3(p.req_grid), dim3(PV_BLOCK), 0, stream, L.m, kw, L.d_verdict, L.gate);
    g_ctx.slots_dirty = false;
    if (p.run_xtab_publish)
        PV_LAUNCH(pv_xtab_publish_kernel, dim3(PV_XT_KEYS / PV_BLOCK), dim3(PV_BLOCK), 0, stream, L.d_pk, kw,
                  g_ctx.xt.htab, PV_XT_HASH - 1, g_ctx.kw.seed, g_ctx.xt.keys, g_ctx.xt.flags);
    if (p.run_dir_publish)
        PV_LAUNCH(pv_dir_publish_kernel, dim3(p.pub_grid), dim3(PV_BLOCK), 0, stream, L.d_pk, kw);
    if (p.run_affine) PV_LAUNCH(pv_dir_affine_kernel, dim3(PV_AFF_CAP), dim3(PV_AFF_THREADS), 0, stream, kw);
    if (p.run_widen) PV_LAUNCH(pv_dir_widen_kernel, dim3(PV_WIDE_GRID), dim3(PV_WIDE_THREADS), 0, stream, kw);
    if (p.dir_use) g_ctx.dir_dirty = false;
    if (p.run_dev_latency)  // the words were zeroed by the unpermute kernel
        return pv_latency_launch(L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.d_bcomb, kc_view(), L.d_verdict, true, stream,
                                 kw.nkeys + PV_SPLIT_LAT);
    return PV_OK;
}

// Chunk c of the batch on `stream` (the workspace is the context's; key / fill / side streams join it):
// plan (chunk_plan.h), apply, launch.
int launch_chunk(int c, uint64_t n, const uint8_t* d_sm, const uint64_t* d_off, const uint8_t* d_pk,
                 uint64_t* d_verdict, hipStream_t stream, const pvhost::BatchPlan& batch, int evb) {
    constexpr int NE = PV_NSTAGES + 1;
    const uint64_t cap = g_ctx.work.stride;
    const uint64_t c0 = (uint64_t)c * cap;
    const uint64_t m = std::min<uint64_t>(cap, n - c0);
    pvhost::ChunkPlan p;
    KeyWork kw = g_ctx.kw;
    ChunkLaunch L{p, kw, Gate{nullptr, nullptr}, d_sm, d_off + c0, m, d_pk + 32 * c0, d_verdict + c0 / 64, stream,
                  g_ctx.timing ? &g_ctx.ev[evb + NE * c] : nullptr};
    int rc = L.mark(PV_STAGE_KEYS);
    if (rc) return rc;
    if (batch.latency) {
        // one kernel: every stage of the verification inside it (timed as MSM)
        g_ctx.last_keyed = false;
        for (int k = PV_STAGE_PREP; k <= PV_STAGE_MSM; k++)
            if ((rc = L.mark(k))) return rc;
        rc = pv_latency_launch(d_sm, L.d_off, m, L.d_pk, g_ctx.d_bcomb, kc_view(), L.d_verdict, g_ctx.verdict_zeroed,
                               stream, nullptr);
        if (rc) return rc;
        if ((rc = L.mark(PV_STAGE_ENCODE)) || (rc = L.mark(PV_NSTAGES))) return rc;
        return PV_OK;
    }
    PvKeyCacheView kcv = kc_view(), xtv;
    pvhost::ChunkFacts f{};
    f.m = m;
    f.path = g_ctx.path;
    f.keyed_hint = g_ctx.keyed_hint;
    f.node_kc = kcv.hmask != 0;
    f.kc_wcap = g_ctx.kc.wcap;
    f.xt_use = g_ctx.xt_use;
    f.xt_fill = g_ctx.xt_fill;
    f.dir_on = g_ctx.dir_on;
    f.dir_cap = g_ctx.dir_cap;
    f.aff_on = g_ctx.aff_on;
    f.wide_cap = g_ctx.wide_cap;
    f.kcap = g_ctx.kw.kcap;
    f.cus = g_ctx.cus;
    f.slots_dirty = g_ctx.slots_dirty;
    f.dir_dirty = g_ctx.dir_dirty;
    const bool keyed = pvhost::chunk_keyed(batch, f);
    g_ctx.last_keyed = keyed;
    if (keyed) g_ctx.last_nkeys = g_ctx.kw.nkeys;
    const uint64_t wide_want = (uint64_t)g_ctx.wide_cap * PV_WIDE_TABLE_BYTES;
    const pvhost::WideTrigger wt = pvhost::plan_wide_pool(keyed, pvhost::chunk_dir_pub(f), g_ctx.wide_failed,
                                                         g_ctx.d_wide.cap, wide_want, g_ctx.wide_dense);
    g_ctx.wide_dense = wt.dense;
    if (wt.attempt) wide_pool_attempt(wide_want);
    f.wide_have = g_ctx.d_wide.cap / PV_WIDE_TABLE_BYTES;
    p = pvhost::plan_chunk(batch, f);
    const uint32_t* kc_flags;
    apply_plan(p, kw, kcv, xtv, kc_flags);
    if (p.keyed) {
        L.gate = Gate{kw.nkeys, kw.slot_req};
        if ((rc = launch_key_stage(L, kcv, xtv, kc_flags))) return rc;
    }
    if ((rc = L.mark(PV_STAGE_PREP))) return rc;
    if (p.keyed) {
        if ((rc = launch_straus_side(L)) || (rc = launch_comb_stage(L))) return rc;
    } else {
        if ((rc = launch_straus_only(L))) return rc;
    }
    if ((rc = L.mark(PV_STAGE_ENCODE))) return rc;
    if ((rc = launch_epilogue(L))) return rc;
    return L.mark(PV_NSTAGES);
}

int launch_chunks(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk, uint64_t* d_verdict,
                  hipStream_t stream) {
    const uint64_t cap = g_ctx.work.stride;
    const int nchunks = (int)((n + cap - 1) / cap);
    constexpr int NE = PV_NSTAGES + 1;
    const pvhost::BatchPlan batch =
        pvhost::plan_batch({g_ctx.path, n, g_ctx.hint_set, g_ctx.keyed_hint, kc_view().hmask != 0});
    g_ctx.last_latency = batch.latency;
    g_ctx.last_dev_choice = batch.dev_choice;
    int evb = 0;
    if (g_ctx.timing) {
        evb = g_ctx.ev_used;
        int rc = ensure_events(evb + NE * nchunks);
        if (rc) return rc;
        g_ctx.ev_used = evb + NE * nchunks;
    }
    int rc = PV_OK;
    for (int c = 0; c < nchunks && rc == PV_OK; c++)
        rc = launch_chunk(c, n, d_sm, d_off, d_pk, d_verdict, stream, batch, evb);
    return rc;
}

// The per-lane workspace: per-request rows (Work) and the keyed path's tables (KeyWork), ~15 GB, owned
// by the context (Work::qb is never allocated: it only keeps the kernel-argument layout).
int lane_alloc_buffers(Work& w, KeyWork& kw) {
    PvOwner& own = g_ctx.own;
    const uint64_t S = PV_CHUNK;
    w.stride = S;
    if (int rc = own.dev(w.atab, S * PV_ATAB_ENT * 160)) return rc;
    if (int rc = own.dev(w.digits, S * PV_DIGIT_ROWS * 4)) return rc;
    if (int rc = own.dev(w.flags, S * 4)) return rc;
    if (int rc = own.dev(w.q, S * 40 * 4)) return rc;
    if (int rc = own.dev(w.aos, S * PV_PREP_AOS_QMAX * 16)) return rc;
    const uint64_t H = 2 * S;
    kw.hmask = (uint32_t)(H - 1);
    kw.kcap = PV_KEY_CAP;
    kw.seed = (uint32_t)std::random_device{}() | 1u;
    if (int rc = own.dev(kw.slot, H * 4)) return rc;
    if (int rc = own.dev(kw.slot_id, H * 4)) return rc;
    if (int rc = own.dev(kw.slot_cnt, H * 4 * PV_RANK_SUB)) return rc;
    if (int rc = own.dev(kw.req_key, S * 4)) return rc;
    if (int rc = own.dev(kw.req_rank, S * 4)) return rc;
    if (int rc = own.dev(kw.nkeys, PV_SPLIT_ALLOC_WORDS * 4)) return rc;
    if (int rc = own.dev(kw.key_owner, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.key_cid, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.comb_key, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.key_flag, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.bases, (uint64_t)kw.kcap * PV_COMB_POS * PV_COMB_PTS * 160)) return rc;
    if (int rc = own.dev(kw.ctab, (uint64_t)kw.kcap * PV_COMB_POS * PV_COMB_ENT * 160)) return rc;
    if (int rc = own.dev(kw.key_count, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.key_cursor, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.slot_req, S * 4)) return rc;
    if (int rc = own.dev(kw.req_pos, S * 4)) return rc;
    if (int rc = own.dev(kw.skey, S * 4)) return rc;
    if (int rc = own.dev(kw.sverdict, S / 64 * 8)) return rc;
    if (int rc = own.dev(kw.key_cslot, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.comb_cslot, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.need, (uint64_t)PV_ALLCOMB_KEYS * PV_COMB_POS * 5 * 4)) return rc;
    PV_HIP(hipMemset(kw.comb_cslot, 0xFF, (uint64_t)kw.kcap * 4), PV_ERR_ALLOC);
    if (int rc = own.dev(kw.comb_tslot, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.dir_htab, (uint64_t)PV_DIR_HASH * 4)) return rc;
    if (int rc = own.dev(kw.dir_keys, (uint64_t)kw.kcap * 32)) return rc;
    if (int rc = own.dev(kw.dir_flags, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.dir_cnt, 2 * 4)) return rc;
    if (int rc = own.dev(kw.dir_stat, PV_DIR_STATS * 8)) return rc;
    if (int rc = own.dev(kw.aff_list, (uint64_t)PV_AFF_CAP * 4)) return rc;
    if (int rc = own.dev(kw.aff_cnt, 4)) return rc;
    if (int rc = own.dev(kw.wide_list, (uint64_t)PV_WIDE_CAP * 2 * 4)) return rc;
    if (int rc = own.dev(kw.wide_cnt, 2 * 4)) return rc;
    if (int rc = own.dev(kw.dir_wslot, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.comb_wslot, (uint64_t)kw.kcap * 4)) return rc;
    PV_HIP(hipMemset(kw.wide_cnt, 0, 2 * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.comb_wslot, 0xFF, (uint64_t)kw.kcap * 4), PV_ERR_ALLOC);
    if (int rc = own.dev(kw.aff_scr, (uint64_t)PV_AFF_CAP * PV_AFF_SEG * 10 * PV_AFF_THREADS * 4)) return rc;
    PV_HIP(hipMemset(kw.aff_cnt, 0, 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.comb_tslot, 0, (uint64_t)kw.kcap * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.dir_htab, 0xFF, (uint64_t)PV_DIR_HASH * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.dir_cnt, 0, 2 * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.dir_stat, 0, PV_DIR_STATS * 8), PV_ERR_ALLOC);
    return PV_OK;
}

// Builds g_ctxs[device] (caller: g_mus[device] held, DevScope(device) active, context not built yet):
// streams and events, the fixed-base tables, the workspace. Sets the calling thread's HIP device.
bool env_flag_devscope() {
    const char* e = getenv("PV_EVENT_DEVSCOPE");
    return !(e && *e == '0');
}

int ctx_init_parts(int device) {
    PV_HIP(hipSetDevice(device), PV_ERR_NO_DEVICE);
    hipDeviceProp_t prop;
    PV_HIP(hipGetDeviceProperties(&prop, device), PV_ERR_NO_DEVICE);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PV_ERR_NO_DEVICE, std::string("pv_init: built for gfx950, device is ") + prop.gcnArchName);
    g_ctx.cus = prop.multiProcessorCount;
    PvOwner& own = g_ctx.own;
    if (int rc = own.stream(g_ctx.stream, hipStreamNonBlocking)) return rc;
    if (int rc = own.stream(g_ctx.kstream, hipStreamNonBlocking)) return rc;
    // stream-to-stream hand-overs inside the engine (one device, never read by the host) are recorded with
    // a device-scope release instead of the default system-scope fence: headline step 2.612-2.618 against
    // 2.620-2.624 ms interleaved (profiles/r05/ab_event_devscope.txt); PV_EVENT_DEVSCOPE=0 restores it
    const unsigned evf = hipEventDisableTiming | (env_flag_devscope() ? hipEventReleaseToDevice : 0u);
    if (int rc = own.event(g_ctx.ev_keys_ready, evf)) return rc;
    if (int rc = own.event(g_ctx.ev_scan_done, evf)) return rc;
    if (int rc = own.event(g_ctx.ev_tables_ready, evf)) return rc;
    if (int rc = own.stream(g_ctx.fstream, hipStreamNonBlocking)) return rc;
    if (int rc = own.event(g_ctx.ev_chain, evf)) return rc;
    if (int rc = own.event(g_ctx.ev_prep_done, evf)) return rc;
    if (int rc = own.stream(g_ctx.sstream, hipStreamNonBlocking)) return rc;
    if (int rc = own.event(g_ctx.ev_straus_done, evf)) return rc;
    if (int rc = g_ctx.hand.ensure()) return rc;
    {
        // the host path's copy stream at the greatest priority: the runtime keeps such streams on hardware
        // queues of their own instead of round-robin over GPU_MAX_HW_QUEUES (4) with the engine's streams,
        // where a copy sat behind the key stream's table fill (profiles/r05/host_path)
        int least = 0, greatest = 0;
        PV_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest), PV_ERR_NO_DEVICE);
        const char* pe = getenv("PV_CSTREAM_PRIO");  // A/B knob: 0 = normal priority
        const bool hi = !(pe && *pe == '0');
        if (int rc = own.stream(g_ctx.cstream, hipStreamNonBlocking, hi ? greatest : least)) return rc;
    }
    if (int rc = own.event(g_ctx.ev_cstart, hipEventDisableTiming)) return rc;
    std::vector<uint32_t> bt(PV_BTAB_ENTRIES * PV_BTAB_STRIDE);
    pv_build_b_table(bt.data());
    if (int rc = own.dev(g_ctx.d_btab, bt.size() * 4)) return rc;
    PV_HIP(hipMemcpy(g_ctx.d_btab, bt.data(), bt.size() * 4, hipMemcpyHostToDevice), PV_ERR_ALLOC);
    {
        if (int rc = lane_alloc_buffers(g_ctx.work, g_ctx.kw)) return rc;
        std::vector<uint32_t> bc((size_t)PV_BCOMB_POS * PV_BCOMB_ENT * PV_BCOMB_STRIDE);
        {
            ge_p3 base[PV_BCOMB_POS];
            pv_bcomb_bases(base);
            std::vector<std::thread> th;
            for (int j = 0; j < PV_BCOMB_POS; j++)
                th.emplace_back(pv_bcomb_build_position, bc.data() + (size_t)j * PV_BCOMB_ENT * PV_BCOMB_STRIDE,
                                std::cref(base[j]));
            for (auto& t : th) t.join();
        }
        if (int rc = own.dev(g_ctx.d_bcomb, bc.size() * 4)) return rc;
        PV_HIP(hipMemcpy(g_ctx.d_bcomb, bc.data(), bc.size() * 4, hipMemcpyHostToDevice), PV_ERR_ALLOC);
        // the wide fixed-base comb, built on the device row by row (one scratch row of Z products)
        {
            const uint64_t rows_ent = (uint64_t)(PV_BC2_POS - 1) * PV_BC2_ENT + PV_BC2_TOP_ENT;
            // not enough HBM for the wide table (a smaller part, several processes on one GPU) or
            // PV_FORCE_BCOMB16 set: [S]B from the radix-65536 comb T_B instead (16 lookups instead of
            // 11, same verdicts; profiles/r02/ab_bcomb_radix.txt: ~2 % slower per step)
            const char* force16 = getenv("PV_FORCE_BCOMB16");
            if (PV_BC2_W == 16 || (force16 && *force16 && *force16 != '0') ||
                own.dev(g_ctx.d_bc2, rows_ent * PV_BCOMB_STRIDE * 4) != PV_OK) {
                (void)hipGetLastError();  // clear a failed allocation's sticky error
                g_ctx.d_bc2 = g_ctx.d_bcomb;  // an alias: the owner holds the one block
                g_ctx.bc2_w = 16;
            }
        }
        if (g_ctx.bc2_w != 16) {
            uint32_t* scratch = nullptr;
            PV_HIP(hipMalloc((void**)&scratch, (uint64_t)PV_BC2_ENT * 40), PV_ERR_ALLOC);
            ge_p3 negB, P;
            ge_frombytes_negate(negB, PV_B_ENC);
            P = negB;
            fe z;
            fe_0(z);
            fe_sub(P.X, z, negB.X);
            fe_carry(P.X, P.X);
            fe_sub(P.T, z, negB.T);
            fe_carry(P.T, P.T);
            int rc = PV_OK;
            for (int j = 0; j < PV_BC2_POS && rc == PV_OK; j++) {
                PvPoint40 arg;
                for (int q = 0; q < 10; q++) {
                    arg.w[q] = P.X.v[q];
                    arg.w[10 + q] = P.Y.v[q];
                    arg.w[20 + q] = P.Z.v[q];
                    arg.w[30 + q] = P.T.v[q];
                }
                const uint32_t ent = j + 1 < PV_BC2_POS ? PV_BC2_ENT : PV_BC2_TOP_ENT;
                const uint32_t threads = (ent + PV_BC2_RUN - 1) / PV_BC2_RUN;
                hipLaunchKernelGGL(pv_bc2_build_kernel, dim3((threads + PV_BLOCK - 1) / PV_BLOCK), dim3(PV_BLOCK), 0,
                                   g_ctx.stream, g_ctx.d_bc2 + (uint64_t)j * PV_BC2_ENT * (PV_BCOMB_STRIDE / 4), ent,
                                   arg, scratch);
                if (hipGetLastError() != hipSuccess || hipStreamSynchronize(g_ctx.stream) != hipSuccess)
                    rc = fail(PV_ERR_LAUNCH, "pv_init: wide fixed-base comb build failed");
                for (int r = 0; r < PV_BC2_W; r++) {  // next row's base: 2^W P
                    ge_p1p1 t;
                    ge_p2_dbl(t, P.X, P.Y, P.Z);
                    ge_p1p1_to_p3(P, t);
                }
            }
            (void)hipFree(scratch);
            if (rc != PV_OK) return rc;
        }
    }
    if (int rc = own.pinned(g_ctx.h_zc_verdict, PV_ZC_MAX_REQ, hipHostMallocCoherent | hipHostMallocPortable)) return rc;
    if (const char* pad = getenv("PV_PREP_LDS_PAD")) g_ctx.prep_lds_pad = (uint32_t)atoi(pad);  // A/B knob
    {  // PV_TABLE_REUSE=0: start with table reuse off (pv_table_reuse), every keyed chunk builds its tables
        const char* tr = getenv("PV_TABLE_REUSE");
        g_ctx.dir_on = !(tr && *tr == '0');
        g_ctx.dir_cap = PV_DIR_DEFAULT_CAP;
        g_ctx.dir_dirty = true;
        const char* ta = getenv("PV_TABLE_AFFINE");  // PV_TABLE_AFFINE=0: resident tables stay in cached form
        g_ctx.aff_on = !(ta && *ta == '0');
        const char* tw = getenv("PV_TABLE_WIDE");  // PV_TABLE_WIDE=0: resident tables get no radix-2^11 rows
        g_ctx.wide_cap = tw && *tw == '0' ? 0u : PV_WIDE_DEFAULT;
    }
    g_ctx.device = device;
    return PV_OK;
}

// Frees g_ctxs[t_dev or primary] (caller holds its mutex).
void ctx_free() {
    if (g_ctx.device < 0) return;
    (void)hipSetDevice(g_ctx.device);
    if (g_ctx.comm) ncclCommDestroy(g_ctx.comm);
    kc_free();  // first: it waits for a pending asynchronous put
    for (PvDevBuf* b : {&g_ctx.d_mg, &g_ctx.d_stage, &g_ctx.sg.d_keys, &g_ctx.sg.d_sk, &g_ctx.d_wide, &g_ctx.d_wide_scr})
        b->release();
    for (PvPinnedBuf* b : {&g_ctx.h_mg, &g_ctx.h_stage, &g_ctx.h_ver, &g_ctx.sg.h_sk}) b->release();
    g_ctx.sg.stage.release();
    g_ctx.hand.destroy();
    g_ctx.sg.hand.destroy();
    g_ctx.own.release_all();
    g_ctx = Ctx();
}

}  // namespace

// What the engine's other translation units call (declared in pv_ctx.h).

// Builds the tables of a put's fresh keys (slot PV_KC_EMPTY = evicted again within the same put) into
// their cache slots, in batches of the workspace's comb capacity. async: one batch only (the caller caps
// the keys), staged through the pinned h_async area and left running on the engine stream (the
// next launch is stream-ordered after it). PV_TEST_FAIL_KC_PUT_BATCH=b (tests only) reports a
// failure after batch b has been enqueued, to exercise the rollback.
int kc_build_tables(const pvhost::KcIndex::Assigned& put, bool async) {
    auto& k = g_ctx.kc;
    hipStream_t s = g_ctx.stream;
    if (int rc = g_ctx.hand.begin(s)) return rc;
    const char* fail_env = getenv("PV_TEST_FAIL_KC_PUT_BATCH");
    const long fail_batch = fail_env ? atol(fail_env) : -1;
    KeyWork kw = g_ctx.kw;
    // the put builds comb index j's table in slot j of a scratch area: the part of ctab above the slots
    // the resident-table directory may list when the batch fits there, else over the directory
    constexpr uint64_t tab_q = (uint64_t)PV_COMB_POS * PV_COMB_ENT * 10;  // uint4 per table
    uint4* const scratch_tab = g_ctx.kw.ctab + g_ctx.dir_cap * tab_q;
    const uint32_t scratch_keys = kw.kcap - g_ctx.dir_cap;
    std::vector<uint8_t> lpk;
    std::vector<uint32_t> lslot;
    long batch = 0;
    for (size_t f0 = 0; f0 < put.fresh.size();) {
        uint8_t* bpk;
        uint32_t* bslot;
        if (async) {  // pinned: keys [kcap][32], then slots [kcap]
            bpk = k.h_async;
            bslot = reinterpret_cast<uint32_t*>(k.h_async + (uint64_t)kw.kcap * 32);
        } else {
            lpk.resize((uint64_t)kw.kcap * 32);
            lslot.resize(kw.kcap);
            bpk = lpk.data();
            bslot = lslot.data();
        }
        uint32_t m;
        f0 = pvhost::KcIndex::pack(put, f0, kw.kcap, bpk, bslot, m);
        if (m == 0) continue;
        if (async && f0 < put.fresh.size()) return fail(PV_ERR_ARG, "kc_build_tables: asynchronous put above one batch");
        if (g_ctx.dir_on && m <= scratch_keys) {
            kw.ctab = scratch_tab;
        } else {
            kw.ctab = g_ctx.kw.ctab;
            g_ctx.dir_dirty = true;
        }
        PV_HIP(hipMemcpyAsync(k.d_put_pk, bpk, 32ull * m, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
        PV_HIP(hipMemcpyAsync(k.d_put_slot, bslot, (uint64_t)m * 4, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
        PV_LAUNCH(pv_kc_put_prep_kernel, dim3((m + PV_BLOCK - 1) / PV_BLOCK), dim3(PV_BLOCK), 0, s, kw, m);
        const Gate gate{kw.nkeys, kw.slot_req};
        PV_LAUNCH(pv_key_chain_lp_kernel, dim3(pvhost::chain_blocks(m)), dim3(64), 0, s, k.d_put_pk, kw, gate, 0,
                  PV_COMB_POS);
        PV_LAUNCH(pv_key_fill_kernel, dim3(pvhost::fill_grid(m)), dim3(PV_BLOCK), 0, s, kw, gate, 0, PV_COMB_POS);
        PV_LAUNCH(pv_kc_scatter_kernel, dim3(64, m), dim3(PV_BLOCK), 0, s, kw.ctab, kw.key_flag, k.d_put_pk,
                  k.d_put_slot, m, k.d_tab, k.d_flags, k.d_keys);
        if (k.d_ntab) {
            PV_LAUNCH(pv_kc_affine_kernel, dim3((m * PV_COMB_POS + 63) / 64), dim3(64), 0, s, k.d_tab,
                      k.d_put_slot, m, k.d_ntab);
        }
        if (k.d_wtab) {
            bool any = false;
            for (uint32_t j = 0; j < m && !any; j++) any = bslot[j] < k.wcap;
            for (uint32_t j0 = 0; any && j0 < m; j0 += PV_KW_GROUP) {
                const uint32_t g = std::min<uint32_t>(PV_KW_GROUP, m - j0);
                const uint64_t threads = (uint64_t)g * PV_KW_POS * PV_KW_RUNS;
                PV_LAUNCH(pv_kc_wide_kernel, dim3((unsigned)((threads + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK),
                          0, s, kw, k.d_put_slot, j0, g, k.wcap, k.d_wtab, k.d_wscr);
            }
        }
        if (!async) PV_HIP(hipStreamSynchronize(s), PV_ERR_LAUNCH);  // bpk / bslot are host locals
        if (batch++ == fail_batch) return fail(PV_ERR_LAUNCH, "pv_key_cache_put: injected failure (PV_TEST_FAIL_KC_PUT_BATCH)");
    }
    return PV_OK;
}

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// One batch on `stream` (caller holds g_mu). Chunks of at most work.stride requests (a multiple of
// 64, so verdict words never straddle).
int launch(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk, uint64_t* d_verdict,
           hipStream_t stream) {
    if (n == 0) return PV_OK;
    int rc = g_ctx.hand.begin(stream);
    if (rc) return rc;
    rc = launch_chunks(d_sm, d_off, n, d_pk, d_verdict, stream);
    // recorded even after a failed enqueue: whatever did get enqueued is covered
    if (int rc2 = g_ctx.hand.end(stream)) return rc2;
    return rc;
}

int check_device_index(int device, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(PV_ERR_NO_DEVICE, std::string(who) + ": no HIP device visible");
    if (device < 0 || device >= ndev || device >= PV_MAX_DEV)
        return fail(PV_ERR_ARG, std::string(who) + ": device index out of range");
    return PV_OK;
}

// ctx_init_parts, and on failure everything it had built is released (streams, events, the workspace,
// the tables): a retry of pv_init / pv_init_devices starts from an empty context instead of allocating
// ~25 GB on top of a half-built one.
int ctx_init(int device) {
    const int rc = ctx_init_parts(device);
    if (rc != PV_OK) {
        const std::string err = g_err;
        g_ctx.device = device;  // ctx_free releases a context of a known device
        ctx_free();
        g_err = err;
    }
    return rc;
}

hipStream_t pv_engine_stream() { return g_ctx.stream; }
int pv_fail(int code, const std::string& msg) { return fail(code, msg); }

extern "C" {

int pv_abi_version(void) { return PV_ABI_VERSION; }
uint32_t pv_build_flags(void) { return PV_BUILD_COMB_FUSED; }

int pv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* pv_last_error(void) { return g_err.c_str(); }

int pv_init(int device) {
    const int p = g_primary.load();
    if (p == device) {
        PV_HIP(hipSetDevice(device), PV_ERR_NO_DEVICE);  // this thread's device as well
        return PV_OK;
    }
    if (p >= 0) return fail(PV_ERR_ARG, "pv_init: already bound to another device");
    int rc = check_device_index(device, "pv_init");
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mus[device]);
        DevScope ds(device);
        if (g_ctx.device != device && (rc = ctx_init(device)) != PV_OK) return rc;
    }
    PV_HIP(hipSetDevice(device), PV_ERR_NO_DEVICE);
    g_primary.store(device);
    return PV_OK;
}

void pv_shutdown(void) {
    pinned_cache_drain();  // freed pv_host_alloc blocks back to the system (live ones stay the caller's)
    pv_ingress_shutdown();
    pv_merkle_shutdown();
    pv_trie_shutdown();
    {
        std::lock_guard<std::mutex> lk(g_mg_mu);
        mg_destroy_comms();
    }
    for (int d = 0; d < PV_MAX_DEV; d++) {
        std::lock_guard<std::mutex> lk(g_mus[d]);
        DevScope ds(d);
        ctx_free();
    }
    const int p = g_primary.exchange(-1);
    if (p >= 0) (void)hipSetDevice(p);
}

int pv_last_path(int* path, uint32_t* nkeys) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_last_path: call pv_init first");
    uint32_t u[PV_SPLIT_WORDS] = {};
    if (g_ctx.last_keyed) {
        PV_HIP(hipStreamSynchronize(g_ctx.stream), PV_ERR_LAUNCH);
        PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
        PV_HIP(hipMemcpy(u, g_ctx.last_nkeys ? g_ctx.last_nkeys : g_ctx.kw.nkeys, sizeof(u), hipMemcpyDeviceToHost),
               PV_ERR_LAUNCH);
    }
    if (nkeys) *nkeys = u[PV_SPLIT_KEYS];
    const bool lat = g_ctx.last_latency || (g_ctx.last_keyed && u[PV_SPLIT_LAT] != 0);
    if (path) *path = lat ? PV_PATH_LATENCY : u[PV_SPLIT_SLOTS] > 0 ? PV_PATH_COMB : PV_PATH_STRAUS;
    g_ctx.last_split[0] = u[PV_SPLIT_KEYS];
    g_ctx.last_split[1] = u[PV_SPLIT_COMB_KEYS];
    g_ctx.last_split[2] = u[PV_SPLIT_SLOTS];
    return PV_OK;
}

int pv_last_split(uint32_t* keys, uint32_t* comb_keys, uint32_t* comb_requests) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_last_split: call pv_init first");
    if (keys) *keys = g_ctx.last_split[0];
    if (comb_keys) *comb_keys = g_ctx.last_split[1];
    if (comb_requests) *comb_requests = g_ctx.last_split[2];
    return PV_OK;
}

int pv_set_path(int mode) {
    if (mode != PV_PATH_AUTO && mode != PV_PATH_STRAUS && mode != PV_PATH_COMB && mode != PV_PATH_LATENCY)
        return fail(PV_ERR_ARG, "pv_set_path: unknown mode");
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        g_ctxs[d].path = mode;
    }
    return PV_OK;
}

int pv_table_reuse(int on, uint32_t capacity) {
    const uint32_t cap = std::min<uint32_t>(capacity, PV_KEY_CAP);
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        Ctx& c = g_ctxs[d];
        const bool want = on != 0;
        if (want != c.dir_on || (cap && cap != c.dir_cap)) c.dir_dirty = true;  // emptied before its next use
        c.dir_on = want;
        if (cap) c.dir_cap = cap;
    }
    return PV_OK;
}

int pv_table_reuse_stats(uint64_t* hits, uint64_t* built, uint64_t* resets) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_table_reuse_stats: call pv_init first");
    unsigned long long u[3] = {0, 0, 0};
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpy(u, g_ctx.kw.dir_stat, sizeof(u), hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    if (hits) *hits = u[0];
    if (built) *built = u[1];
    if (resets) *resets = u[2];
    return PV_OK;
}

int pv_table_affine(int on) {
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        Ctx& c = g_ctxs[d];
        const bool want = on != 0;
        if (want != c.aff_on) c.dir_dirty = true;  // emptied before its next use: never half in one regime
        c.aff_on = want;
    }
    return PV_OK;
}

int pv_table_affine_stats(uint64_t* converted, uint64_t* affine_reads) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_table_affine_stats: call pv_init first");
    unsigned long long u[5] = {0, 0, 0, 0, 0};
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpy(u, g_ctx.kw.dir_stat, sizeof(u), hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    if (converted) *converted = u[3];
    if (affine_reads) *affine_reads = u[4];
    return PV_OK;
}

int pv_table_wide(uint32_t capacity) {
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        Ctx& c = g_ctxs[d];
        if (capacity != c.wide_cap) c.dir_dirty = true;  // emptied before its next use, and the pool with it
        c.wide_cap = capacity;
        if (capacity) c.wide_failed = false;  // a new capacity may fit where the last one did not
    }
    return PV_OK;
}

int pv_table_wide_stats(uint64_t* widened, uint64_t* wide_reads) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_table_wide_stats: call pv_init first");
    unsigned long long u[PV_DIR_STATS] = {};
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpy(u, g_ctx.kw.dir_stat, sizeof(u), hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    if (widened) *widened = u[5];
    if (wide_reads) *wide_reads = u[6];
    return PV_OK;
}

int pv_set_timing(int enable) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_ctx.timing = enable != 0;
    g_ctx.ev_used = 0;
    return PV_OK;
}

int pv_stage_times(double* ms, int max_stages, int* launches) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_stage_times: call pv_init first");
    constexpr int NE = PV_NSTAGES + 1;
    double acc[PV_NSTAGES] = {0};
    const int nq = g_ctx.ev_used / NE;
    for (int c = 0; c < nq; c++) {
        hipEvent_t* e = &g_ctx.ev[NE * c];
        PV_HIP(hipEventSynchronize(e[PV_NSTAGES]), PV_ERR_LAUNCH);
        for (int k = 0; k < PV_NSTAGES; k++) {
            float t = 0;
            PV_HIP(hipEventElapsedTime(&t, e[k], e[k + 1]), PV_ERR_LAUNCH);
            acc[k] += t;
        }
    }
    for (int k = 0; k < max_stages && k < PV_NSTAGES; k++) ms[k] = acc[k];
    if (launches) *launches = nq;
    return PV_OK;
}

int pv_kernel_times(double* prep_ms, double* table_ms, double* msm_ms, int* launches) {
    double t[PV_NSTAGES];
    const int rc = pv_stage_times(t, PV_NSTAGES, launches);
    if (rc) return rc;
    if (prep_ms) *prep_ms = t[PV_STAGE_KEYS] + t[PV_STAGE_PREP];
    if (table_ms) *table_ms = t[PV_STAGE_TABLE];
    if (msm_ms) *msm_ms = t[PV_STAGE_MSM] + t[PV_STAGE_ENCODE];
    return PV_OK;
}

int pv_verify_batch_device(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk,
                           uint64_t* d_verdict_words, void* stream) {
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_verify_batch_device: call pv_init first");
    if (n > 0 && (!d_sm || !d_off || !d_pk || !d_verdict_words)) return fail(PV_ERR_ARG, "null pointer");
    std::lock_guard<std::mutex> lk(g_mu);
    return launch(d_sm, d_off, n, d_pk, d_verdict_words, stream ? (hipStream_t)stream : g_ctx.stream);
}

int pv_test_clock_stamps(uint64_t* out, uint32_t max_blocks) {
#if PV_CLOCK_PROBE
    const uint32_t k = std::min<uint32_t>(max_blocks, PV_CLOCK_SLOTS);
    if (!out || k == 0) return (int)PV_CLOCK_SLOTS;
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(pv_clock_stamps), (size_t)k * 32, 0, hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    return (int)k;
#else
    (void)out;
    (void)max_blocks;
    return 0;
#endif
}

int pv_sync(void) {
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    return PV_OK;
}

int pv_stream_create(void** stream) {
    if (!stream) return fail(PV_ERR_ARG, "pv_stream_create: null pointer");
    hipStream_t s = nullptr;
    PV_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), PV_ERR_NO_DEVICE);
    *stream = (void*)s;
    return PV_OK;
}
int pv_stream_destroy(void* stream) {
    if (!stream) return PV_OK;
    PV_HIP(hipStreamSynchronize((hipStream_t)stream), PV_ERR_LAUNCH);
    {
        // a later launch must not wait on an event of a destroyed stream
        std::lock_guard<std::mutex> lk(g_mu);
        g_ctx.hand.forget((hipStream_t)stream);
        g_ctx.sg.hand.forget((hipStream_t)stream);
    }
    pv_ingress_forget_stream(stream);
    pv_merkle_forget_stream(stream);
    pv_trie_forget_stream(stream);
    PV_HIP(hipStreamDestroy((hipStream_t)stream), PV_ERR_LAUNCH);
    return PV_OK;
}
int pv_stream_sync(void* stream) {
    PV_HIP(hipStreamSynchronize(stream ? (hipStream_t)stream : g_ctx.stream), PV_ERR_LAUNCH);
    return PV_OK;
}

}  // extern "C"
