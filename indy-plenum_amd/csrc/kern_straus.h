// Straus stage of the throughput path: the per-lane table of [j](-A) and [j](-R') (DevATab) and the prep,
// split, table and msm kernels of the requests whose key has no comb table. launch_straus_side and
// launch_straus_only (pv_engine.hip) enqueue them. pv_engine.hip alone includes this header: its
// non-template __global__ functions have external linkage, so a second includer would define them twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "comb.h"
#include "kern_access.h"
#include "pv_engine_dev.h"
#include "verify_core.h"

#ifndef PV_MSM_MINBLOCKS
// workgroups per CU the msm kernel's register budget is sized for (3: <= 168 VGPRs, 3 waves/SIMD)
#define PV_MSM_MINBLOCKS 3
#endif
#ifndef PV_PREP_MINBLOCKS
#define PV_PREP_MINBLOCKS 2  // Straus prep (decompression + SHA-512 + recoding)
#endif

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
        pv_quads_store<10>([&](int q) -> uint4& { return at(j, q); }, w);
    }
    __device__ __forceinline__ void store_p3(int j, const ge_p3& p) const {
        uint32_t w[40];
        ge_p3_store_words(w, p);
        store(j, w);
    }
    __device__ __forceinline__ void load_p3(int j, ge_p3& p) const {
        uint32_t w[40];
        load(j, w);
        ge_p3_load_words(p, w);
    }
    __device__ __forceinline__ void load_half(int j, int h, uint32_t w[20]) const {
        pv_quads_load<5>(w, [&](int q) { return at(j, 5 * h + q); });
    }
    __device__ __forceinline__ void load(int j, uint32_t w[40]) const {
        load_half(j, 0, w);
        load_half(j, 1, w + 20);
    }
};

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
