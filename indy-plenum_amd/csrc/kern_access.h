// Accessors that more than one stage of the throughput path uses: the structure-of-arrays rows (Soa), the
// digit rows (DevDigits) and their row numbers, a table entry's quads to words and back, the staging of a
// 10-piece table entry, a request's key words. No kernel is defined here; the launch functions of pv_engine.hip enqueue the kern_*.h kernels that
// read through these. pv_engine.hip alone includes the kern_*.h headers: their non-template __global__
// functions have external linkage, so a second includer would define them twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "comb.h"
#include "pv_engine_dev.h"

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

// Table entries are stored as uint4 quads and computed on as words (a 160 B entry: 10 quads, 40 words).
// quad(q) names quad q of the entry wherever its storage puts it: a contiguous row, a strided per-lane
// table, a wave's [q][lane] staging area. pv_quads_load reads Q of them into w[0 .. 4 Q); pv_quads_store
// writes them from w, so its quad(q) yields a reference.
template <int Q, class F>
__host__ __device__ __forceinline__ void pv_quads_load(uint32_t* w, F quad) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const uint4 v = quad(q);
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
}
template <int Q, class F>
__host__ __device__ __forceinline__ void pv_quads_store(F quad, const uint32_t* w) {
#pragma unroll
    for (int q = 0; q < Q; q++) quad(q) = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

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
