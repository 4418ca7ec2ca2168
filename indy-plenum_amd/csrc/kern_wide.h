// Wide-row builders: the wide fixed-base comb (ctx_init_parts enqueues pv_bc2_build_kernel row by row), a
// cached key's radix-65536 rows (kc_build_tables enqueues pv_kc_wide_kernel) and a resident table's
// radix-2^11 rows (launch_epilogue enqueues pv_dir_widen_kernel); all in pv_engine.hip, which alone includes
// this header: its non-template __global__ functions have external linkage, so a second includer would
// define them twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "comb.h"
#include "kern_tables.h"
#include "pv_engine_dev.h"
#include "verify_core.h"

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
            pv_quads_load<10>(w, [&](int q) { return e[q]; });
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
