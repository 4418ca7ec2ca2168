// Encode stage of the throughput path: Q's encoding compared with R, one verdict bit per request.
// launch_epilogue (pv_engine.hip) enqueues it. pv_engine.hip alone includes this header, like the other
// kern_*.h: they share accessors, and their non-template __global__ functions have external linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kern_access.h"
#include "pv_engine_dev.h"
#include "verify_core.h"

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
