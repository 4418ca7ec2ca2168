// libplenum_verify: batch Ed25519 signing on the engine's device context (kernels + C ABI entries).
// The arithmetic is sign_core.h; the workspace is the `sg` member of Ctx (pv_ctx.h), used under the
// context's mutex g_mu like the verification workspace; [r]B and [a]B read the engine's wide
// fixed-base comb (Ctx::d_bc2), so the kernels are instantiated per radix like the engine's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>

#include "sign_core.h"
#include "verify_core.h"
#include "pv_ctx.h"
#include "../../include/plenum_verify.h"

// ---------------------------------------------------------------------------------------- signing
// Batch Ed25519 signing (sign_core.h: the arithmetic, and why it is NOT side-channel hardened). One
// lane per item, wave64; every lane of a wave stays active to the end (the LDS staging of the comb
// entries and the wave-wide inversion need whole waves), a lane past the batch or with a bad signer
// index repeats the last item's work and stores nothing / zeros.
static constexpr uint64_t PV_SIGN_CHUNK = 262144;  // messages (or seeds) per launch

__device__ __forceinline__ void pv_ld8(uint32_t o[8], const uint4* p) {
    const uint4 a = p[0], b = p[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void pv_st8(uint4* p, const uint32_t v[8], bool keep = true) {
    p[0] = keep ? make_uint4(v[0], v[1], v[2], v[3]) : make_uint4(0, 0, 0, 0);
    p[1] = keep ? make_uint4(v[4], v[5], v[6], v[7]) : make_uint4(0, 0, 0, 0);
}

// Per signer: key expansion of the seed at seeds[i * seed_q] (seed_q = 2: packed seeds; 4: the seed
// half of 64-byte secret keys) to keys[4 i ..] = a mod L || prefix. With pk_out (the keypair entry,
// kernel-uniform) also A = encode([a]B) to pk_out[2 i ..].
template <int W>
__global__ __launch_bounds__(PV_BLOCK, 2) void pv_sign_keys_kernel(const uint4* __restrict__ seeds, uint32_t seed_q,
                                                                    uint64_t n, uint4* __restrict__ keys,
                                                                    uint4* __restrict__ pk_out,
                                                                    const uint4* __restrict__ bcomb) {
    const uint64_t i0 = (uint64_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    const bool in = i0 < n;
    const uint64_t i = in ? i0 : n - 1;
    uint32_t seed[8], a[8], prefix[8];
    pv_ld8(seed, seeds + i * seed_q);
    pv_sign_expand(a, prefix, seed);
    if (in) {
        pv_st8(keys + 4 * i, a);
        pv_st8(keys + 4 * i + 2, prefix);
    }
    if (!pk_out) return;
    __shared__ uint4 stg[PV_BLOCK / 64][PV_BCOMB_STRIDE / 4][64];
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    ge_p3 acc;
    pv_sign_base_mult<W, Bc2<W>::POS>(acc, a, DevB2Stage<Bc2<W>::ENT>{bcomb, &stg[wv][0][0], threadIdx.x & 63u});
    uint32_t enc[8];
    pv_sign_encode(enc, acc, in, PvWaveInvert{});
    if (in) pv_st8(pk_out + 2 * i, enc);
}

// Per message r of a chunk: signer s = sidx ? sidx[r] : idx_base + r; nonce hash, [r]B from the wide
// comb, R by the wave's shared inversion, second hash over the key bytes as given (sk[s][32:64]), S, and
// the 64-byte signature as four uint4 stores. s >= n_signers: 64 zero bytes.
template <int W>
__global__ __launch_bounds__(PV_BLOCK, 2) void pv_sign_kernel(const uint8_t* __restrict__ msg,
                                                               const uint64_t* __restrict__ off, uint64_t n,
                                                               const uint4* __restrict__ sk,
                                                               const uint4* __restrict__ keys, uint64_t n_signers,
                                                               const uint32_t* __restrict__ sidx, uint64_t idx_base,
                                                               uint4* __restrict__ sig_out,
                                                               const uint4* __restrict__ bcomb) {
    const uint32_t r0 = blockIdx.x * PV_BLOCK + threadIdx.x;
    const bool in = r0 < n;
    const uint32_t r = in ? r0 : (uint32_t)n - 1;  // whole waves stay in step
    const uint64_t s0 = sidx ? (uint64_t)sidx[r] : idx_base + r;
    const bool ok = in && s0 < n_signers;
    const uint64_t s = s0 < n_signers ? s0 : 0;  // a lane without a signer works on signer 0, stores zeros
    const uint64_t o0 = off[r], mlen = off[r + 1] - o0;
    const uint64_t maddr = reinterpret_cast<uint64_t>(msg + o0);
    const DevMsg mw{reinterpret_cast<const uint32_t*>(maddr & ~3ull), (uint32_t)(maddr & 3)};
    uint32_t rr[8], hdr[16];
    {
        uint32_t prefix[8];
        pv_ld8(prefix, keys + 4 * s + 2);
        pv_hash_hm<4>(rr, prefix, mlen, mw);
    }
    {
        __shared__ uint4 stg[PV_BLOCK / 64][PV_BCOMB_STRIDE / 4][64];
        const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        ge_p3 acc;
        pv_sign_base_mult<W, Bc2<W>::POS>(acc, rr, DevB2Stage<Bc2<W>::ENT>{bcomb, &stg[wv][0][0], threadIdx.x & 63u});
        pv_sign_encode(hdr, acc, ok, PvWaveInvert{});
    }
    pv_ld8(hdr + 8, sk + 4 * s + 2);
    uint32_t k[8], a[8], S[8];
    pv_hash_hm<8>(k, hdr, mlen, mw);
    pv_ld8(a, keys + 4 * s);
    pv_sign_s(S, k, a, rr);
    if (in) {
        pv_st8(sig_out + 4 * (uint64_t)r, hdr, ok);
        pv_st8(sig_out + 4 * (uint64_t)r + 2, S, ok);
    }
}

// ------------------------------------------------------------------------------------------ host

namespace {

// One use of the workspace on `stream` (caller holds g_mu): room for `signers` expanded keys, the
// hand-over around `body`, and the expanded keys overwritten behind the kernels that read them, also
// after a failure.
template <class F>
int sg_run(uint64_t signers, hipStream_t stream, F&& body) {
    auto& g = g_ctx.sg;
    if (int rc = g.d_keys.grow(std::max<uint64_t>(signers, 4096) * 64)) return rc;
    return g.hand.run(stream, [&]() -> int {
        const int rc = body();
        const hipError_t e = hipMemsetAsync(g.d_keys.p, 0, signers * 64, stream);
        if (rc) return rc;
        if (e != hipSuccess) return fail(PV_ERR_LAUNCH, std::string("pv_sign: key scrub: ") + hipGetErrorString(e));
        return PV_OK;
    });
}
// Key expansion of `signers` seeds (seed_q uint4 apart); d_pk: also the public keys (keypair entry).
int sg_keys(const uint8_t* d_seeds, uint32_t seed_q, uint64_t signers, uint8_t* d_pk, hipStream_t stream) {
    const unsigned grid = (unsigned)((signers + PV_BLOCK - 1) / PV_BLOCK);
    PV_LAUNCH_BC2(pv_sign_keys_kernel, dim3(grid), dim3(PV_BLOCK), 0, stream, reinterpret_cast<const uint4*>(d_seeds),
                  seed_q, signers, g_ctx.sg.d_keys.as<uint4>(), reinterpret_cast<uint4*>(d_pk), g_ctx.d_bc2);
    return PV_OK;
}
// Messages [c0, c0 + m) of a batch whose offsets d_off (already moved to c0) index d_msg.
int sg_chunk(const uint8_t* d_msg, const uint64_t* d_off, uint64_t m, const uint8_t* d_sk, uint64_t n_signers,
             const uint32_t* d_idx, uint64_t idx_base, uint8_t* d_sig, hipStream_t stream) {
    const unsigned grid = (unsigned)((m + PV_BLOCK - 1) / PV_BLOCK);
    PV_LAUNCH_BC2(pv_sign_kernel, dim3(grid), dim3(PV_BLOCK), 0, stream, d_msg, d_off, m,
                  reinterpret_cast<const uint4*>(d_sk), g_ctx.sg.d_keys.as<uint4>(), n_signers, d_idx, idx_base,
                  reinterpret_cast<uint4*>(d_sig), g_ctx.d_bc2);
    return PV_OK;
}
constexpr uint64_t PV_SIGN_MAX = 0xffffffffull;  // items / signers per call (32-bit lane indices)

// Device-buffer batch on `stream` (caller holds g_mu): expansion of every signer, then the chunks.
int sg_enqueue(const uint8_t* d_msg, const uint64_t* d_off, uint64_t n, const uint8_t* d_sk, uint64_t n_signers,
               const uint32_t* d_idx, uint8_t* d_sig, hipStream_t stream) {
    return sg_run(n_signers, stream, [&]() -> int {
        int rc = sg_keys(d_sk, 4, n_signers, nullptr, stream);
        for (uint64_t c0 = 0; c0 < n && rc == PV_OK; c0 += PV_SIGN_CHUNK)
            rc = sg_chunk(d_msg, d_off + c0, std::min<uint64_t>(PV_SIGN_CHUNK, n - c0), d_sk, n_signers,
                          d_idx ? d_idx + c0 : nullptr, c0, d_sig + 64 * c0, stream);
        return rc;
    });
}

// The host entries' copies of secret keys / seeds, the first `bytes` of d and h: overwritten on the device
// behind the work on `stream` and, once that is done, in pinned memory.
int sg_scrub_secrets(const PvDevBuf& d, const PvPinnedBuf& h, uint64_t bytes, hipStream_t stream) {
    hipError_t e = d.p ? hipMemsetAsync(d.p, 0, std::min(bytes, d.cap), stream) : hipSuccess;
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (h.p) memset(h.p, 0, std::min(bytes, h.cap));
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(PV_ERR_LAUNCH, std::string("pv_sign: secret scrub: ") + hipGetErrorString(e));
    return PV_OK;
}

}  // namespace

extern "C" {

int pv_sign_batch_device(const uint8_t* d_msg, const uint64_t* d_msg_off, uint64_t n, const uint8_t* d_sk,
                         uint64_t n_signers, const uint32_t* d_signer_idx, uint8_t* d_sig_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_sign_batch_device: call pv_init first");
    if (n == 0) return PV_OK;
    if (!d_msg || !d_msg_off || !d_sk || !d_sig_out) return fail(PV_ERR_ARG, "pv_sign_batch_device: null pointer");
    if (n_signers == 0 || n > PV_SIGN_MAX || n_signers > PV_SIGN_MAX)
        return fail(PV_ERR_ARG, "pv_sign_batch_device: no signers, or more than 2^32 - 1 items");
    if (!d_signer_idx && n_signers != n)
        return fail(PV_ERR_ARG, "pv_sign_batch_device: without signer_idx, n_signers must equal n");
    if ((reinterpret_cast<uintptr_t>(d_sk) | reinterpret_cast<uintptr_t>(d_sig_out)) & 15u)
        return fail(PV_ERR_ARG, "pv_sign_batch_device: d_sk and d_sig_out must be 16-byte aligned");
    return sg_enqueue(d_msg, d_msg_off, n, d_sk, n_signers, d_signer_idx, d_sig_out,
                      stream ? (hipStream_t)stream : g_ctx.stream);
}

int pv_sign_batch(const uint8_t* msg, const uint64_t* msg_off, uint64_t n, const uint8_t* sk, uint64_t n_signers,
                  const uint32_t* signer_idx, uint8_t* sig_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_sign_batch: call pv_init first");
    if (n == 0) return PV_OK;
    if (!msg_off || !sk || !sig_out) return fail(PV_ERR_ARG, "pv_sign_batch: null pointer");
    if (n_signers == 0 || n > PV_SIGN_MAX || n_signers > PV_SIGN_MAX)
        return fail(PV_ERR_ARG, "pv_sign_batch: no signers, or more than 2^32 - 1 items");
    if (!signer_idx && n_signers != n) return fail(PV_ERR_ARG, "pv_sign_batch: without signer_idx, n_signers must equal n");
    // everything the kernels index with is validated, so a bad argument is an error and never a fault
    // (of a bad offset and a bad signer index, the one at the earlier item is reported; the offset at a tie)
    uint64_t bad_idx = n;
    for (uint64_t i = 0; i < n && signer_idx && bad_idx == n; i++)
        if (signer_idx[i] >= n_signers) bad_idx = i;
    if (!pv_offsets_monotone(msg_off, std::min(bad_idx + 1, n)))
        return fail(PV_ERR_ARG, "pv_sign_batch: offsets must be non-decreasing");
    if (bad_idx < n) return fail(PV_ERR_ARG, "pv_sign_batch: signer index out of range");
    if (!msg && msg_off[n] != msg_off[0]) return fail(PV_ERR_ARG, "pv_sign_batch: null message blob");
    auto& g = g_ctx.sg;
    const hipStream_t s = g_ctx.stream;
    const uint64_t sk_bytes = n_signers * 64;
    int rc;
    if ((rc = g.h_sk.grow(sk_bytes, hipHostMallocDefault)) || (rc = g.d_sk.grow(sk_bytes))) return rc;
    memcpy(g.h_sk.p, sk, sk_bytes);
    rc = sg_run(n_signers, s, [&]() -> int {
        PV_HIP(hipMemcpyAsync(g.d_sk.p, g.h_sk.p, sk_bytes, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
        int rc = sg_keys(g.d_sk.p, 4, n_signers, nullptr, s);
        PvStage& st = g.stage;
        for (uint64_t c0 = 0; c0 < n && rc == PV_OK; c0 += PV_SIGN_CHUNK) {
            const uint64_t m = std::min<uint64_t>(PV_SIGN_CHUNK, n - c0);
            if ((rc = st.reset(s, true))) break;
            // chunk staging: offsets moved to the chunk's first byte, signer indices, message bytes + slack
            const int off = st.in_offsets(msg_off + c0, m), idx = signer_idx ? st.in(signer_idx + c0, m * 4) : -1,
                      mb = st.in(msg + msg_off[c0], msg_off[c0 + m] - msg_off[c0], PV_BLOB_SLACK),
                      sig = st.out(sig_out + 64 * c0, m * 64);
            if ((rc = st.upload()) ||
                (rc = sg_chunk(st.dev<const uint8_t>(mb), st.dev<const uint64_t>(off), m, g.d_sk.p, n_signers,
                               st.dev<const uint32_t>(idx), c0, st.dev<uint8_t>(sig), s)))
                break;
            rc = st.download();
        }
        return rc;
    });
    const int rc2 = sg_scrub_secrets(g.d_sk, g.h_sk, sk_bytes, s);
    return rc ? rc : rc2;
}

int pv_sign_seed_keypairs(const uint8_t* seeds, uint64_t n, uint8_t* pk_out, uint8_t* sk_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_sign_seed_keypairs: call pv_init first");
    if (n == 0) return PV_OK;
    if (!seeds) return fail(PV_ERR_ARG, "pv_sign_seed_keypairs: null pointer");
    if (n > PV_SIGN_MAX) return fail(PV_ERR_ARG, "pv_sign_seed_keypairs: more than 2^32 - 1 seeds");
    const hipStream_t s = g_ctx.stream;
    const uint64_t cm = std::min<uint64_t>(PV_SIGN_CHUNK, n);
    PvStage& st = g_ctx.sg.stage;  // the seeds travel in its input blocks, scrubbed below
    const int rc = sg_run(cm, s, [&]() -> int {
        for (uint64_t c0 = 0; c0 < n; c0 += PV_SIGN_CHUNK) {
            const uint64_t m = std::min<uint64_t>(PV_SIGN_CHUNK, n - c0);
            int rc = st.reset(s, true);
            if (rc) return rc;
            const int seed = st.in(seeds + 32 * c0, m * 32), pk = st.out(pk_out ? pk_out + 32 * c0 : nullptr, m * 32);
            if ((rc = st.upload()) || (rc = sg_keys(st.dev<const uint8_t>(seed), 2, m, st.dev<uint8_t>(pk), s)) ||
                (rc = st.download()))
                return rc;
            for (uint64_t i = 0; i < m && sk_out; i++) {
                memcpy(sk_out + 64 * (c0 + i), seeds + 32 * (c0 + i), 32);
                memcpy(sk_out + 64 * (c0 + i) + 32, st.host(pk) + 32 * i, 32);
            }
        }
        return PV_OK;
    });
    const int rc2 = sg_scrub_secrets(st.d_in, st.h, pv_up256(cm * 32), s);
    return rc ? rc : rc2;
}

}  // extern "C"
