// Ed25519 signing arithmetic (RFC 8032 / libsodium 1.0.18 crypto_sign_seed_keypair and
// crypto_sign_detached), shared by the signing kernels (pv_sign.hip pv_sign_keys_kernel /
// pv_sign_kernel) and the host check library (tests/native/signcheck.hip). Replaces, per signature,
// stp_core/crypto/nacl_wrappers.py:141 (crypto_sign_seed_keypair) and :170 (crypto_sign) -> libnacl ->
// libsodium.
//
//   key expansion   az = SHA-512(seed); a = az[0:32] clamped (a[0] &= 248, a[31] &= 127, a[31] |= 64);
//                   prefix = az[32:64]. The clamped a can reach 2^255 - 8 while the fixed-base comb covers
//                   253 bits, so a mod L is kept instead: B has order L, so [a mod L]B = [a]B, and S is
//                   taken mod L, so k (a mod L) + r = k a + r (mod L). Both uses are exact.
//   public key      A = encode([a mod L]B)
//   signature       r = SHA-512(prefix || M) mod L, R = encode([r]B),
//                   k = SHA-512(R || sk[32:64] || M) mod L (the key bytes AS GIVEN in the 64-byte secret
//                   key, never a recomputed A: libsodium does exactly this),
//                   S = (k a + r) mod L with r added into the 512-bit product before the one reduction,
//                   sig = R || S.
//
// NOT SIDE-CHANNEL HARDENED. The fixed-base comb lookups ([a]B, [r]B) are indexed by digits of the
// secret scalars, lanes with different message lengths run different numbers of hash blocks, and
// nothing here is written for constant time or constant memory-access patterns. This signer is meant
// for load generation, fixtures and test wallets. It is not meant for custody of production keys.
#pragma once
#include "fe25519.h"
#include "ge25519.h"
#include "sc25519.h"
#include "sha512.h"
#include "comb.h"

// SHA-512(header || M) as 16 little-endian words; header = HW 64-bit words (HW = 4: a 32-byte header,
// HW = 8: 64 bytes) given as 2 HW little-endian 32-bit words, M = mlen bytes read through
// msgword(q) = little-endian bytes [8q, 8q + 8) of M at any byte alignment. The sibling of pv_hash_k
// (verify_core.h), which is tied to the sig || msg record layout: the same branch-free block assembly,
// so lanes with different lengths never diverge inside a block (msgword may be asked for words up to
// 152 bytes past the end of M; what it returns there is masked away).
template <int HW, class MsgWord>
PV_HD void pv_sha512_hm(uint32_t h[16], const uint32_t hdr[2 * HW], uint64_t mlen, const MsgWord& msgword) {
    static_assert(HW == 4 || HW == 8, "pv_sha512_hm: a 32-byte or a 64-byte header");
    const uint32_t T = (uint32_t)mlen + 8u * HW;
    uint64_t st[8];
    sha512_init(st);
    const uint32_t nblocks = (T + 17 + 127) / 128;
    for (uint32_t b = 0; b < nblocks; b++) {
        uint64_t blk[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t q = 16 * b + j;
            // message word q - HW; block 0's first HW words are the header (q - HW wraps there: any
            // word of M will do, it is replaced)
            uint64_t raw = msgword(j < HW ? (b == 0 ? 0u : q - HW) : q - HW);
            if (j < HW) {
                const uint64_t hw = pv_pack64(hdr[2 * j + 1], hdr[2 * j]);
                raw = (b == 0) ? hw : raw;
            }
            // bytes at or beyond T: 0x80, then zeros
            const int32_t rem = (int32_t)T - (int32_t)(8 * q);
            const uint32_t nb = rem < 0 ? 0u : (rem > 8 ? 8u : (uint32_t)rem);
            const uint64_t mask = nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1);
            const uint64_t pad = (rem >= 0 && rem < 8) ? (0x80ull << (8 * rem)) : 0ull;
            raw = (raw & mask) | pad;
            uint64_t be = pv_bswap64(raw);
            if (j == 15 && b == nblocks - 1) be = (uint64_t)T * 8;  // bit length (upper 64 bits zero)
            blk[j] = be;
        }
        sha512_compress(st, blk);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t le = pv_bswap64(st[i]);
        h[2 * i] = (uint32_t)le;
        h[2 * i + 1] = (uint32_t)(le >> 32);
    }
}

// SHA-512(header || M) mod L
template <int HW, class MsgWord>
PV_HD void pv_hash_hm(uint32_t k[8], const uint32_t hdr[2 * HW], uint64_t mlen, const MsgWord& msgword) {
    uint32_t h[16];
    pv_sha512_hm<HW>(h, hdr, mlen, msgword);
    sc_reduce64(k, h);
}

struct PvNoMsg {
    PV_HD uint64_t operator()(uint64_t) const { return 0; }
};

// Key expansion: a mod L and prefix from the 32-byte seed.
PV_HD void pv_sign_expand(uint32_t a[8], uint32_t prefix[8], const uint32_t seed[8]) {
    uint32_t az[16];
    pv_sha512_hm<4>(az, seed, 0, PvNoMsg{});
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        x[i] = az[i];
        x[8 + i] = 0;
        prefix[i] = az[8 + i];
    }
    x[0] &= 0xfffffff8u;
    x[7] = (x[7] & 0x7fffffffu) | 0x40000000u;
    sc_reduce64(a, x);
}

// S = (k a + r) mod L for k, a, r < 2^256: r goes into the 512-bit product (k a + r < 2^512), then one
// sc_reduce64.
PV_HD void pv_sign_s(uint32_t S[8], const uint32_t k[8], const uint32_t a[8], const uint32_t r[8]) {
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = i < 8 ? r[i] : 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t t = (uint64_t)k[i] * a[j] + x[i + j] + c;
            x[i + j] = (uint32_t)t;
            c = t >> 32;
        }
        x[i + 8] = (uint32_t)c;  // still zero before row i (r fills words 0..7 only), as in sc_mul
    }
    sc_reduce64(S, x);
}

// [s]B for s < 2^253 from the wide fixed-base comb of radix 2^W (P positions): sc_recode_w digits, then
// pv_comb_b_acc_w (one entry conversion + P - 1 niels additions). `st` stages the table entries (the
// device: DevB2Stage over ctx.d_bc2; the host: PvRowsStageB over a radix-65536 table).
template <int W, int P, class BStage>
PV_HD void pv_sign_base_mult(ge_p3& acc, const uint32_t s[8], const BStage& st) {
    int32_t fb[P];
    sc_recode_w<W, P>(fb, s);
    pv_comb_b_acc_w<P>(acc, st, [&](int j) {
        int32_t d = 0;
#pragma unroll
        for (int u = 0; u < P; u++) d = j == u ? fb[u] : d;
        return (int)d;
    });
}

// One point's canonical encoding through the batched encoder (a batch of one per lane): the lane's own
// inversion with PvFeInvert, the wave-wide one with the engine's PvWaveInvert. A lane with use = false
// contributes Z = 1 to the shared inversion and gets a meaningless encoding.
struct PvSignEncSrc {
    const ge_p3& p;
    PV_HD void z(int, fe& o) const { o = p.Z; }
    PV_HD void xy(int, fe& x, fe& y) const {
        x = p.X;
        y = p.Y;
    }
};
struct PvSignEncSink {
    uint32_t* out;
    PV_HD void operator()(int, const uint32_t enc[8], bool) const {
#pragma unroll
        for (int q = 0; q < 8; q++) out[q] = enc[q];
    }
};
template <class Inv = PvFeInvert>
PV_HD void pv_sign_encode(uint32_t enc[8], const ge_p3& p, bool use, const Inv& invert = Inv()) {
    bool u[1] = {use};
    pv_encode_batch_stream_b<1>(PvSignEncSrc{p}, u, PvSignEncSink{enc}, invert);
}
