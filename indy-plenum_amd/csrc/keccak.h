// SHA3-256 (FIPS 202): Keccak-f[1600], rate 136 bytes, domain byte 0x06, final bit 0x80. The state
// trie's node hash (state/util/utils.py:7-8 in the reference: hashlib.sha3_256).
//
// One hash per lane: the 25 lanes of state are 25 64-bit words in VGPR pairs. Rho is one pv_rotr64
// (two v_alignbit_b32) per word, chi a ^ (~b & c) one pv_bitop3_64<0xD2> per word (truth table over
// src0 = 0xF0, src1 = 0xCC, src2 = 0xAA: 0xF0 ^ (0x33 & 0xAA)), theta's five-way XOR two 0x96 ops.
// One round is written out with constant lane indices, so the state never leaves registers; the 24
// rounds stay a loop (#pragma unroll 1): unrolled further the kernel spilled to scratch.
//
// Shared by the kernels (pv_trie.hip), the host path (trie_host.cpp, plain C++: the #else branch
// below) and the host-compiled check library (tests/native/triecheck.hip, the device branch's host
// fallbacks of sha512.h).
#ifndef PV_KECCAK_H
#define PV_KECCAK_H

#include <stdint.h>

#if defined(__HIP__)
#include "sha512.h"
template <int N>
PV_HD uint64_t kk_rotl(uint64_t x) {
    return pv_rotr64<64 - N>(x);
}
PV_HD uint64_t kk_chi(uint64_t a, uint64_t b, uint64_t c) { return pv_bitop3_64<0xD2>(a, b, c); }
PV_HD uint64_t kk_xor3(uint64_t a, uint64_t b, uint64_t c) { return pv_bitop3_64<0x96>(a, b, c); }
#else
#ifndef PV_HD
#define PV_HD inline
#endif
namespace {  // internal linkage: the HIP units compile the other branch under the same names
template <int N>
PV_HD uint64_t kk_rotl(uint64_t x) {
    return (x << N) | (x >> (64 - N));
}
PV_HD uint64_t kk_chi(uint64_t a, uint64_t b, uint64_t c) { return a ^ (~b & c); }
PV_HD uint64_t kk_xor3(uint64_t a, uint64_t b, uint64_t c) { return a ^ b ^ c; }
#endif

static constexpr uint32_t PV_SHA3_RATE = 136;  // bytes; 17 lanes
static constexpr uint32_t PV_SHA3_RATE_WORDS = 17;

static constexpr uint64_t PV_KECCAK_RC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
    0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
    0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
    0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};

// chi over one plane: b0..b4 -> a[o .. o + 4]
#define PV_KK_CHI(o)                  \
    do {                              \
        a[o + 0] = kk_chi(b0, b1, b2); \
        a[o + 1] = kk_chi(b1, b2, b3); \
        a[o + 2] = kk_chi(b2, b3, b4); \
        a[o + 3] = kk_chi(b3, b4, b0); \
        a[o + 4] = kk_chi(b4, b0, b1); \
    } while (0)

// Keccak-f[1600] on a[x + 5 y]. Theta; then rho and pi gather each output plane from the five lanes
// that land in it (B[y][2x + 3y] = rot(A[x][y])); chi per plane; iota.
PV_HD void keccak_f1600(uint64_t a[25]) {
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
        const uint64_t c0 = kk_xor3(kk_xor3(a[0], a[5], a[10]), a[15], a[20]);
        const uint64_t c1 = kk_xor3(kk_xor3(a[1], a[6], a[11]), a[16], a[21]);
        const uint64_t c2 = kk_xor3(kk_xor3(a[2], a[7], a[12]), a[17], a[22]);
        const uint64_t c3 = kk_xor3(kk_xor3(a[3], a[8], a[13]), a[18], a[23]);
        const uint64_t c4 = kk_xor3(kk_xor3(a[4], a[9], a[14]), a[19], a[24]);
        const uint64_t d0 = c4 ^ kk_rotl<1>(c1), d1 = c0 ^ kk_rotl<1>(c2), d2 = c1 ^ kk_rotl<1>(c3),
                       d3 = c2 ^ kk_rotl<1>(c4), d4 = c3 ^ kk_rotl<1>(c0);
        // every source lane is read (with its theta term) before the plane that overwrites it is stored
        const uint64_t p00 = a[0] ^ d0, p01 = kk_rotl<44>(a[6] ^ d1), p02 = kk_rotl<43>(a[12] ^ d2),
                       p03 = kk_rotl<21>(a[18] ^ d3), p04 = kk_rotl<14>(a[24] ^ d4);
        const uint64_t p10 = kk_rotl<28>(a[3] ^ d3), p11 = kk_rotl<20>(a[9] ^ d4), p12 = kk_rotl<3>(a[10] ^ d0),
                       p13 = kk_rotl<45>(a[16] ^ d1), p14 = kk_rotl<61>(a[22] ^ d2);
        const uint64_t p20 = kk_rotl<1>(a[1] ^ d1), p21 = kk_rotl<6>(a[7] ^ d2), p22 = kk_rotl<25>(a[13] ^ d3),
                       p23 = kk_rotl<8>(a[19] ^ d4), p24 = kk_rotl<18>(a[20] ^ d0);
        const uint64_t p30 = kk_rotl<27>(a[4] ^ d4), p31 = kk_rotl<36>(a[5] ^ d0), p32 = kk_rotl<10>(a[11] ^ d1),
                       p33 = kk_rotl<15>(a[17] ^ d2), p34 = kk_rotl<56>(a[23] ^ d3);
        const uint64_t p40 = kk_rotl<62>(a[2] ^ d2), p41 = kk_rotl<55>(a[8] ^ d3), p42 = kk_rotl<39>(a[14] ^ d4),
                       p43 = kk_rotl<41>(a[15] ^ d0), p44 = kk_rotl<2>(a[21] ^ d1);
        {
            const uint64_t b0 = p00, b1 = p01, b2 = p02, b3 = p03, b4 = p04;
            PV_KK_CHI(0);
        }
        {
            const uint64_t b0 = p10, b1 = p11, b2 = p12, b3 = p13, b4 = p14;
            PV_KK_CHI(5);
        }
        {
            const uint64_t b0 = p20, b1 = p21, b2 = p22, b3 = p23, b4 = p24;
            PV_KK_CHI(10);
        }
        {
            const uint64_t b0 = p30, b1 = p31, b2 = p32, b3 = p33, b4 = p34;
            PV_KK_CHI(15);
        }
        {
            const uint64_t b0 = p40, b1 = p41, b2 = p42, b3 = p43, b4 = p44;
            PV_KK_CHI(20);
        }
        a[0] ^= PV_KECCAK_RC[r];
    }
}
#undef PV_KK_CHI

// The record's bytes as little-endian 64-bit words, from aligned 64-bit loads only: word q holds bytes
// 8q .. 8q + 7 of the record. A record that starts off an 8-byte boundary is funnel-shifted from two
// neighbouring aligned words; no aligned word beyond the one holding the record's last byte is read.
// Bytes of word q at or past `len` are whatever memory holds: sha3_256 masks them.
struct PvKeccakWords {
    const uint64_t* base;
    uint32_t sh;   // bit offset of the record inside its first aligned word
    uint64_t len;
    PV_HD PvKeccakWords(const uint8_t* data, uint64_t n) {
        const uintptr_t addr = reinterpret_cast<uintptr_t>(data);
        base = reinterpret_cast<const uint64_t*>(addr & ~(uintptr_t)7);
        sh = (uint32_t)(addr & 7) * 8;
        len = n;
    }
    // q with 8 q < len
    PV_HD uint64_t operator()(uint64_t q) const {
        const uint64_t lo = base[q];
        if (sh == 0) return lo;
        const uint64_t got = 8 - sh / 8;  // record bytes of word q that base[q] supplies
        const uint64_t hi = 8 * q + got < len ? base[q + 1] : 0;
        return (lo >> sh) | (hi << (64 - sh));
    }
};

// SHA3-256 of the `len` bytes word(q) yields; out = the digest's four little-endian words (stored as
// they are, they are the 32 digest bytes).
template <class Words>
PV_HD void sha3_256(uint64_t out[4], uint64_t len, const Words& word) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    const uint64_t blocks = len / PV_SHA3_RATE + 1;  // the padding always fits the block holding byte `len`
#pragma unroll 1
    for (uint64_t b = 0; b < blocks; b++) {
        const bool last = b + 1 == blocks;
#pragma unroll
        for (uint32_t i = 0; i < PV_SHA3_RATE_WORDS; i++) {
            const uint64_t q = b * PV_SHA3_RATE_WORDS + i, pos = 8 * q;
            uint64_t w = 0;
            if (pos < len) {
                w = word(q);
                if (len - pos < 8) w &= ~0ull >> (64 - 8 * (len - pos));
            }
            if (pos <= len && len - pos < 8) w ^= 0x06ull << (8 * (len - pos));  // lies in the last block
            if (last && i == PV_SHA3_RATE_WORDS - 1) w ^= 0x80ull << 56;  // len % 136 == 135: same byte, 0x86
            a[i] ^= w;
        }
        keccak_f1600(a);
    }
    out[0] = a[0];
    out[1] = a[1];
    out[2] = a[2];
    out[3] = a[3];
}

#if !defined(__HIP__)
}  // namespace
#endif

#endif  // PV_KECCAK_H
