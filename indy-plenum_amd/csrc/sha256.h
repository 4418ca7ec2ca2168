// SHA-256 (FIPS 180-4) for the ledger's RFC 6962 Merkle hashing (ledger/tree_hasher.py:16-28):
// leaf = SHA-256(0x00 || data), node = SHA-256(0x01 || left || right).
//
// The eight working variables and a 16-word schedule ring stay in VGPRs; every rotation is one
// v_alignbit_b32, Ch / Maj / the three-way XORs one v_bitop3_b32, byte swaps one v_perm_b32 (the
// helpers of sha512.h). Rounds are unrolled 16 at a time with the variables rotated by renaming, so no
// register is indexed at run time.
// sha256_hash_children is the 65-byte node hash as two fixed blocks: the second block holds one
// data byte, the padding and the length, so fifteen of its sixteen words are literals that the
// compiler folds into the round constants of its first sixteen rounds.
// PV_HD like sha512.h: tests/native/merklecheck.hip compiles the same source for the CPU.
#pragma once
#include "sha512.h"

static constexpr uint32_t PV_K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

template <int N>
PV_HD uint32_t pv_rotr32(uint32_t x) {
    return pv_alignbit(x, x, N);
}

PV_HD void sha256_init(uint32_t st[8]) {
    st[0] = 0x6a09e667; st[1] = 0xbb67ae85; st[2] = 0x3c6ef372; st[3] = 0xa54ff53a;
    st[4] = 0x510e527f; st[5] = 0x9b05688c; st[6] = 0x1f83d9ab; st[7] = 0x5be0cd19;
}

#define PV_SHA256_ROUND(a, b, c, d, e, f, g, h, kw)                                                \
    do {                                                                                          \
        const uint32_t S1 = pv_bitop3<0x96>(pv_rotr32<6>(e), pv_rotr32<11>(e), pv_rotr32<25>(e)); \
        const uint32_t ch = pv_bitop3<0xCA>(e, f, g);                                             \
        const uint32_t t1 = h + S1 + ch + (kw);                                                   \
        const uint32_t S0 = pv_bitop3<0x96>(pv_rotr32<2>(a), pv_rotr32<13>(a), pv_rotr32<22>(a)); \
        const uint32_t mj = pv_bitop3<0xE8>(a, b, c);                                             \
        d += t1;                                                                                  \
        h = t1 + S0 + mj;                                                                         \
    } while (0)

// Sixteen rounds from round r (a multiple of 16): the schedule ring w advances in place (not in the first
// sixteen), the working variables rotate by renaming.
template <bool FIRST>
PV_HD void sha256_rounds16(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t& e, uint32_t& f, uint32_t& g,
                           uint32_t& h, uint32_t w[16], int r) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (!FIRST) {
            const uint32_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
            const uint32_t s0 = pv_bitop3<0x96>(pv_rotr32<7>(w15), pv_rotr32<18>(w15), w15 >> 3);
            const uint32_t s1 = pv_bitop3<0x96>(pv_rotr32<17>(w2), pv_rotr32<19>(w2), w2 >> 10);
            w[j] += s0 + w[(j + 9) & 15] + s1;
        }
        const uint32_t kw = PV_K256[r + j] + w[j];
        switch (j & 7) {
            case 0: PV_SHA256_ROUND(a, b, c, d, e, f, g, h, kw); break;
            case 1: PV_SHA256_ROUND(h, a, b, c, d, e, f, g, kw); break;
            case 2: PV_SHA256_ROUND(g, h, a, b, c, d, e, f, kw); break;
            case 3: PV_SHA256_ROUND(f, g, h, a, b, c, d, e, kw); break;
            case 4: PV_SHA256_ROUND(e, f, g, h, a, b, c, d, kw); break;
            case 5: PV_SHA256_ROUND(d, e, f, g, h, a, b, c, kw); break;
            case 6: PV_SHA256_ROUND(c, d, e, f, g, h, a, b, kw); break;
            default: PV_SHA256_ROUND(b, c, d, e, f, g, h, a, kw); break;
        }
    }
}

// One compression of a 64-byte block given as 16 big-endian words; w is the schedule ring (consumed).
// The first sixteen rounds stand alone, so words the caller knows at compile time (the padding block of
// sha256_hash_children) fold into their round constants; the other 48 run as three passes of one body
// with the constants read from the table, which keeps the kernels small and their register need low.
PV_HD void sha256_compress(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    sha256_rounds16<true>(a, b, c, d, e, f, g, h, w, 0);
#pragma unroll 1
    for (int r = 16; r < 64; r += 16) sha256_rounds16<false>(a, b, c, d, e, f, g, h, w, r);
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

#undef PV_SHA256_ROUND

// A 32-byte hash travels as its eight big-endian words ("digest words"): word k = bytes [4k, 4k + 4).
// Memory holds the digest bytes; a little-endian 32-bit load of them is byte-swapped into a digest word.
PV_HD void sha256_words_from_le(uint32_t h[8], const uint32_t le[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = pv_bswap32(le[k]);
}

// out = SHA-256(0x01 || left || right) on digest words: block 1 = the prefix byte, left and the first
// 31 bytes of right; block 2 = right's last byte, 0x80, zeros and the bit length 520.
PV_HD void sha256_hash_children(uint32_t out[8], const uint32_t left[8], const uint32_t right[8]) {
    uint32_t st[8], w[16];
    sha256_init(st);
    w[0] = 0x01000000u | (left[0] >> 8);
#pragma unroll
    for (int k = 1; k < 8; k++) w[k] = pv_alignbit(left[k - 1], left[k], 8);
    w[8] = pv_alignbit(left[7], right[0], 8);
#pragma unroll
    for (int k = 1; k < 8; k++) w[8 + k] = pv_alignbit(right[k - 1], right[k], 8);
    sha256_compress(st, w);
    w[0] = (right[7] << 24) | 0x00800000u;
#pragma unroll
    for (int k = 1; k < 15; k++) w[k] = 0;
    w[15] = 65 * 8;
    sha256_compress(st, w);
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = st[k];
}

// SHA-256(prefix || data) for a message of `len` data bytes behind HAS_PREFIX (0 or 1) prefix bytes of
// value `prefix`. word(q) returns the little-endian 32-bit word of data bytes [4q, 4q + 4); bytes past
// `len` may hold anything (they are masked here), so a loader may read whole aligned words.
template <int HAS_PREFIX, class Words>
PV_HD void sha256_prefixed(uint32_t out[8], uint32_t prefix, uint64_t len, const Words& word) {
    uint32_t st[8];
    sha256_init(st);
    const uint64_t m = len + HAS_PREFIX;         // message bytes
    const uint64_t nblk = (m + 9 + 63) / 64;     // 0x80 and the 64-bit length fit behind them
    uint32_t prev = prefix << 24;                // the data word before the current one (its top byte is used)
    for (uint64_t b = 0; b < nblk; b++) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t g = 16 * b + j;       // message word: message bytes [4g, 4g + 4)
            uint32_t le;                         // those bytes, little-endian
            if (HAS_PREFIX) {
                // data bytes [4g - 1, 4g + 3): the top byte of data word g - 1 and three of word g
                const uint32_t cur = 4 * g < len ? word(g) : 0u;
                le = pv_alignbit(cur, prev, 24);
                prev = cur;
            } else {
                le = 4 * g < len ? word(g) : 0u;
            }
            // keep the message's bytes, then 0x80, then zeros
            if (4 * g + 4 > m) {
                if (4 * g > m) {
                    le = 0;
                } else {
                    const uint32_t v = (uint32_t)(m - 4 * g);  // 0..3 message bytes in this word
                    le = (le & ((1u << (8 * v)) - 1u)) | (0x80u << (8 * v));
                }
            }
            w[j] = pv_bswap32(le);
        }
        if (b == nblk - 1) {
            w[14] = (uint32_t)(m >> 29);
            w[15] = (uint32_t)(m << 3);
        }
        sha256_compress(st, w);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = st[k];
}

// Little-endian data words of one record at any byte address, from aligned 32-bit loads funnel-shifted
// as the SHA-512 loader does; sha256_prefixed calls it for q = 0, 1, 2, ... while 4 q < len, so the aligned
// word above is carried from call to call. Nothing past the last aligned word that holds a data byte
// is read (at most 3 bytes beyond the record, inside PV_BLOB_SLACK).
struct PvRecordWords {
    const uint32_t* p;    // the aligned word that holds data byte 0
    uint32_t sh;          // 8 * (address & 3)
    uint64_t last;        // index of the last aligned word that holds a data byte
    mutable uint32_t lo;  // aligned word q
    PV_HD PvRecordWords(const uint8_t* data, uint64_t len) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(data);
        p = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
        sh = 8u * (uint32_t)(a & 3);
        last = len ? ((a & 3) + len - 1) >> 2 : 0;
        lo = len ? p[0] : 0u;
    }
    PV_HD uint32_t operator()(uint64_t q) const {
        const uint32_t hi = q + 1 <= last ? p[q + 1] : 0u;
        const uint32_t r = pv_alignbit(hi, lo, sh);
        lo = hi;
        return r;
    }
};
