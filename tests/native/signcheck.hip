// Host-only check library over indy-plenum_amd/csrc/sign_core.h: the signing kernels' arithmetic
// (key expansion, both hashes, [s]B from the fixed-base comb's code at radix 2^16, the batched
// encoder, S = k a + r mod L) compiled for the CPU, so tests/test_sign_host.py can hold it against
// libsodium's crypto_sign_seed_keypair / crypto_sign_detached without a GPU. Built with
// --offload-host-only like hostcheck.hip; it includes only the field, group, scalar, SHA and comb
// headers (not the limb-parallel ones), so it compiles in seconds.
#include <stdint.h>
#include <string.h>

#include <functional>
#include <thread>
#include <vector>

#include "sign_core.h"

namespace {

struct HostBRow {
    const uint32_t* r;
    void load_part(int d, int part, uint32_t w[20]) const { memcpy(w, r + d * PV_BCOMB_STRIDE + 20 * part, part ? 40 : 80); }
};
struct HostBRows {
    const uint32_t* base;
    HostBRow row(int i) const { return HostBRow{base + (size_t)i * PV_BCOMB_ENT * PV_BCOMB_STRIDE}; }
};

// the radix-65536 fixed-base comb, as pv_init builds it on the host
const std::vector<uint32_t>& host_bcomb() {
    static std::vector<uint32_t> bcomb;
    if (bcomb.empty()) {
        bcomb.resize((size_t)PV_BCOMB_POS * PV_BCOMB_ENT * PV_BCOMB_STRIDE);
        ge_p3 base[PV_BCOMB_POS];
        pv_bcomb_bases(base);
        std::vector<std::thread> th;
        for (int j = 0; j < PV_BCOMB_POS; j++)
            th.emplace_back(pv_bcomb_build_position, bcomb.data() + (size_t)j * PV_BCOMB_ENT * PV_BCOMB_STRIDE,
                            std::cref(base[j]));
        for (auto& t : th) t.join();
    }
    return bcomb;
}

// little-endian bytes [8q, 8q + 8) of m, zero past its end (the device reads the blob's slack there)
struct HostMsg {
    const uint8_t* m;
    uint64_t len;
    uint64_t operator()(uint64_t q) const {
        uint64_t v = 0;
        for (int i = 0; i < 8; i++)
            if (8 * q + i < len) v |= (uint64_t)m[8 * q + i] << (8 * i);
        return v;
    }
};

void base_mult_encode(uint32_t enc[8], const uint32_t s[8]) {
    const HostBRows brows{host_bcomb().data()};
    ge_p3 acc;
    pv_sign_base_mult<16, PV_BCOMB_POS>(acc, s, PvRowsStageB<HostBRows>{brows, 0, 0});
    pv_sign_encode(enc, acc, true);
}

}  // namespace

extern "C" {

// a mod L and prefix of a seed
void sgc_expand(const uint8_t seed[32], uint8_t a[32], uint8_t prefix[32]) {
    uint32_t s[8], aw[8], pw[8];
    memcpy(s, seed, 32);
    pv_sign_expand(aw, pw, s);
    memcpy(a, aw, 32);
    memcpy(prefix, pw, 32);
}

// crypto_sign_seed_keypair
void sgc_keypair(const uint8_t seed[32], uint8_t pk[32], uint8_t sk[64]) {
    uint32_t s[8], a[8], prefix[8], enc[8];
    memcpy(s, seed, 32);
    pv_sign_expand(a, prefix, s);
    base_mult_encode(enc, a);
    memcpy(pk, enc, 32);
    memcpy(sk, seed, 32);
    memcpy(sk + 32, enc, 32);
}

// crypto_sign_detached with the 64-byte secret key seed || pk (the pk half used as given)
void sgc_sign(const uint8_t sk[64], const uint8_t* m, uint64_t mlen, uint8_t sig[64]) {
    uint32_t seed[8], a[8], prefix[8], r[8], hdr[16], k[8], S[8];
    memcpy(seed, sk, 32);
    pv_sign_expand(a, prefix, seed);
    const HostMsg mw{m, mlen};
    pv_hash_hm<4>(r, prefix, mlen, mw);
    base_mult_encode(hdr, r);
    memcpy(hdr + 8, sk + 32, 32);
    pv_hash_hm<8>(k, hdr, mlen, mw);
    pv_sign_s(S, k, a, r);
    memcpy(sig, hdr, 32);
    memcpy(sig + 32, S, 32);
}

// the scalar step alone: S = (k a + r) mod L for any 256-bit k, a, r
void sgc_scalar_s(const uint8_t k[32], const uint8_t a[32], const uint8_t r[32], uint8_t S[32]) {
    uint32_t kw[8], aw[8], rw[8], sw[8];
    memcpy(kw, k, 32);
    memcpy(aw, a, 32);
    memcpy(rw, r, 32);
    pv_sign_s(sw, kw, aw, rw);
    memcpy(S, sw, 32);
}

// SHA-512(header || m) for a 32- or 64-byte header (the sibling of pv_hash_k), unreduced
int sgc_sha512_hm(const uint8_t* hdr, int hdr_len, const uint8_t* m, uint64_t mlen, uint8_t out[64]) {
    uint32_t h[16], hw[16];
    memcpy(hw, hdr, hdr_len == 32 ? 32 : 64);
    const HostMsg mw{m, mlen};
    if (hdr_len == 32) pv_sha512_hm<4>(h, hw, mlen, mw);
    else if (hdr_len == 64) pv_sha512_hm<8>(h, hw, mlen, mw);
    else return -1;
    memcpy(out, h, 64);
    return 0;
}

}  // extern "C"
