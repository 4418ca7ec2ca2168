// Host-only check library over indy-plenum_amd/csrc/merkle_core.h and sha256.h: the consistency walk the
// kernels run (pv_merkle_consistency_check with the device's two-block hash_children) compiled for the
// CPU, so tests/test_consistency_host.py can hold it against a restatement of the reference's verifier
// without a GPU. Built with --offload-host-only like merklecheck.hip.
#include <stdint.h>
#include <string.h>

#include "merkle_core.h"
#include "sha256.h"

namespace {

struct H {
    uint32_t w[8];  // digest words
};
H load(const uint8_t* p) {
    uint32_t le[8];
    memcpy(le, p, 32);
    H h;
    sha256_words_from_le(h.w, le);
    return h;
}

}  // namespace

extern "C" {

// status[i] of proof i = proof[32 proof_off[i] : 32 proof_off[i + 1]] for (old_size[i], new_size[i]) and the
// two roots at [32 i]
void csc_check(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_root, const uint8_t* new_root,
               const uint8_t* proof, const uint64_t* proof_off, uint64_t n, uint8_t* status) {
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* p = proof + 32 * proof_off[i];
        status[i] = (uint8_t)pv_merkle_consistency_check(
            old_size[i], new_size[i], load(old_root + 32 * i), load(new_root + 32 * i), proof_off[i + 1] - proof_off[i],
            [&](uint64_t k, H& o) { o = load(p + 32 * k); },
            [](H& o, const H& l, const H& r) { sha256_hash_children(o.w, l.w, r.w); },
            [](const H& a, const H& b) { return memcmp(a.w, b.w, 32) == 0; });
    }
}

}  // extern "C"
