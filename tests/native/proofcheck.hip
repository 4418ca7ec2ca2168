// Host-compiled check library for state proofs: the two stages the GPU runs (csrc/keccak.h in the branch the
// GPU compiles, csrc/trie_core.h tr_rlp_canonical and tr_proof_walk), callable from
// tests/test_state_proof_host.py. Built with hipcc --offload-host-only: no GPU needed.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "keccak.h"
#include "trie_core.h"

extern "C" {

// 1 when exactly these bytes are canonical RLP all the way down
int pkc_canonical(const uint8_t* p, uint64_t len) {
    std::vector<uint8_t> own(p, p + len);  // exactly len bytes
    return tr_rlp_canonical(own.data(), len) ? 1 : 0;
}

// One query against the records blob[off[i] .. off[i + 1]): the status the kernels give (0 reject, 1 accept,
// 2 defer). flags[i] = 1 for a record that is not canonical.
int pkc_verify(const uint8_t* blob, const uint64_t* off, uint64_t n, const uint8_t* root, const uint8_t* key,
               uint64_t key_len, const uint8_t* val, uint64_t val_len, uint8_t* flags) {
    std::vector<uint64_t> digest(4 * n + 1);
    bool clean = true;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t len = off[i + 1] - off[i];
        std::vector<uint64_t> buf(len / 8 + 3, 0xEEEEEEEEEEEEEEEEull);
        uint8_t* p = reinterpret_cast<uint8_t*>(buf.data()) + 8 + (i & 7);  // every alignment in turn
        if (len) memcpy(p, blob + off[i], len);
        sha3_256(&digest[4 * i], len, PvKeccakWords(p, len));
        flags[i] = tr_rlp_canonical(blob + off[i], len) ? 0 : 1;
        clean &= flags[i] == 0;
    }
    if (!clean) return TR_PROOF_DEFER;
    return tr_proof_walk(blob, off, nullptr, digest.data(), 0, n, root, key, key_len, val, val_len);
}

}  // extern "C"
