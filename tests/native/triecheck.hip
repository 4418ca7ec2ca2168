// Host-compiled check library for the state-trie feature: the kernels' SHA3-256 (csrc/keccak.h, the
// branch the GPU compiles, with the host fallbacks of sha512.h for its rotations and three-input
// bit operations) and the node format (csrc/trie_core.h), callable from tests/test_trie_host.py.
// Built with hipcc --offload-host-only: no GPU needed.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "keccak.h"
#include "trie_core.h"

extern "C" {

// SHA3-256 of data[0 .. len) read through the kernels' word reader from a copy placed `align` bytes
// off an 8-byte boundary, with 0xEE around it: bytes outside the record must not matter.
void tkc_sha3(const uint8_t* data, uint64_t len, uint32_t align, uint8_t out[32]) {
    std::vector<uint64_t> buf(len / 8 + 4, 0xEEEEEEEEEEEEEEEEull);
    uint8_t* p = reinterpret_cast<uint8_t*>(buf.data()) + 8 + (align & 7);
    if (len) memcpy(p, data, len);
    uint64_t d[4];
    sha3_256(d, len, PvKeccakWords(p, len));
    memcpy(out, d, 32);
}

// encode a string, decode it again: returns the encoded size, 0 when the round trip fails
uint64_t tkc_rlp_str(const uint8_t* p, uint64_t len, uint8_t* enc) {
    const uint64_t n = tr_put_str(enc, p, len);
    TrItem it;
    if (n != tr_str_size(p, len) || !tr_rlp_item(enc, enc + n, &it) || it.list || it.raw_len != n || it.len != len ||
        (len && memcmp(it.p, p, len)))
        return 0;
    return n;
}
// the prefix of a list of `payload` bytes; returns its size
uint32_t tkc_list_prefix(uint64_t payload, uint8_t* enc) { return tr_put_prefix(enc, payload, 0xc0); }

// pack n nibbles, check the packed form unpacks to them: returns the packed size, 0 on a failed round trip
uint32_t tkc_hp(const uint8_t* nib, uint32_t n, int term, uint8_t* packed) {
    const uint32_t size = tr_hp_size(n);
    tr_hp_pack(packed, nib, n, term != 0);
    bool t;
    if (tr_hp_nibbles(packed, size, &t) != (int64_t)n || t != (term != 0)) return 0;
    std::vector<uint8_t> back(n + 2);
    tr_hp_unpack(back.data(), packed, size);
    if (n && memcmp(back.data(), nib, n)) return 0;
    return size;
}

// the node kind (1 leaf, 2 extension, 3 branch) of exactly these bytes, -1 when malformed; for a valid
// node *nibbles, *value_len and a bit mask of its non-blank children
int tkc_decode(const uint8_t* p, uint64_t len, uint32_t* nibbles, uint64_t* value_len, uint32_t* children) {
    std::vector<uint8_t> own(p, p + len);  // exactly len bytes: a read past the record is a read past the block
    TrDecoded d;
    if (!tr_decode_node(own.data(), len, &d)) return -1;
    *nibbles = d.kind == TR_BRANCH ? 0 : d.nibbles;
    *value_len = d.kind == TR_EXT ? 0 : d.value_len;
    *children = 0;
    for (int i = 0; i < (d.kind == TR_BRANCH ? 16 : d.kind == TR_EXT ? 1 : 0); i++)
        if (d.child[i].kind != TR_BLANK) *children |= 1u << i;
    return d.kind;
}

}  // extern "C"
