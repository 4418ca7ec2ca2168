// The structural half of the batched state-trie update and the host path of its hashing
// (trie_host.cpp): plain C++ over trie_core.h and keccak.h. Internal, not ABI.
#ifndef PV_TRIE_HOST_H
#define PV_TRIE_HOST_H

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/plenum_verify.h"

// One node to hash: arena[off .. off + len) is its RLP (off a multiple of 8), its digest goes to
// arena[hole .. hole + 32) in its parent's record (PV_TRIE_NO_HOLE: the root). Records are ordered
// deepest first; `next` is the index of the first record of the next shallower depth.
struct PvTrieRec {
    uint64_t off;
    uint64_t hole;
    uint32_t len;
    uint32_t depth;
    uint32_t next;
    uint32_t pad;
};
static constexpr uint64_t PV_TRIE_NO_HOLE = ~0ull;

struct PvTriePlan {
    std::vector<uint64_t> arena;  // 64-bit words: every record starts on one
    uint64_t arena_bytes = 0;
    std::vector<PvTrieRec> recs;
    std::vector<uint8_t> missing;  // 32 bytes per existing node the update needs and was not given
    bool blank = false;            // the new trie is empty (no record)
};

struct PvTrieIn {
    const uint8_t* root;  // 32 bytes
    const uint8_t* known_hash;
    const uint8_t* known_blob;
    const uint64_t* known_off;
    uint64_t n_known;
    const uint8_t* key_blob;
    const uint64_t* key_off;
    const uint8_t* val_blob;
    const uint64_t* val_off;
    uint64_t n;
};

// The canonical trie of (the mapping under in.root) overlaid with the batch, as records to hash.
// Returns PV_OK, PV_TRIE_NEED_NODES (plan.missing filled, nothing else), PV_ERR_DECODE or PV_ERR_ARG
// (err says why). Arguments are otherwise validated by the caller (offsets monotone, non-null).
int pv_trie_host_build(const PvTrieIn& in, PvTriePlan* plan, std::string* err);
// Hash the records depth by depth on up to 16 threads: digests into their holes and into
// hashes[32 i].
void pv_trie_host_hash(uint8_t* arena, const PvTrieRec* recs, uint64_t n, uint8_t* hashes);
// SHA3-256 of n records data[off[i] .. off[i + 1]) to out[32 i], on up to 16 threads.
void pv_sha3_host_batch(const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* out);

// State proofs on the host path: SHA3-256 and tr_rlp_canonical of every record, then tr_proof_walk of
// every query (trie_core.h), each on up to 16 threads. Arguments are validated by the caller.
void pv_proof_host(const PvProofIn& in, uint8_t* status);
// pv_trie_proof_split (plenum_verify.h) once its pointers are checked.
int pv_proof_split_host(const uint8_t* ser, const uint64_t* ser_off, uint64_t n_proofs, uint64_t* proof_first,
                        uint64_t* node_off, uint64_t* node_len, uint64_t node_cap, uint64_t* n_nodes, uint8_t* proof_ok);
// PV_OK, or PV_ERR_ARG with *err set: the checks of pv_trie_verify_proofs on host-readable arguments.
int pv_proof_check_args(const PvProofIn& in, const char** err);

extern const uint8_t PV_TRIE_BLANK_ROOT[32];

#endif  // PV_TRIE_HOST_H
