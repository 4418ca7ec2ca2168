// The host path of the Merkle entries (merkle_host.cpp): the contract of pv_merkle_append_batch,
// pv_merkle_verify_inclusion_batch, pv_merkle_verify_consistency_batch, pv_merkle_catchup_batch and
// pv_merkle_prove_batch in C++ over merkle_core.h and the host SHA-256, arguments already validated
// (merkle_plan.h). Internal, not ABI.
#ifndef PV_MERKLE_HOST_H
#define PV_MERKLE_HOST_H

#include <stdint.h>

#include "../../include/plenum_verify.h"

void pv_merkle_host_append(uint64_t tree_size, const uint8_t* frontier, const uint8_t* data, const uint64_t* off,
                           uint64_t n, const PvMerkleOut* out);
void pv_merkle_host_verify(const uint8_t* data, const uint64_t* off, const uint8_t* leaf_hash,
                           const uint64_t* leaf_index, const uint64_t* tree_size, const uint8_t* proof,
                           const uint64_t* proof_off, const uint8_t* root, uint64_t n, uint8_t* status,
                           uint8_t* verdict_bits);
void pv_merkle_host_consistency(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_root,
                                const uint8_t* new_root, const uint8_t* proof, const uint64_t* proof_off, uint64_t n,
                                uint8_t* status, uint8_t* verdict_bits);
void pv_merkle_host_catchup(uint64_t tree_size, const uint8_t* frontier, const uint8_t* data, const uint64_t* off, uint64_t n,
                            const uint64_t* reply_end, uint64_t n_replies, uint64_t final_size, const uint8_t* final_root,
                            const uint8_t* proof, const uint64_t* proof_off, const PvMerkleOut* out, uint8_t* status,
                            uint8_t* verdict_bits);
// out_end = out_off[q]: no slot may end beyond it. threads = 0: up to 16.
void pv_merkle_host_prove(const uint8_t* leaf_hash, uint64_t n_leaves, const uint8_t* node_hash, const uint8_t* kind,
                          const uint64_t* a, const uint64_t* b, uint64_t q, const uint64_t* out_off, uint8_t* out,
                          uint8_t* status, unsigned threads = 0);
// Queries that pv_merkle_host_prove would not write (status 1 or 2); arithmetic only.
uint64_t pv_merkle_host_prove_unwritten(uint64_t n_leaves, const uint8_t* kind, const uint64_t* a, const uint64_t* b, uint64_t q,
                                        const uint64_t* out_off);

#endif  // PV_MERKLE_HOST_H
