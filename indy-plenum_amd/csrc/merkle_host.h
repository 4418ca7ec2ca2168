// The host path of the Merkle entries (merkle_host.cpp): the contract of pv_merkle_append_batch and
// pv_merkle_verify_inclusion_batch in C++ over merkle_core.h and the host SHA-256, arguments already
// validated. Internal, not ABI.
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

#endif  // PV_MERKLE_HOST_H
