// TEST INFRASTRUCTURE: the C++ host path of pv_merkle_prove_batch (csrc/merkle_host.cpp, linked from
// libplenum_verify.so) with the number of threads chosen by the caller, so tests/test_prove_host.py can
// hold one thread against sixteen. Arguments as pv_merkle_prove_batch, already validated by the test.
#include "merkle_host.h"

extern "C" void ph_prove(const uint8_t* leaf_hash, uint64_t n_leaves, const uint8_t* node_hash, const uint8_t* kind,
                         const uint64_t* a, const uint64_t* b, uint64_t q, const uint64_t* out_off, uint8_t* out,
                         uint8_t* status, uint32_t threads) {
    pv_merkle_host_prove(leaf_hash, n_leaves, node_hash, kind, a, b, q, out_off, out, status, threads);
}
