// The host SHA-256 of signing_json.cpp (the x86 SHA extensions when the CPU has them, else scalar),
// for the other host translation units of libplenum_verify.so (merkle_host.cpp). Internal, not ABI.
#ifndef PV_SHA256_HOST_H
#define PV_SHA256_HOST_H

#include <stddef.h>
#include <stdint.h>

// SHA-256 of data[0, len) into out[32].
void pv_sha256_host(const uint8_t* data, size_t len, uint8_t out[32]);

#endif  // PV_SHA256_HOST_H
