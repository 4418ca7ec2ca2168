// What a ledger Merkle entry (pv_merkle.hip) decides from numbers alone, before it touches the device: the
// chunks of an append-like call and where each chunk's outputs lie in the call's arrays, the replies of a
// catch-up that a chunk has to look at, the chunks of the proof checks and of proof generation, and the
// argument checks of the eleven entries. Host only, without a runtime call and without pv_fail, so
// tests/native/merkle_plan_check.cpp runs every function on a CPU; the entries ask here, add their own name
// to a refusal and enqueue what the plan names.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "../../include/plenum_verify.h"  // PvMerkleOut
#include "merkle_core.h"
#include "workspace.h"  // pv_offsets_monotone

#pragma GCC visibility push(hidden)  // internal to libplenum_verify.so
namespace pvhost {

// A host-entry chunk also ends at this many data bytes (it is staged whole).
static constexpr uint64_t MK_CHUNK_BYTES = 1ull << 30;

// ---- the chunks of an append-like call: n leaves appended to a tree of size s0 ------------------------------
struct MkChunk {
    uint64_t c0, m;            // leaves [c0, c0 + m) of the call, m >= 1
    uint64_t s;                // the tree's size before the chunk, s0 + c0
    uint64_t pbase, node_off;  // audit-path hashes / new nodes of the call's leaves before c0
    uint64_t n_nodes, n_path;  // ... and of the chunk's own leaves (pv_merkle_plan of s, m)
    bool is_last;
};

// The chunk that starts at leaf c0 < n: at most max_leaves leaves and, where the records' offsets off[0..n]
// are given (the host-buffer entries; null: device data, the leaf bound only), the longest prefix of at most
// max_bytes data bytes, but at least one leaf (a single record above the bound is a chunk of its own).
inline MkChunk append_chunk(uint64_t s0, uint64_t n, uint64_t c0, uint64_t max_leaves, const uint64_t* off = nullptr,
                            uint64_t max_bytes = MK_CHUNK_BYTES) {
    MkChunk c;
    c.c0 = c0;
    c.m = std::min<uint64_t>(max_leaves, n - c0);
    if (off && off[c0 + c.m] - off[c0] > max_bytes) {
        const uint64_t* e = std::upper_bound(off + c0 + 1, off + c0 + c.m + 1, off[c0] + max_bytes);
        c.m = std::max<uint64_t>(1, (uint64_t)(e - (off + c0)) - 1);
    }
    c.s = s0 + c0;
    c.pbase = pv_merkle_popc_sum(c.s) - pv_merkle_popc_sum(s0);
    c.node_off = pv_merkle_node_count(c.s) - pv_merkle_node_count(s0);
    uint64_t n_front;
    pv_merkle_plan_core(c.s, c.m, &c.n_nodes, &n_front, &c.n_path);
    c.is_last = c0 + c.m == n;
    return c;
}

// body(chunk) for every chunk of the call in order, up to the first non-zero return, which is returned.
template <class F>
inline int for_each_append_chunk(uint64_t s0, uint64_t n, uint64_t max_leaves, const uint64_t* off, uint64_t max_bytes,
                                 F&& body) {
    for (uint64_t c0 = 0; c0 < n;) {
        const MkChunk c = append_chunk(s0, n, c0, max_leaves, off, max_bytes);
        if (int rc = body(c)) return rc;
        c0 += c.m;
    }
    return 0;
}

// The chunk's part of the call's outputs: every array of `out` that is wanted, from the chunk's first
// element on (32 m leaf hashes and roots, 32 n_nodes node hashes, 32 n_path path hashes, m + 1 path offsets);
// the root and the frontier belong to the last chunk. An output the caller does not take stays null.
inline PvMerkleOut chunk_outputs(const PvMerkleOut& out, const MkChunk& c) {
    PvMerkleOut o{};
    if (out.leaf_hash) o.leaf_hash = out.leaf_hash + 32 * c.c0;
    if (out.node_hash) o.node_hash = out.node_hash + 32 * c.node_off;
    if (out.roots) o.roots = out.roots + 32 * c.c0;
    if (out.path) o.path = out.path + 32 * c.pbase;
    if (out.path) o.path_off = out.path_off + c.c0;
    if (c.is_last) o.root = out.root;
    if (c.is_last) o.frontier = out.frontier;
    return o;
}

// The replies [r0, r1) of a catch-up that the chunk of m leaves at size s has to look at: those whose end
// lies in (s, s + m], from the start of the first one's verdict word (r0 is a multiple of 64; the earlier
// replies of that word end in earlier chunks and are passed over by the kernel). end[0..R) increases strictly.
struct MkWindow {
    uint64_t r0, r1;
};
inline MkWindow reply_window(const uint64_t* end, uint64_t R, uint64_t s, uint64_t m) {
    const uint64_t first = (uint64_t)(std::upper_bound(end, end + R, s) - end);
    return MkWindow{first & ~63ull, (uint64_t)(std::upper_bound(end, end + R, s + m) - end)};
}

// ---- the chunks of the proof checks and of proof generation: items [c0, c0 + m) --------------------------------
// The proof checks store one verdict word per 64 proofs, so their chunk is the leaf bound rounded up to
// whole words; proof generation stores no words and takes the bound as it is.
inline uint64_t verdict_chunk(uint64_t max_leaves) { return (max_leaves + 63) & ~63ull; }
// body(c0, m) for every chunk of n items in order, up to the first non-zero return, which is returned.
template <class F>
inline int for_each_span(uint64_t n, uint64_t chunk, F&& body) {
    for (uint64_t c0 = 0; c0 < n; c0 += chunk)
        if (int rc = body(c0, std::min<uint64_t>(chunk, n - c0))) return rc;
    return 0;
}

// ---- the argument checks: nullptr, or why the call is refused (the entry puts its name in front) -------------
// a, b and a + b stay below 2^48; `why` is the entry's wording.
inline const char* check_sizes(uint64_t a, uint64_t b, const char* why = "tree_size + n must stay below 2^48") {
    return a >> PV_MERKLE_MAX_BITS || b >> PV_MERKLE_MAX_BITS || (a + b) >> PV_MERKLE_MAX_BITS ? why : nullptr;
}
// At most 2^32 - 1 proofs, replies or queries: `why` names them.
inline const char* check_count(uint64_t n, const char* why) { return n >> 32 ? why : nullptr; }

// The append arguments of a host-buffer entry.
inline const char* check_append_host(uint64_t tree_size, const uint8_t* frontier, const uint8_t* data, const uint64_t* off,
                                     uint64_t n) {
    if (const char* why = check_sizes(tree_size, n)) return why;
    if (tree_size > 0 && !frontier) return "a tree of size > 0 needs its frontier";
    if (n > 0) {
        if (!off) return "null offsets";
        if (!pv_offsets_monotone(off, n)) return "offsets must be non-decreasing";
        if (!data && off[n] != off[0]) return "null data";
    }
    return nullptr;
}
// ... and of a device-buffer entry, which cannot read the offsets.
inline const char* check_append_device(uint64_t tree_size, const void* d_frontier, const void* d_data, const void* d_off,
                                       uint64_t n) {
    if (const char* why = check_sizes(tree_size, n)) return why;
    if (tree_size > 0 && !d_frontier) return "a tree of size > 0 needs its frontier";
    if (n > 0 && (!d_data || !d_off)) return "null pointer";
    return nullptr;
}
inline const char* check_out(const PvMerkleOut* out) {
    if (!out) return "null output struct";
    if ((out->path != nullptr) != (out->path_off != nullptr)) return "path and path_off go together";
    return nullptr;
}
// proof_off[0..n] (not null) over `proof`, which may be null only if no proof holds a hash.
inline const char* check_proof_offsets(const uint8_t* proof, const uint64_t* proof_off, uint64_t n) {
    return !pv_offsets_monotone(proof_off, n) || (!proof && proof_off[n] != proof_off[0])
               ? "proof offsets must be non-decreasing over a proof array"
               : nullptr;
}
// end[0..R), R >= 1 (a catch-up's replies as a host-buffer entry has them).
inline const char* check_reply_ends(const uint64_t* end, uint64_t R, uint64_t tree_size, uint64_t n) {
    uint64_t bad = end[0] <= tree_size || end[R - 1] > tree_size + n;
    for (uint64_t r = 1; r < R; r++) bad |= end[r] <= end[r - 1];
    return bad ? "reply ends must increase strictly within (tree_size, tree_size + n]" : nullptr;
}
// The kernels load and store hashes as 16-byte vectors; null (an array that is not given) passes.
inline const char* check_aligned(std::initializer_list<const void*> hash_arrays) {
    for (const void* p : hash_arrays)
        if (reinterpret_cast<uintptr_t>(p) & 15u) return "hash arrays must be 16-byte aligned";
    return nullptr;
}
// The hash arrays of an append-like device-buffer entry: the input frontier and the outputs.
inline const char* check_append_aligned(const void* d_frontier, const PvMerkleOut& d_out) {
    return check_aligned({d_frontier, d_out.leaf_hash, d_out.node_hash, d_out.frontier, d_out.root, d_out.roots, d_out.path});
}

}  // namespace pvhost
#pragma GCC visibility pop
