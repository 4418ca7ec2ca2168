// The ledger's SHA-256 Merkle tree on the GPU: n sequential CompactMerkleTree.append calls
// (ledger/compact_merkle_tree.py:95-160) as one batch, and MerkleVerifier.verify_leaf_inclusion
// (ledger/merkle_verifier.py:155-266) for a batch of proofs. Index arithmetic: merkle_core.h (shared with
// the host path and the host-compiled check library); hashing: sha256.h; the chunks of a call, where a
// chunk's outputs lie, and the entries' argument checks: merkle_plan.h (tested on a CPU).
//
// A batch of n leaves appended to a tree of size s needs no sequential walk (merkle_core.h): every hash
// the reference would write or return is a leaf hash, an aligned node completed inside the batch, or an
// entry of the input frontier. Per chunk of at most pv_merkle_chunk leaves:
//   1. pv_merkle_leaf_kernel    one lane per leaf: SHA-256(0x00 || data) over variable-length records at
//                               any byte offset (aligned 32-bit loads, funnel-shifted; no byte past the
//                               record's last aligned word is read).
//   2. pv_merkle_tile_kernel    one workgroup per tile of 1,024 leaves BY ABSOLUTE INDEX: heights 1..10 in
//                               LDS, every new node also stored at its hash-store position.
//      pv_merkle_upper_kernel   one workgroup, the same tile routine over heights 10 -> 20 -> 30 -> 40 -> 48
//                               (few nodes); launched only when the chunk completes a node above height 10.
//   3. pv_merkle_proof_kernel   (optional) one lane per leaf: its audit path gathered from the input
//                               frontier, the new nodes and the leaf hashes, and the root after it.
//   4. pv_merkle_finish_kernel  one wave: the frontier after the chunk (the next chunk's input) and its root.
//   5. pv_merkle_catchup_kernel (catch-up only) one lane per reply whose end lies in the chunk: the root at
//                               that size folded from the chunk's view, then the consistency walk against
//                               the call's final size and root.
// and pv_merkle_verify_kernel / pv_merkle_consistency_kernel (MerkleVerifier.verify_tree_consistency,
// ledger/merkle_verifier.py:23-153), one lane per proof, and pv_merkle_prove_kernel (inclusion_proof,
// consistency_proof and merkle_tree_hash from a hash store, ledger/compact_merkle_tree.py:198-249), one lane
// per query. Launches per chunk: at most six, whatever n is; no host round trip between them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/plenum_verify.h"
#include "merkle_core.h"
#include "merkle_host.h"
#include "merkle_plan.h"
#include "pv_internal.h"
#include "sha256.h"

using namespace pvhost;  // merkle_plan.h

// The library's dynamic symbol table has always held this instantiation (the entries built their messages
// through it out of line, forty times; the two sites left are inlined). Instantiated here so that the table
// stays what it was.
template std::string std::operator+(const std::string&, const char*);

namespace {

constexpr int MK_BLOCK = 256;

struct MkHash {
    uint32_t w[8];  // digest words (sha256.h)
};

__device__ __forceinline__ MkHash mk_load(const uint32_t* p) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    const uint32_t le[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    MkHash h;
    sha256_words_from_le(h.w, le);
    return h;
}
__device__ __forceinline__ void mk_store(uint32_t* p, const MkHash& h) {
    reinterpret_cast<uint4*>(p)[0] =
        make_uint4(pv_bswap32(h.w[0]), pv_bswap32(h.w[1]), pv_bswap32(h.w[2]), pv_bswap32(h.w[3]));
    reinterpret_cast<uint4*>(p)[1] =
        make_uint4(pv_bswap32(h.w[4]), pv_bswap32(h.w[5]), pv_bswap32(h.w[6]), pv_bswap32(h.w[7]));
}
__device__ __forceinline__ void mk_copy(uint32_t* dst, const uint32_t* src) {
    reinterpret_cast<uint4*>(dst)[0] = reinterpret_cast<const uint4*>(src)[0];
    reinterpret_cast<uint4*>(dst)[1] = reinterpret_cast<const uint4*>(src)[1];
}
__device__ __forceinline__ MkHash mk_children(const MkHash& l, const MkHash& r) {
    MkHash o;
    sha256_hash_children(o.w, l.w, r.w);
    return o;
}

// The chunk's view of the tree: the input frontier, its leaf hashes and its new nodes (32-byte hashes,
// 16-byte aligned).
struct MkView {
    uint64_t s, n;
    const uint32_t* oldf;
    const uint32_t* leaf;
    const uint32_t* node;
    __device__ __forceinline__ const uint32_t* at(const PvMerkleRef& r) const {
        return (r.kind == PV_MK_OLD ? oldf : r.kind == PV_MK_LEAF ? leaf : node) + 8 * r.idx;
    }
};

__device__ __forceinline__ MkHash mk_leaf_hash(const uint8_t* data, uint64_t len) {
    MkHash h;
    const PvRecordWords words(data, len);
    sha256_prefixed<1>(h.w, 0u, len, words);
    return h;
}

// The hooks of merkle_core.h's walks: hash_children, a hash of the chunk's view, and hash k of the proof that
// starts at hash p0 of `proof`.
struct MkCombine {
    __device__ __forceinline__ void operator()(MkHash& o, const MkHash& l, const MkHash& r) const { o = mk_children(l, r); }
};
struct MkViewLoad {
    const MkView& v;
    __device__ __forceinline__ void operator()(const PvMerkleRef& r, MkHash& o) const { o = mk_load(v.at(r)); }
};
struct MkProofLoad {
    const uint32_t* proof;
    uint64_t p0;
    __device__ __forceinline__ void operator()(uint64_t k, MkHash& o) const { o = mk_load(proof + 8 * (p0 + k)); }
};
__device__ __forceinline__ bool mk_equal(const MkHash& a, const MkHash& b) {
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) diff |= a.w[k] ^ b.w[k];
    return diff == 0;
}

// ------------------------------------------------------------------------------------------ kernels

__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_leaf_kernel(const uint8_t* __restrict__ data,
                                                                  const uint64_t* __restrict__ off, uint64_t n,
                                                                  uint32_t* __restrict__ leaf) {
    const uint64_t i = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], b = off[i + 1];
    mk_store(leaf + 8 * i, mk_leaf_hash(data + a, b - a));
}

// Tile k of pass h0 (merkle_core.h): entries of height h0 into LDS, heights h0 + 1 .. h0 + 10 reduced in
// place (node q of level l lives in the slot of its leftmost entry, q << l), each new node also stored
// at its hash-store position. Called by every thread of the workgroup.
__device__ __forceinline__ void mk_tile_reduce(uint32_t h0, uint64_t k, const MkView& v, uint32_t* node_out, uint4* lds) {
    const uint64_t base = pv_merkle_node_count(v.s);
    for (uint32_t e = threadIdx.x; e < PV_MERKLE_TILE; e += MK_BLOCK) {
        const uint64_t u = ((k << PV_MERKLE_TILE_LOG) + e + 1) << h0;
        if (pv_merkle_is_new(v.s, v.n, u)) {
            const uint32_t* src = v.at(pv_merkle_node_ref(v.s, u, h0));
            lds[2 * e] = reinterpret_cast<const uint4*>(src)[0];
            lds[2 * e + 1] = reinterpret_cast<const uint4*>(src)[1];
        }
    }
    __syncthreads();
    for (uint32_t l = 1; l <= PV_MERKLE_TILE_LOG; l++) {
        const uint32_t h = h0 + l;
        if (h > PV_MERKLE_MAX_BITS) break;  // uniform
        for (uint32_t q = threadIdx.x; q < (PV_MERKLE_TILE >> l); q += MK_BLOCK) {
            const uint64_t u = ((k << PV_MERKLE_TILE_LOG) + ((uint64_t)(q + 1) << l)) << h0;
            if (!pv_merkle_is_new(v.s, v.n, u)) continue;
            const uint32_t ls = (2 * q) << (l - 1), rs = (2 * q + 1) << (l - 1);
            // the left child ends at u - 2^(h-1): inside the old tree it is the input frontier's entry for bit h - 1
            const bool left_new = u - (1ull << (h - 1)) > v.s;
            const uint32_t* lp = left_new ? reinterpret_cast<const uint32_t*>(lds + 2 * ls)
                                          : v.oldf + 8 * pv_popc64(v.s >> h);
            const MkHash left = mk_load(lp), right = mk_load(reinterpret_cast<const uint32_t*>(lds + 2 * rs));
            const MkHash out = mk_children(left, right);
            mk_store(reinterpret_cast<uint32_t*>(lds + 2 * ls), out);
            mk_store(node_out + 8 * (pv_merkle_node_pos(u, h) - base), out);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_tile_kernel(MkView v, uint64_t tile_first, uint32_t* node_out) {
    __shared__ uint4 lds[2 * PV_MERKLE_TILE];
    mk_tile_reduce(0, tile_first + blockIdx.x, v, node_out, lds);
}

// Heights above 10: one workgroup walks the passes h0 = 10, 20, ... while the chunk completes a node above
// h0; a pass reads the nodes of height h0 the previous pass (or the tile kernel) stored.
__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_upper_kernel(MkView v, uint32_t* node_out) {
    __shared__ uint4 lds[2 * PV_MERKLE_TILE];
    for (uint32_t h0 = PV_MERKLE_TILE_LOG; h0 < PV_MERKLE_MAX_BITS && pv_merkle_any_above(v.s, v.n, h0);
         h0 += PV_MERKLE_TILE_LOG) {
        uint64_t first, count;
        pv_merkle_tiles(v.s, v.n, h0, &first, &count);
        for (uint64_t k = 0; k < count; k++) {
            mk_tile_reduce(h0, first + k, v, node_out, lds);
            __syncthreads();
        }
        __threadfence_block();  // the next pass reads this pass's stores
    }
}

// One lane per leaf i of the chunk (appended at size t = s + i): path (may be null) receives its audit
// path at path[32 (path_off[i] - poff_base)...], path_off[i] = poff_base + hashes of the chunk's earlier
// leaves; roots (may be null) the root after the leaf.
__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_proof_kernel(MkView v, uint32_t* __restrict__ path,
                                                                   uint64_t* __restrict__ path_off,
                                                                   uint64_t poff_base, uint32_t* __restrict__ roots) {
    const uint64_t i = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    if (i >= v.n) return;
    const uint64_t t = v.s + i;
    if (path) {
        const uint64_t at = pv_merkle_popc_sum(t) - pv_merkle_popc_sum(v.s);
        path_off[i] = poff_base + at;
        if (i == v.n - 1) path_off[v.n] = poff_base + at + pv_popc64(t);
        uint32_t* dst = path + 8 * at;
        pv_merkle_audit_path(v.s, t, [&](uint32_t k, const PvMerkleRef& r) { mk_copy(dst + 8 * k, v.at(r)); });
    }
    if (roots) {
        MkHash acc;
        pv_merkle_fold_root(
            acc, v.s, t + 1, MkViewLoad{v},
            MkCombine());
        mk_store(roots + 8 * i, acc);
    }
}

// One wave: the frontier of size s + n (largest subtree first, the rest of the 64 entries zero) and, if
// asked for, its root (n = 0: the input tree's).
__global__ __launch_bounds__(64) void pv_merkle_finish_kernel(MkView v, uint32_t* __restrict__ frontier,
                                                              uint32_t* __restrict__ root) {
    const uint64_t t = v.s + v.n;
    const uint32_t lane = threadIdx.x, m = pv_popc64(t);
    // entry `lane` is the lane-th set bit of t from the top
    uint64_t rest = t;
    for (uint32_t k = 0; k < m - 1 - lane && lane < m; k++) rest &= rest - 1;  // drop the m - 1 - lane lowest bits
    if (lane < m) {
        mk_copy(frontier + 8 * lane, v.at(pv_merkle_frontier_ref(v.s, t, (uint32_t)__builtin_ctzll(rest))));
    } else {
        reinterpret_cast<uint4*>(frontier + 8 * lane)[0] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4*>(frontier + 8 * lane)[1] = make_uint4(0, 0, 0, 0);
    }
    if (root && lane == 0 && t == 0) {  // the empty tree: SHA-256 of the empty string
        const MkHash empty{{0xe3b0c442u, 0x98fc1c14u, 0x9afbf4c8u, 0x996fb924u, 0x27ae41e4u, 0x649b934cu, 0xa495991bu, 0x7852b855u}};
        mk_store(root, empty);
    } else if (root && lane == 0) {
        MkHash acc;
        pv_merkle_fold_root(
            acc, v.s, t, MkViewLoad{v},
            MkCombine());
        mk_store(root, acc);
    }
}

// One lane per proof; verdict word w bit b = proof 64 w + b (one ballot per wave). The comparison with the
// root and the ballot's store are written out here and in pv_merkle_consistency_kernel: through mk_equal or
// through a shared epilogue function the compiler emits other instructions for these two kernels.
__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_verify_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ off, const uint32_t* __restrict__ leaf_hash,
    const uint64_t* __restrict__ leaf_index, const uint64_t* __restrict__ tree_size, const uint32_t* __restrict__ proof,
    const uint64_t* __restrict__ proof_off, const uint32_t* __restrict__ root, uint64_t n, uint8_t* __restrict__ status,
    uint64_t* __restrict__ verdict) {
    const uint64_t i = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    bool ok = false;
    if (i < n) {
        MkHash acc;
        if (leaf_hash) {
            acc = mk_load(leaf_hash + 8 * i);
        } else {
            const uint64_t a = off[i], b = off[i + 1];
            acc = mk_leaf_hash(data + a, b - a);
        }
        const uint64_t p0 = proof_off[i], plen = proof_off[i + 1] - p0;
        const uint32_t st = pv_merkle_path_check(
            acc, leaf_index[i], tree_size[i], plen, MkProofLoad{proof, p0},
            MkCombine());
        status[i] = (uint8_t)st;
        if (st == PV_MK_COMPARED) {
            const MkHash want = mk_load(root + 8 * i);
            uint32_t diff = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) diff |= acc.w[k] ^ want.w[k];
            ok = diff == 0;
        }
    }
    const uint64_t word = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && i < n) verdict[i >> 6] = word;
}

// the consistency walk of merkle_core.h over proof hashes [p0, p0 + plen) of `proof`
__device__ __forceinline__ uint32_t mk_consistency(uint64_t old_size, uint64_t new_size, const MkHash& old_root,
                                                   const MkHash& new_root, const uint32_t* __restrict__ proof,
                                                   uint64_t p0, uint64_t plen) {
    return pv_merkle_consistency_check(
        old_size, new_size, old_root, new_root, plen, MkProofLoad{proof, p0},
        MkCombine(),
        [](const MkHash& a, const MkHash& b) { return mk_equal(a, b); });
}

// One lane per consistency proof; verdict words as pv_merkle_verify_kernel.
__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_consistency_kernel(
    const uint64_t* __restrict__ old_size, const uint64_t* __restrict__ new_size, const uint32_t* __restrict__ old_root,
    const uint32_t* __restrict__ new_root, const uint32_t* __restrict__ proof, const uint64_t* __restrict__ proof_off,
    uint64_t n, uint8_t* __restrict__ status, uint64_t* __restrict__ verdict) {
    const uint64_t i = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const uint64_t p0 = proof_off[i];
        const uint32_t st = mk_consistency(old_size[i], new_size[i], mk_load(old_root + 8 * i), mk_load(new_root + 8 * i),
                                           proof, p0, proof_off[i + 1] - p0);
        status[i] = (uint8_t)st;
        ok = st == PV_MK_CONSISTENT;
    }
    const uint64_t word = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && i < n) verdict[i >> 6] = word;
}

// The replies of a catch-up: reply r ends at absolute size end[r] and carries proof hashes
// [proof_off[r], proof_off[r + 1]) for (end[r], final_size). status is preset to PV_MK_REPLY_RANGE and the
// verdict words to zero before the first chunk; a chunk's launch covers replies [r0, r1), r0 a multiple of 64.
struct MkReplies {
    const uint64_t* end;
    const uint32_t* proof;
    const uint64_t* proof_off;
    const uint32_t* final_root;
    uint64_t final_size, r0, r1;
    uint8_t* status;
    uint64_t* verdict;
};

// One lane per reply; the lanes whose reply ends inside the chunk (s < end <= s + n) fold the root at that
// size from the chunk's view (old frontier entries, leaf hashes, new nodes) and walk the proof. A wave's
// 64 replies may end in different chunks, so the ballot is OR-ed into the verdict word.
__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_catchup_kernel(MkView v, MkReplies q) {
    const uint64_t r = q.r0 + (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    bool ok = false;
    if (r < q.r1) {
        const uint64_t e = q.end[r];
        if (e > v.s && e <= v.s + v.n) {
            MkHash old_root;
            pv_merkle_fold_root(
                old_root, v.s, e, MkViewLoad{v},
                MkCombine());
            const uint64_t p0 = q.proof_off[r];
            const uint32_t st = mk_consistency(e, q.final_size, old_root, mk_load(q.final_root), q.proof, p0,
                                               q.proof_off[r + 1] - p0);
            q.status[r] = (uint8_t)st;
            ok = st == PV_MK_CONSISTENT;
        }
    }
    const uint64_t word = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && word) atomicOr(reinterpret_cast<unsigned long long*>(q.verdict + (r >> 6)), word);
}

// The queries of a proof generation (merkle_core.h): one lane per query, the store's leaf hashes by leaf
// index and node hashes by store position. Proof i goes to out[8 out_off[i]...] (32-bit words), and only
// if its own length is the room of its slot and the slot ends at or before *out_end.
struct MkProve {
    const uint32_t* leaf;
    const uint32_t* node;
    uint64_t n_leaves;
    const uint8_t* kind;
    const uint64_t* a;
    const uint64_t* b;
    const uint64_t* out_off;
    const uint64_t* out_end;
    uint32_t* out;
    uint8_t* status;
};

// Aligned subtrees are 32-byte gathers made along the walk; the ragged ones are prefixes of one fold kept in
// registers, run after the walk so that the lanes of a wave hash in step (with the fold inside the walk each
// lane hashed at its own levels, and 4 of 64 lanes were active per instruction on mixed queries). Lanes still
// diverge on the fold length.
__global__ __launch_bounds__(MK_BLOCK) void pv_merkle_prove_kernel(MkProve p, uint64_t q) {
    const uint64_t i = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
    if (i >= q) return;
    const uint32_t kind = p.kind[i];
    const uint64_t a = p.a[i], b = p.b[i];
    if (!pv_merkle_query_valid(kind, a, b, p.n_leaves)) {
        p.status[i] = PV_MK_Q_RANGE;
        return;
    }
    const uint64_t at = p.out_off[i], end = p.out_off[i + 1];
    if (end - at != pv_merkle_prove_len(kind, a, b) || end > *p.out_end) {
        p.status[i] = PV_MK_Q_ROOM;
        return;
    }
    uint32_t* dst = p.out + 8 * at;
    auto src = [&](const PvMerkleElem& e) { return (e.tag == PV_MK_E_LEAF ? p.leaf : p.node) + 8 * e.idx; };
    pv_merkle_prove<MkHash>(
        kind, a, b, [&](uint32_t k, const PvMerkleElem& e) { mk_copy(dst + 8 * k, src(e)); },
        [&](const PvMerkleElem& e, MkHash& o) { o = mk_load(src(e)); },
        MkCombine(),
        [&](uint32_t k, const MkHash& acc) { mk_store(dst + 8 * k, acc); });
    p.status[i] = PV_MK_PROVED;
}

// --------------------------------------------------------------------------------------------- host

// The Merkle code's own workspace: allocated on first use (an engine that never hashes a leaf holds
// nothing), freed by pv_shutdown, handed over between caller streams by an event (workspace.h).
// Launches are serialised on g_mk_mu.
struct MkWork {
    PvDevBuf leaf, node;   // a chunk's leaf hashes / new nodes when the caller does not take them
    PvDevBuf front;        // three frontiers of 64 hashes: two for chunk chaining, one for a host entry's input
    PvStage stage;         // host entries: staged inputs and outputs of one chunk
    PvStage replies;       // the catch-up host entry: replies, proofs, status and verdicts, staged once per call
    PvHandover hand;
};
MkWork g_mk;
std::mutex g_mk_mu;
uint64_t g_mk_chunk = PV_MERKLE_CHUNK;
int g_mk_path = PV_MERKLE_AUTO;
constexpr uint64_t MK_FRONT_BYTES = 64 * 32;

// One use of the workspace on `stream`: the frontiers exist, and the hand-over around `body`. Caller
// holds g_mk_mu.
template <class F>
int mk_run(hipStream_t stream, F&& body) {
    if (int rc = g_mk.front.grow(3 * MK_FRONT_BYTES)) return rc;
    return g_mk.hand.run(stream, body);
}
uint32_t* mk_front(int which) { return g_mk.front.as<uint32_t>() + which * (MK_FRONT_BYTES / 4); }

// One chunk (merkle_plan.h): c.m > 0 leaves (d_off[0..m] into d_data) appended at size c.s with input frontier
// d_fin; the frontier after it goes to d_fout. d: the chunk's outputs as device pointers, null = not wanted
// (its frontier is not looked at). rep (may be null): the replies to check against this chunk. Caller holds
// g_mk_mu and is inside mk_run.
int mk_chunk(const MkChunk& c, const uint32_t* d_fin, const uint8_t* d_data, const uint64_t* d_off, const PvMerkleOut& d,
             uint32_t* d_fout, hipStream_t stream, const MkReplies* rep = nullptr) {
    const auto words = [](uint8_t* p) { return reinterpret_cast<uint32_t*>(p); };
    const uint64_t m = c.m;
    uint32_t* leaf = words(d.leaf_hash);
    uint32_t* node = words(d.node_hash);
    int rc;
    if (!leaf) {
        if ((rc = g_mk.leaf.grow(std::max<uint64_t>(m, 4096) * 32))) return rc;
        leaf = g_mk.leaf.as<uint32_t>();
    }
    if (!node) {
        if ((rc = g_mk.node.grow((std::max<uint64_t>(m, 4096) + 64) * 32))) return rc;  // n_nodes < m + 48
        node = g_mk.node.as<uint32_t>();
    }
    const MkView v{c.s, m, d_fin, leaf, node};
    const unsigned grid = (unsigned)((m + MK_BLOCK - 1) / MK_BLOCK);
    PV_LAUNCH(pv_merkle_leaf_kernel, dim3(grid), dim3(MK_BLOCK), 0, stream, d_data, d_off, m, leaf);
    if (c.n_nodes) {
        uint64_t first, count;
        pv_merkle_tiles(c.s, m, 0, &first, &count);
        PV_LAUNCH(pv_merkle_tile_kernel, dim3((unsigned)count), dim3(MK_BLOCK), 0, stream, v, first, node);
        if (pv_merkle_any_above(c.s, m, PV_MERKLE_TILE_LOG)) {
            PV_LAUNCH(pv_merkle_upper_kernel, dim3(1), dim3(MK_BLOCK), 0, stream, v, node);
        }
    }
    if (d.path || d.roots) {
        PV_LAUNCH(pv_merkle_proof_kernel, dim3(grid), dim3(MK_BLOCK), 0, stream, v, words(d.path), d.path_off, c.pbase,
                  words(d.roots));
    }
    if (rep && rep->r1 > rep->r0) {
        PV_LAUNCH(pv_merkle_catchup_kernel, dim3((unsigned)((rep->r1 - rep->r0 + MK_BLOCK - 1) / MK_BLOCK)), dim3(MK_BLOCK),
                  0, stream, v, *rep);
    }
    PV_LAUNCH(pv_merkle_finish_kernel, dim3(1), dim3(64), 0, stream, v, d_fout, words(d.root));
    return PV_OK;
}

// Before the first chunk of a catch-up: no reply claimed yet.
int mk_replies_preset(const MkReplies& q, uint64_t n_replies, hipStream_t stream) {
    PV_HIP(hipMemsetAsync(q.status, PV_MK_REPLY_RANGE, n_replies, stream), PV_ERR_LAUNCH);
    PV_HIP(hipMemsetAsync(q.verdict, 0, 8 * ((n_replies + 63) / 64), stream), PV_ERR_LAUNCH);
    return PV_OK;
}

// Device buffers on `stream`. Caller holds g_mk_mu.
// rep (may be null): a catch-up's replies, every chunk looks at all of them (their ends are device data).
int mk_enqueue(uint64_t s0, const uint8_t* d_frontier, const uint8_t* d_data, const uint64_t* d_off, uint64_t n,
               const PvMerkleOut& out, hipStream_t stream, const MkReplies* rep = nullptr) {
    return mk_run(stream, [&]() -> int {
        int cur = 0;
        if (rep)
            if (int rc = mk_replies_preset(*rep, rep->r1, stream)) return rc;
        const uint32_t* fin = reinterpret_cast<const uint32_t*>(d_frontier);
        if (n == 0) {  // the input tree's frontier and root
            const MkView v{s0, 0, fin, nullptr, nullptr};
            PV_LAUNCH(pv_merkle_finish_kernel, dim3(1), dim3(64), 0, stream, v, mk_front(0),
                      reinterpret_cast<uint32_t*>(out.root));
            // path_off[0] = 0, as the host path
            if (out.path_off) PV_HIP(hipMemsetAsync(out.path_off, 0, 8, stream), PV_ERR_LAUNCH);
            fin = mk_front(0);
        }
        // the caller's arrays from each chunk's first element on; the leaf bound only
        if (int rc = for_each_append_chunk(s0, n, g_mk_chunk, nullptr, 0, [&](const MkChunk& c) -> int {
                if (int rc = mk_chunk(c, fin, d_data, d_off + c.c0, chunk_outputs(out, c), mk_front(cur), stream, rep)) return rc;
                fin = mk_front(cur);
                cur ^= 1;
                return PV_OK;
            }))
            return rc;
        if (out.frontier)
            PV_HIP(hipMemcpyAsync(out.frontier, fin, MK_FRONT_BYTES, hipMemcpyDeviceToDevice, stream), PV_ERR_LAUNCH);
        return PV_OK;
    });
}

// A catch-up's replies as the host entry has them (validated: ends strictly increasing in (s0, s0 + n]).
struct MkHostReplies {
    const uint64_t* end;
    uint64_t count, final_size;
    const uint8_t* final_root;
    const uint8_t* proof;
    const uint64_t* proof_off;
    uint8_t* status;
    uint8_t* verdict_bits;
};

// The device path of the host entry on the engine stream `st`: chunk by chunk through the stage. Arguments
// validated, n > 0. Caller holds g_mk_mu and is inside mk_run.
int mk_host_entry_device(hipStream_t st, uint64_t s0, const uint8_t* frontier, const uint8_t* data, const uint64_t* off,
                         uint64_t n, const PvMerkleOut& out, const MkHostReplies* hr = nullptr) {
    MkReplies rep{};
    if (hr) {  // staged once for all chunks, in a stage of their own
        PvStage& q = g_mk.replies;
        const uint64_t R = hr->count;
        int rc = q.reset(st, false);
        if (rc) return rc;
        const int i_end = q.in(hr->end, 8 * R), i_poff = q.in_offsets(hr->proof_off, R), i_root = q.in(hr->final_root, 32),
                  i_proof = q.in(hr->proof + 32 * hr->proof_off[0], 32 * (hr->proof_off[R] - hr->proof_off[0]), 32),
                  o_status = q.out(hr->status, R), o_words = q.out(hr->verdict_bits, (R + 7) / 8, 8);
        if ((rc = q.upload())) return rc;
        rep = MkReplies{q.dev<const uint64_t>(i_end), q.dev<const uint32_t>(i_proof), q.dev<const uint64_t>(i_poff),
                        q.dev<const uint32_t>(i_root), hr->final_size, 0, R, q.dev<uint8_t>(o_status),
                        q.dev<uint64_t>(o_words)};
        if ((rc = mk_replies_preset(rep, R, st))) return rc;
    }
    if (s0) PV_HIP(hipMemcpyAsync(mk_front(2), frontier, 32ull * pv_popc64(s0), hipMemcpyHostToDevice, st), PV_ERR_LAUNCH);
    const uint32_t* fin = mk_front(2);
    int cur = 0;
    PvStage& g = g_mk.stage;
    const int rc = for_each_append_chunk(s0, n, g_mk_chunk, off, MK_CHUNK_BYTES, [&](const MkChunk& c) -> int {
        int rc = g.reset(st, false);
        if (rc) return rc;
        const PvMerkleOut h = chunk_outputs(out, c);  // in the caller's memory
        const auto section = [&](void* dst, uint64_t bytes) { return dst ? g.out(dst, bytes) : -1; };  // none if not taken
        const uint64_t* o = off + c.c0;
        const int i_off = g.in_offsets(o, c.m), i_data = g.in(data + o[0], o[c.m] - o[0], PV_BLOB_SLACK),
                  o_leaf = section(h.leaf_hash, 32 * c.m), o_node = section(h.node_hash, 32 * c.n_nodes),
                  o_roots = section(h.roots, 32 * c.m), o_poff = section(h.path_off, 8 * (c.m + 1)),
                  o_path = section(h.path, 32 * c.n_path), o_root = section(h.root, 32);
        if ((rc = g.upload())) return rc;
        const PvMerkleOut d{g.dev<uint8_t>(o_leaf),  g.dev<uint8_t>(o_node), nullptr, g.dev<uint8_t>(o_root),
                            g.dev<uint8_t>(o_roots), g.dev<uint8_t>(o_path), g.dev<uint64_t>(o_poff)};  // ... and in the stage
        if (hr) {
            const MkWindow w = reply_window(hr->end, hr->count, c.s, c.m);
            rep.r0 = w.r0, rep.r1 = w.r1;
        }
        if ((rc = mk_chunk(c, fin, g.dev<const uint8_t>(i_data), g.dev<const uint64_t>(i_off), d, mk_front(cur), st,
                           hr ? &rep : nullptr)))
            return rc;
        fin = mk_front(cur);
        cur ^= 1;
        if (h.frontier) PV_HIP(hipMemcpyAsync(h.frontier, fin, MK_FRONT_BYTES, hipMemcpyDeviceToHost, st), PV_ERR_LAUNCH);
        return g.download();  // synchronised: the stage is free for the next chunk
    });
    if (rc) return rc;
    return hr ? g_mk.replies.download() : PV_OK;
}

// The proof checks in chunks of whole verdict words, proof generation in chunks of the leaf bound
// (merkle_plan.h). Caller holds g_mk_mu (the chunk setting).
int mk_verify_enqueue(const uint8_t* d_data, const uint64_t* d_off, const uint8_t* d_leaf_hash, const uint64_t* d_index,
                      const uint64_t* d_size, const uint8_t* d_proof, const uint64_t* d_proof_off, const uint8_t* d_root,
                      uint64_t n, uint8_t* d_status, uint64_t* d_verdict, hipStream_t stream) {
    return for_each_span(n, verdict_chunk(g_mk_chunk), [&](uint64_t c0, uint64_t m) -> int {
        PV_LAUNCH(pv_merkle_verify_kernel, dim3((unsigned)((m + MK_BLOCK - 1) / MK_BLOCK)), dim3(MK_BLOCK), 0,
                  stream, d_data, d_off ? d_off + c0 : nullptr,
                  d_leaf_hash ? reinterpret_cast<const uint32_t*>(d_leaf_hash + 32 * c0) : nullptr, d_index + c0,
                  d_size + c0, reinterpret_cast<const uint32_t*>(d_proof), d_proof_off + c0,
                  reinterpret_cast<const uint32_t*>(d_root + 32 * c0), m, d_status + c0, d_verdict + c0 / 64);
        return PV_OK;
    });
}

int mk_consistency_enqueue(const uint64_t* d_old_size, const uint64_t* d_new_size, const uint8_t* d_old_root,
                           const uint8_t* d_new_root, const uint8_t* d_proof, const uint64_t* d_proof_off, uint64_t n,
                           uint8_t* d_status, uint64_t* d_verdict, hipStream_t stream) {
    return for_each_span(n, verdict_chunk(g_mk_chunk), [&](uint64_t c0, uint64_t m) -> int {
        PV_LAUNCH(pv_merkle_consistency_kernel, dim3((unsigned)((m + MK_BLOCK - 1) / MK_BLOCK)), dim3(MK_BLOCK), 0,
                  stream, d_old_size + c0, d_new_size + c0, reinterpret_cast<const uint32_t*>(d_old_root + 32 * c0),
                  reinterpret_cast<const uint32_t*>(d_new_root + 32 * c0), reinterpret_cast<const uint32_t*>(d_proof),
                  d_proof_off + c0, m, d_status + c0, d_verdict + c0 / 64);
        return PV_OK;
    });
}

int mk_prove_enqueue(const MkProve& p, uint64_t q, hipStream_t stream) {
    return for_each_span(q, g_mk_chunk, [&](uint64_t c0, uint64_t m) -> int {
        MkProve c = p;
        c.kind += c0, c.a += c0, c.b += c0, c.out_off += c0, c.status += c0;  // offsets are absolute: out stays
        PV_LAUNCH(pv_merkle_prove_kernel, dim3((unsigned)((m + MK_BLOCK - 1) / MK_BLOCK)), dim3(MK_BLOCK), 0, stream, c, m);
        return PV_OK;
    });
}

// An entry's refusals: `why` from merkle_plan.h's checks, or the entry's own.
int mk_refuse(const std::string& who, const char* why) { return pv_fail(PV_ERR_ARG, who + ": " + why); }
int mk_no_init(const std::string& who) { return pv_fail(PV_ERR_NOT_INIT, who + ": call pv_init first"); }
// the store and the count of the three proof-generation entries
const char* mk_check_store(uint64_t n_leaves, uint64_t q) {
    return check_sizes(n_leaves, 0, "the store must stay below 2^48 leaves") ?: check_count(q, "more than 2^32 - 1 queries");
}
hipStream_t mk_stream(void* stream) { return stream ? (hipStream_t)stream : pv_engine_stream(); }

// A host-buffer entry after its checks: the path chosen under g_mk_mu (work and auto_min as pv_choose_path;
// host_only: a device path has nothing to do), then host() with the lock released (the host path shares no
// workspace: CPU-only callers run side by side), or device(st) inside mk_run on the engine stream st.
template <class H, class D>
int mk_dispatch(const char* who, uint64_t work, uint64_t auto_min, bool host_only, H&& host, D&& device) {
    std::unique_lock<std::mutex> lk(g_mk_mu);
    bool dev;
    if (int rc = pv_choose_path(g_mk_path, pv_engine_stream() != nullptr, work, auto_min, who, &dev)) return rc;
    if (!dev || host_only) {
        lk.unlock();
        host();
        return PV_OK;
    }
    const hipStream_t st = pv_engine_stream();
    return mk_run(st, [&]() -> int { return device(st); });
}

}  // namespace

void pv_merkle_forget_stream(void* stream) {
    std::lock_guard<std::mutex> lk(g_mk_mu);
    g_mk.hand.forget((hipStream_t)stream);
}

void pv_merkle_shutdown() {
    std::lock_guard<std::mutex> lk(g_mk_mu);
    for (PvDevBuf* b : {&g_mk.leaf, &g_mk.node, &g_mk.front}) b->release();
    g_mk.stage.release();
    g_mk.replies.release();
    g_mk.hand.destroy();
}

// In every entry `why` is the first refusal in the order of the checks: a ?: b asks b only if a passed.
extern "C" {

int pv_merkle_plan(uint64_t tree_size, uint64_t n, uint64_t* n_nodes, uint64_t* n_frontier, uint64_t* path_hashes) {
    if (const char* why = check_sizes(tree_size, n)) return mk_refuse("pv_merkle_plan", why);
    uint64_t a, b, c;
    pv_merkle_plan_core(tree_size, n, &a, &b, &c);
    if (n_nodes) *n_nodes = a;
    if (n_frontier) *n_frontier = b;
    if (path_hashes) *path_hashes = c;
    return PV_OK;
}

int pv_merkle_chunk(uint64_t leaves) {
    std::lock_guard<std::mutex> lk(g_mk_mu);
    if (leaves > PV_MERKLE_CHUNK_MAX) return pv_fail(PV_ERR_ARG, "pv_merkle_chunk: more than 2^24 leaves");
    g_mk_chunk = leaves ? leaves : PV_MERKLE_CHUNK;
    return PV_OK;
}

int pv_merkle_path(int mode) {
    std::lock_guard<std::mutex> lk(g_mk_mu);
    if (mode != PV_MERKLE_AUTO && mode != PV_MERKLE_HOST && mode != PV_MERKLE_DEVICE)
        return pv_fail(PV_ERR_ARG, "pv_merkle_path: unknown mode");
    g_mk_path = mode;
    return PV_OK;
}

int pv_merkle_append_batch(uint64_t tree_size, const uint8_t* frontier, const uint8_t* data, const uint64_t* off,
                           uint64_t n, const PvMerkleOut* out) {
    const char* who = "pv_merkle_append_batch";
    if (const char* why = check_out(out) ?: check_append_host(tree_size, frontier, data, off, n)) return mk_refuse(who, why);
    return mk_dispatch(
        who, n, out->roots || out->path ? PV_MERKLE_AUTO_MIN_PROOFS : PV_MERKLE_AUTO_MIN, n == 0,
        [&] { pv_merkle_host_append(tree_size, frontier, data, off, n, out); },
        [&](hipStream_t st) { return mk_host_entry_device(st, tree_size, frontier, data, off, n, *out); });
}

int pv_merkle_append_batch_device(uint64_t tree_size, const uint8_t* d_frontier, const uint8_t* d_data,
                                  const uint64_t* d_off, uint64_t n, const PvMerkleOut* d_out, void* stream) {
    const char* who = "pv_merkle_append_batch_device";
    if (!pv_engine_stream()) return mk_no_init(who);
    if (const char* why = check_out(d_out) ?: check_append_device(tree_size, d_frontier, d_data, d_off, n)
                              ?: check_append_aligned(d_frontier, *d_out))
        return mk_refuse(who, why);
    std::lock_guard<std::mutex> lk(g_mk_mu);
    return mk_enqueue(tree_size, d_frontier, d_data, d_off, n, *d_out, mk_stream(stream));
}

int pv_merkle_verify_inclusion_batch(const uint8_t* data, const uint64_t* off, const uint8_t* leaf_hash,
                                     const uint64_t* leaf_index, const uint64_t* tree_size, const uint8_t* proof,
                                     const uint64_t* proof_off, const uint8_t* root, uint64_t n, uint8_t* status,
                                     uint8_t* verdict_bits) {
    const char* who = "pv_merkle_verify_inclusion_batch";
    if (n == 0) return PV_OK;
    const char* why;
    if (!leaf_index || !tree_size || !proof_off || !root || !status || !verdict_bits) why = "null pointer";
    else if ((leaf_hash != nullptr) == (off != nullptr)) why = "give either data and off, or leaf_hash";
    else if (off && (!pv_offsets_monotone(off, n) || (!data && off[n] != off[0])))
        why = "offsets must be non-decreasing over a data blob";
    else why = check_proof_offsets(proof, proof_off, n) ?: check_count(n, "more than 2^32 - 1 proofs");
    if (why) return mk_refuse(who, why);
    return mk_dispatch(
        who, n, PV_MERKLE_AUTO_MIN_VERIFY, false,
        [&] { pv_merkle_host_verify(data, off, leaf_hash, leaf_index, tree_size, proof, proof_off, root, n, status, verdict_bits); },
        [&](hipStream_t st) -> int {
            PvStage& g = g_mk.stage;
            int rc = g.reset(st, false);
            if (rc) return rc;
            // staged whole: the leaves as data and offsets or as hashes, and the proofs with room for one hash more
            const int i_off = off ? g.in_offsets(off, n) : -1,
                      i_data = off ? g.in(data + off[0], off[n] - off[0], PV_BLOB_SLACK) : -1,
                      i_leaf = off ? -1 : g.in(leaf_hash, 32 * n), i_index = g.in(leaf_index, 8 * n),
                      i_size = g.in(tree_size, 8 * n), i_poff = g.in_offsets(proof_off, n), i_root = g.in(root, 32 * n),
                      i_proof = g.in(proof + 32 * proof_off[0], 32 * (proof_off[n] - proof_off[0]), 32),
                      o_status = g.out(status, n), o_words = g.out(verdict_bits, (n + 7) / 8, 8);  // whole words written
            if ((rc = g.upload()) ||
                (rc = mk_verify_enqueue(g.dev<const uint8_t>(i_data), g.dev<const uint64_t>(i_off),
                                        g.dev<const uint8_t>(i_leaf), g.dev<const uint64_t>(i_index),
                                        g.dev<const uint64_t>(i_size), g.dev<const uint8_t>(i_proof),
                                        g.dev<const uint64_t>(i_poff), g.dev<const uint8_t>(i_root), n,
                                        g.dev<uint8_t>(o_status), g.dev<uint64_t>(o_words), st)))
                return rc;
            return g.download();
        });
}

int pv_merkle_verify_inclusion_batch_device(const uint8_t* d_data, const uint64_t* d_off, const uint8_t* d_leaf_hash,
                                            const uint64_t* d_leaf_index, const uint64_t* d_tree_size,
                                            const uint8_t* d_proof, const uint64_t* d_proof_off, const uint8_t* d_root,
                                            uint64_t n, uint8_t* d_status, uint64_t* d_verdict_words, void* stream) {
    const char* who = "pv_merkle_verify_inclusion_batch_device";
    if (!pv_engine_stream()) return mk_no_init(who);
    if (n == 0) return PV_OK;
    const char* why;
    if (!d_leaf_index || !d_tree_size || !d_proof || !d_proof_off || !d_root || !d_status || !d_verdict_words)
        why = "null pointer";
    else if ((d_leaf_hash != nullptr) == (d_off != nullptr) || (d_off && !d_data))
        why = "give either data and off, or leaf_hash";
    else why = check_aligned({d_leaf_hash, d_proof, d_root}) ?: check_count(n, "more than 2^32 - 1 proofs");
    if (why) return mk_refuse(who, why);
    std::lock_guard<std::mutex> lk(g_mk_mu);  // the chunk setting; this entry uses no workspace, so no hand-over
    return mk_verify_enqueue(d_data, d_off, d_leaf_hash, d_leaf_index, d_tree_size, d_proof, d_proof_off, d_root, n, d_status,
                             d_verdict_words, mk_stream(stream));
}

int pv_merkle_verify_consistency_batch(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_root,
                                       const uint8_t* new_root, const uint8_t* proof, const uint64_t* proof_off,
                                       uint64_t n, uint8_t* status, uint8_t* verdict_bits) {
    const char* who = "pv_merkle_verify_consistency_batch";
    if (n == 0) return PV_OK;
    if (!old_size || !new_size || !old_root || !new_root || !proof_off || !status || !verdict_bits)
        return mk_refuse(who, "null pointer");
    if (const char* why = check_count(n, "more than 2^32 - 1 proofs") ?: check_proof_offsets(proof, proof_off, n))
        return mk_refuse(who, why);
    uint64_t all = 0;
    for (uint64_t i = 0; i < n; i++) all |= old_size[i] | new_size[i];
    if (const char* why = check_sizes(all, 0, "tree sizes must stay below 2^48")) return mk_refuse(who, why);
    return mk_dispatch(
        who, n, PV_MERKLE_AUTO_MIN_CONSISTENCY, false,
        [&] { pv_merkle_host_consistency(old_size, new_size, old_root, new_root, proof, proof_off, n, status, verdict_bits); },
        [&](hipStream_t st) -> int {
            PvStage& g = g_mk.stage;
            int rc = g.reset(st, false);
            if (rc) return rc;
            const int i_old = g.in(old_size, 8 * n), i_new = g.in(new_size, 8 * n), i_oroot = g.in(old_root, 32 * n),
                      i_nroot = g.in(new_root, 32 * n), i_poff = g.in_offsets(proof_off, n),
                      i_proof = g.in(proof + 32 * proof_off[0], 32 * (proof_off[n] - proof_off[0]), 32),
                      o_status = g.out(status, n), o_words = g.out(verdict_bits, (n + 7) / 8, 8);  // whole words written
            if ((rc = g.upload()) ||
                (rc = mk_consistency_enqueue(g.dev<const uint64_t>(i_old), g.dev<const uint64_t>(i_new),
                                             g.dev<const uint8_t>(i_oroot), g.dev<const uint8_t>(i_nroot),
                                             g.dev<const uint8_t>(i_proof), g.dev<const uint64_t>(i_poff), n,
                                             g.dev<uint8_t>(o_status), g.dev<uint64_t>(o_words), st)))
                return rc;
            return g.download();
        });
}

int pv_merkle_verify_consistency_batch_device(const uint64_t* d_old_size, const uint64_t* d_new_size,
                                              const uint8_t* d_old_root, const uint8_t* d_new_root, const uint8_t* d_proof,
                                              const uint64_t* d_proof_off, uint64_t n, uint8_t* d_status,
                                              uint64_t* d_verdict_words, void* stream) {
    const char* who = "pv_merkle_verify_consistency_batch_device";
    if (!pv_engine_stream()) return mk_no_init(who);
    if (n == 0) return PV_OK;
    if (!d_old_size || !d_new_size || !d_old_root || !d_new_root || !d_proof || !d_proof_off || !d_status || !d_verdict_words)
        return mk_refuse(who, "null pointer");
    if (const char* why = check_aligned({d_old_root, d_new_root, d_proof}) ?: check_count(n, "more than 2^32 - 1 proofs"))
        return mk_refuse(who, why);
    std::lock_guard<std::mutex> lk(g_mk_mu);  // the chunk setting; this entry uses no workspace, so no hand-over
    return mk_consistency_enqueue(d_old_size, d_new_size, d_old_root, d_new_root, d_proof, d_proof_off, n, d_status,
                                  d_verdict_words, mk_stream(stream));
}

int pv_merkle_prove_plan(uint64_t n_leaves, const uint8_t* kind, const uint64_t* a, const uint64_t* b, uint64_t q,
                         uint64_t* out_off, uint8_t* status) {
    const char* who = "pv_merkle_prove_plan";
    if (const char* why = mk_check_store(n_leaves, q)) return mk_refuse(who, why);
    if (!out_off || (q && (!kind || !a || !b))) return mk_refuse(who, "null pointer");
    out_off[0] = 0;
    for (uint64_t i = 0; i < q; i++) {
        const bool ok = pv_merkle_query_valid(kind[i], a[i], b[i], n_leaves);
        out_off[i + 1] = out_off[i] + (ok ? pv_merkle_prove_len(kind[i], a[i], b[i]) : 0);
        if (status) status[i] = ok ? PV_MK_PROVED : PV_MK_Q_RANGE;
    }
    return PV_OK;
}

int pv_merkle_prove_batch(const uint8_t* leaf_hash, uint64_t n_leaves, const uint8_t* node_hash, const uint8_t* kind,
                          const uint64_t* a, const uint64_t* b, uint64_t q, const uint64_t* out_off, uint8_t* out,
                          uint8_t* status) {
    const char* who = "pv_merkle_prove_batch";
    if (const char* why = mk_check_store(n_leaves, q)) return mk_refuse(who, why);
    if (q == 0) return PV_OK;
    const uint64_t n_nodes = pv_merkle_node_count(n_leaves);
    if (!kind || !a || !b || !out_off || !status || (n_leaves && !leaf_hash) || (n_nodes && !node_hash))
        return mk_refuse(who, "null pointer");
    if (!pv_offsets_monotone(out_off, q) || (!out && out_off[q] != out_off[0]))
        return mk_refuse(who, "out_off must be non-decreasing over an output array");
    return mk_dispatch(
        who, q, PV_MERKLE_AUTO_MIN_PROVE, false,
        [&] { pv_merkle_host_prove(leaf_hash, n_leaves, node_hash, kind, a, b, q, out_off, out, status); },
        [&](hipStream_t st) -> int {
            // a slot no lane writes keeps the caller's bytes: out goes up as well only when there is one
            const bool all_written = out_off[0] == 0 && pv_merkle_host_prove_unwritten(n_leaves, kind, a, b, q, out_off) == 0;
            PvStage& g = g_mk.stage;
            int rc = g.reset(st, false);
            if (rc) return rc;
            // the store and the queries staged whole; out keeps its absolute offsets
            const int i_leaf = g.in(leaf_hash, 32 * n_leaves), i_node = g.in(node_hash, 32 * n_nodes), i_kind = g.in(kind, q),
                      i_a = g.in(a, 8 * q), i_b = g.in(b, 8 * q), i_off = g.in(out_off, 8 * (q + 1)),
                      o_out = all_written ? g.out(out, 32 * out_off[q]) : g.inout(out, out, 32 * out_off[q]),
                      o_status = g.out(status, q);
            if ((rc = g.upload())) return rc;
            const MkProve p{g.dev<const uint32_t>(i_leaf), g.dev<const uint32_t>(i_node), n_leaves, g.dev<const uint8_t>(i_kind),
                            g.dev<const uint64_t>(i_a), g.dev<const uint64_t>(i_b), g.dev<const uint64_t>(i_off),
                            g.dev<const uint64_t>(i_off) + q, g.dev<uint32_t>(o_out), g.dev<uint8_t>(o_status)};
            if ((rc = mk_prove_enqueue(p, q, st))) return rc;
            return g.download();
        });
}

int pv_merkle_prove_batch_device(const uint8_t* d_leaf_hash, uint64_t n_leaves, const uint8_t* d_node_hash,
                                 const uint8_t* d_kind, const uint64_t* d_a, const uint64_t* d_b, uint64_t q,
                                 const uint64_t* d_out_off, uint8_t* d_out, uint8_t* d_status, void* stream) {
    const char* who = "pv_merkle_prove_batch_device";
    if (!pv_engine_stream()) return mk_no_init(who);
    if (const char* why = mk_check_store(n_leaves, q)) return mk_refuse(who, why);
    if (q == 0) return PV_OK;
    if (!d_kind || !d_a || !d_b || !d_out_off || !d_out || !d_status || (n_leaves && !d_leaf_hash) ||
        (pv_merkle_node_count(n_leaves) && !d_node_hash))
        return mk_refuse(who, "null pointer");
    if (const char* why = check_aligned({d_leaf_hash, d_node_hash, d_out})) return mk_refuse(who, why);
    const MkProve p{reinterpret_cast<const uint32_t*>(d_leaf_hash), reinterpret_cast<const uint32_t*>(d_node_hash), n_leaves,
                    d_kind, d_a, d_b, d_out_off, d_out_off + q, reinterpret_cast<uint32_t*>(d_out), d_status};
    std::lock_guard<std::mutex> lk(g_mk_mu);  // the chunk setting; this entry uses no workspace, so no hand-over
    return mk_prove_enqueue(p, q, mk_stream(stream));
}

int pv_merkle_catchup_batch(uint64_t tree_size, const uint8_t* frontier, const uint8_t* data, const uint64_t* off, uint64_t n,
                            const uint64_t* reply_end, uint64_t n_replies, uint64_t final_size, const uint8_t* final_root,
                            const uint8_t* proof, const uint64_t* proof_off, const PvMerkleOut* out, uint8_t* status,
                            uint8_t* verdict_bits) {
    const char* who = "pv_merkle_catchup_batch";
    const PvMerkleOut none{};
    if (!out) out = &none;
    const char* why = check_out(out) ?: check_append_host(tree_size, frontier, data, off, n)
                          ?: check_sizes(final_size, 0, "final_size must stay below 2^48")
                          ?: check_count(n_replies, "more than 2^32 - 1 replies");
    if (!why && n_replies) {
        if (!reply_end || !final_root || !proof_off || !status || !verdict_bits) why = "null pointer";
        else why = check_proof_offsets(proof, proof_off, n_replies) ?: check_reply_ends(reply_end, n_replies, tree_size, n);
    }
    if (why) return mk_refuse(who, why);
    const MkHostReplies hr{reply_end, n_replies, final_size, final_root, proof, proof_off, status, verdict_bits};
    return mk_dispatch(
        who, n, PV_MERKLE_AUTO_MIN_PROOFS, n == 0,
        [&] {
            pv_merkle_host_catchup(tree_size, frontier, data, off, n, reply_end, n_replies, final_size, final_root, proof,
                                   proof_off, out, status, verdict_bits);
        },
        [&](hipStream_t st) {
            return mk_host_entry_device(st, tree_size, frontier, data, off, n, *out, n_replies ? &hr : nullptr);
        });
}

int pv_merkle_catchup_batch_device(uint64_t tree_size, const uint8_t* d_frontier, const uint8_t* d_data,
                                   const uint64_t* d_off, uint64_t n, const uint64_t* d_reply_end, uint64_t n_replies,
                                   uint64_t final_size, const uint8_t* d_final_root, const uint8_t* d_proof,
                                   const uint64_t* d_proof_off, const PvMerkleOut* d_out, uint8_t* d_status,
                                   uint64_t* d_verdict_words, void* stream) {
    const char* who = "pv_merkle_catchup_batch_device";
    if (!pv_engine_stream()) return mk_no_init(who);
    const PvMerkleOut none{};
    if (!d_out) d_out = &none;
    const char* const sizes = "tree_size + n and final_size must stay below 2^48";
    const char* why = check_out(d_out) ?: check_sizes(tree_size, n, sizes) ?: check_sizes(final_size, 0, sizes)
                          ?: check_count(n_replies, "more than 2^32 - 1 replies")
                          ?: check_append_device(tree_size, d_frontier, d_data, d_off, n);
    if (!why && n_replies && (!d_reply_end || !d_final_root || !d_proof || !d_proof_off || !d_status || !d_verdict_words))
        why = "null pointer";
    if (!why) why = check_append_aligned(d_frontier, *d_out) ?: check_aligned({d_final_root, d_proof});
    if (why) return mk_refuse(who, why);
    const MkReplies rep{d_reply_end, reinterpret_cast<const uint32_t*>(d_proof), d_proof_off,
                        reinterpret_cast<const uint32_t*>(d_final_root), final_size, 0, n_replies, d_status, d_verdict_words};
    std::lock_guard<std::mutex> lk(g_mk_mu);
    return mk_enqueue(tree_size, d_frontier, d_data, d_off, n, *d_out, mk_stream(stream), n_replies ? &rep : nullptr);
}

}  // extern "C"
