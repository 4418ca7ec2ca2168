// Index arithmetic of the batched ledger Merkle append (ledger/compact_merkle_tree.py:95-160 append /
// _push_subtree, :81-88 root_hash), of the audit-path check (ledger/merkle_verifier.py:155-181) and of the
// consistency check (:23-153). One source for the kernels (pv_merkle.hip), the host path (merkle_host.cpp)
// and the host-compiled check libraries (tests/native/merklecheck.hip, conscheck.hip); no hashing here,
// hashes pass through template hooks.
//
// A tree is its size s and its frontier: one hash per set bit of s, largest subtree first. A batch
// appends n leaves with absolute indices s .. s + n - 1. The node of height h >= 1 "completed at size
// u" (u a multiple of 2^h) covers leaves [u - 2^h, u); the reference writes it to the node store when
// the leaf that brings the size to u is appended, after the nodes of smaller height completed at u.
#pragma once
#include <stdint.h>

#ifndef PV_HD
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define PV_HD __host__ __device__ __forceinline__
#else
#define PV_HD inline
#endif
#endif

static constexpr uint32_t PV_MERKLE_MAX_BITS = 48;  // tree_size + n < 2^48
static constexpr uint32_t PV_MERKLE_TILE_LOG = 10;  // the level kernel reduces 2^10 entries per workgroup
static constexpr uint32_t PV_MERKLE_TILE = 1u << PV_MERKLE_TILE_LOG;

PV_HD uint32_t pv_popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

// Node hashes the store holds for a tree of size s (CompactMerkleTree.get_expected_node_count).
PV_HD uint64_t pv_merkle_node_count(uint64_t s) { return s - pv_popc64(s); }

// 0-based position in the node store of the node of height h >= 1 completed at size u.
PV_HD uint64_t pv_merkle_node_pos(uint64_t u, uint32_t h) { return (u - 1) - pv_popc64(u - 1) + (h - 1); }

// sum of popcount(j) over 0 <= j < x: the audit paths of leaves [0, x) hold this many hashes
PV_HD uint64_t pv_merkle_popc_sum(uint64_t x) {
    uint64_t total = 0;
    for (uint32_t b = 0; b < PV_MERKLE_MAX_BITS + 1; b++) {
        const uint64_t period = 2ull << b, half = 1ull << b, rem = x & (period - 1);
        total += (x >> (b + 1)) * half + (rem > half ? rem - half : 0);
    }
    return total;
}

// pv_merkle_plan's three figures for n leaves appended to a tree of size s
PV_HD void pv_merkle_plan_core(uint64_t s, uint64_t n, uint64_t* n_nodes, uint64_t* n_frontier, uint64_t* path_hashes) {
    *n_nodes = pv_merkle_node_count(s + n) - pv_merkle_node_count(s);
    *n_frontier = pv_popc64(s + n);
    *path_hashes = pv_merkle_popc_sum(s + n) - pv_merkle_popc_sum(s);
}

// Where a hash of the batch's view of the tree lives.
enum : uint32_t { PV_MK_OLD = 0, PV_MK_LEAF = 1, PV_MK_NODE = 2 };
struct PvMerkleRef {
    uint32_t kind;  // PV_MK_OLD: entry idx of the input frontier; PV_MK_LEAF: leaf hash idx of the batch;
    uint64_t idx;   // PV_MK_NODE: node idx of the batch (store position minus the old node count)
};

// The aligned node of height h (0 = a leaf) completed at size u <= s + n, seen from a batch that starts
// at size s. If it lies wholly in the old tree it must be the old frontier's entry for bit h (the
// callers below only ask for such nodes: s has bit h set and agrees with u above it).
PV_HD PvMerkleRef pv_merkle_node_ref(uint64_t s, uint64_t u, uint32_t h) {
    if (u <= s) return PvMerkleRef{PV_MK_OLD, pv_popc64(s >> (h + 1))};
    if (h == 0) return PvMerkleRef{PV_MK_LEAF, u - 1 - s};
    return PvMerkleRef{PV_MK_NODE, pv_merkle_node_pos(u, h) - pv_merkle_node_count(s)};
}

// The frontier entry for set bit b of size t >= s: the node [p, p + 2^b), p = t cleared below bit b + 1.
PV_HD PvMerkleRef pv_merkle_frontier_ref(uint64_t s, uint64_t t, uint32_t b) {
    const uint64_t u = ((t >> (b + 1)) << (b + 1)) + (1ull << b);
    return pv_merkle_node_ref(s, u, b);
}

// The audit path append() returns for the leaf appended at size t: the frontier at t, smallest subtree
// first. emit(k, ref) receives hash k of the path; returns the path length popcount(t).
template <class Emit>
PV_HD uint32_t pv_merkle_audit_path(uint64_t s, uint64_t t, const Emit& emit) {
    uint32_t k = 0;
    for (uint64_t rest = t; rest; rest &= rest - 1) emit(k++, pv_merkle_frontier_ref(s, t, (uint32_t)__builtin_ctzll(rest)));
    return k;
}

// root_hash of the tree of size t > 0 (s <= t): the frontier folded from the smallest subtree up,
// acc = hash_children(larger, acc). get(ref, out) loads a hash, hash(out, left, right) is hash_children.
template <class T, class Get, class Hash>
PV_HD void pv_merkle_fold_root(T& acc, uint64_t s, uint64_t t, const Get& get, const Hash& hash) {
    uint64_t rest = t;
    get(pv_merkle_frontier_ref(s, t, (uint32_t)__builtin_ctzll(rest)), acc);
    for (rest &= rest - 1; rest; rest &= rest - 1) {
        T larger, next;
        get(pv_merkle_frontier_ref(s, t, (uint32_t)__builtin_ctzll(rest)), larger);
        hash(next, larger, acc);
        acc = next;
    }
}

// MerkleVerifier._calculate_root_hash_from_audit_path behind verify_leaf_hash_inclusion's index check.
// acc enters as the leaf hash and leaves as the calculated root (status 0 only). proof(k, out) loads
// hash k of a proof of plen hashes. Status: 0 walked (compare acc with the root), 1 tree_size <=
// leaf_index (the reference's ValueError), 2 proof too short, 3 proof too long.
enum : uint32_t { PV_MK_COMPARED = 0, PV_MK_BAD_INDEX = 1, PV_MK_TOO_SHORT = 2, PV_MK_TOO_LONG = 3 };
template <class T, class Proof, class Hash>
PV_HD uint32_t pv_merkle_path_check(T& acc, uint64_t index, uint64_t size, uint64_t plen, const Proof& proof,
                                    const Hash& hash) {
    if (size <= index) return PV_MK_BAD_INDEX;
    uint64_t used = 0;
    for (uint64_t last = size - 1; last > 0; index >>= 1, last >>= 1) {
        if (used == plen) return PV_MK_TOO_SHORT;  // the reference tests this at every level
        if (index & 1) {
            T sib, next;
            proof(used++, sib);
            hash(next, sib, acc);
            acc = next;
        } else if (index < last) {
            T sib, next;
            proof(used++, sib);
            hash(next, acc, sib);
            acc = next;
        }
    }
    return used < plen ? PV_MK_TOO_LONG : PV_MK_COMPARED;
}

// MerkleVerifier.verify_tree_consistency (ledger/merkle_verifier.py:23-153). A consistency proof is the
// audit path of node old_size - 1 in the new tree, already hashed together up to the first node that
// only the new tree has: trailing one-bits of old_size - 1 are stripped (right children, in both trees),
// both chains start from proof[0], or from old_root when nothing is left of the node (old_size a power
// of two), a right child extends both chains with its left sibling, a left child below `last` extends
// the new chain only, and the new chain then climbs while `last` is non-zero. proof(k, out) loads hash k
// of a proof of plen hashes; a hash is asked for only where the walk needs one (unlike the inclusion
// walk above), so "too short" is a needed hash that is missing, and hashes left over are accepted.
// eq(a, b) compares two hashes. Verdict 1 iff the status is PV_MK_CONSISTENT.
enum : uint32_t {
    PV_MK_CONSISTENT = 0,
    PV_MK_OLD_LARGER = 1,      // old_size > new_size (the reference's ValueError)
    PV_MK_CONS_TOO_SHORT = 2,  // ProofError "Merkle proof is too short"
    PV_MK_NEW_DIFFERS = 3,     // the second (new) root differs: ProofError
    PV_MK_OLD_DIFFERS = 4,     // the new root matches, the first (old) one does not: ConsistencyError
    PV_MK_SAME_SIZE = 5,       // equal sizes, different roots: ConsistencyError
    PV_MK_REPLY_RANGE = 6      // catch-up only: the reply's end is not in (tree_size, tree_size + n]
};
template <class T, class Proof, class Hash, class Eq>
PV_HD uint32_t pv_merkle_consistency_check(uint64_t old_size, uint64_t new_size, const T& old_root, const T& new_root,
                                           uint64_t plen, const Proof& proof, const Hash& hash, const Eq& eq) {
    if (old_size > new_size) return PV_MK_OLD_LARGER;
    if (old_size == new_size) return eq(old_root, new_root) ? PV_MK_CONSISTENT : PV_MK_SAME_SIZE;  // the proof is ignored
    if (old_size == 0) return PV_MK_CONSISTENT;  // anything is consistent with the empty tree
    uint64_t node = old_size - 1, last = new_size - 1, used = 0;
    while (node & 1) {
        node >>= 1;
        last >>= 1;
    }
    T old_acc = old_root, new_acc = old_root;
    if (node) {
        if (used == plen) return PV_MK_CONS_TOO_SHORT;
        proof(used++, new_acc);
        old_acc = new_acc;
    }
    for (; node; node >>= 1, last >>= 1) {
        if (node & 1) {
            if (used == plen) return PV_MK_CONS_TOO_SHORT;
            T sib, next;
            proof(used++, sib);
            hash(next, sib, old_acc);
            old_acc = next;
            hash(next, sib, new_acc);
            new_acc = next;
        } else if (node < last) {
            if (used == plen) return PV_MK_CONS_TOO_SHORT;
            T sib, next;
            proof(used++, sib);
            hash(next, new_acc, sib);
            new_acc = next;
        }
    }
    for (; last; last >>= 1) {
        if (used == plen) return PV_MK_CONS_TOO_SHORT;
        T sib, next;
        proof(used++, sib);
        hash(next, new_acc, sib);
        new_acc = next;
    }
    if (!eq(new_acc, new_root)) return PV_MK_NEW_DIFFERS;
    if (!eq(old_acc, old_root)) return PV_MK_OLD_DIFFERS;
    return PV_MK_CONSISTENT;
}

// ---- the level kernel's tiling (absolute indices, so node alignment is the tree's) ----------------
// Pass h0 reduces entries of height h0 (h0 = 0: leaf hashes) in tiles of PV_MERKLE_TILE entries: tile k
// holds the entries completed at u = (k * TILE + e + 1) << h0 and produces heights h0 + 1 .. h0 + TILE_LOG.
// An entry or node is the batch's own ("new") iff s < u <= s + n.
PV_HD bool pv_merkle_is_new(uint64_t s, uint64_t n, uint64_t u) { return u > s && u <= s + n; }
// the tiles of pass h0 that hold a new entry: [first, first + count)
PV_HD void pv_merkle_tiles(uint64_t s, uint64_t n, uint32_t h0, uint64_t* first, uint64_t* count) {
    const uint64_t lo = ((s >> h0) + 1), hi = (s + n) >> h0;  // new entries are e-th multiples lo..hi of 2^h0
    if (hi < lo) {
        *first = 0;
        *count = 0;
        return;
    }
    *first = (lo - 1) >> PV_MERKLE_TILE_LOG;
    *count = ((hi - 1) >> PV_MERKLE_TILE_LOG) - *first + 1;
}
// whether the batch completes any node higher than h
PV_HD bool pv_merkle_any_above(uint64_t s, uint64_t n, uint32_t h) { return ((s + n) >> (h + 1)) != (s >> (h + 1)); }
