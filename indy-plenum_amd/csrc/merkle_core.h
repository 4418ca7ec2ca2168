// Index arithmetic of the batched ledger Merkle append (ledger/compact_merkle_tree.py:95-160 append /
// _push_subtree, :81-88 root_hash), of the audit-path check (ledger/merkle_verifier.py:155-181) and of the
// consistency check (:23-153), and of proof generation from a hash store (ledger/compact_merkle_tree.py:
// 198-249). One source for the kernels (pv_merkle.hip), the host path (merkle_host.cpp) and the check
// libraries (tests/native/merklecheck.hip, conscheck.hip, provecheck.hip); no hashing here, hashes pass
// through template hooks.
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

// ---- proof generation from a hash store (ledger/compact_merkle_tree.py:198-249 merkle_tree_hash,
// consistency_proof, inclusion_proof, _subproof, _path), bottom-up and without recursion -----------------------
// A query (kind, a, b) against a store of n leaves: leaf hashes by 0-based index, node hashes by
// pv_merkle_node_pos. Every hash of a proof is an aligned full subtree (one gather) or the ragged range
// [x, b) that ends at the query's own b: the right-to-left fold of the full subtrees of b below the level
// it is asked at, so all ragged hashes of one query are prefixes of one fold.
#ifndef PV_MK_Q_INCLUSION  // as include/plenum_verify.h
#define PV_MK_Q_INCLUSION 0    // inclusion_proof(a, b) = PATH(a, D[0:b]), 0 <= a < b <= n
#define PV_MK_Q_CONSISTENCY 1  // consistency_proof(a, b) = PROOF(a, D[0:b]), 1 <= a <= b <= n, empty when a == b
#define PV_MK_Q_ROOT 2         // merkle_tree_hash(0, b), 1 <= b <= n, one hash, a ignored
#endif
enum : uint32_t { PV_MK_PROVED = 0, PV_MK_Q_RANGE = 1, PV_MK_Q_ROOM = 2 };  // status of a query
enum : uint32_t { PV_MK_E_LEAF = 0, PV_MK_E_NODE = 1, PV_MK_E_RAGGED = 2 };
struct PvMerkleElem {
    uint32_t tag;  // PV_MK_E_LEAF: leaf hash idx; PV_MK_E_NODE: node store position idx;
    uint64_t idx;  // PV_MK_E_RAGGED: the fold of the full subtrees of b below level idx
};

PV_HD bool pv_merkle_query_valid(uint32_t kind, uint64_t a, uint64_t b, uint64_t n) {
    if (b > n || b == 0) return false;
    return kind == PV_MK_Q_INCLUSION ? a < b : kind == PV_MK_Q_CONSISTENCY ? (a >= 1 && a <= b) : kind == PV_MK_Q_ROOT;
}

// From node `node` of level l0 up to the root of the tree of b leaves: at every level the sibling, which
// covers [sib << l, min((sib + 1) << l, b)) and does not exist when sib << l >= b. emit(k, elem) receives
// hash k of the proof; returns the k after the last one.
template <class Emit>
PV_HD uint32_t pv_merkle_sibling_walk(uint64_t node, uint32_t l0, uint64_t b, uint32_t k, const Emit& emit) {
    for (uint32_t l = l0; ((b - 1) >> l) != 0; l++, node >>= 1) {
        const uint64_t sib = node ^ 1;
        if ((sib << l) >= b) continue;
        const uint64_t end = (sib + 1) << l;
        if (end > b) emit(k++, PvMerkleElem{PV_MK_E_RAGGED, l});
        else if (l == 0) emit(k++, PvMerkleElem{PV_MK_E_LEAF, sib});
        else emit(k++, PvMerkleElem{PV_MK_E_NODE, pv_merkle_node_pos(end, l)});
    }
    return k;
}

// The proof of a valid query, hash by hash in the reference's order; returns its length (at most
// PV_MERKLE_MAX_BITS + 1). A consistency proof starts from the largest aligned subtree that ends at a,
// which is itself the first hash unless a is a power of two (the old root, which the verifier has).
template <class Emit>
PV_HD uint32_t pv_merkle_prove_walk(uint32_t kind, uint64_t a, uint64_t b, const Emit& emit) {
    if (kind == PV_MK_Q_ROOT) {
        emit(0, PvMerkleElem{PV_MK_E_RAGGED, PV_MERKLE_MAX_BITS});
        return 1;
    }
    if (kind == PV_MK_Q_INCLUSION) return pv_merkle_sibling_walk(a, 0, b, 0, emit);
    if (a == b) return 0;
    const uint32_t l = (uint32_t)__builtin_ctzll(a);
    const uint64_t node = (a >> l) - 1;
    uint32_t k = 0;
    if (node) {
        if (l == 0) emit(k++, PvMerkleElem{PV_MK_E_LEAF, a - 1});
        else emit(k++, PvMerkleElem{PV_MK_E_NODE, pv_merkle_node_pos(a, l)});
    }
    return pv_merkle_sibling_walk(node, l, b, k, emit);
}

// Hashes in the proof of a valid query, without a store.
PV_HD uint32_t pv_merkle_prove_len(uint32_t kind, uint64_t a, uint64_t b) {
    return pv_merkle_prove_walk(kind, a, b, [](uint32_t, const PvMerkleElem&) {});
}

// The ragged hashes of one query, after its walk. `levels` has bit l set for every ragged hash (asked for at
// level l) and `slots` bit k for its place in the proof; both grow along the walk, so their i-th set bits
// belong together. One fold over the full subtrees of b from the smallest up, acc = hash_children(larger,
// acc): after the subtree of bit j the fold is the ragged hash of every level in (j, next set bit of b], and
// no two ragged hashes of one proof share such a span (they would cover the same leaves). At most popcount(b)
// - 1 hash_children, none when the query has no ragged hash. get(elem, out) loads a leaf or node hash,
// put(k, acc) stores hash k of the proof. The fold is apart from the walk so that the lanes of a wave,
// which meet their ragged hashes at different levels, hash in step: one subtree of b per iteration.
template <class T, class Get, class Hash, class Put>
PV_HD void pv_merkle_ragged_fold(uint64_t b, uint64_t levels, uint64_t slots, const Get& get, const Hash& hash,
                                 const Put& put) {
    T acc;
    bool have = false;
    for (uint64_t rest = b; levels && rest;) {
        const uint32_t j = (uint32_t)__builtin_ctzll(rest);
        const uint64_t u = ((b >> (j + 1)) << (j + 1)) + (1ull << j);  // the full subtree of bit j ends here
        const PvMerkleElem e = j ? PvMerkleElem{PV_MK_E_NODE, pv_merkle_node_pos(u, j)} : PvMerkleElem{PV_MK_E_LEAF, u - 1};
        if (have) {
            T larger, next;
            get(e, larger);
            hash(next, larger, acc);
            acc = next;
        } else {
            get(e, acc);
            have = true;
        }
        rest &= rest - 1;
        const uint32_t upto = rest ? (uint32_t)__builtin_ctzll(rest) : 63;
        while (levels && (uint32_t)__builtin_ctzll(levels) <= upto) {
            put((uint32_t)__builtin_ctzll(slots), acc);
            levels &= levels - 1;
            slots &= slots - 1;
        }
    }
}

// A whole query: the walk stores the aligned hashes through copy(k, elem) and notes the ragged ones, the fold
// follows. Returns the proof's length.
template <class T, class Copy, class Get, class Hash, class Put>
PV_HD uint32_t pv_merkle_prove(uint32_t kind, uint64_t a, uint64_t b, const Copy& copy, const Get& get, const Hash& hash,
                               const Put& put) {
    uint64_t levels = 0, slots = 0;
    const uint32_t len = pv_merkle_prove_walk(kind, a, b, [&](uint32_t k, const PvMerkleElem& e) {
        if (e.tag == PV_MK_E_RAGGED) {
            levels |= 1ull << e.idx;
            slots |= 1ull << k;
        } else {
            copy(k, e);
        }
    });
    pv_merkle_ragged_fold<T>(b, levels, slots, get, hash, put);
    return len;
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
