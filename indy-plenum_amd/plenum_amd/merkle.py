"""The ledger's compact Merkle tree with batched appends and audit-proof checks.

The interface (member names, arguments, exception classes and texts) of the reference's
ledger/tree_hasher.py, ledger/compact_merkle_tree.py, ledger/hash_stores (the in-memory store) and
ledger/merkle_verifier.py, implemented independently: a tree is its size and its
frontier (one hash per set bit of the size, largest subtree first), an append is a binary-counter carry
over that frontier, node positions are closed forms, and the store-backed hashes and proofs follow the
RFC 6962 definitions of MTH, PATH and PROOF. Added: one library call for a whole batch.

    CompactMerkleTree.append_batch(leaves)    n appends (plenum/common/ledger.py:75-100 commitTxns)
    CompactMerkleTree.extended_batch(leaves)  a new tree, no store (ledger.py:129-143 treeWithAppliedTxns)
    TreeHasher.hash_leaves(leaves)            the leaf hashes of a batch (catch-up)
    MerkleVerifier.verify_leaf_inclusion_batch(items)
    MerkleVerifier.verify_tree_consistency_batch(items)
    CompactMerkleTree.verify_catchup_replies(replies, final_size, final_root)
                                              a chain of CatchupReps checked as plenum/server/catchup/
                                              catchup_rep_service.py:375-426 checks them one by one
    CompactMerkleTree.inclusion_proof_batch(pairs) / consistency_proof_batch(pairs) / merkle_tree_hash_batch(sizes)
                                              the store-backed proofs and roots, many per call
    CompactMerkleTree.audit_proofs(seq_nos, size=None)
                                              Ledger.auditProof / merkleInfo (ledger/ledger.py:196-217) per read
    CompactMerkleTree.catchup_proofs(reply_ends, catchup_till)
                                              the seeder's consistency_proof(end, catchupTill) per CatchupReq
                                              (plenum/server/catchup/seeder_service.py:85)

The batch calls go through libplenum_verify (pv_merkle_append_batch, pv_merkle_verify_inclusion_batch,
pv_merkle_verify_consistency_batch, pv_merkle_catchup_batch, pv_merkle_prove_batch), which runs them on the GPU or, for small
batches and on a machine without one, in C++ on the host; the results are byte-identical to the
sequential methods below. Not here: the persistent hash stores and the Ledger class."""
import hashlib
from binascii import hexlify
from collections import namedtuple

from . import _native
from .exceptions import ConsistencyError, ConsistencyVerificationFailed, ProofError

STH = namedtuple("STH", ["tree_size", "sha256_root_hash"])


def _popcount(i):
    return bin(i).count("1")


def _split(n):
    """The largest power of two below n (n >= 2): where RFC 6962 splits a range of n leaves."""
    return 1 << ((n - 1).bit_length() - 1)


def _carry(frontier, size, node, hasher, on_node=None):
    """Push the subtree root `node` that brings the tree to `size` leaves onto `frontier` (hashes, largest
    first): one merge with the frontier's last entry per trailing zero of `size`, as a binary counter
    carries. on_node(height, hash) sees every merged node, lowest first."""
    height = 0
    while not (size >> height) & 1:
        height += 1
        node = hasher.hash_children(frontier.pop(), node)
        if on_node:
            on_node(height, node)
    frontier.append(node)


class TreeHasher(object):
    """Merkle hasher with domain separation for leaves and nodes (RFC 6962 section 2.1)."""

    def __init__(self, hashfunc=hashlib.sha256):
        self.hashfunc = hashfunc

    def __repr__(self):
        return "%s(%r)" % (self.__class__.__name__, self.hashfunc)

    def __str__(self):
        return repr(self)

    def hash_empty(self):
        return self.hashfunc().digest()

    def hash_leaf(self, data):
        return self.hashfunc(b"\x00" + data).digest()

    def hash_children(self, left, right):
        return self.hashfunc(b"\x01" + left + right).digest()

    def hash_leaves(self, leaves):
        """hash_leaf of every leaf, one library call."""
        leaves = list(leaves)
        if self.hashfunc is not hashlib.sha256:
            return [self.hash_leaf(x) for x in leaves]
        blob, off = _native._blob(leaves)
        out = _native.merkle_append(0, b"", blob, off, want=("leaf_hash",))["leaf_hash"]
        return [out[i].tobytes() for i in range(len(leaves))]

    def _hash_full(self, leaves, l_idx, r_idx):
        """(root, hashes of the full subtrees, largest first) of leaves[l_idx:r_idx] as an entire tree."""
        if not 0 <= l_idx <= r_idx <= len(leaves):
            raise IndexError("{},{} not a valid range over [0,{}]".format(l_idx, r_idx, len(leaves)))
        frontier = []
        for count, leaf in enumerate(leaves[l_idx:r_idx], 1):
            _carry(frontier, count, self.hash_leaf(leaf), self)
        return (self._hash_fold(frontier) if frontier else self.hash_empty()), tuple(frontier)

    def _hash_fold(self, hashes):
        """Root of a frontier: folded from the smallest subtree up, the larger one on the left."""
        acc = hashes[-1]
        for larger in reversed(hashes[:-1]):
            acc = self.hash_children(larger, acc)
        return acc

    def hash_full_tree(self, leaves):
        return self._hash_full(leaves, 0, len(leaves))[0]


class MemoryHashStore:
    """Leaf and node hashes by 1-based sequence number, in memory (the interface of the reference's
    HashStore / MemoryHashStore). writeNode takes the (size, height, hash) tuple a tree writes, or a bare
    hash, and keeps the hash. Nodes lie in completion order: the node of height h whose last leaf is
    leaf number u follows every node completed earlier, u - 1 - popcount(u - 1) of them, and the lower
    nodes completed by the same leaf. Beside the two lists it keeps the same hashes as two contiguous byte
    arrays (hash_arrays), so a batched proof call hands the library the whole store without joining it."""

    def __init__(self):
        self.reset()
        self.open()

    @property
    def is_persistent(self) -> bool:
        return False

    def writeLeaf(self, leafHash):
        self._leafs.append(leafHash)
        self._leaf_bytes += leafHash

    def writeNode(self, node):
        node = node[2] if isinstance(node, tuple) else node
        self._nodes.append(node)
        self._node_bytes += node

    def hash_arrays(self):
        """(leaf hashes, node hashes) as two bytearrays, hash after hash in store order; None when a hash of
        another length than 32 bytes was written (a hasher other than SHA-256)."""
        if len(self._leaf_bytes) != 32 * len(self._leafs) or len(self._node_bytes) != 32 * len(self._nodes):
            return None
        return self._leaf_bytes, self._node_bytes

    def readLeaf(self, pos):
        return self._leafs[pos - 1]

    def readNode(self, pos):
        return self._nodes[pos - 1]

    def readLeafs(self, startpos, endpos):
        return list(self._leafs[startpos - 1:endpos])

    def readNodes(self, startpos, endpos):
        return list(self._nodes[startpos - 1:endpos])

    @property
    def leafCount(self) -> int:
        return len(self._leafs)

    @property
    def nodeCount(self) -> int:
        return len(self._nodes)

    @classmethod
    def getNodePosition(cls, start, height=None) -> int:
        """1-based position of the node of `height` whose last leaf is leaf number `start`; without a
        height (or with 0), floor(log2(start)): the whole tree when start is a power of two."""
        height = height or (start.bit_length() - 1)
        return start - _popcount(start - 1) + height - 1

    @classmethod
    def getPath(cls, seqNo, offset=0):
        """(leaf positions, node positions) that, with leaf seqNo itself, cover leaves offset + 1 .. seqNo:
        the aligned subtrees of the leaves before the last two, smallest first, and leaf seqNo - 1 when
        seqNo is even."""
        if offset >= seqNo:
            raise ValueError("Offset should be less than serial number")
        nodes, end = [], offset
        while seqNo - 1 - end >= 2:
            height = (seqNo - 1 - end).bit_length() - 1
            end += 1 << height
            nodes.insert(0, cls.getNodePosition(end, height))
        return ([seqNo - 1] if seqNo % 2 == 0 else []), nodes

    def readNodeByTree(self, start, height=None):
        return self.readNode(self.getNodePosition(start, height))

    @property
    def is_consistent(self) -> bool:
        return self.nodeCount == CompactMerkleTree.get_expected_node_count(self.leafCount)

    def reset(self):
        self._nodes, self._leafs = [], []
        self._leaf_bytes, self._node_bytes = bytearray(), bytearray()
        return True

    def open(self):
        self._closed = False

    def close(self):
        self._closed = True

    @property
    def closed(self):
        return self._closed


class CompactMerkleTree:
    """A Merkle tree that only grows: tree_size and `hashes`, the roots of the full subtrees that form it,
    largest first (the interface of the reference's CompactMerkleTree)."""

    def __init__(self, hasher=None, tree_size=0, hashes=(), hashStore=None):
        self._store = hashStore or MemoryHashStore()
        self._hasher = hasher or TreeHasher()
        self._update(tree_size, hashes)

    @property
    def hashStore(self):
        return self._store

    def _update(self, tree_size, hashes):
        if len(hashes) != _popcount(tree_size):
            raise ValueError("number of hashes != bits set in tree_size: %s vs %s" % (len(hashes), _popcount(tree_size)))
        self._size, self._hashes, self._root = tree_size, tuple(hashes), None

    def load(self, other):
        """Take size and hashes from an object with tree_size and hashes."""
        self._update(other.tree_size, other.hashes)

    def save(self, other):
        """Leave size and hashes on a plain data object, under the attribute names the reference uses."""
        setattr(other, "_CompactMerkleTree__tree_size", self._size)
        setattr(other, "_CompactMerkleTree__hashes", self._hashes)

    def __copy__(self):
        return self.__class__(self._hasher, self._size, self._hashes)

    def __repr__(self):
        return "%s(%r, %r, %r)" % (self.__class__.__name__, self._hasher, self._size, self._hashes)

    def __len__(self):
        return self._size

    @property
    def tree_size(self) -> int:
        return self._size

    @property
    def hashes(self):
        return self._hashes

    @property
    def root_hash(self):
        if self._root is None:
            self._root = self._hasher._hash_fold(self._hashes) if self._hashes else self._hasher.hash_empty()
        return self._root

    @property
    def root_hash_hex(self):
        return hexlify(self.root_hash)

    def _grow(self, leaves, store):
        frontier, size = list(self._hashes), self._size
        for leaf in leaves:
            size += 1
            leaf_hash = self._hasher.hash_leaf(leaf)
            if store is None:
                _carry(frontier, size, leaf_hash, self._hasher)
            else:
                store.writeLeaf(leaf_hash)
                _carry(frontier, size, leaf_hash, self._hasher, lambda h, node, u=size: store.writeNode((u, h, node)))
        self._update(size, frontier)

    def append(self, new_leaf):
        """Append one leaf; returns its audit path: the frontier before it, smallest subtree first. The hash
        store receives the leaf hash and every node the leaf completes, lowest first."""
        path = list(self._hashes[::-1])
        self._grow([new_leaf], self._store)
        return path

    def _batch(self, leaves, want):
        leaves = list(leaves)
        blob, off = _native._blob(leaves)
        return leaves, _native.merkle_append(self._size, b"".join(self._hashes), blob, off, want=want)

    def append_batch(self, leaves):
        """n sequential append() calls as one library call. Returns (audit_paths, root_hashes): what append
        returned for each leaf and root_hash after it. The tree and the hash store end exactly as after the
        n appends (same writeLeaf / writeNode values in the same positions)."""
        if self._hasher.hashfunc is not hashlib.sha256:
            paths, roots = [], []
            for leaf in leaves:
                paths.append(self.append(leaf))
                roots.append(self.root_hash)
            return paths, roots
        leaves, r = self._batch(leaves, ("leaf_hash", "node_hash", "frontier", "roots", "path"))
        n = len(leaves)
        if n == 0:
            return [], []
        lh, nh, po, pb = r["leaf_hash"].tobytes(), r["node_hash"].tobytes(), r["path_off"], r["path"].tobytes()
        store = self.hashStore
        # the reference interleaves writeLeaf and writeNode; the two stores are independent sequences, so
        # writing all leaves and then all nodes leaves both exactly as the n appends do
        for i in range(n):
            store.writeLeaf(lh[32 * i:32 * i + 32])
        k = 0
        for u in range(self._size + 1, self._size + n + 1):
            for height in range(1, (u & -u).bit_length()):
                store.writeNode((u, height, nh[32 * k:32 * k + 32]))
                k += 1
        paths = [[pb[32 * j:32 * j + 32] for j in range(int(po[i]), int(po[i + 1]))] for i in range(n)]
        roots = [r["roots"][i].tobytes() for i in range(n)]
        self._update(self._size + n, [r["frontier"][i].tobytes() for i in range(len(r["frontier"]))])
        self._root = roots[-1]
        return paths, roots

    def extended_batch(self, leaves):
        """A new tree equal to this one extended with `leaves` (no hash store written), one library call:
        treeWithAppliedTxns' copy-and-append loop."""
        if self._hasher.hashfunc is not hashlib.sha256:
            return self.extended(list(leaves))
        leaves, r = self._batch(leaves, ("frontier", "root"))
        new_tree = self.__class__(self._hasher, self._size + len(leaves),
                                  [r["frontier"][i].tobytes() for i in range(len(r["frontier"]))])
        new_tree._root = r["root"].tobytes()
        return new_tree

    def extend(self, new_leaves):
        """Grow by new_leaves without writing the hash store (append / append_batch maintain it)."""
        self._grow(new_leaves, None)

    def extended(self, new_leaves):
        new_tree = self.__copy__()
        new_tree.extend(new_leaves)
        return new_tree

    # ---- store-backed hashes and proofs (RFC 6962 section 2.1 over readLeaf / readNode, one at a time) ----
    def merkle_tree_hash_hex(self, start, end):
        return hexlify(self.merkle_tree_hash(start, end))

    def merkle_tree_hash(self, start, end):
        """MTH of leaves start .. end - 1 (0-based): an aligned full subtree is one store read, any other
        range splits at the largest power of two below its length."""
        if not end > start:
            raise ValueError("end must be greater than start")
        n = end - start
        if n == 1:
            return self._store.readLeaf(end)
        if n & (n - 1) == 0 and start % n == 0:
            return self._store.readNode(self._store.getNodePosition(end, n.bit_length() - 1))
        mid = start + _split(n)
        return self._hasher.hash_children(self.merkle_tree_hash(start, mid), self.merkle_tree_hash(mid, end))

    def inclusion_proof(self, start, end):
        """PATH(start, D[0:end]): the siblings met going down to leaf `start`, listed from the leaf up."""
        siblings, lo, hi = [], 0, end
        while hi - lo > 1:
            mid = lo + _split(hi - lo)
            if start < mid:
                siblings.append((mid, hi))
                hi = mid
            else:
                siblings.append((lo, mid))
                lo = mid
        return [self.merkle_tree_hash(a, b) for a, b in reversed(siblings)]

    def consistency_proof(self, first, second):
        """PROOF(first, D[0:second]): going down towards the boundary of the first `first` leaves, the
        subtree left aside at each step, and the subtree the descent ends on unless it is the old tree
        itself; listed from the bottom up."""
        parts, lo, hi, whole = [], 0, second, True
        while hi - lo != first - lo:
            mid = lo + _split(hi - lo)
            if first <= mid:
                parts.append((mid, hi))
                hi = mid
            else:
                parts.append((lo, mid))
                lo, whole = mid, False
        if not whole:
            parts.append((lo, hi))
        return [self.merkle_tree_hash(a, b) for a, b in reversed(parts)]

    # ---- the same proofs in batches: one library call (pv_merkle_prove_batch) over the store's arrays ----
    def _store_arrays(self):
        """(leaf bytes, node bytes) of the store for the library, or None (a hasher other than SHA-256, or a
        store that cannot hand them over): the caller then loops over the sequential methods. A store without
        hash_arrays is read once through readLeafs / readNodes."""
        if self._hasher.hashfunc is not hashlib.sha256:
            return None
        store = self._store
        if hasattr(store, "hash_arrays"):
            return store.hash_arrays()
        try:
            n = store.leafCount
            leafs = store.readLeafs(1, n)
            nodes = [x[2] if isinstance(x, tuple) else x for x in store.readNodes(1, self.get_expected_node_count(n))]
            leaf_bytes, node_bytes = b"".join(leafs), b"".join(nodes)
        except Exception:  # whatever a foreign store raises: the sequential methods will say it
            return None
        if len(leaf_bytes) != 32 * n or len(node_bytes) != 32 * self.get_expected_node_count(n):
            return None
        return leaf_bytes, node_bytes

    def _check_queries(self, who, queries, arrays):
        """ValueError naming the first query outside its kind's range (the sequential methods do not define
        those cases, and some never return)."""
        n = len(arrays[0]) // 32 if arrays else self._store.leafCount
        for i, (kind, a, b) in enumerate(queries):
            try:
                ok = int(a) == a and int(b) == b and b <= n and (
                    0 <= a < b if kind == _native.PV_MK_Q_INCLUSION else 1 <= a <= b if kind == _native.PV_MK_Q_CONSISTENCY
                    else 1 <= b)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("%s: query %d %r is out of range for a store of %d leaves" % (
                    who, i, (b,) if kind == _native.PV_MK_Q_ROOT else (a, b), n))

    def _prove(self, who, queries):
        """queries: (kind, a, b). Returns one list of hashes per query."""
        queries = list(queries)
        arrays = self._store_arrays()
        self._check_queries(who, queries, arrays)
        if arrays is None:
            return [self.inclusion_proof(a, b) if kind == _native.PV_MK_Q_INCLUSION
                    else self.consistency_proof(a, b) if kind == _native.PV_MK_Q_CONSISTENCY
                    else [self.merkle_tree_hash(0, b)] for kind, a, b in queries]
        if not queries:
            return []
        off, hashes, status = _native.merkle_prove(arrays[0], arrays[1], [q[0] for q in queries],
                                                   [int(q[1]) for q in queries], [int(q[2]) for q in queries])
        if status.any():
            raise _native.NativeError("%s: the library refused a query it was given in range" % who)
        flat, off = hashes.tobytes(), off.tolist()
        return [[flat[32 * j:32 * j + 32] for j in range(off[i], off[i + 1])] for i in range(len(queries))]

    def inclusion_proof_batch(self, pairs):
        """inclusion_proof(start, end) for every (start, end) of pairs, 0 <= start < end <= leafCount."""
        return self._prove("inclusion_proof_batch", [(_native.PV_MK_Q_INCLUSION, a, b) for a, b in pairs])

    def consistency_proof_batch(self, pairs):
        """consistency_proof(first, second) for every (first, second) of pairs, 1 <= first <= second <= leafCount."""
        return self._prove("consistency_proof_batch", [(_native.PV_MK_Q_CONSISTENCY, a, b) for a, b in pairs])

    def merkle_tree_hash_batch(self, sizes):
        """merkle_tree_hash(0, size) for every size of sizes, 1 <= size <= leafCount."""
        return [x[0] for x in self._prove("merkle_tree_hash_batch", [(_native.PV_MK_Q_ROOT, 0, b) for b in sizes])]

    def audit_proofs(self, seq_nos, size=None):
        """Per 1-based sequence number, (root_hash, audit_path, size): the contents of Ledger.auditProof
        (ledger/ledger.py:207-217) for the tree of `size` leaves (default: all the store holds). size may also
        be one size per sequence number; with the numbers themselves, audit_proofs(seq_nos, seq_nos), each is
        proved in the tree that ends with it: the contents of Ledger.merkleInfo (:196-205). Raw hashes;
        hashToStr stays with the caller. One library call for all roots and paths."""
        seq_nos = [int(x) for x in seq_nos]
        if size is None:
            size = self._store.leafCount
        sizes = [int(size)] * len(seq_nos) if isinstance(size, int) else [int(x) for x in size]
        if len(sizes) != len(seq_nos):
            raise ValueError("audit_proofs: one size per sequence number")
        distinct = sorted(set(sizes))
        queries = [(_native.PV_MK_Q_INCLUSION, s - 1, b) for s, b in zip(seq_nos, sizes)]
        got = self._prove("audit_proofs", queries + [(_native.PV_MK_Q_ROOT, 0, b) for b in distinct])
        roots = {b: got[len(seq_nos) + k][0] for k, b in enumerate(distinct)}
        return [(roots[b], got[i], b) for i, b in enumerate(sizes)]

    def catchup_proofs(self, reply_ends, catchup_till):
        """consistency_proof(end, catchup_till) for every end of reply_ends: what the seeder builds per
        CatchupReq (plenum/server/catchup/seeder_service.py:85), one library call for all of them."""
        return self.consistency_proof_batch([(end, catchup_till) for end in reply_ends])

    def get_tree_head(self, seq=None):
        seq = self._size if seq is None else seq
        if seq > self._size:
            raise IndexError
        return {"tree_size": seq, "sha256_root_hash": self.merkle_tree_hash(0, seq) if seq else None}

    @property
    def leafCount(self) -> int:
        return self._store.leafCount

    @property
    def nodeCount(self) -> int:
        return self._store.nodeCount

    @staticmethod
    def get_expected_node_count(leaf_count):
        """Interior nodes of the full subtrees of a tree of leaf_count leaves."""
        return leaf_count - _popcount(leaf_count) if leaf_count > 0 else 0

    def verify_consistency(self, expected_leaf_count) -> bool:
        """True, or ConsistencyVerificationFailed when the store's leaf or node count is not what a tree of
        expected_leaf_count leaves has."""
        if (self.leafCount, self.nodeCount) != (expected_leaf_count, self.get_expected_node_count(self.leafCount)):
            raise ConsistencyVerificationFailed()
        return True

    def reset(self):
        self._store.reset()
        self._update(0, ())

    def verify_catchup_replies(self, replies, final_size, final_root):
        """replies: (leaves, proof) per CatchupRep, chained: reply r's old tree is this tree plus the leaves
        of replies 0..r. Returns, per reply, True or the exception that
        MerkleVerifier.verify_tree_consistency(temp.tree_size, final_size, temp.root_hash, final_root, proof)
        raises for temp = self.extended(all leaves up to and including the reply): what
        catchup_rep_service.py:375-426 computes per reply. Replies are chained whether or not earlier ones
        verified; the tree and its store are untouched. One library call (pv_merkle_catchup_batch); a reply
        that does not verify is re-run sequentially for the reference's exception and text, and a reply
        without leaves or a hasher other than SHA-256 sends the whole call through the sequential path."""
        replies = [(list(leaves), list(proof)) for leaves, proof in replies]
        out = [None] * len(replies)
        try:
            total = self._size + sum(len(lv) for lv, _ in replies)
            fast = (bool(replies) and self._hasher.hashfunc is hashlib.sha256 and all(lv for lv, _ in replies)
                    and 0 <= int(final_size) < 2 ** 48 and total < 2 ** 48 and len(final_root) == 32
                    and all(len(h) == 32 for _, proof in replies for h in proof))
        except (TypeError, ValueError):
            fast = False
        if fast:
            blob, off = _native._blob([bytes(x) for lv, _ in replies for x in lv])
            ends, at = [], self._size
            for lv, _ in replies:
                at += len(lv)
                ends.append(at)
            verdicts, _status, _ = _native.merkle_catchup(self._size, b"".join(self._hashes), blob, off, ends,
                                                          int(final_size), bytes(final_root), [p for _, p in replies])
            for r, v in enumerate(verdicts):
                if v:
                    out[r] = True
        if None in out:
            verifier = MerkleVerifier(self._hasher)
            temp = self.__copy__()
            last = max(r for r, x in enumerate(out) if x is None)
            for r, (leaves, proof) in enumerate(replies[:last + 1]):
                temp.extend(leaves)
                if out[r] is None:
                    try:
                        out[r] = verifier.verify_tree_consistency(temp.tree_size, final_size, temp.root_hash, final_root,
                                                                  proof)
                    except Exception as ex:  # the reference's ValueError / ProofError / ConsistencyError, per reply
                        out[r] = ex
        return out


class MerkleVerifier(object):
    """Merkle audit-path and consistency-proof checks (the reference's MerkleVerifier)."""

    def __init__(self, hasher=None):
        self.hasher = hasher or TreeHasher()

    def __repr__(self):
        return "%r(hasher: %r)" % (self.__class__.__name__, self.hasher)

    def __str__(self):
        return "%s(hasher: %s)" % (self.__class__.__name__, self.hasher)

    def verify_tree_consistency(self, old_tree_size, new_tree_size, old_root, new_root, proof):
        """True, or raises ValueError / ProofError / ConsistencyError with the reference's texts. The walk is
        csrc/merkle_core.h's pv_merkle_consistency_check: the proof is the audit path of node old_size - 1
        in the new tree, hashed together up to the first node only the new tree has. A proof hash is taken
        only where one is needed; hashes left over are accepted."""
        old_size, new_size = old_tree_size, new_tree_size
        if old_size < 0 or new_size < 0:
            raise ValueError("Negative tree size")
        if old_size > new_size:
            raise ValueError("Older tree has bigger size (%d vs %d), did you supply inputs in the wrong order?" %
                             (old_size, new_size))
        if old_size == new_size:
            if old_root == new_root:
                return True
            raise ConsistencyError("Inconsistency: different root hashes for the same tree size")
        if old_size == 0:
            return True
        node, last = old_size - 1, new_size - 1
        while node & 1:
            node, last = node >> 1, last >> 1
        hashes = iter(proof)
        try:
            new_hash = old_hash = next(hashes) if node else old_root
            while node:
                if node & 1:
                    sibling = next(hashes)
                    old_hash = self.hasher.hash_children(sibling, old_hash)
                    new_hash = self.hasher.hash_children(sibling, new_hash)
                elif node < last:
                    new_hash = self.hasher.hash_children(new_hash, next(hashes))
                node, last = node >> 1, last >> 1
            while last:
                new_hash = self.hasher.hash_children(new_hash, next(hashes))
                last >>= 1
        except StopIteration:
            raise ProofError("Merkle proof is too short")
        if new_hash != new_root:
            raise ProofError("Bad Merkle proof: second root hash does not match. Expected hash: %s , computed hash: %s" %
                             (hexlify(new_root).strip(), hexlify(new_hash).strip()))
        if old_hash != old_root:
            raise ConsistencyError("Inconsistency: first root hash does not match. Expected hash: %s, computed hash: %s" %
                                   (hexlify(old_root).strip(), hexlify(old_hash).strip()))
        return True

    def verify_tree_consistency_batch(self, items):
        """items: (old_tree_size, new_tree_size, old_root, new_root, proof) tuples. Returns a list with True or
        the exception the reference's verify_tree_consistency raises, per item. One library call for the
        batch; an item that does not verify, or that the library cannot represent (negative or huge sizes,
        odd-sized hashes, a hasher other than SHA-256), is re-run through the sequential method so the
        exception and its text are the reference's."""
        items = list(items)
        out = [None] * len(items)
        fast = []
        for i, (old, new, old_root, new_root, proof) in enumerate(items):
            try:
                ok = (self.hasher.hashfunc is hashlib.sha256 and 0 <= int(old) < 2 ** 48 and 0 <= int(new) < 2 ** 48
                      and int(old) == old and int(new) == new and len(old_root) == 32 and len(new_root) == 32
                      and all(len(p) == 32 for p in proof))
            except (TypeError, ValueError):
                ok = False
            if ok:
                fast.append(i)
        if fast:
            verdicts, _status = _native.merkle_verify_consistency(
                [int(items[i][0]) for i in fast], [int(items[i][1]) for i in fast], [bytes(items[i][2]) for i in fast],
                [bytes(items[i][3]) for i in fast], [list(items[i][4]) for i in fast])
            for i, v in zip(fast, verdicts):
                if v:
                    out[i] = True
        for i, item in enumerate(items):
            if out[i] is None:
                try:
                    out[i] = self.verify_tree_consistency(*item)
                except Exception as ex:  # the reference's ValueError / ProofError / ConsistencyError, per item
                    out[i] = ex
        return out

    @classmethod
    def audit_path_length(cls, index, tree_size):
        """Hashes in the audit path of leaf `index`: one per level at which the node has a sibling."""
        last = tree_size - 1
        return sum(1 for lv in range(max(last, 0).bit_length()) if (index >> lv) & 1 or (index >> lv) < (last >> lv))

    def verify_leaf_hash_inclusion(self, leaf_hash, leaf_index, proof, sth):
        """True, or raises ProofError / ValueError with the reference's texts. The walk is
        csrc/merkle_core.h's pv_merkle_path_check: level by level, an odd node takes its left sibling from
        the proof, an even node that is not the last of its level its right sibling, and a proof that runs
        out at any level (even one that needs no hash) is too short."""
        index, size = int(leaf_index), int(sth.tree_size)
        if size <= index:
            raise ValueError("Provided STH is for a tree that is smaller than the leaf index. Tree size: %d Leaf "
                             "index: %d" % (size, index))
        if size < 0 or index < 0:
            raise ValueError("Negative tree size or leaf index: Tree size: %d Leaf index: %d" % (size, index))
        acc, used = leaf_hash, 0
        for level in range((size - 1).bit_length()):
            node, last = index >> level, (size - 1) >> level
            if used == len(proof):
                raise ProofError("Proof too short: left with node index %d" % node)
            if node & 1:
                acc, used = self.hasher.hash_children(proof[used], acc), used + 1
            elif node < last:
                acc, used = self.hasher.hash_children(acc, proof[used]), used + 1
        if used < len(proof):
            raise ProofError("Proof too long: Left with %d hashes." % (len(proof) - used))
        if acc == sth.sha256_root_hash:
            return True
        raise ProofError("Constructed root hash differs from provided root hash. Constructed: %s Expected: %s" %
                         (hexlify(acc).strip(), hexlify(sth.sha256_root_hash).strip()))

    def verify_leaf_inclusion(self, leaf, leaf_index, proof, sth):
        return self.verify_leaf_hash_inclusion(self.hasher.hash_leaf(leaf), leaf_index, proof, sth)

    def verify_leaf_inclusion_batch(self, items):
        """items: (leaf, leaf_index, proof, sth) tuples. Returns a list with True or the exception the
        reference's verify_leaf_inclusion raises, per item. One library call for the batch; an item that does
        not verify, or that the library cannot represent (negative or huge numbers, odd-sized hashes), is
        re-run through the sequential method so the exception and its text are the reference's."""
        items = list(items)
        out = [None] * len(items)
        fast = []
        for i, (leaf, index, proof, sth) in enumerate(items):
            try:
                ok = (self.hasher.hashfunc is hashlib.sha256 and 0 <= int(index) < 2 ** 48
                      and 0 <= int(sth.tree_size) < 2 ** 48 and len(sth.sha256_root_hash) == 32
                      and all(len(p) == 32 for p in proof))
            except (TypeError, ValueError):
                ok = False
            if ok:
                fast.append(i)
        if fast:
            verdicts, _status = _native.merkle_verify_inclusion(
                [int(items[i][1]) for i in fast], [int(items[i][3].tree_size) for i in fast],
                [list(items[i][2]) for i in fast], [items[i][3].sha256_root_hash for i in fast],
                leaves=[bytes(items[i][0]) for i in fast])
            for i, v in zip(fast, verdicts):
                if v:
                    out[i] = True
        for i, (leaf, index, proof, sth) in enumerate(items):
            if out[i] is None:
                try:
                    out[i] = self.verify_leaf_inclusion(leaf, index, proof, sth)
                except Exception as ex:  # the reference's ValueError / ProofError, returned per item
                    out[i] = ex
        return out
