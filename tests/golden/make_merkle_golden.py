"""Generate tests/golden/merkle.json by running the REFERENCE's own Merkle tree and verifier.

TEST INFRASTRUCTURE, run only where the reference is checked out (the tests read the JSON alone):
    python tests/golden/make_merkle_golden.py
The reference (swcurran/indy-plenum, checked out beside this repository) is imported, never copied.
Output (JSON, data only, hex strings, one case per line):
  appends  per (start size, start hashes, leaves): what CompactMerkleTree.append returned for every leaf,
           root_hash after it, the hash store's leaf and node writes in order, the final tree.hashes. The
           reference's MemoryHashStore keeps the whole (start, height, hash) tuple and its own
           inclusion_proof fails on that, so the store is wrapped: readNode returns the hash.
  proofs   valid inclusion proofs of trees built from size 0 and, for each variant of
           tests/merkle_ref.py proof_variants (valid, truncated, extended, wrong root / leaf / index,
           index >= size), MerkleVerifier.verify_leaf_inclusion's outcome: True or the exception's
           class and text.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("PLENUM_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path[:0] = [REF, os.path.dirname(HERE)]

from ledger.compact_merkle_tree import CompactMerkleTree  # noqa: E402
from ledger.hash_stores.memory_hash_store import MemoryHashStore  # noqa: E402
from ledger.merkle_verifier import MerkleVerifier  # noqa: E402
from ledger.tree_hasher import TreeHasher  # noqa: E402
from ledger.util import STH  # noqa: E402
from merkle_ref import proof_variants  # noqa: E402

LENGTHS = (0, 1, 54, 55, 56, 62, 63, 64, 118, 119, 120, 126, 127, 128, 7, 33)
SHAPES = ((0, 0), (0, 1), (0, 2), (0, 3), (0, 8), (1, 1), (1, 3), (2, 2), (3, 1), (3, 4), (4, 2), (5, 3), (6, 1),
          (7, 1), (7, 2), (8, 2), (9, 2), (15, 1), (16, 2), (31, 1), (63, 1), (64, 1), (65, 2), (127, 1), (128, 1),
          (257, 1), (2 ** 20 - 1, 1))
PROOFS = ((1, 0), (2, 1), (3, 2), (4, 2), (5, 0), (6, 5), (7, 3), (8, 7), (13, 12), (16, 9))  # (size, leaf index)


class HashOnlyStore(MemoryHashStore):
    def readNode(self, pos):
        return self._nodes[pos - 1][2]


def det(tag, i, n):
    out = b"".join(hashlib.sha256(b"merkle golden %s %d %d" % (tag, i, k)).digest() for k in range(n // 32 + 1))
    return out[:n]


def leaves_of(case, n):
    return [det(b"leaf", 1000 * case + j, LENGTHS[(case + j) % len(LENGTHS)]) for j in range(n)]


def main():
    appends, proofs = [], []
    for case, (start, n) in enumerate(SHAPES):
        hashes = [det(b"frontier", 100 * case + k, 32) for k in range(bin(start).count("1"))]
        store = HashOnlyStore()
        tree = CompactMerkleTree(TreeHasher(), start, hashes, store)
        leaves = leaves_of(case, n)
        paths, roots = [], []
        for leaf in leaves:
            paths.append(tree.append(leaf))
            roots.append(tree.root_hash)
        appends.append({"start": start, "hashes": [h.hex() for h in hashes], "leaves": [x.hex() for x in leaves],
                        "paths": [[h.hex() for h in p] for p in paths], "roots": [r.hex() for r in roots],
                        "store_leaves": [h.hex() for h in store._leafs],
                        "store_nodes": [[s, h, x.hex()] for (s, h, x) in store._nodes],
                        "final_hashes": [h.hex() for h in tree.hashes], "final_root": tree.root_hash.hex()})
    verifier = MerkleVerifier()
    for case, (size, i) in enumerate(PROOFS):
        tree = CompactMerkleTree(TreeHasher(), 0, (), HashOnlyStore())
        leaves = leaves_of(100 + case, size)
        for leaf in leaves:
            tree.append(leaf)
        proof, out = tree.inclusion_proof(i, size), {}
        for kind, (leaf, index, prf, root, sz) in proof_variants(leaves[i], i, size, proof, tree.root_hash).items():
            try:
                out[kind] = {"value": verifier.verify_leaf_inclusion(leaf, index, list(prf), STH(sz, root))}
            except Exception as ex:
                out[kind] = {"exc": type(ex).__name__, "msg": str(ex)}
        proofs.append({"size": size, "index": i, "leaf": leaves[i].hex(), "root": tree.root_hash.hex(),
                       "proof": [h.hex() for h in proof], "out": out})
    path = os.path.join(HERE, "merkle.json")
    with open(path, "w") as f:  # one case per line
        f.write('{"appends": [\n' + ",\n".join(json.dumps(c, sort_keys=True) for c in appends) + '],\n"proofs": [\n' +
                ",\n".join(json.dumps(c, sort_keys=True) for c in proofs) + "]}\n")
    print("wrote %s: %d append cases, %d proof bases" % (path, len(appends), len(proofs)))


if __name__ == "__main__":
    main()
