"""Generate tests/golden/merkle_consistency.json by running the REFERENCE's own
CompactMerkleTree.consistency_proof and MerkleVerifier.verify_tree_consistency.

TEST INFRASTRUCTURE, run only where the reference is checked out (the tests read the JSON alone):
    python tests/golden/make_consistency_golden.py
The reference (swcurran/indy-plenum, checked out beside this repository) is imported, never copied.
Output (JSON, data only, one case per line, in the compact form tests/consistency_ref.py load_golden expands: a
table of the hashes that recur, named by index, and per exception its kind and the hash its text quotes;
this generator asserts that every text rebuilt from that form is the reference's, character for character):
  pairs    per (old, new): both roots and the consistency proof of one 300-leaf tree, and for each variant
           of tests/consistency_ref.py variants() (valid, truncated, empty, extended, a bit flipped in each
           proof hash in turn, wrong old / new root, sizes swapped, equal sizes with different roots, old
           size 0 with junk) verify_tree_consistency's outcome: True or the exception's class and text.
  catchups chains of catch-up replies checked as plenum/server/catchup/catchup_rep_service.py:375-426 checks
           them: a temporary tree extended by every reply's leaves in turn (treeWithAppliedTxns) and
           verify_tree_consistency(temp size, final size, temp root, final root, proof) per reply.
Every "valid" variant and every untampered reply is asserted to be accepted by the reference."""
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
from consistency_ref import load_golden, pack_outcome, variants  # noqa: E402

PAIRS = [(a, b) for b in range(18) for a in range(b + 1)]
PAIRS += [p for k in range(9) for p in ((2 ** k - 1, 2 ** k), (2 ** k, 2 ** k + 1), (2 ** k, 2 ** k))]
PAIRS += [(37, 101), (64, 101), (1, 300), (299, 300)]
PAIRS = sorted(set(PAIRS))
# (ledger size, reply lengths, leaves the final tree has beyond the last reply, index of the tampered leaf or None)
CATCHUPS = ((3, [1] * 8, 0, None), (5, [5] * 4, 3, None), (0, [64, 64], 0, None), (7, [1, 5, 64, 5, 1], 9, None),
            (3, [5, 8, 5, 64, 1], 0, 10),   # the tampered reply ends at 16: the new chain starts from its root
            (3, [5, 7, 5, 64, 1], 2, 10))   # it ends at 15


class HashOnlyStore(MemoryHashStore):
    def readNode(self, pos):
        return self._nodes[pos - 1][2]


def leaf(i):
    return hashlib.sha256(b"consistency golden leaf %d" % i).digest()[:8 + i % 5]


def outcome(verifier, args):
    old, new, old_root, new_root, proof = args
    try:
        return {"value": verifier.verify_tree_consistency(old, new, old_root, new_root, list(proof))}
    except Exception as ex:
        return {"exc": type(ex).__name__, "msg": str(ex)}


def main():
    verifier = MerkleVerifier()
    tree = CompactMerkleTree(TreeHasher(), 0, (), HashOnlyStore())
    for i in range(300):
        tree.append(leaf(i))
    index, texts = {}, {}  # hash -> its index in the table; kind -> [class, text with named parts]

    def ref(h):
        return index.setdefault(h, len(index))

    pairs = []
    for a, b in PAIRS:
        old_root = tree.merkle_tree_hash(0, a) if a else TreeHasher().hash_empty()
        new_root = tree.merkle_tree_hash(0, b) if b else TreeHasher().hash_empty()
        proof = tree.consistency_proof(a, b) if 0 < a < b else []
        head = [a, b, ref(old_root), ref(new_root), [ref(h) for h in proof]]
        vs = variants(a, b, old_root, new_root, proof)
        assert outcome(verifier, vs["valid"]) == {"value": True}, (a, b)
        pairs.append(head + [{k: pack_outcome(outcome(verifier, v), v, texts, index) for k, v in vs.items()}])
    catchups = []
    for start, lens, beyond, tampered in CATCHUPS:
        n = sum(lens)
        final_size = start + n + beyond
        final_root = tree.merkle_tree_hash(0, final_size)
        ledger = CompactMerkleTree(TreeHasher(), 0, ())
        ledger.extend([leaf(i) for i in range(start)])
        temp, at, replies = ledger.__copy__(), start, []
        for length in lens:
            leaves = [leaf(i) if i != tampered else b"tampered" for i in range(at, at + length)]
            at += length
            proof = tree.consistency_proof(at, final_size) if at < final_size else []
            temp.extend(leaves)  # the temporary tree of treeWithAppliedTxns, one reply further
            out = outcome(verifier, (temp.tree_size, final_size, temp.root_hash, final_root, proof))
            bad = tampered is not None and at > tampered
            assert ("exc" in out) == bad, (start, lens, at, out)
            replies.append({"leaves": [x.hex() for x in leaves], "proof": [ref(h) for h in proof], "out": out})
        catchups.append({"start": start, "hashes": [ref(h) for h in ledger.hashes], "final_size": final_size,
                         "final_root": ref(final_root), "tampered": tampered, "replies": replies})
    path = os.path.join(HERE, "merkle_consistency.json")
    dumps = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))  # noqa: E731
    with open(path, "w") as f:  # one case per line
        f.write('{"texts":' + dumps(texts) + ',\n"hashes":' + dumps([h.hex() for h in index]) + ',\n"pairs":[\n' +
                ",\n".join(dumps(c) for c in pairs) + '],\n"catchups":[\n' + ",\n".join(dumps(c) for c in catchups) + "]}\n")
    back = load_golden(path)
    assert len(back["pairs"]) == len(pairs) and all(c["out"]["valid"] == {"value": True} for c in back["pairs"])
    print("wrote %s: %d pairs, %d catch-up cases, %d bytes" % (path, len(pairs), len(catchups), os.path.getsize(path)))


if __name__ == "__main__":
    main()
