"""Generate tests/golden/merkle_prove.json by running the REFERENCE's own CompactMerkleTree.inclusion_proof and
merkle_tree_hash.

TEST INFRASTRUCTURE, run only where the reference is checked out (the tests read the JSON alone):
    python tests/golden/make_prove_golden.py
The reference (swcurran/indy-plenum, checked out beside this repository) is imported, never copied.
The tree is the 300-leaf tree of make_consistency_golden.py (the same leaf(i)), so the 187 consistency proofs
that tests/golden/merkle_consistency.json records are expected outputs for consistency queries against the
same store, with no new recording; this generator asserts that the two trees have the same roots.
Output (JSON, data only, in the compact form of the consistency golden: a table of hashes, named by index):
  leaves      the 300 leaves, hex (leaf(i) of make_consistency_golden.py)
  hashes      the table
  inclusions  [m, n, [hash indices]]: inclusion_proof(m, n) for every 0 <= m < n <= 33, and for n in
              {2^k - 1, 2^k, 2^k + 1 for k <= 8} and 300 with m in {0, 1, n // 2, n - 2, n - 1}
  roots       hash index of merkle_tree_hash(0, n) for n = 1 .. 300, in order"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("PLENUM_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path[:0] = [REF, os.path.dirname(HERE), HERE]

from ledger.compact_merkle_tree import CompactMerkleTree  # noqa: E402
from ledger.tree_hasher import TreeHasher  # noqa: E402
from consistency_ref import load_golden  # noqa: E402
from make_consistency_golden import HashOnlyStore, leaf  # noqa: E402

N = 300


def cases():
    out = [(m, n) for n in range(1, 34) for m in range(n)]
    sizes = sorted({x for k in range(9) for x in (2 ** k - 1, 2 ** k, 2 ** k + 1)} | {N})
    for n in sizes:
        out += [(m, n) for m in (0, 1, n // 2, n - 2, n - 1) if 0 <= m < n]
    return sorted(set(out), key=lambda c: (c[1], c[0]))


def main():
    tree = CompactMerkleTree(TreeHasher(), 0, (), HashOnlyStore())
    for i in range(N):
        tree.append(leaf(i))
    index = {}

    def ref(h):
        return index.setdefault(h, len(index))

    inclusions = [[m, n, [ref(h) for h in tree.inclusion_proof(m, n)]] for m, n in cases()]
    roots = [ref(tree.merkle_tree_hash(0, n)) for n in range(1, N + 1)]
    by_root = {n + 1: h for n, h in enumerate(roots)}
    table = list(index)
    for c in load_golden(os.path.join(HERE, "merkle_consistency.json"))["pairs"]:  # the same tree
        for size, root in ((c["old"], c["old_root"]), (c["new"], c["new_root"])):
            assert size == 0 or table[by_root[size]].hex() == root, size
    path = os.path.join(HERE, "merkle_prove.json")
    dumps = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(path, "w") as f:
        f.write('{"leaves":' + dumps([leaf(i).hex() for i in range(N)]) + ',\n"hashes":' + dumps([h.hex() for h in table]) +
                ',\n"inclusions":[\n' + ",\n".join(dumps(c) for c in inclusions) + '],\n"roots":' + dumps(roots) + "}\n")
    print("wrote %s: %d inclusion proofs, %d roots, %d hashes, %d bytes" % (path, len(inclusions), len(roots), len(table),
                                                                            os.path.getsize(path)))


if __name__ == "__main__":
    main()
