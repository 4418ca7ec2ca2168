"""An independent restatement of the ledger's compact Merkle tree for the Merkle tests: hashlib plus a
frontier stack. Shared (and computed once per case) by tests/test_merkle_host.py and
tests/test_gpu_merkle.py; it imports nothing of the project and nothing of the reference."""
import hashlib

import numpy as np

EMPTY = hashlib.sha256(b"").digest()


def leaf_hash(data):
    return hashlib.sha256(b"\x00" + data).digest()


def node_hash(left, right):
    return hashlib.sha256(b"\x01" + left + right).digest()


def fold(frontier):
    """Root of a frontier (largest subtree first)."""
    if not frontier:
        return EMPTY
    acc = frontier[-1]
    for h in reversed(frontier[:-1]):
        acc = node_hash(h, acc)
    return acc


class RefTree:
    """size + frontier (largest subtree first); append() is one sequential append of the reference."""

    def __init__(self, size=0, frontier=()):
        assert len(frontier) == bin(size).count("1")
        self.size, self.frontier = size, list(frontier)
        self.leaves, self.nodes = [], []  # the hash-store writes, in order

    def append(self, data):
        path = self.frontier[::-1]
        node = leaf_hash(data)
        self.leaves.append(node)
        self.size += 1
        height = 0
        while not (self.size >> height) & 1:  # one carry per trailing zero of the new size
            node = node_hash(self.frontier.pop(), node)
            self.nodes.append(node)
            height += 1
        self.frontier.append(node)
        return path

    @property
    def root(self):
        return fold(self.frontier)


def append_all(size, frontier, leaves):
    """Everything pv_merkle_append_batch returns, from n sequential appends."""
    t = RefTree(size, frontier)
    paths, roots = [], []
    for d in leaves:
        paths.append(t.append(d))
        roots.append(t.root)
    return {"leaf_hash": t.leaves, "node_hash": t.nodes, "frontier": list(t.frontier), "root": t.root, "roots": roots,
            "paths": paths, "size": t.size}


def check_path(leaf_h, index, size, proof):
    """(status, calculated root) of the audit-path walk: 0 walked, 1 size <= index, 2 too short, 3 too long."""
    if size <= index:
        return 1, None
    acc, used, last = leaf_h, 0, size - 1
    while last > 0:
        if used == len(proof):
            return 2, None
        if index & 1:
            acc = node_hash(proof[used], acc)
            used += 1
        elif index < last:
            acc = node_hash(acc, proof[used])
            used += 1
        index >>= 1
        last >>= 1
    return (3, None) if used < len(proof) else (0, acc)


def proof_variants(leaf, index, size, proof, root):
    """The (leaf, index, proof, root, size) variants of one valid inclusion proof that tests/golden/merkle.json
    records the reference's outcome for, by name (make_merkle_golden.py and the tests build them here)."""
    extra, other = hashlib.sha256(b"extra").digest(), hashlib.sha256(b"root").digest()
    return {"valid": (leaf, index, proof, root, size), "truncated": (leaf, index, proof[:-1], root, size),
            "extended": (leaf, index, proof + [extra], root, size), "wrong_root": (leaf, index, proof, other, size),
            "wrong_leaf": (leaf + b"x", index, proof, root, size),
            "wrong_index": (leaf, (index + 1) % size, proof, root, size),
            "index_ge_size": (leaf, size + index, proof, root, size)}


def golden_proof_items(golden):
    """[(kind, (leaf, index, proof, root, size), recorded outcome)] of every proof case of the goldens."""
    out = []
    for b in golden["proofs"]:
        vs = proof_variants(bytes.fromhex(b["leaf"]), b["index"], b["size"], [bytes.fromhex(h) for h in b["proof"]],
                            bytes.fromhex(b["root"]))
        out += [(kind, vs[kind], b["out"][kind]) for kind in sorted(vs)]
    return out


def random_frontier(rng, size):
    return [rng.bytes(32) for _ in range(bin(size).count("1"))]


def random_leaves(rng, n, lo=0, hi=120):
    return [rng.bytes(int(rng.integers(lo, hi + 1))) for _ in range(n)]


def pack(leaves, lead=0):
    """(uint8 blob, uint64 offsets) with `lead` unused bytes in front, so records start at odd addresses."""
    off = np.zeros(len(leaves) + 1, np.uint64)
    np.cumsum([len(x) for x in leaves], out=off[1:])
    off += np.uint64(lead)
    blob = np.frombuffer(bytes(lead) + b"".join(leaves) + b"\0", np.uint8)
    return blob, off


def assert_batch_equals(res, want, n, what=""):
    """res: plenum_amd._native.merkle_append's dict; want: append_all's."""
    if "leaf_hash" in res:
        assert res["leaf_hash"].tobytes() == b"".join(want["leaf_hash"]), what + " leaf hashes"
    if "node_hash" in res:
        assert res["node_hash"].tobytes() == b"".join(want["node_hash"]), what + " node hashes"
    if "frontier" in res:
        assert res["frontier"].tobytes() == b"".join(want["frontier"]), what + " frontier"
    if "root" in res:
        assert res["root"].tobytes() == want["root"], what + " root"
    if "roots" in res:
        assert res["roots"].tobytes() == b"".join(want["roots"]), what + " roots"
    if "path" in res:
        lens = np.array([len(p) for p in want["paths"]], np.uint64)
        assert np.array_equal(np.diff(res["path_off"]), lens) and int(res["path_off"][0]) == 0, what + " path offsets"
        assert res["path"].tobytes() == b"".join(b"".join(p) for p in want["paths"]), what + " paths"
