"""An independent restatement of the ledger's proof generation for the prove tests (tests/test_prove_host.py,
tests/test_gpu_prove.py): hashlib and the recursive RFC 6962 definitions of MTH, PATH and PROOF over a list
of leaf hashes. It imports nothing of the project and nothing of the reference.

A query is (kind, a, b): kind 0 PATH(a, D[0:b]) for 0 <= a < b, kind 1 PROOF(a, D[0:b]) for 1 <= a <= b,
kind 2 MTH(D[0:b]) for 1 <= b. *_ranges give a proof as the leaf ranges [lo, hi) its hashes cover, which
needs no tree and so works at any size."""
import hashlib

INCLUSION, CONSISTENCY, ROOT = 0, 1, 2


def leaf_hash(data):
    return hashlib.sha256(b"\x00" + data).digest()


def node_hash(left, right):
    return hashlib.sha256(b"\x01" + left + right).digest()


def split(n):
    """The largest power of two smaller than n (n >= 2)."""
    k = 1
    while 2 * k < n:
        k *= 2
    return k


def path_ranges(m, lo, hi):
    """PATH(m, D[lo:hi]) as ranges, m relative to lo (RFC 6962 2.1.1)."""
    out = []
    while hi - lo > 1:  # the recursion unrolled: its results are appended on the way back up
        k = split(hi - lo)
        if m < k:
            out.append((lo + k, hi))
            hi = lo + k
        else:
            out.append((lo, lo + k))
            lo, m = lo + k, m - k
    return out[::-1]


def proof_ranges(m, lo, hi, whole=True):
    """SUBPROOF(m, D[lo:hi], whole) as ranges (RFC 6962 2.1.2), recursive as the RFC states it."""
    n = hi - lo
    if m == n:
        return [] if whole else [(lo, hi)]
    k = split(n)
    if m <= k:
        return proof_ranges(m, lo, lo + k, whole) + [(lo + k, hi)]
    return proof_ranges(m - k, lo + k, hi, False) + [(lo, lo + k)]


def ranges(kind, a, b):
    if kind == INCLUSION:
        assert 0 <= a < b
        return path_ranges(a, 0, b)
    if kind == CONSISTENCY:
        assert 1 <= a <= b
        return proof_ranges(a, 0, b)
    assert kind == ROOT and b >= 1
    return [(0, b)]


class Tree:
    """A list of leaf hashes with memoised MTH."""

    def __init__(self, leaf_hashes):
        self.leaves = list(leaf_hashes)
        self.memo = {}

    def mth(self, lo, hi):
        if hi - lo == 1:
            return self.leaves[lo]
        got = self.memo.get((lo, hi))
        if got is None:
            k = split(hi - lo)
            got = self.memo[(lo, hi)] = node_hash(self.mth(lo, lo + k), self.mth(lo + k, hi))
        return got

    def prove(self, kind, a, b):
        assert b <= len(self.leaves)
        return [self.mth(lo, hi) for lo, hi in ranges(kind, a, b)]

    def store(self):
        """(leaf hashes, node hashes) as the reference's hash store holds them after len(leaves) appends: a
        node is written when the leaf that completes it is appended, lower nodes first."""
        nodes = []
        for u in range(1, len(self.leaves) + 1):
            h = 1
            while u % (1 << h) == 0:
                nodes.append(self.mth(u - (1 << h), u))
                h += 1
        return list(self.leaves), nodes


def valid(kind, a, b, n):
    if kind == INCLUSION:
        return 0 <= a < b <= n
    if kind == CONSISTENCY:
        return 1 <= a <= b <= n
    return kind == ROOT and 1 <= b <= n
