"""An independent restatement of the ledger's consistency-proof check and of catch-up verification for the
consistency tests (tests/test_consistency_host.py, tests/test_gpu_consistency.py and the golden generator):
hashlib and the RFC 6962 definitions of MTH and PROOF. It imports nothing of the project and nothing of
the reference.

Status codes (csrc/merkle_core.h): 0 consistent, 1 old_size > new_size, 2 proof too short, 3 the second
(new) root differs, 4 the new root matches and the first (old) one differs, 5 equal sizes with different
roots, 6 (catch-up only) the reply's end is out of range."""
import hashlib
import json
from binascii import hexlify

import numpy as np

from merkle_ref import EMPTY, leaf_hash, node_hash

GIANT = 2 ** 48 - 1  # the largest size the library represents


def chains(old_size, new_size, old_root, proof):
    """(old chain end, new chain end, hashes used) of the consistency walk for 0 < old_size < new_size, or
    None when the proof runs out where a hash is needed."""
    node, last = old_size - 1, new_size - 1
    while node % 2:
        node, last = node // 2, last // 2
    used = 0
    if node:
        if not proof:
            return None
        old_h = new_h = proof[0]
        used = 1
    else:
        old_h = new_h = old_root
    while node:
        if node % 2:
            if used == len(proof):
                return None
            old_h, new_h, used = node_hash(proof[used], old_h), node_hash(proof[used], new_h), used + 1
        elif node < last:
            if used == len(proof):
                return None
            new_h, used = node_hash(new_h, proof[used]), used + 1
        node, last = node // 2, last // 2
    while last:
        if used == len(proof):
            return None
        new_h, used = node_hash(new_h, proof[used]), used + 1
        last //= 2
    return old_h, new_h, used


def check(old_size, new_size, old_root, new_root, proof):
    """The status of verify_tree_consistency for non-negative sizes."""
    if old_size > new_size:
        return 1
    if old_size == new_size:
        return 0 if old_root == new_root else 5
    if old_size == 0:
        return 0
    ends = chains(old_size, new_size, old_root, proof)
    if ends is None:
        return 2
    if ends[1] != new_root:
        return 3
    return 0 if ends[0] == old_root else 4


def proof_length(old_size, new_size):
    """Hashes the walk consumes for 0 < old_size < new_size."""
    node, last = old_size - 1, new_size - 1
    while node % 2:
        node, last = node // 2, last // 2
    used = 1 if node else 0
    while node:
        used += 1 if node % 2 or node < last else 0
        node, last = node // 2, last // 2
    return used + last.bit_length()


def status_of(outcome):
    """The status a recorded outcome ({"value": True} or {"exc", "msg"}) of the reference stands for."""
    if "exc" not in outcome:
        return 0
    msg = outcome["msg"]
    if outcome["exc"] == "ValueError":
        return 1
    if "too short" in msg:
        return 2
    if "second root hash" in msg:
        return 3
    return 4 if "first root hash" in msg else 5


def flip(h, bit):
    a = bytearray(h)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def variants(a, b, old_root, new_root, proof):
    """The (old_size, new_size, old_root, new_root, proof) variants of one valid consistency proof that
    tests/golden/merkle_consistency.json records the reference's outcome for, by name."""
    extra, other, junk = (hashlib.sha256(x).digest() for x in (b"extra", b"other root", b"junk"))
    out = {"valid": (a, b, old_root, new_root, proof), "truncated": (a, b, old_root, new_root, proof[:-1]),
           "empty": (a, b, old_root, new_root, []), "extended": (a, b, old_root, new_root, proof + [extra]),
           "wrong_old_root": (a, b, other, new_root, proof), "wrong_new_root": (a, b, old_root, other, proof),
           "swapped": (b, a, old_root, new_root, proof), "same_size_differs": (b, b, other, new_root, proof),
           "zero_old": (0, b, junk, new_root, [junk, extra])}
    for k in range(len(proof)):
        out["flip_%02d" % k] = (a, b, old_root, new_root, proof[:k] + [flip(proof[k], (37 * k + 5) % 256)] + proof[k + 1:])
    return out


def golden_items(golden):
    """[(name, (old, new, old_root, new_root, proof), recorded outcome)] of every pair of the goldens
    (as load_golden returns them)."""
    out = []
    for c in golden["pairs"]:
        vs = variants(c["old"], c["new"], bytes.fromhex(c["old_root"]), bytes.fromhex(c["new_root"]),
                      [bytes.fromhex(h) for h in c["proof"]])
        assert sorted(vs) == sorted(c["out"])
        out += [("%d,%d %s" % (c["old"], c["new"], k), vs[k], c["out"][k]) for k in sorted(vs)]
    return out


# ---- the goldens' compact form. tests/golden/merkle_consistency.json keeps every hash that occurs more than
# once in a table ("hashes") and names it by its index, and keeps an exception as its kind (the status it
# stands for) and, where its text quotes a hash the reference computed, that hash; "texts" holds, per kind,
# the class and the text with its variable parts named. unpack_outcome rebuilds class and text exactly: the
# generator asserts, for every outcome it records, that the rebuilt text is the reference's.
def _quoted(h):
    return "%s" % hexlify(h).strip()  # as the reference formats a hash: b'..'


def pack_outcome(out, args, texts, index):
    """Generator side: the compact record of outcome `out` of verify_tree_consistency(*args)."""
    if "exc" not in out:
        return 0
    kind, msg = status_of(out), out["msg"]
    template, computed = msg, None
    if kind == 1:
        template = msg.replace("(%d vs %d)" % args[:2], "({old} vs {new})")
    elif kind in (3, 4):
        computed = bytes.fromhex(msg.rsplit("computed hash: b'", 1)[1][:64])
        template = msg.replace(_quoted(args[3] if kind == 3 else args[2]), "{expected}", 1)
        template = template.rsplit(_quoted(computed), 1)[0] + "{computed}"
    assert texts.setdefault(str(kind), [out["exc"], template]) == [out["exc"], template], (kind, template)
    rec = kind if computed is None else [kind, index.get(computed, computed.hex())]
    assert unpack_outcome(rec, args, texts, {v: k for k, v in index.items()}) == out, (out, rec)
    return rec


def unpack_outcome(rec, args, texts, table):
    """{"value": True} or {"exc", "msg"}, as the reference gave it, from the compact record. table: index -> hash."""
    if rec == 0:
        return {"value": True}
    kind, computed = (rec, None) if isinstance(rec, int) else rec
    if computed is not None:
        computed = table[computed] if isinstance(computed, int) else bytes.fromhex(computed)
    exc, template = texts[str(kind)]
    msg = template.format(old=args[0], new=args[1], expected=_quoted(args[3] if kind == 3 else args[2]),
                          computed=_quoted(computed) if computed else "")
    return {"exc": exc, "msg": msg}


def load_golden(path):
    """The goldens expanded: pairs as {"old", "new", "old_root", "new_root", "proof", "out": {variant: outcome}},
    catchups as {"start", "hashes", "final_size", "final_root", "tampered", "replies": [{"leaves", "proof",
    "out"}]}; hashes and leaves in hex."""
    with open(path) as f:
        g = json.load(f)
    table = {i: bytes.fromhex(h) for i, h in enumerate(g["hashes"])}
    pairs = []
    for old, new, old_root, new_root, proof, outs in g["pairs"]:
        prf = [table[i] for i in proof]
        vs = variants(old, new, table[old_root], table[new_root], prf)
        pairs.append({"old": old, "new": new, "old_root": table[old_root].hex(), "new_root": table[new_root].hex(),
                      "proof": [h.hex() for h in prf],
                      "out": {k: unpack_outcome(rec, vs[k], g["texts"], table) for k, rec in outs.items()}})
    catchups = []
    for c in g["catchups"]:
        c = dict(c, hashes=[table[i].hex() for i in c["hashes"]], final_root=table[c["final_root"]].hex(),
                 replies=[dict(r, proof=[table[i].hex() for i in r["proof"]]) for r in c["replies"]])
        catchups.append(c)
    return {"pairs": pairs, "catchups": catchups}


def _split(n):
    return 1 << ((n - 1).bit_length() - 1)


class PartialTree:
    """A tree known from size s on: its frontier at s (largest subtree first) and the hashes of the leaves
    appended since. root(e) and proof(e, f) for s <= e <= f <= size follow RFC 6962's MTH and PROOF; a
    range that lies wholly below s is only ever asked for as an aligned node [p, p + 2^b) with
    p + 2^b <= s on the path to a leaf at or above s - 1, which is s's frontier entry for bit b."""

    def __init__(self, s, frontier, leaf_hashes=()):
        assert len(frontier) == bin(s).count("1")
        self.s, self.frontier, self.leaves = s, list(frontier), list(leaf_hashes)
        self.memo = {}

    @property
    def size(self):
        return self.s + len(self.leaves)

    def extend(self, data):
        self.leaves += [leaf_hash(x) for x in data]

    def mth(self, lo, hi):
        n = hi - lo
        if hi <= self.s:
            b = n.bit_length() - 1
            assert n == 1 << b and lo % n == 0 and (self.s >> b) & 1 and (self.s >> (b + 1)) << (b + 1) == lo, (lo, hi, self.s)
            return self.frontier[bin(self.s >> (b + 1)).count("1")]
        if n == 1:
            return self.leaves[lo - self.s]
        got = self.memo.get((lo, hi))
        if got is None:
            k = _split(n)
            got = self.memo[(lo, hi)] = node_hash(self.mth(lo, lo + k), self.mth(lo + k, hi))
        return got

    def root(self, e):
        return self.mth(0, e) if e else EMPTY

    def _subproof(self, m, lo, hi, whole):
        if m == hi:
            return [] if whole else [self.mth(lo, hi)]
        k = _split(hi - lo)
        if m <= lo + k:
            return self._subproof(m, lo, lo + k, whole) + [self.mth(lo + k, hi)]
        return self._subproof(m, lo + k, hi, False) + [self.mth(lo, lo + k)]

    def proof(self, e, f):
        """PROOF(e, D[0:f]) for 0 < e <= f."""
        return self._subproof(e, 0, f, True)


def giant_cases(rng, count):
    """(old, new, old_root, new_root, proof) with sizes up to 2^48 - 1 that no tree can be built for: random
    proof hashes of the needed length, and the roots the walk itself ends on, so the expected status is 0.
    Half of them straddle 2^32."""
    out = []
    for i in range(count):
        if i % 2:
            a = int(rng.integers(1, 2 ** 32 + 2 ** 20))
            b = a + int(rng.integers(1, 2 ** 33))
        else:
            a = int(rng.integers(1, GIANT))
            b = int(rng.integers(a + 1, GIANT + 1))
        if i % 7 == 0:
            a = 1 << int(rng.integers(0, 47))  # the walk seeded from old_root
            b = max(b, a + 1)
        old_root = rng.bytes(32)
        proof = [rng.bytes(32) for _ in range(proof_length(a, b))]
        old_h, new_h, used = chains(a, b, old_root, proof)
        assert used == len(proof)
        out.append((a, b, old_root if a & (a - 1) == 0 else old_h, new_h, proof))
    return out


def catchup_expected(tree, replies, final_size, final_root):
    """Per reply (leaves, proof) chained onto PartialTree `tree` (extended in place): the status of the check
    of the temporary tree against (final_size, final_root)."""
    out = []
    for leaves, proof in replies:
        tree.extend(leaves)
        out.append(check(tree.size, final_size, tree.root(tree.size), final_root, proof))
    return out


def pack_bits(verdicts):
    return np.packbits(np.asarray(verdicts, bool), bitorder="little")


def make_catchup(rng, s, lens, beyond, tamper=None, leaf_len=(0, 40)):
    """A chain of catch-up replies onto a tree of size s with a random frontier: reply r has lens[r] leaves, the
    final tree has `beyond` leaves more than the last reply ends on, and leaf number `tamper` (0-based within
    the replies' leaves) is altered on the way. Returns a dict: s, frontier, replies [(leaves, proof)], ends,
    final_size, final_root, and `status`, the expected status per reply."""
    frontier = [rng.bytes(32) for _ in range(bin(s).count("1"))]
    n = sum(lens)
    leaves = [rng.bytes(int(rng.integers(leaf_len[0], leaf_len[1] + 1))) for _ in range(n + beyond)]
    true = PartialTree(s, frontier)
    true.extend(leaves)
    final_size = s + n + beyond
    final_root = true.root(final_size)
    replies, ends, at = [], [], 0
    for length in lens:
        sent = [x if at + j != tamper else x + b"!" for j, x in enumerate(leaves[at:at + length])]
        at += length
        ends.append(s + at)
        replies.append((sent, true.proof(s + at, final_size) if s + at < final_size else []))
    status = catchup_expected(PartialTree(s, frontier), replies, final_size, final_root)
    return {"s": s, "frontier": frontier, "replies": replies, "ends": ends, "final_size": final_size,
            "final_root": final_root, "status": status, "n": n}
