"""Batched proof generation without a GPU: the library's host path (pv_merkle_path(HOST)) for
pv_merkle_prove_plan and pv_merkle_prove_batch against the goldens recorded from the reference
(tests/golden/merkle_prove.json and the consistency proofs of tests/golden/merkle_consistency.json, one
300-leaf tree) and against an independent restatement (tests/prove_ref.py); the Python methods of
plenum_amd.merkle against the sequential ones; the status codes, the out_off guard and the argument checks.
The walker is the kernels' (csrc/merkle_core.h); tests/test_gpu_prove.py runs it on the device."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as C
import prove_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "indy-plenum_amd", "csrc")
VP = ctypes.c_void_p
GIANT = 2 ** 48 - 1
FILL = 0xEE
GUARD = 96  # bytes behind out and behind status that no call may touch


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    return _native


@pytest.fixture()
def host_path(native):
    native.merkle_path(native.PV_MERKLE_HOST)
    yield native
    native.merkle_path(native.PV_MERKLE_AUTO)
    native.merkle_chunk(0)


def ptr(a):
    return a.ctypes.data_as(VP)


def load_golden():
    """(leaves, cases): the 300 leaves and every recorded (kind, a, b, proof) of the one tree: the inclusion
    proofs and roots of merkle_prove.json and the consistency proofs of merkle_consistency.json."""
    with open(os.path.join(HERE, "golden", "merkle_prove.json")) as f:
        g = json.load(f)
    table = [bytes.fromhex(h) for h in g["hashes"]]
    cases = [(P.INCLUSION, m, n, [table[i] for i in proof]) for m, n, proof in g["inclusions"]]
    cases += [(P.ROOT, 0, n + 1, [table[i]]) for n, i in enumerate(g["roots"])]
    pairs = C.load_golden(os.path.join(HERE, "golden", "merkle_consistency.json"))["pairs"]
    cases += [(P.CONSISTENCY, c["old"], c["new"], [bytes.fromhex(h) for h in c["proof"]]) for c in pairs if c["old"] >= 1]
    return [bytes.fromhex(x) for x in g["leaves"]], cases, len(pairs)


@pytest.fixture(scope="module")
def golden(native):
    """The goldens, and the store as the library's own append writes it (host path)."""
    leaves, cases, n_pairs = load_golden()
    assert len(leaves) == 300 and n_pairs == 187 and len(cases) > 1000
    native.merkle_path(native.PV_MERKLE_HOST)
    blob, off = native._blob(leaves)
    r = native.merkle_append(0, b"", blob, off, want=("leaf_hash", "node_hash"))
    native.merkle_path(native.PV_MERKLE_AUTO)
    return (r["leaf_hash"].reshape(-1).copy(), r["node_hash"].reshape(-1).copy()), cases


def make_tree(n, seed):
    rng = np.random.default_rng(seed)
    return P.Tree([P.leaf_hash(rng.bytes(int(rng.integers(0, 20)))) for _ in range(n)])


def store_of(tree):
    leafs, nodes = tree.store()
    assert len(nodes) == len(leafs) - bin(len(leafs)).count("1")
    return np.frombuffer(b"".join(leafs) + bytes(32), np.uint8)[:32 * len(leafs)], \
        np.frombuffer(b"".join(nodes) + bytes(32), np.uint8)[:32 * len(nodes)]


@pytest.fixture(scope="module")
def tree70():
    """A 70-leaf tree, every valid (kind, a, b) with b <= 70 and the restatement's proofs; computed once."""
    tree = make_tree(70, 61)
    queries = [(k, a, b) for b in range(1, 71) for a in range(b + 1) for k in (0, 1, 2) if P.valid(k, a, b, 70) and (k != 2 or a == 0)]
    assert len(queries) == 70 * 71 // 2 * 2 + 70
    return store_of(tree), queries, [tree.prove(*q) for q in queries]


def q_arrays(queries):
    return (np.array([q[0] for q in queries], np.uint8), np.array([q[1] for q in queries], np.uint64),
            np.array([q[2] for q in queries], np.uint64))


def plan(native, n_leaves, queries):
    kind, a, b = q_arrays(queries)
    off, status = np.zeros(len(queries) + 1, np.uint64), np.full(len(queries) + 1, FILL, np.uint8)
    native.check(native.lib().pv_merkle_prove_plan(n_leaves, ptr(kind), ptr(a), ptr(b), len(queries), ptr(off), ptr(status)),
                 "pv_merkle_prove_plan")
    assert status[-1] == FILL
    return off, status[:-1]


def prove(native, store, queries, off=None, call=None):
    """The C entry on host buffers with stale bytes in out and status beforehand. Returns (out_off, the hashes
    as bytes, status) after checking that the bytes behind both outputs are untouched. call(args) replaces
    the product entry (the thread-count shim)."""
    leaf, node = store
    n_leaves, q = leaf.size // 32, len(queries)
    kind, a, b = q_arrays(queries)
    if off is None:
        off, _ = plan(native, n_leaves, queries)
    total = int(off[q])
    out, status = np.full(32 * total + GUARD, FILL, np.uint8), np.full(q + GUARD, FILL, np.uint8)
    args = [ptr(leaf), n_leaves, ptr(node), ptr(kind), ptr(a), ptr(b), q, ptr(off), ptr(out), ptr(status)]
    if call:
        call(args)
    else:
        native.check(native.lib().pv_merkle_prove_batch(*args), "pv_merkle_prove_batch")
    assert (out[32 * total:] == FILL).all() and (status[q:] == FILL).all()
    return off, out[:32 * total].tobytes(), status[:q]


def split(off, flat):
    return [[flat[32 * j:32 * j + 32] for j in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]


def assert_proofs(native, store, queries, want, **kw):
    off, flat, status = prove(native, store, queries, **kw)
    assert not status.any()
    got = split(off, flat)
    for q, g, w in zip(queries, got, want):
        assert g == w, q
    return flat


# ------------------------------------------------------------------------------------- the C entries

def test_every_golden_case_byte_for_byte(host_path, golden):
    store, cases = golden
    assert {c[0] for c in cases} == {0, 1, 2}
    assert_proofs(host_path, store, [c[:3] for c in cases], [c[3] for c in cases])


def test_restatement_agrees_with_the_reference_recordings(golden):
    store, cases = golden
    tree = P.Tree([store[0][32 * i:32 * i + 32].tobytes() for i in range(300)])
    for kind, a, b, proof in cases:
        assert tree.prove(kind, a, b) == proof, (kind, a, b)
    leafs, nodes = tree.store()
    assert b"".join(nodes) == store[1].tobytes()


def test_every_query_up_to_70_leaves_in_one_call(host_path, tree70):
    store, queries, want = tree70
    assert_proofs(host_path, store, queries, want)


def test_plan_lengths_up_to_the_largest_size(native):
    rng = np.random.default_rng(62)
    queries = [(P.CONSISTENCY, 2 ** 47 - 1, GIANT), (P.INCLUSION, 0, GIANT), (P.INCLUSION, GIANT - 1, GIANT),
               (P.CONSISTENCY, GIANT - 1, GIANT), (P.CONSISTENCY, GIANT, GIANT), (P.ROOT, 0, GIANT), (P.CONSISTENCY, 2 ** 47, GIANT)]
    for i in range(3000):
        hi = GIANT if i % 2 else 2 ** int(rng.integers(2, 49)) - 1
        b = int(rng.integers(2, hi + 1))
        a = int(rng.integers(1, b))
        if i % 5 == 0:
            a = 1 << int(rng.integers(0, b.bit_length() - 1))
        queries.append((int(rng.integers(0, 3)), a, b))
    off, status = plan(native, GIANT, queries)
    assert not status.any()
    lens = np.diff(off).tolist()
    assert lens == [len(P.ranges(*q)) for q in queries]
    assert lens[0] == 49 == max(lens) and lens[1] == 48 == max(n for n, q in zip(lens, queries) if q[0] == P.INCLUSION)
    assert lens[4] == 0 and lens[5] == 1


BAD_QUERIES = [(0, 5, 5), (0, 6, 5), (0, 0, 71), (0, 0, 0), (0, 2 ** 63, 2 ** 63 + 1), (1, 0, 5), (1, 6, 5), (1, 3, 71), (1, 0, 0),
               (2, 0, 0), (2, 0, 71), (2, 7, 2 ** 48), (3, 1, 2), (255, 1, 2)]


def test_status_1_for_each_out_of_range_form(host_path, tree70):
    store, queries, want = tree70
    mixed, expect = [], []
    for i, bad in enumerate(BAD_QUERIES):  # good queries in between
        mixed += [bad, queries[37 * i]]
        expect += [[], want[37 * i]]
    off, status = plan(host_path, 70, mixed)
    assert status.tolist() == [1, 0] * len(BAD_QUERIES)
    assert np.diff(off).tolist() == [len(x) for x in expect]
    off, flat, status = prove(host_path, store, mixed)
    assert status.tolist() == [1, 0] * len(BAD_QUERIES) and split(off, flat) == expect


def guarded(native, store, queries, want, victim, **kw):
    """out_off one hash too small for query `victim`: status 2 there and nothing written, every other query
    written in its (shifted) slot."""
    off, _ = plan(native, store[0].size // 32, queries)
    off[victim + 1:] -= np.uint64(1)
    off, flat, status = prove(native, store, queries, off=off, **kw)
    expect = [0] * len(queries)
    expect[victim] = 2
    assert status.tolist() == expect
    got = split(off, flat)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == (w if i != victim else [bytes([FILL]) * 32] * (len(w) - 1)), i


def test_status_2_when_a_slot_is_one_hash_too_small(host_path, tree70):
    store, queries, want = tree70
    sel = [i for i in range(len(queries)) if want[i]][::41]  # a slot of no hashes cannot be too small
    assert len(sel) > 100 and {queries[i][0] for i in sel} == {0, 1, 2}
    for victim in (0, len(sel) // 2, len(sel) - 1):
        guarded(host_path, store, [queries[i] for i in sel], [want[i] for i in sel], victim)


def test_argument_errors(native, tree70):
    store, queries, _ = tree70
    L, ARG = native.lib(), native.PV_ERR_ARG
    kind, a, b = q_arrays(queries[:3])
    off, _ = plan(native, 70, queries[:3])
    out, st = np.zeros(32 * int(off[3]) + 32, np.uint8), np.zeros(3, np.uint8)
    good = [ptr(store[0]), 70, ptr(store[1]), ptr(kind), ptr(a), ptr(b), 3, ptr(off), ptr(out), ptr(st)]
    native.merkle_path(native.PV_MERKLE_HOST)
    try:
        assert L.pv_merkle_prove_batch(*good) == native.PV_OK
        for k, v, text in ((1, 2 ** 48, b"2^48"), (6, 2 ** 32, b"2^32"), (7, ptr(np.array([0, 3, 2, 4], np.uint64)), b"non-decreasing"),
                           (3, None, b"null"), (9, None, b"null"), (0, None, b"null")):
            bad = list(good)
            bad[k] = v
            assert L.pv_merkle_prove_batch(*bad) == ARG and text in L.pv_last_error(), k
        assert L.pv_merkle_prove_plan(2 ** 48, ptr(kind), ptr(a), ptr(b), 3, ptr(off), None) == ARG
        assert L.pv_merkle_prove_plan(70, ptr(kind), ptr(a), ptr(b), 2 ** 32, ptr(off), None) == ARG
        assert L.pv_merkle_prove_plan(70, ptr(kind), ptr(a), ptr(b), 3, None, None) == ARG
        assert L.pv_merkle_prove_batch(*(good[:6] + [0, None, None, None])) == native.PV_OK  # q = 0
    finally:
        native.merkle_path(native.PV_MERKLE_AUTO)


def test_argument_errors_code_and_message(native, tree70):
    """One bad call per check of pv_merkle_prove_plan and pv_merkle_prove_batch, and pairs of bad arguments for
    the order of the checks: the return code and the message as the library gave them when every entry wrote its
    checks out itself (the bounds are csrc/merkle_plan.h's now)."""
    from test_merkle_host import assert_refusals
    store, queries, _ = tree70
    L, ARG = native.lib(), native.PV_ERR_ARG
    kind, a, b = q_arrays(queries[:3])
    off, _ = plan(native, 70, queries[:3])
    out, st = np.zeros(32 * int(off[3]) + 32, np.uint8), np.zeros(3, np.uint8)
    good = [ptr(store[0]), 70, ptr(store[1]), ptr(kind), ptr(a), ptr(b), 3, ptr(off), ptr(out), ptr(st)]
    dec = np.array([0, 3, 2, 4], np.uint64)

    def batch(**kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return L.pv_merkle_prove_batch(*args)

    def planned(n_leaves=70, q=3, out_off=ptr(off), kind_=ptr(kind)):
        return L.pv_merkle_prove_plan(n_leaves, kind_, ptr(a), ptr(b), q, out_off, None)

    P, B = "pv_merkle_prove_plan: ", "pv_merkle_prove_batch: "
    STORE, COUNT = "the store must stay below 2^48 leaves", "more than 2^32 - 1 queries"
    native.merkle_path(native.PV_MERKLE_HOST)
    try:
        assert batch() == native.PV_OK and planned() == native.PV_OK
        assert_refusals(L, [
            (lambda: planned(n_leaves=2 ** 48), ARG, P + STORE),
            (lambda: planned(q=2 ** 32), ARG, P + COUNT),
            (lambda: planned(out_off=None), ARG, P + "null pointer"),
            (lambda: planned(kind_=None), ARG, P + "null pointer"),
            (lambda: planned(n_leaves=2 ** 48, q=2 ** 32), ARG, P + STORE),
            (lambda: planned(q=2 ** 32, out_off=None), ARG, P + COUNT),
            (lambda: batch(a1=2 ** 48), ARG, B + STORE),
            (lambda: batch(a6=2 ** 32), ARG, B + COUNT),
            (lambda: batch(a3=None), ARG, B + "null pointer"),
            (lambda: batch(a0=None), ARG, B + "null pointer"),
            (lambda: batch(a2=None), ARG, B + "null pointer"),
            (lambda: batch(a7=ptr(dec)), ARG, B + "out_off must be non-decreasing over an output array"),
            (lambda: batch(a8=None), ARG, B + "out_off must be non-decreasing over an output array"),
            (lambda: batch(a1=2 ** 48, a6=2 ** 32), ARG, B + STORE),
            (lambda: batch(a6=2 ** 32, a3=None), ARG, B + COUNT),
            (lambda: batch(a9=None, a7=ptr(dec)), ARG, B + "null pointer"),
        ])
    finally:
        native.merkle_path(native.PV_MERKLE_AUTO)


def test_auto_serves_a_machine_without_a_device(native, tree70, monkeypatch):
    store, queries, want = tree70
    native.merkle_path(native.PV_MERKLE_AUTO)
    monkeypatch.setattr(native, "ensure_device", lambda *a: pytest.fail("a 100-query AUTO batch bound a device"))
    off, hashes, status = native.merkle_prove(store[0], store[1], *q_arrays(queries[:100]))
    assert not status.any() and split(off, hashes.tobytes()) == want[:100]


def provehost_lib(native):
    """tests/native/provehost.cpp beside the product library it links (rebuilt when older than either)."""
    src, lib = os.path.join(HERE, "native", "provehost.cpp"), os.path.join(HERE, "native", "libprovehost.so")
    product = native.LIB_PATH
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in (src, product, CSRC + "/merkle_host.h")):
        subprocess.check_call(["g++", "-O1", "-fPIC", "-shared", "-I" + CSRC, src, "-o", lib, product,
                               "-Wl,-rpath," + os.path.dirname(product)])
    L = ctypes.CDLL(lib)
    L.ph_prove.restype = None
    L.ph_prove.argtypes = [VP, ctypes.c_uint64, VP, VP, VP, VP, ctypes.c_uint64, VP, VP, VP, ctypes.c_uint32]
    return L


def test_one_thread_against_sixteen(native):
    """40,000 queries against a 2,051-leaf store: enough for the host path to start all its threads."""
    tree = make_tree(2051, 63)
    store = store_of(tree)
    rng = np.random.default_rng(64)
    b = rng.integers(1, 2052, 40000)
    a = (rng.integers(0, 2 ** 31, 40000) % b)
    kind = rng.integers(0, 3, 40000)
    queries = [(int(k), int(x) + (k == 1), int(y)) for k, x, y in zip(kind, a, b)]
    assert all(P.valid(*q, 2051) for q in queries)
    L = provehost_lib(native)
    off1, flat1, st1 = prove(native, store, queries, call=lambda args: L.ph_prove(*args, 1))
    off16, flat16, st16 = prove(native, store, queries, call=lambda args: L.ph_prove(*args, 16))
    assert not st1.any() and not st16.any() and flat1 == flat16
    for i in range(0, 40000, 397):  # and both are right
        assert split(off1[i:i + 2], flat1)[0] == tree.prove(*queries[i]), queries[i]


# ------------------------------------------------------------------------------- the Python methods

@pytest.fixture(scope="module")
def tree300(native):
    from plenum_amd.merkle import CompactMerkleTree
    leaves = [hashlib.sha256(b"prove leaf %d" % i).digest()[:5 + i % 7] for i in range(300)]
    tree = CompactMerkleTree()
    native.merkle_path(native.PV_MERKLE_HOST)
    tree.append_batch(leaves[:7])
    tree.append_batch(leaves[7:])
    native.merkle_path(native.PV_MERKLE_AUTO)
    return tree, leaves


def test_batch_methods_equal_the_sequential_ones(host_path, tree300):
    tree, _ = tree300
    pairs = [(a, b) for b in range(1, 301) for a in {0, 1, b // 2, b - 2, b - 1} if 0 <= a < b] + [(a, 97) for a in range(97)]
    assert tree.inclusion_proof_batch(pairs) == [tree.inclusion_proof(a, b) for a, b in pairs]
    pairs = [(a, b) for b in range(1, 301) for a in {1, 2, b // 2, b - 1, b} if 1 <= a <= b] + [(a, 300) for a in range(1, 301)]
    assert tree.consistency_proof_batch(pairs) == [tree.consistency_proof(a, b) for a, b in pairs]
    assert tree.merkle_tree_hash_batch(range(1, 301)) == [tree.merkle_tree_hash(0, b) for b in range(1, 301)]
    assert tree.inclusion_proof_batch([]) == [] and tree.merkle_tree_hash_batch([]) == []
    assert tree.consistency_proof_batch([(300, 300)]) == [[]]


def test_batch_methods_name_the_first_bad_query(host_path, tree300):
    tree, _ = tree300
    for method, arg, text in ((tree.inclusion_proof_batch, [(0, 1), (5, 5)], "query 1 (5, 5)"),
                              (tree.inclusion_proof_batch, [(0, 301)], "query 0 (0, 301)"),
                              (tree.inclusion_proof_batch, [(-1, 3)], "query 0 (-1, 3)"),
                              (tree.consistency_proof_batch, [(1, 2), (2, 2), (0, 2), (9, 2)], "query 2 (0, 2)"),
                              (tree.consistency_proof_batch, [(3, 2)], "query 0 (3, 2)"),
                              (tree.merkle_tree_hash_batch, [300, 0], "query 1 (0,)"),
                              (tree.merkle_tree_hash_batch, [301], "query 0 (301,)"),
                              (tree.merkle_tree_hash_batch, [1.5], "query 0 (1.5,)")):
        with pytest.raises(ValueError) as e:
            method(arg)
        assert text in str(e.value) and "300 leaves" in str(e.value)


def test_audit_proofs_are_accepted_by_the_batched_check(host_path, tree300):
    from plenum_amd.merkle import STH, MerkleVerifier
    tree, leaves = tree300
    seq_nos = list(range(1, 301))
    for size in (None, 300, 257, seq_nos):  # Ledger.auditProof at two sizes, and Ledger.merkleInfo
        nos = [s for s in seq_nos if isinstance(size, list) or s <= (size or 300)]
        got = tree.audit_proofs(nos, size if not isinstance(size, list) else nos)
        for s, (root, path, n) in zip(nos, got):
            assert n == (s if isinstance(size, list) else size or 300)
            assert root == tree.merkle_tree_hash(0, n) and path == tree.inclusion_proof(s - 1, n)
        verdicts = MerkleVerifier().verify_leaf_inclusion_batch(
            [(leaves[s - 1], s - 1, path, STH(n, root)) for s, (root, path, n) in zip(nos, got)])
        assert verdicts == [True] * len(nos)
    with pytest.raises(ValueError):
        tree.audit_proofs([0])
    with pytest.raises(ValueError):
        tree.audit_proofs([5], 4)


def test_catchup_proofs_are_accepted_by_the_catchup_check(host_path, tree300):
    from plenum_amd.merkle import CompactMerkleTree
    seeder, leaves = tree300
    for start, lens, till in ((0, [5] * 60, 300), (13, [1, 5, 64, 100, 1], 250), (299, [1], 300)):
        ends = list(np.cumsum(lens) + start)
        proofs = seeder.catchup_proofs(ends, till)
        assert proofs == [seeder.consistency_proof(int(e), till) for e in ends]
        behind = CompactMerkleTree()
        behind.extend(leaves[:start])
        replies = [(leaves[e - n:e], p) for e, n, p in zip(ends, lens, proofs)]
        assert behind.verify_catchup_replies(replies, till, seeder.merkle_tree_hash(0, till)) == [True] * len(lens)


def test_memory_hash_store_arrays_follow_the_lists(host_path):
    from plenum_amd.merkle import CompactMerkleTree
    tree = CompactMerkleTree()
    store = tree.hashStore

    def check():
        leafs, nodes = store.hash_arrays()
        assert bytes(leafs) == b"".join(store.readLeafs(1, store.leafCount))
        assert bytes(nodes) == b"".join(store.readNodes(1, store.nodeCount))
        assert store.is_consistent and store.leafCount == tree.tree_size

    for round_ in range(2):
        tree.append(b"a")
        tree.append_batch([b"b%d" % i for i in range(37)])
        tree.append(b"c")
        tree.append_batch([])
        tree.append_batch([b"d%d" % i for i in range(90)])
        check()
        assert tree.tree_size == 129
        assert tree.inclusion_proof_batch([(128, 129)]) == [tree.inclusion_proof(128, 129)]
        tree.reset()
        assert store.hash_arrays() == (bytearray(), bytearray())
        check()


class ListStore:
    """A foreign store: no hash_arrays, nodes kept as the (size, height, hash) tuples a tree writes."""

    def __init__(self):
        self.leafs, self.nodes, self.reads = [], [], 0

    def writeLeaf(self, h):
        self.leafs.append(h)

    def writeNode(self, node):
        self.nodes.append(node)

    def readLeaf(self, pos):
        return self.leafs[pos - 1]

    def readNode(self, pos):
        return self.nodes[pos - 1][2]

    def readLeafs(self, lo, hi):
        self.reads += 1
        return self.leafs[lo - 1:hi]

    def readNodes(self, lo, hi):
        self.reads += 1
        return self.nodes[lo - 1:hi]

    leafCount = property(lambda self: len(self.leafs))
    nodeCount = property(lambda self: len(self.nodes))

    @staticmethod
    def getNodePosition(start, height=None):
        from plenum_amd.merkle import MemoryHashStore
        return MemoryHashStore.getNodePosition(start, height)


def test_foreign_store_and_other_hasher(host_path, monkeypatch):
    from plenum_amd.merkle import CompactMerkleTree, TreeHasher
    foreign = CompactMerkleTree(hashStore=ListStore())
    plain = CompactMerkleTree()
    other = CompactMerkleTree(TreeHasher(hashlib.sha512))
    for i in range(45):
        for t in (foreign, plain, other):
            t.append(b"leaf %d" % i)
    pairs = [(a, b) for b in range(1, 46) for a in range(b)]
    want = plain.inclusion_proof_batch(pairs)
    assert foreign.inclusion_proof_batch(pairs) == want and foreign.hashStore.reads == 2  # read once per call
    assert foreign.merkle_tree_hash_batch([45]) == [plain.root_hash]
    # a hasher other than SHA-256 loops over the sequential methods and never reaches the library
    monkeypatch.setattr(host_path, "merkle_prove", lambda *a: pytest.fail("a SHA-512 tree reached the library"))
    assert other.inclusion_proof_batch(pairs) == [other.inclusion_proof(a, b) for a, b in pairs]
    assert other.consistency_proof_batch([(3, 45)]) == [other.consistency_proof(3, 45)]
    assert other.merkle_tree_hash_batch([45]) == [other.root_hash] and len(other.root_hash) == 64
    with pytest.raises(ValueError):
        other.inclusion_proof_batch([(45, 45)])
