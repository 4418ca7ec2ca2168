"""The ledger Merkle kernels on the GPU (device path forced): byte-for-byte against the independent
restatement in tests/merkle_ref.py and the goldens recorded from the reference. Shapes are the smallest
at which a kernel can go wrong: every SHA-256 padding edge mixed within one wave, the tile of 1,024
leaves by absolute index (s and s + n one below, on and one above a tile edge), the upper-level kernel's
passes (sizes crossing 2^11, 2^20 and 2^32), chunk chaining, and proofs of every status in one launch."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import merkle_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDARY_LENGTHS = (0, 1, 54, 55, 56, 62, 63, 64, 118, 119, 120, 126, 127, 128)
TILE = 1024  # PV_MERKLE_TILE: the level kernel's only tile size
START_SIZES = (0, 1, 2, 3, 5, 7, 8, 63, 64, 65, 255, 256, 257, 2 ** 20 - 1, 2 ** 20, 2 ** 32 - 3)
BATCH_SIZES = (1, 2, 3, 63, 64, 65, 257, 1000, 4097)


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    _native.ensure_device(0)
    return _native


@pytest.fixture()
def dev(native):
    native.merkle_path(native.PV_MERKLE_DEVICE)
    native.merkle_chunk(0)
    yield native
    native.merkle_path(native.PV_MERKLE_AUTO)
    native.merkle_chunk(0)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "merkle.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def shared_case():
    """One mid-sized case and its restatement, computed once and left unchanged."""
    rng = np.random.default_rng(31)
    s, n = 65, 3001
    frontier, leaves = R.random_frontier(rng, s), R.random_leaves(rng, n, 0, 90)
    return s, n, frontier, leaves, R.append_all(s, frontier, leaves)


def test_leaf_hashing_boundary_lengths_in_one_wave(dev):
    rng = np.random.default_rng(32)
    lens = list(BOUNDARY_LENGTHS) * 5 + list(range(0, 301))
    rng.shuffle(lens)
    leaves = [rng.bytes(int(n)) for n in lens] + [b"\x80" * 55, b"\xff" * 119, rng.bytes(1000), rng.bytes(5000)]
    for lead in (0, 1, 3):  # records at odd addresses
        blob, off = R.pack(leaves, lead=lead)
        got = dev.merkle_append(0, b"", blob, off, want=("leaf_hash",))["leaf_hash"]
        assert got.tobytes() == b"".join(R.leaf_hash(x) for x in leaves), lead


@pytest.mark.parametrize("s", START_SIZES)
def test_append_all_outputs(dev, s):
    rng = np.random.default_rng(33 + s % 1000)
    frontier = R.random_frontier(rng, s)
    for n in BATCH_SIZES:
        leaves = R.random_leaves(rng, n, 0, 70)
        blob, off = R.pack(leaves, lead=n % 4)
        res = dev.merkle_append(s, b"".join(frontier), blob, off)
        R.assert_batch_equals(res, R.append_all(s, frontier, leaves), n, "s=%d n=%d" % (s, n))


@pytest.mark.parametrize("s_mod", (TILE - 1, 0, 1))
def test_append_tile_edges(dev, s_mod):
    """s mod T and (s + n) mod T each one below, on and one above a tile edge, for one, two and three tiles;
    ends at 2,048 +- 1 also switch the upper-level kernel on and off."""
    rng = np.random.default_rng(34 + s_mod)
    for base in (0, 4 * TILE):
        s = base + (s_mod if s_mod != TILE - 1 else TILE - 1) + (TILE if s_mod != TILE - 1 else 0)
        frontier = R.random_frontier(rng, s)
        for end_tile in (2, 3, 4):
            for end_mod in (TILE - 1, 0, 1):
                end = base + end_tile * TILE + (end_mod if end_mod != TILE - 1 else -1)
                n = end - s
                assert n > 0 and end % TILE == end_mod and s % TILE == s_mod
                leaves = R.random_leaves(rng, n, 0, 24)
                res = dev.merkle_append(s, b"".join(frontier), *R.pack(leaves))
                R.assert_batch_equals(res, R.append_all(s, frontier, leaves), n, "s=%d n=%d" % (s, n))


def test_optional_outputs_do_not_change_the_others(dev, shared_case):
    s, _, frontier, leaves, want = shared_case
    n = 257
    leaves = leaves[:n]
    want = R.append_all(s, frontier, leaves)
    blob, off = R.pack(leaves)
    full = dev.MERKLE_OUTPUTS
    for sel in [(k,) for k in full] + [tuple(x for x in full if x != k) for k in full] + [()]:
        res = dev.merkle_append(s, b"".join(frontier), blob, off, want=sel)
        assert set(res) == set(sel) | ({"path_off"} if "path" in sel else set())
        R.assert_batch_equals(res, want, n, str(sel))


def test_chunk_chaining(dev, shared_case):
    s, n, frontier, leaves, want = shared_case
    blob, off = R.pack(leaves, lead=1)
    whole = dev.merkle_append(s, b"".join(frontier), blob, off)
    dev.merkle_chunk(1000)
    chunked = dev.merkle_append(s, b"".join(frontier), blob, off)
    for k in whole:
        assert np.array_equal(whole[k], chunked[k]), k
    R.assert_batch_equals(chunked, want, n)
    R.assert_batch_equals(dev.merkle_append(s, b"".join(frontier), blob, off, want=("frontier", "root")), want, n)


class DevBuf:
    def __init__(self, native, data):
        self.n, self.L = native, native.lib()
        arr = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.size = max(arr.size, 32) + native.PV_BLOB_SLACK
        p = ctypes.c_void_p()
        native.check(self.L.pv_dev_alloc(ctypes.byref(p), self.size), "pv_dev_alloc")
        self.p = p.value
        if arr.size:
            native.check(self.L.pv_memcpy_h2d(self.p, native._ptr(arr), arr.size), "pv_memcpy_h2d")

    def read(self, nbytes):
        out = np.zeros(nbytes, np.uint8)
        if nbytes:
            self.n.check(self.L.pv_memcpy_d2h(self.n._ptr(out), self.p, nbytes), "pv_memcpy_d2h")
        return out

    def free(self):
        self.L.pv_dev_free(self.p)


def device_entry(native, s, frontier, blob, off, n, stream, bufs, skip=()):
    """pv_merkle_append_batch_device with every output on but `skip` (NULL: the library's own workspace
    holds those); returns the output DevBufs (not yet read)."""
    nn, nf, npath = native.merkle_plan(s, n)
    sizes = dict(leaf_hash=32 * n, node_hash=32 * nn, frontier=2048, root=32, roots=32 * n, path=32 * npath,
                 path_off=8 * (n + 1))
    outs = {k: DevBuf(native, np.zeros(max(v, 32), np.uint8)) for k, v in sizes.items()}
    bufs += list(outs.values())
    o = native.PvMerkleOut()
    for k in sizes:
        if k not in skip:
            setattr(o, k, outs[k].p)
    d_f, d_blob, d_off = DevBuf(native, np.frombuffer(b"".join(frontier) or bytes(32), np.uint8)), DevBuf(native, blob), \
        DevBuf(native, off)
    bufs += [d_f, d_blob, d_off]
    native.check(native.lib().pv_merkle_append_batch_device(s, d_f.p if s else None, d_blob.p, d_off.p, n, ctypes.byref(o),
                                                            stream), "pv_merkle_append_batch_device")
    return outs, sizes


def test_device_entry_two_streams_and_host_entry_agree(dev, shared_case):
    s, n, frontier, leaves, want = shared_case
    blob, off = R.pack(leaves)
    L = dev.lib()
    s1, s2 = ctypes.c_void_p(), ctypes.c_void_p()
    dev.check(L.pv_stream_create(ctypes.byref(s1)), "pv_stream_create")
    dev.check(L.pv_stream_create(ctypes.byref(s2)), "pv_stream_create")
    bufs = []
    try:
        dev.merkle_chunk(1024)
        # c and d keep their leaf hashes and nodes in the library's workspace, on different streams right
        # after each other: the second must wait for the first to release those blocks (and the frontiers)
        a, sizes = device_entry(dev, s, frontier, blob, off, n, s1, bufs)
        b, _ = device_entry(dev, s, frontier, blob, off, n, s2, bufs)
        c, _ = device_entry(dev, s, frontier, blob, off, n, s1, bufs, skip=("leaf_hash", "node_hash"))
        d, _ = device_entry(dev, s, frontier, blob, off, n, s2, bufs, skip=("leaf_hash", "node_hash"))
        dev.check(L.pv_stream_sync(s1), "pv_stream_sync")
        dev.check(L.pv_stream_sync(s2), "pv_stream_sync")
        host = dev.merkle_append(s, b"".join(frontier), blob, off)
        nf = bin(s + n).count("1")
        for outs in (a, b):
            got = {k: outs[k].read(v) for k, v in sizes.items()}
            res = {k: got[k].reshape(-1, 32) for k in ("leaf_hash", "node_hash", "roots", "path")}
            res["root"] = got["root"]
            res["frontier"] = got["frontier"][:32 * nf]
            assert not got["frontier"][32 * nf:].any()
            res["path_off"] = got["path_off"].view(np.uint64)
            R.assert_batch_equals(res, want, n, "device entry")
            for k in ("leaf_hash", "node_hash", "roots", "path", "root", "frontier"):
                assert res[k].tobytes() == host[k].tobytes(), k
        for outs in (c, d):
            for k in ("roots", "path", "root"):
                assert outs[k].read(sizes[k]).tobytes() == host[k].tobytes(), k
            assert outs["frontier"].read(32 * nf).tobytes() == host["frontier"].tobytes()
            assert outs["path_off"].read(sizes["path_off"]).view(np.uint64).tolist() == host["path_off"].tolist()
    finally:
        L.pv_stream_destroy(s1)
        L.pv_stream_destroy(s2)
        for x in bufs:
            x.free()


def test_round_trip_paths_verify(dev, shared_case):
    """Every audit path and root append_batch returns verifies: the path append returns for leaf i (the
    frontier before it) is leaf i's inclusion proof in the tree of i + 1 leaves."""
    rng = np.random.default_rng(35)
    n = 1500
    leaves = R.random_leaves(rng, n, 0, 60)
    res = dev.merkle_append(0, b"", *R.pack(leaves))
    po, path = res["path_off"], res["path"]
    proofs = [[path[j].tobytes() for j in range(int(po[i]), int(po[i + 1]))] for i in range(n)]
    roots = [res["roots"][i].tobytes() for i in range(n)]
    verdicts, status = dev.merkle_verify_inclusion(list(range(n)), [i + 1 for i in range(n)], proofs, roots, leaves=leaves)
    assert verdicts.all() and not status.any()
    v2, st2 = dev.merkle_verify_inclusion(list(range(n)), [i + 1 for i in range(n)], proofs, roots,
                                          leaf_hashes=[res["leaf_hash"][i].tobytes() for i in range(n)])
    assert v2.all() and not st2.any()


def flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def test_inclusion_statuses_mixed_in_one_launch(dev):
    rng = np.random.default_rng(36)
    size = 300
    leaves = R.random_leaves(rng, size, 1, 80)
    t = R.append_all(0, [], leaves)
    lh, root = t["leaf_hash"], t["root"]
    from test_merkle_host import brute_force_proof
    items, want = [], []
    for i in [int(x) for x in rng.integers(0, size, 120)] + [0, size - 1]:
        proof = brute_force_proof(lh, i)
        kind = len(items) % 7
        leaf, idx, prf, rt, sz = leaves[i], i, proof, root, size
        if kind == 1:
            leaf = flip(leaf, int(rng.integers(0, 8 * len(leaf))))
        elif kind == 2:
            k = int(rng.integers(0, len(prf)))
            prf = prf[:k] + [flip(prf[k], int(rng.integers(0, 256)))] + prf[k + 1:]
        elif kind == 3:
            rt = flip(rt, int(rng.integers(0, 256)))
        elif kind == 4:
            prf = prf[:-1]
        elif kind == 5:
            prf = prf + [rng.bytes(32)]
        elif kind == 6:
            idx = size + int(rng.integers(0, 3))
        items.append((leaf, idx, prf, rt, sz))
        want.append({0: (True, 0), 1: (False, 0), 2: (False, 0), 3: (False, 0), 4: (False, 2), 5: (False, 3),
                     6: (False, 1)}[kind])
    for (leaf, idx, prf, rt, sz), w in zip(items, want):  # the expectations agree with the restated walk
        st, calc = R.check_path(R.leaf_hash(leaf), idx, sz, prf)
        assert (st == 0 and calc == rt, st) == w
    verdicts, status = dev.merkle_verify_inclusion([x[1] for x in items], [x[4] for x in items], [x[2] for x in items],
                                                   [x[3] for x in items], leaves=[x[0] for x in items])
    assert [(bool(v), int(s)) for v, s in zip(verdicts, status)] == want
    dev.merkle_chunk(50)  # proofs chunked across verdict words
    v2, s2 = dev.merkle_verify_inclusion([x[1] for x in items], [x[4] for x in items], [x[2] for x in items],
                                         [x[3] for x in items], leaves=[x[0] for x in items])
    assert np.array_equal(v2, verdicts) and np.array_equal(s2, status)


def test_goldens_through_the_python_classes(dev, golden):
    from plenum_amd.merkle import STH, CompactMerkleTree, MemoryHashStore, MerkleVerifier, TreeHasher
    for c in golden["appends"]:
        hashes = [bytes.fromhex(h) for h in c["hashes"]]
        leaves = [bytes.fromhex(x) for x in c["leaves"]]
        tree = CompactMerkleTree(TreeHasher(), c["start"], hashes, MemoryHashStore())
        paths, roots = tree.append_batch(leaves)
        assert [[h.hex() for h in p] for p in paths] == c["paths"] and [r.hex() for r in roots] == c["roots"]
        assert [h.hex() for h in tree.hashes] == c["final_hashes"] and tree.root_hash.hex() == c["final_root"]
        assert [h.hex() for h in tree.hashStore.readLeafs(1, len(leaves))] == c["store_leaves"]
        assert [h.hex() for h in tree.hashStore.readNodes(1, tree.nodeCount)] == [x[2] for x in c["store_nodes"]]
        ext = CompactMerkleTree(TreeHasher(), c["start"], hashes).extended_batch(leaves)
        assert [h.hex() for h in ext.hashes] == c["final_hashes"] and ext.root_hash.hex() == c["final_root"]
    cases = R.golden_proof_items(golden)
    items = [(leaf, index, proof, STH(size, root)) for _, (leaf, index, proof, root, size), _ in cases]
    for (kind, _, out), g in zip(cases, MerkleVerifier().verify_leaf_inclusion_batch(items)):
        if "exc" in out:
            assert type(g).__name__ == out["exc"] and str(g) == out["msg"], kind
        else:
            assert g is True
    h = TreeHasher()
    leaves = [bytes.fromhex(x) for c in golden["appends"] for x in c["leaves"]]
    assert h.hash_leaves(leaves) == [h.hash_leaf(x) for x in leaves]


def test_no_leaves_and_single_leaf_into_the_empty_tree(dev):
    res = dev.merkle_append(0, b"", np.zeros(1, np.uint8), np.zeros(1, np.uint64))
    assert res["root"].tobytes() == hashlib.sha256(b"").digest() and res["frontier"].shape == (0, 32)
    rng = np.random.default_rng(37)
    frontier = R.random_frontier(rng, 13)
    res = dev.merkle_append(13, b"".join(frontier), np.zeros(1, np.uint8), np.zeros(1, np.uint64))
    assert res["frontier"].tobytes() == b"".join(frontier) and res["root"].tobytes() == R.fold(frontier)
    one = dev.merkle_append(0, b"", *R.pack([b"only"]))
    assert one["root"].tobytes() == one["leaf_hash"].tobytes() == one["roots"].tobytes() == R.leaf_hash(b"only")
    assert one["node_hash"].size == 0 and one["path"].size == 0 and one["frontier"].tobytes() == R.leaf_hash(b"only")
    # n = 0 on device buffers: the input tree's frontier and root, one small launch
    L = dev.lib()
    d_f, d_front, d_root = DevBuf(dev, np.frombuffer(b"".join(frontier), np.uint8)), DevBuf(dev, np.zeros(2048, np.uint8)), \
        DevBuf(dev, np.zeros(32, np.uint8))
    d_path, d_poff = DevBuf(dev, np.zeros(32, np.uint8)), DevBuf(dev, np.full(1, 77, np.uint64))
    try:
        o = dev.PvMerkleOut()
        o.frontier, o.root, o.path, o.path_off = d_front.p, d_root.p, d_path.p, d_poff.p
        dev.check(L.pv_merkle_append_batch_device(13, d_f.p, None, None, 0, ctypes.byref(o), None), "n = 0")
        dev.check(L.pv_stream_sync(None), "pv_stream_sync")
        assert d_front.read(96).tobytes() == b"".join(frontier) and d_root.read(32).tobytes() == R.fold(frontier)
        assert d_poff.read(8).view(np.uint64)[0] == 0
    finally:
        for x in (d_f, d_front, d_root, d_path, d_poff):
            x.free()


def test_device_entries_argument_errors(dev):
    """One bad call per check of the five device-buffer entries, with small valid device buffers and one bad
    argument (a null pointer, a hash array at offset 8, a size of 2^48, a count of 2^32): the return code and the
    message as the library gave them when every entry wrote its checks out itself (they are csrc/merkle_plan.h's
    now). Without a device these entries answer PV_ERR_NOT_INIT before their checks, so only a GPU run sees the
    strings. Every bad call returns before anything is enqueued; a valid append on the same stream afterwards
    still gives the reference root."""
    from test_merkle_host import assert_refusals
    L, ARG = dev.lib(), dev.PV_ERR_ARG
    buf = DevBuf(dev, np.zeros(4096, np.uint8))
    bufs = [buf]
    p, p8 = buf.p, buf.p + 8
    assert p % 16 == 0

    def outs(**kw):
        o = dev.PvMerkleOut()
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def replace(good, kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return args

    def append(**kw):  # tree_size, frontier, data, off, n, out, stream
        return L.pv_merkle_append_batch_device(*replace([0, None, p, p, 2, outs(root=p), None], kw))

    def catchup(**kw):  # ... n, reply_end, n_replies, final_size, final_root, proof, proof_off, out, status, words, stream
        return L.pv_merkle_catchup_batch_device(*replace([0, None, p, p, 2, p, 1, 2, p, p, p, None, p, p, None], kw))

    def verify(**kw):  # data, off, leaf_hash, leaf_index, tree_size, proof, proof_off, root, n, status, words, stream
        return L.pv_merkle_verify_inclusion_batch_device(*replace([p, p, None, p, p, p, p, p, 2, p, p, None], kw))

    def cons(**kw):  # old_size, new_size, old_root, new_root, proof, proof_off, n, status, words, stream
        return L.pv_merkle_verify_consistency_batch_device(*replace([p, p, p, p, p, p, 2, p, p, None], kw))

    def prove(**kw):  # leaf_hash, n_leaves, node_hash, kind, a, b, q, out_off, out, status, stream
        return L.pv_merkle_prove_batch_device(*replace([p, 4, p, p, p, p, 1, p, p, p, None], kw))

    A, K, V = "pv_merkle_append_batch_device: ", "pv_merkle_catchup_batch_device: ", "pv_merkle_verify_inclusion_batch_device: "
    C_, P = "pv_merkle_verify_consistency_batch_device: ", "pv_merkle_prove_batch_device: "
    NULL, ALIGNED, FRONTIER = "null pointer", "hash arrays must be 16-byte aligned", "a tree of size > 0 needs its frontier"
    EITHER, BOTH_SIZES = "give either data and off, or leaf_hash", "tree_size + n and final_size must stay below 2^48"
    try:
        assert_refusals(L, [
            (lambda: append(a5=None), ARG, A + "null output struct"),
            (lambda: append(a5=outs(path=p)), ARG, A + "path and path_off go together"),
            (lambda: append(a0=2 ** 48, a1=p, a4=0), ARG, A + "tree_size + n must stay below 2^48"),
            (lambda: append(a0=5), ARG, A + FRONTIER),
            (lambda: append(a2=None), ARG, A + NULL),
            (lambda: append(a3=None), ARG, A + NULL),
            (lambda: append(a0=5, a1=p8), ARG, A + ALIGNED),
            (lambda: append(a5=outs(root=p8)), ARG, A + ALIGNED),
            (lambda: append(a5=outs(leaf_hash=p8)), ARG, A + ALIGNED),
            (lambda: append(a5=outs(path=p8, path_off=p8)), ARG, A + ALIGNED),
            (lambda: catchup(a11=outs(path=p)), ARG, K + "path and path_off go together"),
            (lambda: catchup(a0=2 ** 48, a1=p), ARG, K + BOTH_SIZES),
            (lambda: catchup(a7=2 ** 48), ARG, K + BOTH_SIZES),
            (lambda: catchup(a6=2 ** 32), ARG, K + "more than 2^32 - 1 replies"),
            (lambda: catchup(a0=5), ARG, K + FRONTIER),
            (lambda: catchup(a2=None), ARG, K + NULL),
            (lambda: catchup(a5=None), ARG, K + NULL),
            (lambda: catchup(a12=None), ARG, K + NULL),
            (lambda: catchup(a8=p8), ARG, K + ALIGNED),
            (lambda: catchup(a9=p8), ARG, K + ALIGNED),
            (lambda: catchup(a11=outs(frontier=p8)), ARG, K + ALIGNED),
            (lambda: verify(a3=None), ARG, V + NULL),
            (lambda: verify(a5=None), ARG, V + NULL),
            (lambda: verify(a2=p), ARG, V + EITHER),
            (lambda: verify(a0=None, a1=None), ARG, V + EITHER),
            (lambda: verify(a0=None), ARG, V + EITHER),
            (lambda: verify(a5=p8), ARG, V + ALIGNED),
            (lambda: verify(a7=p8), ARG, V + ALIGNED),
            (lambda: verify(a0=None, a1=None, a2=p8), ARG, V + ALIGNED),
            (lambda: verify(a8=2 ** 32), ARG, V + "more than 2^32 - 1 proofs"),
            (lambda: cons(a0=None), ARG, C_ + NULL),
            (lambda: cons(a8=None), ARG, C_ + NULL),
            (lambda: cons(a2=p8), ARG, C_ + ALIGNED),
            (lambda: cons(a4=p8), ARG, C_ + ALIGNED),
            (lambda: cons(a6=2 ** 32), ARG, C_ + "more than 2^32 - 1 proofs"),
            (lambda: prove(a1=2 ** 48), ARG, P + "the store must stay below 2^48 leaves"),
            (lambda: prove(a6=2 ** 32), ARG, P + "more than 2^32 - 1 queries"),
            (lambda: prove(a3=None), ARG, P + NULL),
            (lambda: prove(a0=None), ARG, P + NULL),
            (lambda: prove(a2=None), ARG, P + NULL),
            (lambda: prove(a0=p8), ARG, P + ALIGNED),
            (lambda: prove(a8=p8), ARG, P + ALIGNED),
        ])
        # nothing was enqueued, and the workspace serves the next call on the same stream
        leaves = [b"first", b"second"]
        blob, off = R.pack(leaves)
        got, sizes = device_entry(dev, 0, [], blob, off, 2, None, bufs)
        dev.check(L.pv_stream_sync(None), "pv_stream_sync")
        assert got["root"].read(32).tobytes() == R.append_all(0, [], leaves)["root"]
    finally:
        for x in bufs:
            x.free()
