"""The state-trie hashing on the GPU (device path forced): pv_sha3_256_batch against hashlib at every padding
edge mixed within one wave; the golden cases recorded from the reference; batches against the sequential
Python classes and against the library's host path. Shapes are the smallest at which a kernel can go wrong:
records at odd addresses, multi-block records next to empty ones, a depth of more than one workgroup beside
depths of a few nodes (the per-depth launches and the single-workgroup tail in one call), existing nodes
fetched in rounds."""
import ctypes
import hashlib

import numpy as np
import pytest

import trie_ref as R

pytestmark = pytest.mark.gpu

CASES = R.load_golden()


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    _native.ensure_device(0)
    return _native


@pytest.fixture(scope="module")
def S():
    from plenum_amd import state_trie
    return state_trie


@pytest.fixture()
def dev(native):
    native.trie_path(native.PV_TRIE_DEVICE)
    yield native
    native.trie_path(native.PV_TRIE_AUTO)


def pairs(tag, n, vlen=150):
    return [(hashlib.sha256(b"%s%d" % (tag, i)).digest(), R.det("%s%d" % (tag.decode(), i), vlen)) for i in range(n)]


def batch_nodes(native, S, mode, root, kv, sets):
    """(new root, {hash: rlp}) of one update through the library in `mode`."""
    native.trie_path(mode)
    new_root, nodes = native.trie_update(root, kv.get if kv else None, [k for k, _ in sets],
                                         [S.rlp_encode([v]) for _, v in sets])
    return new_root, dict(nodes), dict(native.trie_last)


def test_sha3_boundary_lengths_in_one_wave(dev):
    rng = np.random.default_rng(81)
    lens = list(R.SHA3_LENGTHS[:-1]) * 4 + list(range(120, 150)) + list(range(260, 285))
    rng.shuffle(lens)
    recs = [rng.bytes(int(n)) for n in lens] + [b"\x06" * 135, b"\x80" * 135, b"", rng.bytes(70003)]
    want = b"".join(R.sha3(x) for x in recs)
    for lead in (0, 1, 3, 8):  # records at odd addresses
        blob, off = R.pack(recs, lead)
        assert dev.sha3_256_batch(blob, off).tobytes() == want, lead


def test_sha3_4096_random_records(dev):
    rng = np.random.default_rng(82)
    recs = [rng.bytes(int(n)) for n in rng.integers(1, 701, 4096)]
    blob, off = R.pack(recs, 5)
    assert dev.sha3_256_batch(blob, off).tobytes() == b"".join(R.sha3(x) for x in recs)


def test_sha3_device_buffers(dev):
    rng = np.random.default_rng(83)
    recs = [rng.bytes(int(n)) for n in list(R.SHA3_LENGTHS[:-1]) + list(rng.integers(0, 300, 500))]
    blob, off = R.pack(recs, 3)
    L, n = dev.lib(), len(recs)
    blob = np.concatenate([blob, np.zeros(8, np.uint8)])
    d_blob, d_off, d_out = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    for d, size in ((d_blob, blob.size), (d_off, off.nbytes), (d_out, 32 * n)):
        dev.check(L.pv_dev_alloc(ctypes.byref(d), size), "pv_dev_alloc")
    try:
        dev.check(L.pv_memcpy_h2d(d_blob, dev._ptr(blob), blob.size), "h2d")
        dev.check(L.pv_memcpy_h2d(d_off, dev._ptr(off), off.nbytes), "h2d")
        assert L.pv_sha3_256_batch_device(d_blob, d_off, n, ctypes.c_void_p(d_out.value + 4), None) == dev.PV_ERR_ARG
        assert L.pv_sha3_256_batch_device(d_blob, None, n, d_out, None) == dev.PV_ERR_ARG
        dev.check(L.pv_sha3_256_batch_device(d_blob, d_off, n, d_out, None), "pv_sha3_256_batch_device")
        dev.check(L.pv_sync(), "pv_sync")
        out = np.zeros(32 * n, np.uint8)
        dev.check(L.pv_memcpy_d2h(dev._ptr(out), d_out, out.size), "d2h")
        assert out.tobytes() == b"".join(R.sha3(x) for x in recs)
    finally:
        for d in (d_blob, d_off, d_out):
            L.pv_dev_free(d)


def test_golden_cases_on_the_device_path(dev, S):
    for case in CASES:
        for parts in (1, 3):
            kv = S.KeyValueStorageInMemory()
            st = S.PruningState(kv)
            for chunk in R.split(case["sets"], parts):
                st.set_batch(chunk)
            assert st.headHash.hex() == case["final"], (case["name"], parts)
            assert R.recorded(st.as_dict, case["as_dict"]) == case["as_dict"], (case["name"], parts)
            R.reachable(S, kv, st.headHash)
        assert S.PruningState.root_of(case["sets"]).hex() == case["final"], case["name"]


def test_4096_onto_4096_against_the_sequential_classes(dev, S):
    first, second = pairs(b"a", 4096, 60), pairs(b"b", 3800, 60) + pairs(b"a", 296, 61)  # 296 overwrites
    seq_kv = S.KeyValueStorageInMemory()
    seq = S.PruningState(seq_kv)
    for k, v in first + second:
        seq.set(k, v)
    kv = S.KeyValueStorageInMemory()
    st = S.PruningState(kv)
    st.set_batch(first)
    st.set_batch(second)
    how = dict(dev.trie_last)
    assert st.headHash == seq.headHash
    assert how["launches"] >= 2 and how["rounds"] >= 3, how
    assert st.as_dict == seq.as_dict
    R.reachable(S, kv, st.headHash)
    for k, v in kv._dict.items():
        assert seq_kv._dict[k] == v


def test_65536_device_path_equals_host_path(native, S):
    base, more = pairs(b"c", 65536), pairs(b"d", 65536)
    try:
        root_d, nodes_d, how = batch_nodes(native, S, native.PV_TRIE_DEVICE, S.BLANK_ROOT, None, base)
        root_h, nodes_h, _ = batch_nodes(native, S, native.PV_TRIE_HOST, S.BLANK_ROOT, None, base)
        assert how["launches"] >= 3 and how["tail_records"] > 0
        assert root_d == root_h and nodes_d == nodes_h
        assert root_d == S.PruningState.root_of(base)
        assert all(R.sha3(v) == k for k, v in list(nodes_d.items())[::97])
        kv = S.KeyValueStorageInMemory()
        for k, v in nodes_d.items():
            kv.put(k, v)
        root2_d, nodes2_d, how = batch_nodes(native, S, native.PV_TRIE_DEVICE, root_d, kv, more)
        root2_h, nodes2_h, _ = batch_nodes(native, S, native.PV_TRIE_HOST, root_d, kv, more)
        assert how["rounds"] >= 3 and how["launches"] >= 3
        assert root2_d == root2_h and nodes2_d == nodes2_h and root2_d != root_d
    finally:
        native.trie_path(native.PV_TRIE_AUTO)


def test_deep_batch_runs_level_launches_and_the_tail(dev, S):
    """ASCII keys under a 40-byte prefix that is itself split at four points: the dirty nodes span more
    than 12 depths, the digits below hold more nodes per depth than one workgroup takes at three depths
    (per-depth launches), and the thin top is the single-workgroup tail."""
    prefix = b"did:sov:ledger/state/namespace/000/attr/"
    assert len(prefix) == 40
    sets = [(prefix[:k], b"stop %d" % k) for k in (8, 16, 24, 32)]
    sets += [(prefix + b"%07d" % (i * 2503 % 10 ** 7), b'{"n":%d,"pad":"%s"}' % (i, b"x" * (i % 40))) for i in range(4000)]
    seq_kv = S.KeyValueStorageInMemory()
    seq = S.PruningState(seq_kv)
    for k, v in sets:
        seq.set(k, v)
    kv = S.KeyValueStorageInMemory()
    st = S.PruningState(kv)
    st.set_batch(sets[:3000])
    first = dict(dev.trie_last)
    st.set_batch(sets[3000:])
    assert st.headHash == seq.headHash and st.as_dict == seq.as_dict
    assert first["launches"] >= 3 and 0 < first["tail_records"] <= 256, first  # at least two depths launched on their own
    assert dev.trie_last["tail_records"] > 0
    # hashed nodes on the path of one deep key
    depth, ref, path = 0, st.headHash, S.bin_to_nibbles(sets[-1][0])
    while ref != b"":
        node = ref if isinstance(ref, list) else S.rlp_decode(kv.get(ref))
        depth += not isinstance(ref, list)
        if len(node) == 17:
            ref, path = (node[path[0]], path[1:]) if path else (b"", path)
        else:
            cur, term = S.hp_unpack(node[0])
            ref, path = (b"", path) if term else (node[1], path[len(cur):])
    assert depth >= 12, depth
    R.reachable(S, kv, st.headHash)
    for k, v in kv._dict.items():
        assert seq_kv._dict[k] == v
