"""The device trie builder on the GPU (pv_trie_root under a forced device path, and pv_trie_root_device): the
golden roots recorded from the reference, and byte-equal roots against the library's host structural path at the
smallest shapes at which a pass can go wrong: sizes around a wave and a workgroup, key lengths that are no
multiple of the sort's 8-byte word, every RLP length-prefix edge of a value, overwrites, the embedded shapes, one
long extension, a comb deeper than 64 nodes, sorted and reverse-sorted input, one key a thousand times. The same
source runs on the CPU under sanitizers in tests/test_trie_build_host.py.

The comb of 64 keys holds 189 records, fewer than the 256 the single-workgroup tail takes, so that call is one
tail launch; the per-depth launches beside the tail are asserted on the same comb with four more leaves under
every tooth (320 leaves, more than one tail)."""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

import trie_ref as R

pytestmark = pytest.mark.gpu

VALUE_LENGTHS = (1, 2, 30, 31, 32, 33, 54, 55, 56, 150, 255, 256)
GOLDEN = [c for c in R.load_golden() if len({len(k) for k, _ in c["sets"]}) == 1 and 1 <= len(c["sets"][0][0]) <= 64]


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


def arrays(keys, vals):
    kl = len(keys[0])
    off = np.zeros(len(vals) + 1, np.uint64)
    np.cumsum([len(v) for v in vals], out=off[1:])
    blob = np.frombuffer(b"".join(vals) or b"\0", np.uint8)
    return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), kl), blob, off


def both(native, keys, vals, wrap):
    """(device root, how it ran, host root, how it ran) of one set of pairs."""
    k, blob, off = arrays(keys, vals)
    try:
        native.trie_path(native.PV_TRIE_DEVICE)
        d = native.trie_root(k, blob, off, wrap)
        how_d = dict(native.trie_last)
        native.trie_path(native.PV_TRIE_HOST)
        h = native.trie_root(k, blob, off, wrap)
        how_h = dict(native.trie_last)
    finally:
        native.trie_path(native.PV_TRIE_AUTO)
    assert how_d["built_on_device"] and not how_h["built_on_device"]
    return d, how_d, h, how_h


def same(native, keys, vals, wrap):
    d, how_d, h, how_h = both(native, keys, vals, wrap)
    assert d == h, (len(keys), len(keys[0]), wrap)
    assert how_d["nodes"] == how_h["nodes"] and how_d["arena_bytes"] == how_h["arena_bytes"]
    assert how_d["n_keys"] == len(set(keys))
    return how_d


def test_golden_cases_through_the_builder(dev, S):
    assert len(GOLDEN) >= 20
    for c in GOLDEN:
        k, blob, off = arrays([k for k, _ in c["sets"]], [v for _, v in c["sets"]])
        assert dev.trie_root(k, blob, off, True).hex() == c["final"], c["name"]
        assert dev.trie_last["built_on_device"]
        assert S.PruningState.root_of(c["sets"]).hex() == c["final"], c["name"]
        assert dev.trie_last["built_on_device"]


@pytest.mark.parametrize("key_len", [1, 2, 3, 8, 9, 32, 64])
def test_sizes_and_key_lengths_against_the_host_path(native, key_len):
    rng = np.random.default_rng(100 + key_len)
    for n in (1, 2, 3, 63, 64, 65, 257, 4096):
        for wrap in (False, True):
            keys = [rng.bytes(key_len) for _ in range(n)]
            for i in range(1, n):
                if rng.random() < 0.05:
                    keys[i] = keys[int(rng.integers(0, i))]
            choice = list(VALUE_LENGTHS) + ([0] if wrap else [])
            vals = [rng.bytes(int(rng.choice(choice))) for _ in range(n)]
            vals = [bytes([v[0] & 0x7F]) if len(v) == 1 and i % 2 else v for i, v in enumerate(vals)]
            if n == 257 and key_len == 9:
                vals[100] = rng.bytes(70000)  # one lane writes a long value
            same(native, keys, vals, wrap)


def test_two_full_levels_and_overwrites(native):
    rng = np.random.default_rng(7)
    keys = [bytes([b]) for b in range(256)] + [bytes([int(b)]) for b in rng.integers(0, 256, 100)]
    how = same(native, keys, [rng.bytes(3) for _ in keys], False)
    assert how["n_keys"] == 256 and how["n_nodes"] == 256 + 17


def test_dense_two_byte_keys_embed_leaves_and_branches(native):
    rng = np.random.default_rng(8)
    dense = sorted(set(int(x) for x in rng.integers(0, 65536, 6000)))[:5000]
    how = same(native, [struct.pack(">H", x) for x in dense], [bytes([x & 0x7F]) for x in dense], False)
    assert how["n_nodes"] > 2 * how["nodes"]  # most nodes are embedded


def test_embedded_shapes_of_the_sizing_argument(native):
    how = same(native, [b"\x10\x00", b"\x10\x01", b"\x20\x00"], [b"", b"", b"v" * 40], True)
    assert (how["n_nodes"], how["nodes"]) == (6, 2)  # a branch embedded in an extension
    how = same(native, [bytes([a | b]) for a in range(0, 256, 16) for b in (0, 1)], [b""] * 32, True)
    assert (how["n_nodes"], how["nodes"]) == (49, 1)  # 16 embedded branches
    same(native, [bytes([7, b]) for b in range(6)] + [b"\x90\x00"], [b"\x05"] * 6 + [b"w" * 50], False)
    same(native, [bytes([7, b]) for b in range(7)] + [b"\x90\x00"], [b"\x05"] * 7 + [b"w" * 50], False)


def test_keys_that_differ_in_one_nibble_and_one_long_extension(native):
    same(native, [b"\xab" * 7 + bytes([0xC0 | x]) for x in range(16)], [b"x" * 33] * 16, True)
    same(native, [bytes([(x << 4) | 5]) + b"\xcd" * 7 for x in range(16)], [b"x" * 33] * 16, True)
    how = same(native, [b"\x55" * 63 + bytes([x]) for x in (1, 2, 0x31, 0xF0)], [b"y" * 40] * 4, True)
    assert how["max_depth"] == 3  # extension, branch, branch, leaf


def comb_keys(rng):
    comb, cur = [], bytearray(rng.bytes(64))
    for i in range(64):  # key i shares exactly i bytes with key i + 1
        comb.append(bytes(cur))
        cur[i] ^= 0x80
    return comb


def test_comb_deeper_than_64_nodes(native):
    rng = np.random.default_rng(9)
    comb = comb_keys(rng)
    how = same(native, comb, [rng.bytes(150) for _ in comb], True)
    assert how["max_depth"] > 64, how
    assert how["launches"] == 1 and how["tail_records"] == how["nodes"] == 189, how
    # four more leaves under every tooth: more records than one tail takes
    wide = [k[:63] + bytes([k[63] ^ x]) for k in comb for x in (0, 1, 2, 3, 4)]
    how = same(native, wide, [rng.bytes(150) for _ in wide], True)
    assert how["max_depth"] > 64 and how["launches"] > 1 and 0 < how["tail_records"] <= 256, how


def test_sorted_reverse_sorted_and_one_key_a_thousand_times(native):
    rng = np.random.default_rng(10)
    srt = sorted(rng.bytes(8) for _ in range(300))
    vals = [rng.bytes(40) for _ in srt]
    a = same(native, srt, vals, True)
    b = same(native, srt[::-1], vals[::-1], True)
    assert a["nodes"] == b["nodes"]
    how = same(native, [b"samekey!"] * 1000, [b"%d" % i for i in range(1000)], True)
    assert how["n_keys"] == 1 and how["n_nodes"] == 1
    k, blob, off = arrays([b"samekey!"], [b"999"])
    assert native.trie_root(k, blob, off, True) == both(native, [b"samekey!"] * 1000, [b"%d" % i for i in range(1000)], True)[0]


def test_65536_pairs_equal_the_host_path_and_root_of(native, S):
    items = [(hashlib.sha256(b"e%d" % i).digest(), R.det("e%d" % i, 150)) for i in range(65536)]
    keys, vals = [k for k, _ in items], [v for _, v in items]
    d, how_d, h, how_h = both(native, keys, vals, True)
    assert d == h
    assert how_d["n_nodes"] == how_d["nodes"] == how_h["nodes"]  # 150-byte values: nothing is embedded
    assert how_d["launches"] >= 3 and how_d["tail_records"] > 0
    try:
        native.trie_path(native.PV_TRIE_DEVICE)
        assert S.PruningState.root_of(items) == d
        assert native.trie_last["built_on_device"]
        k, blob, off = arrays(keys, vals)
        assert S.PruningState.root_of_arrays(k, blob, off) == d
        assert native.trie_update(S.BLANK_ROOT, None, keys, [S.rlp_encode([v]) for v in vals])[0] == d
    finally:
        native.trie_path(native.PV_TRIE_AUTO)


def test_root_of_arrays_equals_root_of(dev, S):
    rng = np.random.default_rng(11)
    items = [(rng.bytes(20), rng.bytes(int(n))) for n in rng.integers(0, 300, 500)]
    k, blob, off = arrays([k for k, _ in items], [v for _, v in items])
    assert S.PruningState.root_of_arrays(k, blob, off) == S.PruningState.root_of(items)
    assert S.PruningState.root_of([]) == S.BLANK_ROOT
    assert dev.trie_root(np.zeros((0, 4), np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint64), True) == S.BLANK_ROOT


def test_mixed_lengths_go_where_they_went(dev, S):
    items = [(b"ab", b"1"), (b"abc", b"2"), (b"b", b"3")]
    seq = S.PruningState(S.KeyValueStorageInMemory())
    for k, v in items:
        seq.set(k, v)
    assert S.PruningState.root_of(items) == seq.headHash
    assert dev.trie_last["built_on_device"] is False


def test_device_buffers(dev):
    rng = np.random.default_rng(12)
    keys = [rng.bytes(32) for _ in range(1000)]
    vals = [rng.bytes(int(n)) for n in rng.integers(1, 200, 1000)]
    k, blob, off = arrays(keys, vals)
    want = dev.trie_root(k, blob, off, True)
    bad_off = off.copy()
    bad_off[501] = bad_off[500]  # an empty value, refused without the wrapping
    L, n = dev.lib(), len(keys)
    d_keys, d_blob, d_off, d_bad, d_root = (ctypes.c_void_p() for _ in range(5))
    for d, size in ((d_keys, k.size), (d_blob, blob.size), (d_off, off.nbytes), (d_bad, off.nbytes), (d_root, 32)):
        dev.check(L.pv_dev_alloc(ctypes.byref(d), size), "pv_dev_alloc")
    try:
        for d, a in ((d_keys, k), (d_blob, blob), (d_off, off), (d_bad, bad_off)):
            dev.check(L.pv_memcpy_h2d(d, dev._ptr(a), a.nbytes), "h2d")
        out = dev.PvTrieRootOut()

        def call(keys_=d_keys, key_len=32, blob_=d_blob, off_=d_off, flags=1, root_=d_root, out_=ctypes.byref(out)):
            return L.pv_trie_root_device(keys_, key_len, n, blob_, off_, flags, root_, out_, None)

        def root():
            dev.check(L.pv_sync(), "pv_sync")
            got = np.zeros(32, np.uint8)
            dev.check(L.pv_memcpy_d2h(dev._ptr(got), d_root, 32), "d2h")
            return got.tobytes()

        assert call(key_len=0) == dev.PV_ERR_ARG and call(key_len=65) == dev.PV_ERR_ARG
        for null in ("keys_", "blob_", "off_", "root_", "out_"):
            assert call(**{null: None}) == dev.PV_ERR_ARG, null
        dev.check(call(), "pv_trie_root_device")
        assert root() == want and out.built_on_device == 1 and out.n_keys == len(set(keys))
        # the device error word: a clean status, and the workspace serves the next call
        assert call(off_=d_bad, flags=0) == dev.PV_ERR_ARG
        assert b"value" in L.pv_last_error()
        dev.check(call(off_=d_bad), "pv_trie_root_device")  # with the wrapping an empty value is a value
        assert root() != want
        dev.check(call(), "pv_trie_root_device")
        assert root() == want
    finally:
        for d in (d_keys, d_blob, d_off, d_bad, d_root):
            L.pv_dev_free(d)
