"""State-proof verification on the GPU (device path forced): pv_proof_node_kernel's digests against hashlib and
its flags against the host-compiled canonical check, at every SHA3 padding edge and record alignment mixed inside
one wave; the golden corruptions; a 4,096-key trie with 1,037 queries (several workgroups, a partial last wave)
against the host path and the sequential classes; a deep trie whose proofs of 12 and more nodes sit next to
proofs of 2, with embedded children on the path; one proof with many queries, up to the limit of 1,024 records;
the device-buffer entry on caller buffers and a caller stream; serialized and wire-form input end to end."""
import ctypes
import hashlib
import subprocess
import sys

import numpy as np
import pytest

import proof_ref as P
import trie_ref as R

pytestmark = pytest.mark.gpu

GOLD = P.load_proof_golden()
U64 = ctypes.c_uint64


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


@pytest.fixture(scope="module")
def tries(S, native):
    native.trie_path(native.PV_TRIE_HOST)
    try:
        return P.build_tries(S)
    finally:
        native.trie_path(native.PV_TRIE_AUTO)


def on_host(N, f):
    N.trie_path(N.PV_TRIE_HOST)
    try:
        return f()
    finally:
        N.trie_path(N.PV_TRIE_DEVICE)


def canonical_string(n, rng):
    """Canonical RLP of exactly n bytes (n >= 1): a byte string or, at the totals no string has (57, 258), a list."""
    if n == 1:
        return b"\x05"
    for ones in (0, 1, 2):
        for head in (1, 2, 3, 4, 5, 6):
            body = rng.bytes(max(n - head - ones, 0))
            item = P.rlp_str(body if len(body) != 1 else b"\x90")
            enc = P.rlp_list([b"\x01"] * ones + [item]) if ones else item
            if len(enc) == n:
                return enc
    raise AssertionError(n)


def device_verify(N, blob, off, node_len, proof_first, query_proof, roots, keys, values, stream=None, hash_shift=0):
    """pv_trie_verify_proofs_device on buffers allocated here. Returns (rc, statuses, digests (n, 32))."""
    L = N.lib()
    kb, ko = N._blob(keys)
    vb, vo = N._blob(values)
    nn, nq = len(off) - 1, len(query_proof)
    host = {"blob": np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(8, np.uint8)]),
            "off": np.ascontiguousarray(off, np.uint64), "first": np.ascontiguousarray(proof_first, np.uint64),
            "qp": np.ascontiguousarray(query_proof, np.uint32), "root": np.frombuffer(b"".join(roots), np.uint8),
            "kb": kb, "ko": ko, "vb": vb, "vo": vo}
    if node_len is not None:
        host["len"] = np.ascontiguousarray(node_len, np.uint64)
    d = {}
    try:
        for name, a in list(host.items()) + [("status", np.zeros(nq, np.uint8)), ("hash", np.zeros(32 * nn + 8, np.uint8))]:
            d[name] = ctypes.c_void_p()
            N.check(L.pv_dev_alloc(ctypes.byref(d[name]), max(a.nbytes, 8)), "pv_dev_alloc")
            if name in host:
                N.check(L.pv_memcpy_h2d(d[name], N._ptr(a), a.nbytes), "h2d")
        arg = N.PvProofIn(d["blob"].value, d["off"].value, nn, d["first"].value, len(proof_first) - 1, d["qp"].value,
                          d["root"].value, d["kb"].value, d["ko"].value, d["vb"].value, d["vo"].value, nq,
                          d["len"].value if node_len is not None else None)
        rc = L.pv_trie_verify_proofs_device(ctypes.byref(arg), d["status"], ctypes.c_void_p(d["hash"].value + hash_shift), stream)
        status, digests = np.zeros(nq, np.uint8), np.zeros(32 * nn, np.uint8)
        if rc == 0:
            N.check(L.pv_stream_sync(stream) if stream else L.pv_sync(), "sync")
            N.check(L.pv_memcpy_d2h(N._ptr(status), d["status"], nq), "d2h")
            if nn:
                N.check(L.pv_memcpy_d2h(N._ptr(digests), d["hash"], 32 * nn), "d2h")
        return rc, status, digests.reshape(nn, 32)
    finally:
        for p in d.values():
            L.pv_dev_free(p)


def test_node_kernel_digests_and_flags_at_every_padding_edge(dev):
    C = P.proofcheck_lib()
    rng = np.random.default_rng(101)
    lens = [n for n in R.SHA3_LENGTHS[:-1] if n] * 2 + list(range(130, 141)) + list(range(268, 276))
    rng.shuffle(lens)
    recs = []
    for i, n in enumerate(lens):  # canonical and non-canonical interleaved inside the waves
        recs.append(canonical_string(int(n), rng) if i % 2 else rng.bytes(int(n)))
    recs += [b"", b"\x81\x05", b"\xc1\x80", b"\xc2\x80", P.rlp_list([P.rlp_list([P.rlp_list([P.rlp_list([P.rlp_list([b"x"])])])])]),
             P.rlp_list([P.rlp_list([P.rlp_list([P.rlp_list([b"x"])])])]), canonical_string(70003, rng), rng.bytes(70003)]
    want_flag = [0 if C.pkc_canonical(r, U64(len(r))) else 1 for r in recs]
    assert 20 < sum(want_flag) < len(recs) - 20
    want_hash = b"".join(R.sha3(r) for r in recs)
    n = len(recs)
    for lead in (0, 1, 3, 8):
        blob, off = R.pack(recs, lead)
        for node_len in (None, np.diff(off)):
            # one proof per record, asked for a root nothing hashes to: REJECT where the record is canonical, DEFER where flagged
            rc, status, digests = device_verify(dev, blob, off, node_len, np.arange(n + 1), np.arange(n), [bytes(32)] * n,
                                                [b"k"] * n, [b""] * n)
            assert rc == 0 and digests.tobytes() == want_hash, lead
            assert [int(s == dev.PV_PROOF_DEFER) for s in status] == want_flag, lead
            assert set(status) == {dev.PV_PROOF_REJECT, dev.PV_PROOF_DEFER}


def test_golden_entries_on_the_device_path(dev, S, tries):
    cases = P.all_corruptions(tries, skip=("serialized_empty",))
    want = [GOLD[name]["corruptions"][c] == "true" for name, c, _ in cases]
    assert S.PruningState.verify_state_proof_batch([a for _, _, a in cases], serialized=True) == want
    assert dev.proof_last["launches"] == 2 and dev.proof_last["queries"] > 100
    native_cases = [x for x in P.all_corruptions(tries, skip=P.ROOT_LENGTH_CLASSES + P.UNSPLITTABLE) if x[0] != "blank"]
    status = P.native_statuses(dev, S, [a for _, _, a in native_cases])
    assert list(status) == list(on_host(dev, lambda: P.native_statuses(dev, S, [a for _, _, a in native_cases])))
    for (name, c, _), s in zip(native_cases, status):
        if c in P.CANONICAL_CLASSES:
            assert s == int(GOLD[name]["corruptions"][c] == "true"), (name, c)
        elif c in P.DEFER_CLASSES:
            assert s == dev.PV_PROOF_DEFER, (name, c)
    for name in P.TRIES:
        for c, a in tries[name][3].items():
            assert P.outcome(lambda: S.PruningState.verify_state_proof_multi(a[0], a[1], a[2], serialized=True)) == GOLD[name]["multi"][c]
            assert dev.proof_last["launches"] == 2 and dev.proof_last["deferred"] == 0


def pairs(tag, n, vlen):
    return [(hashlib.sha256(b"%s%d" % (tag, i)).digest(), R.det("%s%d" % (tag.decode(), i), vlen)) for i in range(n)]


def test_4096_key_trie_1037_queries(dev, S, tries):
    sets = pairs(b"p", 4096, 60)
    st = S.PruningState(S.KeyValueStorageInMemory())
    st.set_batch(sets)
    root = st.headHash
    absent = [hashlib.sha256(b"absent%d" % i).digest() for i in range(500)]
    keys = [k for pair in zip([k for k, _ in sets[:500]], absent) for k in pair]  # present and absent interleaved
    values = dict(sets)
    proofs = st.generate_state_proof_batch(keys, serialize=True)
    items = [(root, k, values.get(k), p) for k, p in zip(keys, proofs)]
    sib = S.PruningState(S.KeyValueStorageInMemory())
    sib.set_batch(sets[:-1] + [(sets[-1][0], b"other")])
    base = P.base_of(st, sib, S.rlp_encode, sets)
    classes = {c: a for c, a in P.corruptions(base).items() if c != "serialized_empty"}
    corrupt = list(classes.items())
    for i, (c, a) in enumerate(corrupt):  # one query per corruption class, spread over the batch
        items.insert(37 * i + 5, a)
    items += [(root, k, b"wrong", p) for k, p in zip(keys[:1037 - len(items)], proofs)]
    assert len(items) == 1037
    seq = [S.PruningState.verify_state_proof(*it, serialized=True) for it in items]
    assert 900 < sum(seq) < 1037 - 20
    assert S.PruningState.verify_state_proof_batch(items, serialized=True) == seq
    assert dev.proof_last["launches"] == 2 and dev.proof_last["queries"] > 1024 and dev.proof_last["nodes"] > 3000
    # the statuses themselves: equal to the host path's, and no DEFER among the canonical ones
    lib_items = [it for it in items if isinstance(it[0], bytes) and len(it[0]) == 32 and it[3] not in (b"\xc1", classes["serialized_truncated"][3])]
    status = P.native_statuses(dev, S, lib_items)
    assert list(status) == list(on_host(dev, lambda: P.native_statuses(dev, S, lib_items)))
    deferred = {c for c, a in corrupt if a in lib_items and status[lib_items.index(a)] == dev.PV_PROOF_DEFER}
    assert set(P.DEFER_CLASSES) <= deferred and not deferred & set(P.CANONICAL_CLASSES)
    assert (status == dev.PV_PROOF_DEFER).sum() == len(deferred)
    for it, s in zip(lib_items, status):
        if s != dev.PV_PROOF_DEFER:
            assert s == int(seq[items.index(it)])


@pytest.fixture(scope="module")
def deep(S, native):
    """The 40-byte-prefix key set of test_gpu_trie.py's deep test, plus keys that extend stored keys by two bytes
    with one-byte values: their leaves are embedded in a branch that is itself reached through the deep path."""
    prefix = b"did:sov:ledger/state/namespace/000/attr/"
    sets = [(prefix[:k], b"stop %d" % k) for k in (8, 16, 24, 32)]
    sets += [(prefix + b"%07d" % (i * 2503 % 10 ** 7), b'{"n":%d,"pad":"%s"}' % (i, b"x" * (i % 40))) for i in range(4000)]
    sets += [(sets[4 + 97 * i][0] + b"/a", b"%d" % (i % 10)) for i in range(16)]
    st = S.PruningState(S.KeyValueStorageInMemory())
    native.trie_path(native.PV_TRIE_DEVICE)
    try:
        st.set_batch(sets)
    finally:
        native.trie_path(native.PV_TRIE_AUTO)
    return st, sets, prefix


def test_deep_trie_long_and_short_proofs_and_embedded_children(dev, S, deep):
    st, sets, prefix = deep
    root, values = st.headHash, dict(sets)
    keys = []
    for i in range(0, 4020, 67):  # deep keys next to keys answered at the top
        keys += [sets[i][0], b"zz%d" % i, prefix[:8], prefix + b"%07d" % (i + 1), sets[-1 - i % 16][0]]
    proofs = st.generate_state_proof_batch(keys)
    sizes = [len(p) for p in proofs]
    assert max(sizes) >= 12 and min(sizes) <= 2, (max(sizes), min(sizes))
    # an embedded child on the path of the extended keys: the leaf is not among the proof nodes
    embedded = 0
    for k, p in zip(keys, proofs):
        if values.get(k) is not None and len(values[k]) == 1:
            raw = S.rlp_encode([values[k]])
            assert not any(len(n) == 2 and n[1] == raw for n in p) and any(isinstance(c, list) for n in p for c in n)
            embedded += 1
    assert embedded >= 10
    items = [(root, k, values.get(k), p) for k, p in zip(keys, proofs)]
    items += [(root, k, b"x", p) for k, p in zip(keys[::3], proofs[::3])]
    seq = [S.PruningState.verify_state_proof(*it) for it in items]
    assert S.PruningState.verify_state_proof_batch(items) == seq and sum(seq) == len(keys)
    assert dev.proof_last["launches"] == 2 and dev.proof_last["deferred"] == 0
    ser = [(r, k, v, S.Trie.serialize_proof(p)) for r, k, v, p in items]
    status = P.native_statuses(dev, S, ser)
    assert list(status) == [int(x) for x in seq] == list(on_host(dev, lambda: P.native_statuses(dev, S, ser)))


def test_one_proof_many_queries_up_to_1024_records(dev, S, deep):
    st, sets, prefix = deep
    root, values = st.headHash, dict(sets)
    pre = prefix + b"0"
    proof, found = st.generate_state_proof_for_keys_with_prefix(pre, get_value=True)
    assert 200 < len(proof) < 1000 and len(found) > 300 and all(k.startswith(pre) for k in found)
    kv = {k: S.PruningState.get_decoded(v) for k, v in found.items()}
    assert kv == {k: v for k, v in values.items() if k.startswith(pre)}
    assert S.PruningState.verify_state_proof_multi(root, kv, proof)
    assert dev.proof_last == {"nodes": len(proof), "queries": len(kv), "deferred": 0, "launches": 2}
    wrong = dict(kv)
    wrong[sorted(kv)[len(kv) // 2]] = b"forged"
    assert not S.PruningState.verify_state_proof_multi(root, wrong, proof)
    assert S.PruningState.verify_state_proof_multi(root, dict(kv, **{"zz-absent": None}), S.Trie.serialize_proof(proof), serialized=True)
    # a pool of exactly 1,024 records: the proof's own, then canonical leaves nothing refers to, the root record last
    recs = [S.rlp_encode(n) for n in proof]
    pool = recs[:-1] + [S.rlp_encode([S.hp_pack([i % 16, i // 16 % 16, 3], True), b"filler %d" % i]) for i in range(dev.PV_PROOF_MAX_NODES - len(recs))]
    pool.append(recs[-1])
    assert len(pool) == dev.PV_PROOF_MAX_NODES
    keys = sorted(kv) + [b"zz-absent"]
    vals = [P.stored(S, kv.get(k)) for k in keys]
    vals[7] = P.stored(S, b"forged")
    blob, off = R.pack(pool, 1)
    kb, ko = dev._blob(keys)
    vb, vo = dev._blob(vals)
    status = dev.trie_verify_proofs_raw(blob, off, None, [0, len(pool)], np.zeros(len(keys), np.uint32),
                                        np.frombuffer(root * len(keys), np.uint8), kb, ko, vb, vo)
    want = [dev.PV_PROOF_ACCEPT] * len(keys)
    want[7] = dev.PV_PROOF_REJECT
    assert list(status) == want and dev.proof_last["nodes"] == 1024 and dev.proof_last["launches"] == 2


def test_device_buffer_entry_on_a_caller_stream(dev, S, tries):
    L = dev.lib()
    st, sets = tries["ascii_300"][:2]
    values = P.final_map(sets)
    keys = sorted(values)[::3] + [b"zz-absent"]
    proofs = [P.split_list(st.generate_state_proof(k, serialize=True)) for k in keys]
    recs = [r for p in proofs for r in p]
    first = np.concatenate([[0], np.cumsum([len(p) for p in proofs])])
    vals = [P.stored(S, values.get(k)) for k in keys]
    vals[1] = P.stored(S, b"forged")
    want = [dev.PV_PROOF_ACCEPT] * len(keys)
    want[1] = dev.PV_PROOF_REJECT
    blob, off = R.pack(recs, 5)
    roots = [st.headHash] * len(keys)
    stream = ctypes.c_void_p()
    dev.check(L.pv_stream_create(ctypes.byref(stream)), "pv_stream_create")
    try:
        for s in (stream, None, stream):  # the flags' workspace is handed from one stream to the other and back
            rc, status, digests = device_verify(dev, blob, off, None, first, np.arange(len(keys)), roots, keys, vals, stream=s)
            assert rc == 0 and list(status) == want
            assert digests.tobytes() == b"".join(R.sha3(r) for r in recs)
        assert device_verify(dev, blob, off, None, first, np.arange(len(keys)), roots, keys, vals, hash_shift=4)[0] == dev.PV_ERR_ARG
        assert b"8-byte aligned" in L.pv_last_error()
        # indices the host cannot see are checked on the device: such a query is deferred, nothing is read for it
        qp = np.arange(len(keys))
        qp[3] = len(keys) + 100
        rc, status, _ = device_verify(dev, blob, off, None, first, qp, roots, keys, vals, stream=stream)
        want[3] = dev.PV_PROOF_DEFER
        assert rc == 0 and list(status) == want
    finally:
        L.pv_stream_destroy(stream)
    z = np.zeros(8, np.uint64)
    arg = dev.PvProofIn(z.ctypes.data, z.ctypes.data, 1, z.ctypes.data, 1, None, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                        z.ctypes.data, z.ctypes.data, 1, None)
    assert L.pv_trie_verify_proofs_device(ctypes.byref(arg), z.ctypes.data, z.ctypes.data, None) == dev.PV_ERR_ARG  # null query_proof
    assert L.pv_trie_verify_proofs_device(None, z.ctypes.data, z.ctypes.data, None) == dev.PV_ERR_ARG


def test_device_entry_before_pv_init():
    """A fresh process that never calls pv_init: PV_ERR_NOT_INIT, nothing launched."""
    import os
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "indy-plenum_amd")
    code = ("import sys, ctypes, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "from plenum_amd import _native as N\n"
            "z = np.zeros(8, np.uint64)\n"
            "p = z.ctypes.data\n"
            "arg = N.PvProofIn(p, p, 1, p, 1, p, p, p, p, p, p, 1, None)\n"
            "assert N.lib().pv_trie_verify_proofs_device(ctypes.byref(arg), p, p, None) == N.PV_ERR_NOT_INIT\n" % pkg)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_serialized_and_wire_form_end_to_end(dev, S, deep):
    from plenum_amd.serialization import proof_nodes_serializer, state_roots_serializer
    st, sets, prefix = deep
    chosen = sets[::9]
    proofs = st.generate_state_proof_batch([k for k, _ in chosen], serialize=True, get_value=True)
    replies = []
    for (k, v), (ser, raw) in zip(chosen, proofs):
        assert raw == S.rlp_encode([v])
        replies.append((state_roots_serializer.serialize(st.headHash), k, v, proof_nodes_serializer.serialize(ser)))
    items = [(state_roots_serializer.deserialize(r), k, v, proof_nodes_serializer.deserialize(p)) for r, k, v, p in replies]
    items[2] = items[2][:2] + (b"forged",) + items[2][3:]
    items[5] = items[5][:3] + (items[5][3][:-1],)  # truncated by a byte: the split refuses it, Python decides
    want = [True] * len(items)
    want[2] = want[5] = False
    assert len(items) > 400 and S.PruningState.verify_state_proof_batch(items, serialized=True) == want
    assert dev.proof_last["launches"] == 2 and dev.proof_last["queries"] == len(items) - 1 and dev.proof_last["deferred"] == 0
