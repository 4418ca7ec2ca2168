"""State proofs without a GPU: the sequential classes of plenum_amd.state_trie against goldens recorded from the
reference (tests/golden/state_proof.json: proofs for keys and prefixes, the verdict for every corruption class);
the batch calls through the library's host path against the sequential ones; the library's statuses asserted
directly, so that the fallback for deferred queries cannot hide a broken walk; pv_trie_proof_split against a
Python split; the ABI's argument checks; the shared canonical check and walk (csrc/trie_core.h) compiled for the
HOST (tests/native/proofcheck.hip) against the Python walk on random mutations; and the new host code once more
as a stand-alone program under AddressSanitizer and UBSan. Same source as the GPU kernels;
tests/test_gpu_state_proof.py closes the gap."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import proof_ref as P
import trie_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
HOST_CHECK = os.path.join(HERE, "native", "proof_host_check")
GOLD = P.load_proof_golden()
U64 = ctypes.c_uint64
ROOT_LENGTH_CLASSES, UNSPLITTABLE = P.ROOT_LENGTH_CLASSES, P.UNSPLITTABLE
all_corruptions, stored, native_statuses = P.all_corruptions, P.stored, P.native_statuses


proofcheck_lib = P.proofcheck_lib


@pytest.fixture(scope="module")
def S():
    from plenum_amd import state_trie
    return state_trie


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    return _native


@pytest.fixture()
def host_path(native):
    native.trie_path(native.PV_TRIE_HOST)
    yield native
    native.trie_path(native.PV_TRIE_AUTO)


@pytest.fixture(scope="module")
def tries(S):
    """name -> (state, sets, corruptions of the first key's proof, multi cases). Built once, left unchanged."""
    return P.build_tries(S)


# ---------------------------------------------------------------------- generation vs the golden
@pytest.mark.parametrize("name", P.TRIES)
def test_generated_proofs_match_the_reference(S, tries, name):
    st, sets = tries[name][:2]
    gold = GOLD[name]
    assert st.headHash.hex() == gold["root"]
    present, absent = P.query_keys(sets)
    assert [k.hex() for k in present + absent] == [e["key"] for e in gold["keys"]]
    for e in gold["keys"]:
        key = bytes.fromhex(e["key"])
        nodes, rn, ser_len, value = P.proof_of(st, S.rlp_encode, key)
        assert (P.forms(nodes), R.form(rn), ser_len) == (e["nodes"], e["root_node"], e["ser_len"]), e["key"]
        assert (R.form(value) if value is not None else None) == e["value"]
        proof = st.generate_state_proof(key)
        assert proof[-1] == st.head and len({S.rlp_encode(n) for n in proof[:-1]}) == len(proof) - 1  # root last, no duplicates
        assert S.Trie.deserialize_proof(st.generate_state_proof(key, serialize=True)) == proof
        assert st.generate_state_proof(key, root=st.head) == proof
    assert [p.hex() for p in P.prefixes(sets)] == [e["prefix"] for e in gold["prefixes"]]
    for e in gold["prefixes"]:
        nodes, rn, ser_len, values = P.proof_of(st, S.rlp_encode, bytes.fromhex(e["prefix"]), prefix=True)
        assert (P.forms(nodes), R.form(rn), ser_len) == (e["nodes"], e["root_node"], e["ser_len"]), e["prefix"]
        assert P.value_forms(values) == e["values"], e["prefix"]


def test_blank_proof_is_c1_80(S):
    st = S.PruningState(S.KeyValueStorageInMemory())
    assert st.generate_state_proof(b"k", serialize=True, get_value=True) == (b"\xc1\x80", None)
    assert st.generate_state_proof(b"k") == [b""]
    assert S.PruningState.verify_state_proof(S.BLANK_ROOT, b"k", None, [b""])


def test_proof_of_an_earlier_root_and_all_leaves(S, tries):
    sets = P.trie_sets("ascii_300")
    st = S.PruningState(S.KeyValueStorageInMemory())
    st.set_batch(sets[:150])
    old = st.headHash
    st.set_batch(sets[150:])
    k, v = sets[3]
    proof, raw = st.generate_state_proof(k, root=st.get_head_by_hash(old), get_value=True)
    assert raw == S.rlp_encode([v]) and S.PruningState.verify_state_proof(old, k, v, proof)
    assert not S.PruningState.verify_state_proof(st.headHash, k, v, proof)
    leaves = st.get_all_leaves_for_root_hash(old)
    assert {key: S.PruningState.get_decoded(x) for key, x in leaves.items()} == P.final_map(sets[:150])


def test_generate_state_proof_batch_equals_the_per_key_calls(S, tries):
    st, sets = tries["ascii_300"][:2]
    keys = [k for k, _ in sets[::7]] + [b"zz-absent", b""]
    for kw in ({}, {"serialize": True}, {"get_value": True}, {"serialize": True, "get_value": True}):
        assert st.generate_state_proof_batch(keys, **kw) == [st.generate_state_proof(k, **kw) for k in keys]
    old = st.get_head_by_hash(st.headHash)
    assert st.generate_state_proof_batch(keys[:5], root=old) == [st.generate_state_proof(k, root=old) for k in keys[:5]]


# -------------------------------------------------------------------- verification vs the golden
@pytest.mark.parametrize("name", P.TRIES)
def test_sequential_verification_matches_the_reference(S, tries, name, capsys):
    st, sets, cases, multi = tries[name]
    gold = GOLD[name]
    got = {c: P.outcome(lambda a=a: S.PruningState.verify_state_proof(a[0], a[1], a[2], a[3], serialized=True))
           for c, a in cases.items()}
    assert got == gold["corruptions"]
    got = {c: P.outcome(lambda a=a: S.Trie.verify_spv_proof_multi(
        a[0], dict(S.PruningState.encode_kv_for_verification(k, v) for k, v in a[1].items()), a[2], serialized=True))
        for c, a in multi.items()}
    assert got == gold["multi"]
    assert capsys.readouterr().out == ""  # the caught exception is not printed
    # the unserialized forms: the honest proof as a list of nodes
    root, key, value, ser = cases["honest"]
    assert S.PruningState.verify_state_proof(root, key, value, S.Trie.deserialize_proof(ser))
    assert not S.PruningState.verify_state_proof(root, key, (value or b"") + b"x", S.Trie.deserialize_proof(ser))


@pytest.mark.parametrize("name", P.TRIES)
def test_verify_state_proof_multi_through_the_library(S, host_path, tries, name):
    for c, a in tries[name][3].items():
        assert P.outcome(lambda: S.PruningState.verify_state_proof_multi(a[0], a[1], a[2], serialized=True)) == GOLD[name]["multi"][c]
        assert host_path.proof_last["queries"] == len(a[1]) and host_path.proof_last["deferred"] == 0
        nodes = S.Trie.deserialize_proof(a[2])
        assert P.outcome(lambda: S.PruningState.verify_state_proof_multi(a[0], a[1], nodes)) == GOLD[name]["multi"][c]


def test_batch_verification_on_the_host_path_equals_sequential(S, host_path, tries):
    cases = all_corruptions(tries, skip=("serialized_empty",))
    items = [a for _, _, a in cases]
    want = [GOLD[name]["corruptions"][c] == "true" for name, c, _ in cases]
    assert S.PruningState.verify_state_proof_batch(items, serialized=True) == want
    assert host_path.proof_last["queries"] > 100  # the library did take them
    # as lists of nodes (whatever the lenient decoder makes of each proof)
    lists = [(r, k, v, S.Trie.deserialize_proof(ser)) for r, k, v, ser in items]
    seq = [S.PruningState.verify_state_proof(*it) for it in lists]
    assert S.PruningState.verify_state_proof_batch(lists) == seq
    assert S.Trie.verify_spv_proof_batch([(r, k, stored(S, v), p) for r, k, v, p in lists]) == seq
    assert S.PruningState.verify_state_proof_batch([]) == []
    # what raises sequentially raises from the batch
    with pytest.raises(IndexError):
        S.PruningState.verify_state_proof_batch(items[:3] + [tries["single"][2]["serialized_empty"]], serialized=True)


def test_items_outside_the_limits_are_settled_in_python(S, host_path, tries):
    st, sets, cases, _ = tries["single"]
    root, key, value, ser = cases["honest"]
    nodes = S.Trie.deserialize_proof(ser)
    many = [[S.hp_pack([1], True), b"%d" % i] for i in range(host_path.PV_PROOF_MAX_NODES)] + nodes  # above 1,024 nodes
    host_path.proof_last.update(queries=-1)
    assert S.PruningState.verify_state_proof_batch([(root, key, value, many), (root, "k" * 65536, None, nodes),
                                                    (S.BLANK_ROOT, key, None, [b""]), (root[:31], key, value, nodes)]) \
        == [True, True, True, False]
    assert host_path.proof_last["queries"] == -1  # none of them reached the library
    assert S.PruningState.verify_state_proof_batch([(root, key, value, many[1:])]) == [True]  # 1,024: the library's
    assert host_path.proof_last["queries"] == 1 and host_path.proof_last["nodes"] == host_path.PV_PROOF_MAX_NODES


# ------------------------------------------------------------------- the library's own statuses
def test_native_statuses_without_the_fallback(S, host_path, tries):
    """Honest proofs and every corruption made of canonical, well-formed nodes: ACCEPT or REJECT as the
    reference says, never DEFER. Non-canonical and malformed nodes on the path: DEFER, never a verdict."""
    N = host_path
    cases = [x for x in all_corruptions(tries, skip=ROOT_LENGTH_CLASSES + UNSPLITTABLE) if x[0] != "blank"]  # Python's
    status = native_statuses(N, S, [a for _, _, a in cases])
    for (name, c, _), s in zip(cases, status):
        verdict = GOLD[name]["corruptions"][c] == "true"
        if c in P.CANONICAL_CLASSES:
            assert s == (N.PV_PROOF_ACCEPT if verdict else N.PV_PROOF_REJECT), (name, c)
        elif c in P.DEFER_CLASSES:
            assert s == N.PV_PROOF_DEFER, (name, c)
        else:  # a flipped byte may or may not leave canonical RLP
            assert s == N.PV_PROOF_DEFER or s == int(verdict), (name, c)
    assert sum(c in P.DEFER_CLASSES for _, c, _ in cases) >= 12
    # every present and absent key of every trie, honest: no DEFER at all
    honest = []
    for name in P.TRIES:
        st, sets = tries[name][:2]
        if st.headHash == S.BLANK_ROOT:
            continue
        for k in sum(P.query_keys(sets), []):
            honest.append((st.headHash, k, P.final_map(sets).get(k), st.generate_state_proof(k, serialize=True)))
    assert (native_statuses(N, S, honest) == N.PV_PROOF_ACCEPT).all() and len(honest) > 40


def test_a_malformed_node_the_walk_never_visits_does_not_defer(S, host_path, tries):
    N = host_path
    root, key, value, ser = tries["ascii_300"][2]["honest"]
    nodes = P.split_list(ser)
    junk = [bad for bad in R.malformed_nodes(S).values() if proofcheck_lib().pkc_canonical(bad, U64(len(bad)))]
    assert len(junk) >= 10  # canonical RLP that is no trie node: lists of 0, 1, 3, 16, 18 items, bad paths and children
    status = native_statuses(N, S, [(root, key, value, P.serialized(junk + nodes)), (root, key, b"other", P.serialized(nodes + junk)),
                                    (root, key, value, P.serialized(nodes + [b"\xc4\x20\xb8\x01\x90"]))])
    assert list(status) == [N.PV_PROOF_ACCEPT, N.PV_PROOF_REJECT, N.PV_PROOF_DEFER]  # the last pool holds non-canonical RLP


def test_blank_root_at_the_abi_is_deferred(S, host_path):
    assert list(native_statuses(host_path, S, [(S.BLANK_ROOT, b"k", None, b"\xc1\x80")])) == [host_path.PV_PROOF_DEFER]


def test_one_proof_many_queries_and_both_record_layouts(S, host_path, tries):
    N = host_path
    st, sets = tries["ascii_300"][:2]
    nodes, rn = P.proof_of(st, S.rlp_encode, b"", prefix=True)[:2]
    recs = nodes + [rn]
    values = P.final_map(sets)
    keys = sorted(values) + [b"zz-absent"]
    vals = [stored(S, values.get(k)) for k in keys]
    vals[5] = stored(S, b"wrong")
    want = [N.PV_PROOF_ACCEPT] * len(keys)
    want[5] = N.PV_PROOF_REJECT
    blob, off = R.pack(recs, 3)
    kb, ko = N._blob(keys)
    vb, vo = N._blob(vals)
    roots = np.frombuffer(st.headHash * len(keys), np.uint8)
    for node_len in (None, np.diff(off)):
        got = N.trie_verify_proofs_raw(blob, off, node_len, [0, len(recs)], np.zeros(len(keys), np.uint32), roots, kb, ko, vb, vo)
        assert list(got) == want
    assert N.proof_last == {"nodes": len(recs), "queries": len(keys), "deferred": 0, "launches": 0}


# --------------------------------------------------------------------------- pv_trie_proof_split
def test_proof_split_against_python(S, host_path, tries):
    N = host_path
    good = [a[3] for _, c, a in all_corruptions(tries) if c in P.CANONICAL_CLASSES] + [b"\xc0", P.serialized([b"\x80"])]
    leaf = S.rlp_encode([b"\x20", b"v"])
    bad = [b"", b"\xc1", b"\x83abc", P.serialized([leaf]) + b"\x00", P.serialized([leaf])[:-1], b"\xf8\x02\x80\x80",
           b"\xc3\x81\x05\x80", b"\xc2\xb8\x00"]
    sers = [x for pair in zip(good, bad * (len(good) // len(bad) + 1)) for x in pair]
    blob, first, off, lens, ok = N.trie_proof_split(sers)
    data, at = blob.tobytes(), 0
    for p, ser in enumerate(sers):
        recs = [data[int(off[i]):int(off[i]) + int(lens[i])] for i in range(int(first[p]), int(first[p + 1]))]
        if p % 2:
            assert ok[p] == 0 and recs == [], ser
        else:
            assert ok[p] == 1 and recs == P.split_list(ser)
            assert all(at <= int(off[i]) for i in range(int(first[p]), int(first[p + 1])))  # in place: inside this proof
        at += len(ser)
    assert first[0] == 0 and first[-1] == len(lens) and off.shape[0] == len(lens) + 1
    # too little room: the count needed, nothing written past the capacity
    L = N.lib()
    sb, so = N._blob(good[:4])
    pf, okb, cnt = np.zeros(5, np.uint64), np.zeros(4, np.uint8), U64()
    no, nl = np.full(3, 77, np.uint64), np.full(2, 77, np.uint64)
    rc = L.pv_trie_proof_split(N._ptr(sb), N._ptr(so), 4, N._ptr(pf), N._ptr(no), N._ptr(nl), 2, ctypes.byref(cnt), N._ptr(okb))
    assert rc == N.PV_TRIE_NEED_SPACE and cnt.value == sum(len(P.split_list(s)) for s in good[:4]) > 2 and no[2] == 77
    assert L.pv_trie_proof_split(N._ptr(sb), None, 4, N._ptr(pf), N._ptr(no), N._ptr(nl), 2, ctypes.byref(cnt), N._ptr(okb)) == N.PV_ERR_ARG
    assert L.pv_trie_proof_split(N._ptr(sb), N._ptr(so), 4, None, N._ptr(no), N._ptr(nl), 2, ctypes.byref(cnt), N._ptr(okb)) == N.PV_ERR_ARG
    assert L.pv_trie_proof_split(N._ptr(sb), N._ptr(so), 4, N._ptr(pf), N._ptr(no), None, 2, ctypes.byref(cnt), N._ptr(okb)) == N.PV_ERR_ARG
    assert L.pv_trie_proof_split(N._ptr(sb), N._ptr(np.array([9, 0, 0, 0, 0], np.uint64)), 4, N._ptr(pf), N._ptr(no), N._ptr(nl), 2,
                                 ctypes.byref(cnt), N._ptr(okb)) == N.PV_ERR_ARG
    assert L.pv_trie_proof_split(None, None, 0, N._ptr(pf), N._ptr(no), None, 0, ctypes.byref(cnt), None) == 0 and cnt.value == 0


def test_serialized_and_wire_form_end_to_end(S, host_path, tries):
    from plenum_amd.serialization import proof_nodes_serializer, state_roots_serializer
    st, sets = tries["ascii_300"][:2]
    replies = []
    for k, v in sets[::11]:
        ser, raw = st.generate_state_proof(k, serialize=True, get_value=True)
        assert raw == S.rlp_encode([v])
        replies.append((state_roots_serializer.serialize(st.headHash), k, v, proof_nodes_serializer.serialize(ser)))
    assert all(isinstance(r, str) and isinstance(p, bytes) for r, _, _, p in replies)
    items = [(state_roots_serializer.deserialize(r), k, v, proof_nodes_serializer.deserialize(p)) for r, k, v, p in replies]
    items[2] = items[2][:2] + (b"forged",) + items[2][3:]
    want = [True] * len(items)
    want[2] = False
    assert S.PruningState.verify_state_proof_batch(items, serialized=True) == want
    assert host_path.proof_last["queries"] == len(items) and host_path.proof_last["deferred"] == 0


# ----------------------------------------------------------------------------------------- the ABI
def test_argument_checks(S, host_path, tries):
    N = host_path
    L = N.lib()
    root, key, value, ser = tries["single"][2]["honest"]
    recs = P.split_list(ser)
    blob, off = R.pack(recs)
    arrays = dict(node_blob=blob, node_off=off, proof_first=np.array([0, len(recs)], np.uint64), query_proof=np.zeros(1, np.uint32),
                  root=np.frombuffer(root, np.uint8), key_blob=np.frombuffer(key, np.uint8), key_off=np.array([0, len(key)], np.uint64),
                  val_blob=np.frombuffer(stored(S, value), np.uint8), val_off=np.array([0, len(stored(S, value))], np.uint64),
                  node_len=None)
    status = np.full(1, 9, np.uint8)

    def call(status=status, n_nodes=len(recs), n_proofs=1, n_queries=1, **kw):
        a = dict(arrays, **kw)
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        arg = N.PvProofIn(p(a["node_blob"]), p(a["node_off"]), n_nodes, p(a["proof_first"]), n_proofs, p(a["query_proof"]),
                          p(a["root"]), p(a["key_blob"]), p(a["key_off"]), p(a["val_blob"]), p(a["val_off"]), n_queries,
                          p(a["node_len"]))
        return L.pv_trie_verify_proofs(ctypes.byref(arg), None if status is None else N._ptr(status))

    assert call() == 0 and status[0] == N.PV_PROOF_ACCEPT
    assert call(node_len=np.diff(off)) == 0 and status[0] == N.PV_PROOF_ACCEPT
    assert L.pv_trie_verify_proofs(None, N._ptr(status)) == N.PV_ERR_ARG
    assert call(status=None) == N.PV_ERR_ARG
    assert call(n_queries=0, status=None) == 0
    for name in ("node_blob", "node_off", "proof_first", "query_proof", "root", "key_blob", "key_off", "val_blob", "val_off"):
        assert call(**{name: None}) == N.PV_ERR_ARG, name
    assert call(node_off=off[::-1].copy()) == N.PV_ERR_ARG
    assert call(proof_first=np.array([len(recs), 0], np.uint64)) == N.PV_ERR_ARG
    assert call(proof_first=np.array([0, len(recs) + 1], np.uint64)) == N.PV_ERR_ARG  # past the records
    assert call(key_off=np.array([len(key), 0], np.uint64)) == N.PV_ERR_ARG
    assert call(val_off=np.array([3, 0], np.uint64)) == N.PV_ERR_ARG
    assert call(query_proof=np.ones(1, np.uint32)) == N.PV_ERR_ARG  # query_proof[i] >= n_proofs
    # the limits: 1,024 records per proof, 65,535 key bytes, values below 2^24
    many = np.zeros(N.PV_PROOF_MAX_NODES + 2, np.uint64)
    assert call(node_off=many, n_nodes=N.PV_PROOF_MAX_NODES + 1, proof_first=np.array([0, N.PV_PROOF_MAX_NODES + 1], np.uint64)) \
        == N.PV_ERR_ARG
    assert call(node_off=many, n_nodes=N.PV_PROOF_MAX_NODES, proof_first=np.array([0, N.PV_PROOF_MAX_NODES], np.uint64)) == 0
    assert status[0] == N.PV_PROOF_DEFER  # 1,024 empty records: none is canonical RLP
    assert call(key_blob=np.zeros(65536, np.uint8), key_off=np.array([0, 65536], np.uint64)) == N.PV_ERR_ARG
    assert call(key_blob=np.zeros(65536, np.uint8), key_off=np.array([0, 65535], np.uint64)) == 0 and status[0] == N.PV_PROOF_REJECT
    assert call(val_blob=np.zeros(1 << 24, np.uint8), val_off=np.array([0, 1 << 24], np.uint64)) == N.PV_ERR_ARG
    assert b"2^24" in L.pv_last_error()
    assert call(val_blob=np.zeros(1 << 24, np.uint8), val_off=np.array([0, (1 << 24) - 1], np.uint64)) == 0


def test_forced_device_path_without_a_device():
    """In a fresh process that never calls pv_init: PV_ERR_NO_DEVICE, no silent host fallback; the device entry
    PV_ERR_NOT_INIT."""
    code = ("import sys, ctypes, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "from plenum_amd import _native as N\n"
            "L = N.lib()\n"
            "assert L.pv_trie_path(N.PV_TRIE_DEVICE) == 0\n"
            "z8, z64, z32, st = np.zeros(64, np.uint8), np.zeros(2, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint8)\n"
            "p = lambda a: a.ctypes.data\n"
            "arg = N.PvProofIn(p(z8), p(z64), 1, p(z64), 1, p(z32), p(z8), p(z8), p(z64), p(z8), p(z64), 1, None)\n"
            "assert L.pv_trie_verify_proofs(ctypes.byref(arg), p(st)) == N.PV_ERR_NO_DEVICE\n"
            "assert L.pv_trie_verify_proofs_device(ctypes.byref(arg), p(st), p(z8), None) == N.PV_ERR_NOT_INIT\n"
            "assert L.pv_trie_path(N.PV_TRIE_AUTO) == 0\n"
            "assert L.pv_trie_verify_proofs(ctypes.byref(arg), p(st)) == 0 and st[0] == N.PV_PROOF_REJECT\n"
            % os.path.join(ROOT, "indy-plenum_amd"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    subprocess.run([sys.executable, "-c", code], check=True, env=env)


# ------------------------------------------------------------ the shared source compiled for the host
def mutate(rng, recs, root, key, value):
    """One random mutation of an honest (records, root, key, stored value)."""
    recs = list(recs)
    kind = int(rng.integers(0, 12))
    i = int(rng.integers(0, len(recs)))
    if kind == 0:
        pass
    elif kind in (1, 2, 3):  # a byte of a record changed, near its head more often than not
        b = bytearray(recs[i])
        at = int(rng.integers(0, min(len(b), 4 if kind == 3 else len(b))))
        b[at] = (b[at] ^ (1 << int(rng.integers(0, 8)))) if kind == 1 else int(rng.integers(0, 256))
        recs[i] = bytes(b)
    elif kind == 4:
        del recs[i]
    elif kind == 5:
        recs[i] = recs[i][:int(rng.integers(0, len(recs[i])))]
    elif kind == 6:
        recs[i] = recs[i] + bytes(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8))
    elif kind == 7:
        key = bytearray(key or b"\x00")
        at = int(rng.integers(0, len(key)))
        key[at] ^= 1 << int(rng.integers(0, 8))
        key = bytes(key)
    elif kind == 8:
        key = key[:int(rng.integers(0, len(key) + 1))] + bytes(rng.integers(0, 256, int(rng.integers(0, 3)), dtype=np.uint8))
    elif kind == 9:
        value = b"" if value else b"\xc2\x80\x80"
    elif kind == 10:
        value = value[:-1] + bytes([value[-1] ^ 1]) if value else b"\xc1\x80"
    else:
        rng.shuffle(recs)
        recs = recs + recs[:1]
    return recs, root, key, value


def test_check_library_against_the_python_walk_on_random_mutations(S, tries):
    """A few thousand mutations of honest proofs through the host-compiled canonical check and walk: whenever
    the verdict is not DEFER it is the sequential Python result; honest input is never deferred."""
    L = proofcheck_lib()
    rng = np.random.default_rng(91)
    honest = []
    for name in ("single", "empty_key", "prefix_short_first", "anchor_small", "full_branch_embedded", "full_branch_hashed", "ascii_300"):
        st, sets = tries[name][:2]
        for k in sum(P.query_keys(sets), []):
            honest.append((P.split_list(st.generate_state_proof(k, serialize=True)), st.headHash, k, stored(S, P.final_map(sets).get(k))))
    counts = {0: 0, 1: 0, 2: 0}
    for n in range(3000):
        base = honest[n % len(honest)]
        recs, root, key, value = mutate(rng, *base) if n >= len(honest) else base
        blob, off = R.pack(recs)
        flags = np.zeros(len(recs) + 1, np.uint8)
        got = L.pkc_verify(blob.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), U64(len(recs)), root, key,
                           U64(len(key)), value, U64(len(value)), flags.ctypes.data_as(ctypes.c_void_p))
        counts[got] += 1
        if n < len(honest):
            assert got == 1, n
        if got != 2:
            assert not flags.any()
            assert got == int(S.Trie.verify_spv_proof(root, key, value, P.serialized(recs), serialized=True)), (n, recs, key, value)
    assert counts[0] > 300 and counts[1] > 300 and counts[2] > 300, counts


def test_canonical_check_and_the_nesting_bound(S):
    L = proofcheck_lib()
    canon = lambda b: L.pkc_canonical(b, U64(len(b)))  # noqa: E731
    enc = S.rlp_encode
    leaf = [b"\x31", b"v"]
    deepest_honest = [b""] * 3 + [[b"\x11", [b""] * 5 + [leaf] + [b""] * 11]] + [b""] * 13  # branch > extension > branch > leaf
    assert len(enc(deepest_honest[3])) < 32 and canon(enc(deepest_honest))
    assert not canon(enc([[[[[b"x"]]]]])) and canon(enc([[[[b"x"]]]]))  # five lists deep: not taken
    for good in (b"\x80", b"\x7f", enc(b"x" * 56), enc([]), enc([b"", [b"", []], b"\x05"]), enc([b"k" * 60, [b"v" * 70]])):
        assert canon(good), good
    for bad in (b"", b"\x81\x05", b"\xb8\x05hello", b"\xc2\x80", b"\xc1\x80\x80", b"\xc3\x81\x05\x80", b"\xc4\xc2\x80\x80\x80"[:4],
                b"\xc3\xc1\x81\x05"[:4], b"\xc4\xc3\xb8\x01\x90", b"\xf8\x01\x80", b"\xc2\xc2\x80", b"\xf9\x00\x40" + b"\x80" * 64):
        assert not canon(bad), bad
    for name, node in R.malformed_nodes(S).items():  # tr_rlp_item's rules, nothing about node shape
        try:
            strict = S.rlp_encode(S.rlp_decode(node)) == node
        except (ValueError, IndexError):
            strict = False
        assert bool(canon(node)) == strict, name


# ------------------------------------------------------------------ the host code under sanitizers
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer runs belong on machines without a GPU")
def test_host_code_stand_alone_under_sanitizers(S, host_path, tries, tmp_path):
    """The new code of csrc/trie_host.cpp (split, argument checks, hashing, canonical check, walk) in a program of
    its own, built with -fsanitize=address,undefined, on every corruption of every golden trie plus proofs the
    split must refuse. Never loaded into Python."""
    N = host_path
    srcs = [os.path.join(HERE, "native", "proof_host_check.cpp"), os.path.join(CSRC, "trie_host.cpp")]
    deps = srcs + [os.path.join(CSRC, f) for f in ("keccak.h", "trie_core.h", "trie_host.h")]
    if not os.path.exists(HOST_CHECK) or os.path.getmtime(HOST_CHECK) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan",
                               "-Wno-unknown-pragmas", "-pthread", "-I" + CSRC] + srcs + ["-o", HOST_CHECK])
    cases = [a for _, _, a in all_corruptions(tries, skip=ROOT_LENGTH_CLASSES)]
    cases += [(bytes(32), b"k", None, bad) for bad in R.malformed_nodes(S).values()]  # as whole proofs
    junk = [bad for bad in R.malformed_nodes(S).values() if bad]
    root, key, value, ser = tries["ascii_300"][2]["honest"]
    cases += [(root, key, value, P.serialized(P.split_list(ser) + [j])) for j in junk]
    _, first, _, _, ok = N.trie_proof_split([a[3] for a in cases])
    good = [a for a, o in zip(cases, ok) if o]
    status = iter(native_statuses(N, S, good))
    blob = [struct.pack("<I", len(cases))]
    for (r, k, v, ser), o in zip(cases, ok):
        sv = stored(S, v)
        blob.append(struct.pack("<I", len(ser)) + ser + r + struct.pack("<I", len(k)) + k + struct.pack("<I", len(sv)) + sv
                    + bytes([o, next(status) if o else 0]))
    path = tmp_path / "proof_host_check.in"
    path.write_bytes(b"".join(blob))
    res = subprocess.run([HOST_CHECK, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, res.stderr.decode(errors="replace")[-2000:]
    assert res.stdout.decode().startswith("ok %d cases %d queries" % (len(cases), len(good)))
