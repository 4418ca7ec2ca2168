"""The host-buffer entries that stage through PvStage (csrc/stage.h), device paths forced, each called
with what the staging exists for: blobs with 37 bytes of junk in front, so that every offset array (records,
proofs, keys, values) starts at 37 and arrives on the device rebased to the bytes that were copied. 70
records each (one verdict word and a part of the next), among them an empty one and one of 300 bytes.
Expected values never come from the product: hashlib, the restatements in tests/merkle_ref.py, the signing
recipe of tests/test_sign_host.py, the ingress checkers of tests/test_gpu_ingress.py, the goldens recorded
from the reference and the host-compiled canonical check of tests/proof_ref.py."""
import ctypes
import hashlib

import numpy as np
import pytest

import merkle_ref as MR
import proof_ref as P
from test_gpu_ingress import expected as ingress_expected, signature_variant, signer_forms
from test_gpu_sign import pack_msgs
from test_merkle_host import brute_force_proof
from test_sign_host import recipe_keypair, recipe_sign

pytestmark = pytest.mark.gpu

LEAD, N = 37, 70
JUNK = b"\xa5" * LEAD


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    _native.ensure_device(0)
    return _native


@pytest.fixture()
def dev(native):
    native.merkle_path(native.PV_MERKLE_DEVICE)
    native.trie_path(native.PV_TRIE_DEVICE)
    native.merkle_chunk(0)
    yield native
    native.merkle_path(native.PV_MERKLE_AUTO)
    native.trie_path(native.PV_TRIE_AUTO)
    native.merkle_chunk(0)


@pytest.fixture(scope="module")
def records():
    """70 records: the empty one, one of 300 bytes, lengths around the SHA-256 and SHA3-256 block edges, random ones."""
    rng = np.random.default_rng(370)
    lens = [0, 300, 1, 55, 56, 63, 64, 65, 119, 135, 136, 137, 271, 272] + [int(x) for x in rng.integers(0, 200, N - 14)]
    order = rng.permutation(N)
    return [rng.bytes(lens[i]) for i in order]


def lead_pack(items):
    """(uint8 blob, uint64 offsets): LEAD junk bytes in front, offsets from LEAD on, a few junk bytes behind."""
    off = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(JUNK + b"".join(items) + b"\x5a" * 3, np.uint8), off + np.uint64(LEAD)


def test_sha3_256_batch(dev, records):
    blob, off = lead_pack(records)
    got = dev.sha3_256_batch(blob, off)
    assert got.tobytes() == b"".join(hashlib.sha3_256(r).digest() for r in records)


@pytest.mark.parametrize("chunk", (0, 64))
def test_merkle_append(dev, records, chunk):
    """chunk 64: the second chunk's offsets start far from 0 as well."""
    rng = np.random.default_rng(371)
    s = 13
    frontier = MR.random_frontier(rng, s)
    blob, off = lead_pack(records)
    dev.merkle_chunk(chunk)
    res = dev.merkle_append(s, b"".join(frontier), blob, off)
    assert res["leaf_hash"].tobytes() == b"".join(hashlib.sha256(b"\x00" + r).digest() for r in records)
    MR.assert_batch_equals(res, MR.append_all(s, frontier, records), N, "chunk=%d" % chunk)


def flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


@pytest.mark.parametrize("by_hash", (False, True))
def test_merkle_verify_inclusion(dev, records, by_hash):
    """pv_merkle_verify_inclusion_batch itself: the Python wrapper always packs from offset 0."""
    rng = np.random.default_rng(372)
    lh = [MR.leaf_hash(r) for r in records]
    root = MR.append_all(0, [], records)["root"]
    leaves, index, size, proofs, roots = [], [], [], [], []
    for i in range(N):
        leaf, prf, rt, idx = records[i], brute_force_proof(lh, i), root, i
        kind = i % 6
        if kind == 1:
            prf = prf[:2] + [flip(prf[2], int(rng.integers(0, 256)))] + prf[3:]
        elif kind == 2:
            rt = flip(rt, int(rng.integers(0, 256)))
        elif kind == 3:
            prf = prf[:-1]
        elif kind == 4:
            prf = prf + [rng.bytes(32)]
        elif kind == 5:
            idx = N + i
        leaves.append(leaf)
        index.append(idx)
        size.append(N)
        proofs.append(prf)
        roots.append(rt)
    want = []
    for leaf, idx, prf, rt in zip(leaves, index, proofs, roots):
        st, calc = MR.check_path(MR.leaf_hash(leaf), idx, N, prf)
        want.append((st == 0 and calc == rt, st))
    assert sum(w[0] for w in want) >= 10 and {w[1] for w in want} == {0, 1, 2, 3}
    blob, off = lead_pack(leaves)
    hashes = np.frombuffer(b"".join(MR.leaf_hash(x) for x in leaves), np.uint8)
    lead_hashes = 3  # proof hashes nobody refers to in front: proof_off starts at 3
    poff = np.zeros(N + 1, np.uint64)
    np.cumsum([len(p) for p in proofs], out=poff[1:])
    poff += np.uint64(lead_hashes)
    pbuf = np.frombuffer(b"\xa5" * (32 * lead_hashes) + b"".join(b"".join(p) for p in proofs), np.uint8)
    rbuf = np.frombuffer(b"".join(roots), np.uint8)
    idx_a, size_a = np.array(index, np.uint64), np.array(size, np.uint64)
    status, bits = np.full(N, 9, np.uint8), np.zeros((N + 7) // 8, np.uint8)
    p = dev._ptr
    dev.check(dev.lib().pv_merkle_verify_inclusion_batch(
        None if by_hash else p(blob), None if by_hash else p(off), p(hashes) if by_hash else None, p(idx_a), p(size_a),
        p(pbuf), p(poff), p(rbuf), N, p(status), p(bits)), "pv_merkle_verify_inclusion_batch")
    verdicts = np.unpackbits(bits, count=N, bitorder="little").view(bool)
    assert [(bool(v), int(s)) for v, s in zip(verdicts, status)] == want


def test_sign_batch(dev, oracle, records):
    """70 messages over 3 signers, and the form without signer indices (message i with key i)."""
    rng = np.random.default_rng(373)
    keys = [recipe_keypair(oracle, rng.bytes(32))[1] for _ in range(N)]
    blob, off = pack_msgs(records, LEAD)
    idx = (np.arange(N) % 3).astype(np.uint32)
    got = dev.sign_batch(blob, off, np.frombuffer(b"".join(keys[:3]), np.uint8), idx)
    assert [g.tobytes() for g in got] == [recipe_sign(oracle, keys[i % 3], m) for i, m in enumerate(records)]
    got = dev.sign_batch(blob, off, np.frombuffer(b"".join(keys), np.uint8))
    assert [g.tobytes() for g in got] == [recipe_sign(oracle, keys[i], m) for i, m in enumerate(records)]


def test_ingress_verify_arrays(dev, sodium, records):
    """70 requests over 3 signers; the signature, message, identifier and verkey blobs all start at 37."""
    rng = np.random.default_rng(374)
    signers = signer_forms(sodium, rng, 3)
    idrs, vks = [s[0] for s in signers], [s[1] for s in signers]
    # 23 messages shared between the requests, the empty record and the one of 300 bytes among them
    msgs = [r for r in records if len(r) in (0, 300)][:2] + [r for r in records if len(r) not in (0, 300)][:21]
    assert {len(m) for m in msgs} >= {0, 300} and len(msgs) == 23
    sigs, msg_idx, signer_idx = [], [], []
    for j in range(N):
        mi, si = j % len(msgs), j % 3
        sigs.append(signature_variant(j % 13 if j % 2 else 0, sodium.sign_detached(msgs[mi], signers[si][2]), rng))
        msg_idx.append(mi)
        signer_idx.append(si)
    want_st, want_v = ingress_expected(sodium, dev, sigs, msgs, msg_idx, signer_idx, idrs, vks)
    assert 35 <= want_v.sum() < N and set(int(x) for x in want_st) >= {0, 1, 2}
    sb, so = lead_pack(sigs)
    mb, mo = lead_pack(msgs)
    ib, io = lead_pack(idrs)
    vb, vo = lead_pack([v if v is not None else b"" for v in vks])
    st, v = dev.ingress_verify_arrays(sb, so, mb, mo, np.array(msg_idx, np.uint32), np.array(signer_idx, np.uint32), ib, io,
                                      vb, vo, np.array([k is not None for k in vks], np.uint8))
    assert np.array_equal(st, want_st) and np.array_equal(v, want_v)


@pytest.fixture(scope="module")
def proof_cases(native):
    """Golden corruption cases, whole proofs chosen until they hold 68 records, and what the reference answered."""
    from plenum_amd import state_trie as S
    native.trie_path(native.PV_TRIE_HOST)
    try:
        tries = P.build_tries(S)
    finally:
        native.trie_path(native.PV_TRIE_AUTO)
    gold = P.load_proof_golden()
    chosen, want, count = [], [], 0
    for name, c, a in P.all_corruptions(tries, skip=P.ROOT_LENGTH_CLASSES + P.UNSPLITTABLE):
        if name == "blank" or c not in P.CANONICAL_CLASSES + P.DEFER_CLASSES:
            continue
        k = len(P.split_list(a[3]))
        if k == 0 or count + k > N - 2 or any(len(r) > 250 for r in P.split_list(a[3])):
            continue
        chosen.append((a[0], a[1], P.stored(S, a[2]), P.split_list(a[3])))
        want.append(native.PV_PROOF_DEFER if c in P.DEFER_CLASSES else int(gold[name]["corruptions"][c] == "true"))
        count += k
    assert count == N - 2 and {0, 1, 2} <= set(want)
    return chosen, want


def test_trie_verify_proofs_raw(dev, proof_cases):
    """70 records in proofs one after another, the last proof an empty record and one of 300 bytes; 70 queries that
    go round the proofs. Node, key and value offsets all start at 37."""
    chosen, want = proof_cases
    C = P.proofcheck_lib()
    odd = [b"", P.rlp_str(bytes(range(256)) + bytes(41))]
    assert len(odd[1]) == 300 and C.pkc_canonical(odd[1], ctypes.c_uint64(300)) and not C.pkc_canonical(b"", ctypes.c_uint64(0))
    # a proof with a record that is not canonical RLP is deferred whatever is asked of it
    chosen = chosen + [(bytes(32), b"key", b"", odd)]
    want = want + [dev.PV_PROOF_DEFER]
    recs = [r for c in chosen for r in c[3]]
    assert len(recs) == N
    first = np.zeros(len(chosen) + 1, np.uint64)
    np.cumsum([len(c[3]) for c in chosen], out=first[1:])
    which = [q % len(chosen) for q in range(N)]
    blob, off = lead_pack(recs)
    kb, ko = lead_pack([chosen[p][1] for p in which])
    vb, vo = lead_pack([chosen[p][2] for p in which])
    roots = np.frombuffer(b"".join(chosen[p][0] for p in which), np.uint8)
    for node_len in (None, np.diff(off)):
        status = dev.trie_verify_proofs_raw(blob, off, node_len, first, np.array(which, np.uint32), roots, kb, ko, vb, vo)
        assert dev.proof_last["launches"] == 2
        assert list(status) == [want[p] for p in which]
