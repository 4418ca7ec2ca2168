"""Batch Ed25519 signing on the GPU (pv_sign_seed_keypairs / pv_sign_batch / pv_sign_batch_device and the
Python surface over them) against crypto_sign_detached, byte for byte, no tolerance: signing is
deterministic. The expectation is the libsodium-free recipe of tests/test_sign_host.py (hashlib + the C
oracle; pinned to libsodium there), and libsodium itself as well when it is present."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_sign_host import BOUNDARY_LENGTHS, recipe_keypair, recipe_sign

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_POOL = 3000  # messages and signers of the shared pool


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    _native.ensure_device()
    return _native


@pytest.fixture(scope="module")
def maybe_sodium():
    from oracle.libsodium_ref import LibSodium, find_libsodium
    return LibSodium() if find_libsodium() else None


class Pool:
    """N_POOL seeds with their key pairs and N_POOL messages (the boundary lengths, then random lengths
    0..1,200), computed once; expected signatures are computed on demand and remembered."""

    def __init__(self, oracle, sodium):
        self.oracle, self.sodium = oracle, sodium
        rng = np.random.default_rng(41)
        self.seeds = [bytes(32), b"\xff" * 32] + [rng.bytes(32) for _ in range(N_POOL - 2)]
        self.pks, self.sks = [], []
        for seed in self.seeds:
            pk, sk = recipe_keypair(oracle, seed)
            if sodium:
                assert sodium.seed_keypair(seed) == (pk, sk)
            self.pks.append(pk)
            self.sks.append(sk)
        lens = list(BOUNDARY_LENGTHS) + [int(x) for x in rng.integers(0, 1201, N_POOL - len(BOUNDARY_LENGTHS))]
        self.msgs = [rng.bytes(n) for n in lens]
        self._sig = {}

    def sig(self, sk, m):
        key = (sk, m)
        if key not in self._sig:
            s = recipe_sign(self.oracle, sk, m)
            if self.sodium:
                assert self.sodium.sign_detached(m, sk) == s
            self._sig[key] = s
        return self._sig[key]

    def sk_table(self, k):
        return np.frombuffer(b"".join(self.sks[:k]), np.uint8).reshape(k, 64)


@pytest.fixture(scope="module")
def pool(oracle, maybe_sodium):
    return Pool(oracle, maybe_sodium)


def pack_msgs(msgs, lead=0):
    """(blob, offsets) of msgs with `lead` bytes of garbage in front of the first message."""
    off = np.zeros(len(msgs) + 1, np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    off += np.uint64(lead)
    return np.frombuffer(b"\xa5" * lead + b"".join(msgs) + b"\x5a" * 3, np.uint8), off


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_seed_keypairs(native, pool, n):
    pks, sks = native.seed_keypairs(np.frombuffer(b"".join(pool.seeds[:n]), np.uint8))
    assert pks.shape == (n, 32) and sks.shape == (n, 64)
    assert [p.tobytes() for p in pks] == pool.pks[:n]
    assert [s.tobytes() for s in sks] == pool.sks[:n]
    # either output may be NULL
    L = native.lib()
    seeds = np.frombuffer(b"".join(pool.seeds[:n]), np.uint8)
    only_pk, only_sk = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    assert L.pv_sign_seed_keypairs(native._ptr(seeds), n, native._ptr(only_pk), None) == 0
    assert L.pv_sign_seed_keypairs(native._ptr(seeds), n, None, native._ptr(only_sk)) == 0
    assert np.array_equal(only_pk, pks) and np.array_equal(only_sk, sks)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, N_POOL])
def test_sign_batch_matches_crypto_sign_detached(native, pool, n):
    rng = np.random.default_rng(n)
    msgs = pool.msgs[:n]
    blob, off = pack_msgs(msgs)
    for k in sorted({1, min(5, n), n}):
        idx = rng.integers(0, k, n).astype(np.uint32)  # shuffled, repeating
        idx[: min(k, n)] = rng.permutation(k)[: min(k, n)]
        got = native.sign_batch(blob, off, pool.sk_table(k), idx)
        assert got.shape == (n, 64)
        for i in range(n):
            assert got[i].tobytes() == pool.sig(pool.sks[idx[i]], msgs[i]), (n, k, i, len(msgs[i]))
    # the NULL-index form: message i with secret key i
    got = native.sign_batch(blob, off, pool.sk_table(n))
    for i in range(n):
        assert got[i].tobytes() == pool.sig(pool.sks[i], msgs[i]), (n, i)


@pytest.mark.parametrize("lead", range(1, 8))
def test_message_alignment(native, pool, lead):
    """The blob shifted by 1..7 bytes of leading garbage: with the pool's mixed lengths every start
    residue mod 8 occurs in every run."""
    n = 130
    msgs = pool.msgs[:n]
    blob, off = pack_msgs(msgs, lead)
    assert {int(o) % 8 for o in off[:-1]} == set(range(8))
    idx = (np.arange(n) % 5).astype(np.uint32)
    got = native.sign_batch(blob, off, pool.sk_table(5), idx)
    for i in range(n):
        assert got[i].tobytes() == pool.sig(pool.sks[idx[i]], msgs[i]), (lead, i)


def test_key_half_is_used_as_given(native, pool):
    """sk[32:64] that is another signer's key: libsodium's signature for that 64-byte key."""
    mixed = [pool.sks[i][:32] + pool.pks[i + 1] for i in range(6)]
    msgs = pool.msgs[10:16]
    blob, off = pack_msgs(msgs)
    got = native.sign_batch(blob, off, np.frombuffer(b"".join(mixed), np.uint8))
    for i in range(6):
        want = pool.sig(mixed[i], msgs[i])
        assert want != pool.sig(pool.sks[i], msgs[i])
        assert got[i].tobytes() == want


def test_host_entry_validates_arguments(native, pool):
    L = native.lib()
    blob, off = pack_msgs(pool.msgs[:4])
    sk = pool.sk_table(2)
    sig = np.zeros((4, 64), np.uint8)
    idx = np.array([0, 1, 0, 1], np.uint32)
    p = native._ptr
    assert L.pv_sign_batch(p(blob), p(off), 0, p(sk), 0, None, p(sig)) == native.PV_OK  # n = 0: nothing to do
    assert L.pv_sign_batch(p(blob), p(off), 4, p(sk), 0, p(idx), p(sig)) == native.PV_ERR_ARG  # no signers
    bad_idx = np.array([0, 2, 0, 1], np.uint32)
    assert L.pv_sign_batch(p(blob), p(off), 4, p(sk), 2, p(bad_idx), p(sig)) == native.PV_ERR_ARG
    bad_off = off.copy()
    bad_off[3] = bad_off[2] - np.uint64(1)  # off[2] = 1 (the pool's first lengths are 0, 1, 47)
    assert L.pv_sign_batch(p(blob), p(bad_off), 4, p(sk), 2, p(idx), p(sig)) == native.PV_ERR_ARG
    assert L.pv_sign_batch(p(blob), p(off), 4, p(sk), 2, None, p(sig)) == native.PV_ERR_ARG  # NULL idx: n_signers == n
    assert not sig.any()
    assert L.pv_sign_batch(p(blob), p(off), 4, p(sk), 2, p(idx), p(sig)) == native.PV_OK
    assert sig[3].tobytes() == pool.sig(pool.sks[1], pool.msgs[3])


class DevBuf:
    def __init__(self, native):
        self.nat, self.L, self.ptrs = native, native.lib(), []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self.nat.check(self.L.pv_dev_alloc(ctypes.byref(p), nbytes), "pv_dev_alloc")
        self.ptrs.append(p)
        return p

    def put(self, a, slack=0):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes + slack)
        self.nat.check(self.L.pv_memcpy_h2d(p, a.ctypes.data, a.nbytes), "pv_memcpy_h2d")
        return p

    def free(self):
        for p in self.ptrs:
            self.L.pv_dev_free(p)


def test_device_entry_on_a_caller_stream(native, pool):
    """pv_sign_batch_device on the library stream and on a pv_stream_create stream: the same signatures;
    an out-of-range signer index gives 64 zero bytes and its neighbours stay correct."""
    L = native.lib()
    n, k = 300, 7
    msgs = pool.msgs[:n]
    blob, off = pack_msgs(msgs, lead=3)
    idx = (np.arange(n) * 3 % k).astype(np.uint32)
    bad = [0, 63, 64, 130, n - 1]
    idx[bad] = [k, 0xFFFFFFFF, k + 1000, k, k]
    d = DevBuf(native)
    s = ctypes.c_void_p()
    native.check(L.pv_stream_create(ctypes.byref(s)), "pv_stream_create")
    try:
        d_msg = d.put(blob, slack=native.PV_BLOB_SLACK)
        d_off, d_idx, d_sk = d.put(off), d.put(idx), d.put(pool.sk_table(k))
        d_sig = d.alloc(n * 64)
        for stream in (None, s, None, s):
            stale = np.full((n, 64), 0xA5, np.uint8)
            native.check(L.pv_memcpy_h2d(d_sig, stale.ctypes.data, stale.nbytes), "h2d")
            native.check(L.pv_sign_batch_device(d_msg, d_off, n, d_sk, k, d_idx, d_sig, stream), "pv_sign_batch_device")
            if stream:
                native.check(L.pv_stream_sync(stream), "pv_stream_sync")
            got = np.zeros((n, 64), np.uint8)
            native.check(L.pv_memcpy_d2h(got.ctypes.data, d_sig, got.nbytes), "d2h")
            for i in range(n):
                want = bytes(64) if i in bad else pool.sig(pool.sks[idx[i]], msgs[i])
                assert got[i].tobytes() == want, (stream, i)
        assert L.pv_sign_batch_device(d_msg, d_off, 0, d_sk, k, d_idx, d_sig, s) == native.PV_OK
        assert L.pv_sign_batch_device(d_msg, d_off, n, d_sk, 0, d_idx, d_sig, s) == native.PV_ERR_ARG
    finally:
        native.check(L.pv_stream_destroy(s), "pv_stream_destroy")
        d.free()


def test_chunk_boundary(native, pool):
    """One chunk + 65 messages of 8 bytes from 4 signers: every signature verifies (verify_sm_batch is
    pinned to libsodium by the existing suite), and the first 512, the last 512 and the 1,024 around the
    chunk boundary are byte-identical to the expectation."""
    C = native.PV_SIGN_CHUNK
    n = C + 65
    body = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8) ^ np.uint8(0x5C)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(8)
    idx = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(4)).astype(np.uint32)
    sigs = native.sign_batch(body.reshape(-1), off, pool.sk_table(4), idx)
    assert sigs.shape == (n, 64)
    # the windows overlap behind the boundary: the batch ends 65 records after it
    check = sorted(set(range(512)) | {i for i in range(C - 512, C + 512) if i < n} | set(range(n - 512, n)))
    for i in check:
        assert sigs[i].tobytes() == pool.sig(pool.sks[idx[i]], body[i].tobytes()), i
    sm = np.concatenate([sigs, body], axis=1).reshape(-1)
    pks = np.frombuffer(b"".join(pool.pks[:4]), np.uint8).reshape(4, 32)[idx]
    ok = native.verify_sm_batch(sm, np.arange(n + 1, dtype=np.uint64) * np.uint64(72), pks)
    assert ok.all(), np.nonzero(~ok)[0][:10]


_RADIX16_SCRIPT = r"""
import json, sys
import numpy as np
root = sys.argv[1]
sys.path[:0] = [root, root + "/indy-plenum_amd", root + "/tests"]
from plenum_amd import _native
d = json.load(open(sys.argv[2]))
blob = np.frombuffer(bytes.fromhex(d["blob"]), np.uint8)
off = np.array(d["off"], np.uint64)
sks = np.frombuffer(bytes.fromhex(d["sks"]), np.uint8)
idx = np.array(d["idx"], np.uint32)
pks, _ = _native.seed_keypairs(np.frombuffer(bytes.fromhex(d["seeds"]), np.uint8))
sigs = _native.sign_batch(blob, off, sks, idx)
print(json.dumps({"sigs": sigs.tobytes().hex(), "pks": pks.tobytes().hex()}))
"""


def test_radix16_comb_fallback(pool, tmp_path):
    """pv_init's radix-2^16 fallback of the wide fixed-base comb (forced with PV_FORCE_BCOMB16, in a
    fresh process: the radix is chosen once per pv_init): the 257-record case and 65 key pairs."""
    n, k = 257, 5
    msgs = pool.msgs[:n]
    blob, off = pack_msgs(msgs)
    idx = (np.arange(n) * 7 % k).astype(np.uint32)
    arg = tmp_path / "case.json"
    arg.write_text(json.dumps({"blob": blob.tobytes().hex(), "off": [int(o) for o in off],
                               "sks": b"".join(pool.sks[:k]).hex(), "idx": [int(i) for i in idx],
                               "seeds": b"".join(pool.seeds[:65]).hex()}))
    env = dict(os.environ, PV_FORCE_BCOMB16="1")
    p = subprocess.run([sys.executable, "-c", _RADIX16_SCRIPT, ROOT, str(arg)], env=env, capture_output=True,
                       text=True, timeout=170)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    sigs = bytes.fromhex(res["sigs"])
    for i in range(n):
        assert sigs[64 * i: 64 * i + 64] == pool.sig(pool.sks[idx[i]], msgs[i]), i
    assert bytes.fromhex(res["pks"]) == b"".join(pool.pks[:65])


# ------------------------------------------------------------------------------------- Python surface

@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "signing.json")) as f:
        return json.load(f)


def make_signer(rec):
    from plenum_amd.signing import DidSigner, SimpleSigner
    cls = DidSigner if rec["kind"] == "did" else SimpleSigner
    return cls(identifier=rec["identifier_arg"], seed=bytes.fromhex(rec["seed"]))


def test_signers_match_the_reference_goldens(native, golden):
    signers = [make_signer(r) for r in golden["signers"]]
    for s, r in zip(signers, golden["signers"]):
        assert (s.identifier, s.verkey, s.seedHex.decode()) == (r["identifier"], r["verkey"], r["seedHex"])
        assert s.naclSigner.verraw.hex() == r["verraw"]
        if r["kind"] == "did":
            assert s.full_verkey == r["full_verkey"]
    for c in golden["cases"]:
        assert signers[c["signer"]].sign(json.loads(json.dumps(c["msg"]))) == c["sig"], c


def test_sign_requests_matches_the_reference_goldens(native, golden):
    from plenum_amd.signing import sign_requests
    signers = [make_signer(r) for r in golden["signers"]]
    cases = golden["cases"]
    got = sign_requests([signers[c["signer"]] for c in cases], [c["msg"] for c in cases])
    assert got == [c["sig"] for c in cases]
    one = [c for c in cases if c["signer"] == cases[0]["signer"]]
    assert sign_requests(signers[cases[0]["signer"]], [c["msg"] for c in one]) == [c["sig"] for c in one]
    assert sign_requests([], []) == [] and sign_requests(signers[0], []) == []
    with pytest.raises(ValueError):
        sign_requests(signers[:2], [{}])


def test_nacl_signer_and_verifier_round_trip(native, pool):
    from plenum_amd.nacl_wrappers import HexEncoder, SignedMessage, Signer, SigningKey, Verifier, crypto_sign
    seed, m = pool.seeds[5], pool.msgs[20]
    s = Signer(seed)
    assert (s.keyraw, s.verraw) == (seed, pool.pks[5]) and s.keyhex == seed.hex().encode()
    assert Signer(seed.hex().encode()).verhex == pool.pks[5].hex().encode()
    sig = s.signature(m)
    assert sig == pool.sig(pool.sks[5], m)
    assert Verifier(s.verraw).verify(sig, m)
    assert not Verifier(s.verraw).verify(sig, m + b"x")
    signed = s.sign(m)
    assert isinstance(signed, SignedMessage) and bytes(signed) == sig + m
    assert (signed.signature, signed.message) == (sig, m)
    assert crypto_sign(m, pool.sks[5]) == sig + m
    hexed = SigningKey(seed).sign(m, encoder=HexEncoder)
    assert hexed.signature == sig.hex().encode() and bytes(hexed) == (sig + m).hex().encode()
    assert bytes(SigningKey(seed)) == seed and len(bytes(SigningKey.generate())) == 32


def test_signed_request_authenticates(native):
    """A request signed by plenum_amd.signing.DidSigner passes CoreAuthNr.authenticate; a tampered one
    does not."""
    from plenum_amd.client_authn import CoreAuthNr
    from plenum_amd.exceptions import InsufficientCorrectSignatures
    from plenum_amd.signing import DidSigner
    from plenum_amd.state_utils import DictState
    signer = DidSigner(seed=b"\x07" * 32)
    req = {"identifier": signer.identifier, "reqId": 1700000000000001, "protocolVersion": 2,
           "operation": {"type": "1", "dest": signer.identifier, "verkey": signer.verkey}}
    req["signature"] = signer.sign(req)
    a = CoreAuthNr(["1", "101"], ["105"], ["action"], state=DictState({}))
    a.addIdr(signer.identifier, signer.verkey)
    assert a.authenticate(json.loads(json.dumps(req))) == [signer.identifier]
    req["reqId"] += 1
    with pytest.raises(InsufficientCorrectSignatures):
        a.authenticate(req)
