"""The signing arithmetic (indy-plenum_amd/csrc/sign_core.h) compiled for the HOST
(tests/native/signcheck.hip) against libsodium's crypto_sign_seed_keypair / crypto_sign_detached and
Python big integers, byte for byte; the signing entry points without a device; and the committed
goldens of the reference's own signers. Same source as the GPU kernels, so a pass here means the
kernels' arithmetic is right up to compilation; tests/test_gpu_sign.py closes that gap."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
LIB = os.path.join(HERE, "native", "libsigncheck.so")
L = 2 ** 252 + 27742317777372353535851937790883648493
# block boundaries of the two hashes: 32 + len + 17 and 64 + len + 17 against multiples of 128
BOUNDARY_LENGTHS = (0, 1, 47, 48, 79, 80, 175, 176, 207, 208, 303, 304, 335, 336)


def build_signcheck():
    src = os.path.join(HERE, "native", "signcheck.hip")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-pthread", "--offload-arch=gfx950",
                           "--offload-host-only", "-I" + CSRC, src, "-o", LIB])


def signcheck_lib():
    srcs = [os.path.join(CSRC, f) for f in ("sign_core.h", "fe25519.h", "ge25519.h", "sc25519.h", "sha512.h",
                                            "comb.h", "btable.h", "verify_core.h")]
    srcs.append(os.path.join(HERE, "native", "signcheck.hip"))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_signcheck()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def sc():
    return signcheck_lib()


def sc_keypair(sc, seed):
    pk, sk = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    sc.sgc_keypair(seed, pk, sk)
    return pk.raw, sk.raw


def sc_sign(sc, sk, m):
    sig = ctypes.create_string_buffer(64)
    sc.sgc_sign(sk, m, ctypes.c_uint64(len(m)), sig)
    return sig.raw


def expand(seed):
    """(clamped a, prefix) of a seed with hashlib: the libsodium-free recipe's first step."""
    az = bytearray(hashlib.sha512(seed).digest())
    az[0] &= 248
    az[31] &= 127
    az[31] |= 64
    return int.from_bytes(az[:32], "little"), bytes(az[32:])


def recipe_keypair(oracle, seed):
    a, _ = expand(seed)
    pk = oracle.scalarmult_base((a % L).to_bytes(32, "little"))
    return pk, seed + pk


def recipe_sign(oracle, sk, m):
    """crypto_sign_detached without libsodium: hashlib for az and r, the C oracle for [r]B, k and S (a is
    passed reduced mod L, which is exact: B has order L and S is taken mod L)."""
    a, prefix = expand(sk[:32])
    r = int.from_bytes(hashlib.sha512(prefix + m).digest(), "little") % L
    return oracle.sign_raw(r.to_bytes(32, "little"), (a % L).to_bytes(32, "little"), sk[32:], m)


def test_keypair_and_signature_equal_libsodium_random(sc, sodium):
    rng = random.Random(20)
    for _ in range(2000):
        seed = rng.randbytes(32)
        pk, sk = sc_keypair(sc, seed)
        assert (pk, sk) == sodium.seed_keypair(seed)
        m = rng.randbytes(rng.randrange(0, 1200))
        assert sc_sign(sc, sk, m) == sodium.sign_detached(m, sk)


def test_every_length_to_400_and_block_boundaries(sc, sodium):
    rng = random.Random(21)
    _, sk = sodium.seed_keypair(rng.randbytes(32))
    for n in list(range(401)) + list(BOUNDARY_LENGTHS):
        m = rng.randbytes(n)
        assert sc_sign(sc, sk, m) == sodium.sign_detached(m, sk), n


def test_extreme_seeds(sc, sodium):
    for seed in (bytes(32), b"\xff" * 32):
        pk, sk = sc_keypair(sc, seed)
        assert (pk, sk) == sodium.seed_keypair(seed)
        for n in BOUNDARY_LENGTHS:
            m = bytes(range(256)) * 2
            assert sc_sign(sc, sk, m[:n]) == sodium.sign_detached(m[:n], sk)


def test_key_half_is_used_as_given(sc, sodium):
    """An sk whose second half is another signer's key: libsodium hashes the bytes as given."""
    rng = random.Random(22)
    _, sk1 = sodium.seed_keypair(rng.randbytes(32))
    pk2, _ = sodium.seed_keypair(rng.randbytes(32))
    mixed = sk1[:32] + pk2
    for n in (0, 5, 80, 300):
        m = rng.randbytes(n)
        want = sodium.sign_detached(m, mixed)
        assert want != sodium.sign_detached(m, sk1)
        assert sc_sign(sc, mixed, m) == want


def test_recipe_without_libsodium_equals_libsodium(oracle, sodium):
    """The hashlib + oracle recipe the GPU tests use when libsodium is absent is libsodium's signature."""
    rng = random.Random(23)
    seeds = [bytes(32), b"\xff" * 32] + [rng.randbytes(32) for _ in range(40)]
    for i, seed in enumerate(seeds):
        pk, sk = sodium.seed_keypair(seed)
        assert recipe_keypair(oracle, seed) == (pk, sk)
        for n in (BOUNDARY_LENGTHS[i % len(BOUNDARY_LENGTHS)], rng.randrange(0, 1200)):
            m = rng.randbytes(n)
            assert recipe_sign(oracle, sk, m) == sodium.sign_detached(m, sk)


def test_signcheck_equals_recipe(sc, oracle):
    """The same comparison with no libsodium in the loop (runs where it is absent)."""
    rng = random.Random(24)
    for seed in [bytes(32), b"\xff" * 32] + [rng.randbytes(32) for _ in range(60)]:
        pk, sk = sc_keypair(sc, seed)
        assert (pk, sk) == recipe_keypair(oracle, seed)
        for n in (rng.choice(BOUNDARY_LENGTHS), rng.randrange(0, 1200)):
            m = rng.randbytes(n)
            assert sc_sign(sc, sk, m) == recipe_sign(oracle, sk, m)


def test_expand_keeps_a_mod_l(sc):
    rng = random.Random(25)
    for seed in [bytes(32), b"\xff" * 32] + [rng.randbytes(32) for _ in range(200)]:
        a, prefix = expand(seed)
        ao, po = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        sc.sgc_expand(seed, ao, po)
        assert int.from_bytes(ao.raw, "little") == a % L and po.raw == prefix


def test_header_hash_against_hashlib(sc):
    """pv_sha512_hm (the sibling of pv_hash_k) for both header sizes, every length around the block
    boundaries, message bytes past the end ignored."""
    rng = random.Random(26)
    lengths = sorted(set(range(0, 140)) | {n + d for n in BOUNDARY_LENGTHS for d in (-1, 0, 1) if n + d >= 0} | {1199})
    for hl in (32, 64):
        hdr = rng.randbytes(hl)
        for n in lengths:
            m = rng.randbytes(n)
            out = ctypes.create_string_buffer(64)
            assert sc.sgc_sha512_hm(hdr, hl, m, ctypes.c_uint64(n), out) == 0
            assert out.raw == hashlib.sha512(hdr + m).digest(), (hl, n)


def test_scalar_step_edges(sc):
    """S = (k a + r) mod L alone against Python integers: r = 0, r = L - 1, a = L - 1, k = 0, the
    largest 256-bit operands, random ones."""
    rng = random.Random(27)
    top = 2 ** 256 - 1
    cases = [(k, a, r) for k in (0, 1, L - 1, top) for a in (0, 1, L - 1, top) for r in (0, L - 1, top)]
    cases += [(rng.randrange(L), rng.randrange(L), rng.randrange(L)) for _ in range(500)]
    cases += [(rng.randrange(2 ** 256), rng.randrange(2 ** 256), rng.randrange(2 ** 256)) for _ in range(500)]
    for k, a, r in cases:
        out = ctypes.create_string_buffer(32)
        sc.sgc_scalar_s(k.to_bytes(32, "little"), a.to_bytes(32, "little"), r.to_bytes(32, "little"), out)
        assert int.from_bytes(out.raw, "little") == (k * a + r) % L, (k, a, r)


def test_no_gpu_fails_loudly():
    from plenum_amd import _native
    from plenum_amd.nacl_wrappers import SigningKey
    lib = _native.lib()
    with pytest.raises(ValueError, match="The seed must be exactly 32 bytes long"):
        SigningKey(bytes(31))
    with pytest.raises(ValueError, match="The seed must be exactly 32 bytes long"):
        SigningKey(bytes(33))
    if lib.pv_device_count() > 0:
        pytest.skip("a GPU is visible")
    off = np.array([0, 3], np.uint64)
    msg, sk, sig = np.zeros(3, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    assert lib.pv_sign_batch(_native._ptr(msg), _native._ptr(off), 1, _native._ptr(sk), 1, None, _native._ptr(sig)) < 0
    assert lib.pv_sign_seed_keypairs(_native._ptr(sk), 1, _native._ptr(sig), None) < 0
    assert lib.pv_sign_batch_device(None, None, 1, None, 1, None, None, None) < 0
    with pytest.raises(_native.NativeUnavailable):
        SigningKey(bytes(32))
    with pytest.raises(_native.NativeUnavailable):
        _native.sign_batch(msg, off, sk)
    with pytest.raises(_native.NativeUnavailable):
        _native.seed_keypairs(np.zeros(32, np.uint8))


def test_golden_fixture_shape():
    """tests/golden/signing.json (the reference's own DidSigner / SimpleSigner, see
    make_signing_golden.py): small, both signer kinds, requests with the ignored keys. The identities are
    checked here from the recorded public keys (no GPU); the signatures in tests/test_gpu_sign.py."""
    from plenum_amd.signing import DidIdentity, hexToFriendly
    path = os.path.join(HERE, "golden", "signing.json")
    assert os.path.getsize(path) < 100 * 1024
    with open(path) as f:
        g = json.load(f)
    assert len(g["signers"]) >= 12 and len(g["cases"]) >= 40
    assert {s["kind"] for s in g["signers"]} == {"did", "simple"}
    assert any("signature" in c["msg"] for c in g["cases"]) and any("signatures" in c["msg"] for c in g["cases"])
    for s in g["signers"]:
        assert s["seedHex"] == s["seed"]
        verraw = bytes.fromhex(s["verraw"])
        if s["kind"] == "did":
            d = DidIdentity(s["identifier_arg"], rawVerkey=verraw)
            assert (d.identifier, d.verkey, d.full_verkey) == (s["identifier"], s["verkey"], s["full_verkey"])
        else:
            assert hexToFriendly(s["verraw"]) == s["verkey"]
            assert s["identifier"] == (s["identifier_arg"] or s["verkey"])
