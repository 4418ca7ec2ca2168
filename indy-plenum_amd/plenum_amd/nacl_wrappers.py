"""Drop-in for ``stp_core/crypto/nacl_wrappers.py``: the verification half and the signing half.

  VerifyKey (nacl_wrappers.py:62-108)   32-byte Ed25519 public key; ``verify(smessage, signature=None)``
                                        returns the message or raises ValueError, like libnacl.
  Verifier  (nacl_wrappers.py:212-242)  ``verify(signature, msg) -> bool``; never raises on a bad
                                        signature; a falsy key makes every verify False.
  crypto_sign_open                      libnacl 1.6.1 ``crypto_sign_open(sm, vk)`` semantics
                                        (ValueError('Invalid public key') / ('Failed to validate
                                        message')), computed by the HIP engine.

  SigningKey (nacl_wrappers.py:111-178) 32-byte seed; ``verify_key``, ``generate()``, ``sign(message,
                                        encoder) -> SignedMessage``; ``bytes(key)`` is the seed.
  Signer    (nacl_wrappers.py:181-209)  ``keyhex`` / ``keyraw`` (the seed), ``verhex`` / ``verraw``,
                                        ``sign(msg)``, ``signature(msg)``.
  crypto_sign_seed_keypair, crypto_sign libnacl semantics, computed by the HIP engine, byte-identical to
                                        libsodium. One call is one small launch (slower than libsodium's
                                        20-40 us on a CPU): batches go through
                                        ``plenum_amd.signing.sign_requests``. The signer is not hardened
                                        against side channels (csrc/sign_core.h): load generation,
                                        fixtures and test wallets, not custody of production keys.

Every verification goes to the GPU engine. Inside an ``authenticate_batch`` call the verdicts were
already computed in one batched launch and are looked up (plenum_amd.batch); outside one, a
single-request launch is made. There is no CPU fallback: without the library/GPU this raises
``plenum_amd._native.NativeUnavailable``.
"""
import binascii

import os

import numpy as np

from . import _native, batch

crypto_sign_PUBLICKEYBYTES = 32
crypto_sign_BYTES = 64
crypto_sign_SEEDBYTES = 32
crypto_sign_SECRETKEYBYTES = 64


def randombytes(size):
    return os.urandom(size)


class RawEncoder:
    @staticmethod
    def encode(data):
        return data

    @staticmethod
    def decode(data):
        return data


class HexEncoder:
    @staticmethod
    def encode(data):
        return binascii.hexlify(data)

    @staticmethod
    def decode(data):
        return binascii.unhexlify(data)


class Encodable:
    def encode(self, encoder=RawEncoder):
        return encoder.encode(bytes(self))


def crypto_sign_open(sm, vk):
    """libnacl.crypto_sign_open: returns the message part of ``sm`` or raises ValueError."""
    if len(vk) != crypto_sign_PUBLICKEYBYTES:
        raise ValueError('Invalid public key')
    sm = bytes(sm)
    if not batch.verdict(bytes(vk), sm):
        raise ValueError('Failed to validate message')
    return sm[crypto_sign_BYTES:]


def crypto_sign_seed_keypair(seed):
    """libnacl.crypto_sign_seed_keypair: (public key, 64-byte secret key = seed || public key)."""
    if len(seed) != crypto_sign_SEEDBYTES:
        raise ValueError('Invalid Seed')
    pks, sks = _native.seed_keypairs(np.frombuffer(bytes(seed), np.uint8))
    return pks.tobytes(), sks.tobytes()


def crypto_sign(msg, sk):
    """libnacl.crypto_sign: the 64-byte signature followed by the message."""
    if len(sk) != crypto_sign_SECRETKEYBYTES:
        raise ValueError('Invalid secret key')
    msg = bytes(msg)
    sig = _native.sign_batch(np.frombuffer(msg or b"\0", np.uint8), np.array([0, len(msg)], np.uint64),
                             np.frombuffer(bytes(sk), np.uint8))
    return sig.tobytes() + msg


class SignedMessage(bytes):
    """The signed message (signature + message) with its two parts."""

    @classmethod
    def _from_parts(cls, signature, message, combined):
        obj = cls(combined)
        obj._signature = signature
        obj._message = message
        return obj

    @property
    def signature(self):
        return self._signature

    @property
    def message(self):
        return self._message


class VerifyKey(Encodable):
    def __init__(self, key, encoder=RawEncoder):
        key = encoder.decode(key)
        if len(key) != crypto_sign_PUBLICKEYBYTES:
            raise ValueError("The key must be exactly %s bytes long" % crypto_sign_PUBLICKEYBYTES)
        self._key = key

    def __bytes__(self):
        return self._key

    def verify(self, smessage, signature=None, encoder=RawEncoder):
        if signature is not None:
            smessage = signature + smessage
        smessage = encoder.decode(smessage)
        return crypto_sign_open(smessage, self._key)


class SigningKey(Encodable):
    def __init__(self, seed, encoder=RawEncoder):
        seed = encoder.decode(seed)
        if len(seed) != crypto_sign_SEEDBYTES:
            raise ValueError("The seed must be exactly %d bytes long" % crypto_sign_SEEDBYTES)
        public_key, secret_key = crypto_sign_seed_keypair(seed)
        self._seed = seed
        self._signing_key = secret_key
        self.verify_key = VerifyKey(public_key)

    def __bytes__(self):
        return self._seed

    @classmethod
    def generate(cls):
        return cls(randombytes(crypto_sign_SEEDBYTES), encoder=RawEncoder)

    def sign(self, message, encoder=RawEncoder):
        raw_signed = crypto_sign(message, self._signing_key)
        signature = encoder.encode(raw_signed[:crypto_sign_BYTES])
        message = encoder.encode(raw_signed[crypto_sign_BYTES:])
        signed = encoder.encode(raw_signed)
        return SignedMessage._from_parts(signature, message, signed)


class Signer:
    def __init__(self, key=None):
        if key:
            if not isinstance(key, SigningKey):  # a seed, raw or hex
                if len(key) == 32:
                    key = SigningKey(seed=key, encoder=RawEncoder)
                else:
                    key = SigningKey(seed=key, encoder=HexEncoder)
        else:
            key = SigningKey.generate()
        self.key = key
        self.keyhex = self.key.encode(HexEncoder)  # the seed
        self.keyraw = self.key.encode(RawEncoder)
        self.verhex = self.key.verify_key.encode(HexEncoder)
        self.verraw = self.key.verify_key.encode(RawEncoder)

    def sign(self, msg):
        return self.key.sign(msg)

    def signature(self, msg):
        return self.key.sign(msg).signature


class Verifier:
    def __init__(self, key=None):
        if key and not isinstance(key, VerifyKey):
            key = VerifyKey(key, RawEncoder) if len(key) == 32 else VerifyKey(key, HexEncoder)
        self.key = key
        if isinstance(key, VerifyKey):
            self.keyhex = key.encode(HexEncoder)
            self.keyraw = key.encode(RawEncoder)
        else:
            self.keyhex = ''
            self.keyraw = ''

    def verify(self, signature, msg):
        if not self.key:
            return False
        try:
            self.key.verify(signature + msg)
        except ValueError:
            return False
        return True
