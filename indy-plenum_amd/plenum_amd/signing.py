"""Request signers: drop-ins for ``plenum/common/signer_did.py`` and ``signer_simple.py``, and the
batch entry they lack.

  DidIdentity  (signer_did.py:14-73)    identifier / verkey / full_verkey with the reference's
                                        constructor rules (abbreviated '~' verkeys, cryptonyms).
  DidSigner    (signer_did.py:76-129)   ``sign(msg: dict) -> str``: base58 signature over
                                        ``serialize_msg_for_signing(msg)`` minus the top-level
                                        ``signature`` key.
  SimpleSigner (signer_simple.py:13-70) the same minus ``signature`` AND ``signatures``; the verkey is
                                        the full key, the identifier defaults to it.
  sign_requests(signers, msgs)          the batch form: every dict serialized with each signer's own
                                        rule, ONE pv_sign_batch call for all of them (distinct signers
                                        deduplicated into the key table), base58 results.

Signatures are computed by the HIP engine, byte-identical to libsodium. A single ``sign`` is one small
GPU launch, slower than libsodium on a CPU; ``sign_requests`` is the integration, as
``authenticate_batch`` is for verification. Not hardened against side channels (csrc/sign_core.h):
for load generation, fixtures and test wallets, not for custody of production keys.
"""
from binascii import hexlify, unhexlify

import numpy as np

from . import _native
from .base58 import b58decode, b58encode
from .nacl_wrappers import Signer as NaclSigner, SigningKey, randombytes
from .serialization import serialize_msg_for_signing

SIG = "signature"    # f.SIG.nm
SIGS = "signatures"  # f.SIGS.nm


def rawToFriendly(raw):
    return b58encode(raw).decode("utf-8")


def friendlyToRaw(f):
    return b58decode(f)


def hexToFriendly(hx):
    if isinstance(hx, str):
        hx = hx.encode()
    return rawToFriendly(unhexlify(hx))


class DidIdentity:
    abbr_prfx = '~'

    def __init__(self, identifier, verkey=None, rawVerkey=None):
        self.abbreviated = None
        if (verkey is None or verkey == '') and (rawVerkey is None or rawVerkey == ''):
            if identifier:
                self._identifier = identifier
                self._verkey = None if (verkey is None and rawVerkey is None) else ''
                return

        if not ((verkey or rawVerkey) and not (verkey and rawVerkey)):
            raise ValueError("Both verkey {} and rawVerkey {} can't be specified".format(verkey, rawVerkey))

        if identifier:
            self._identifier = identifier
            if rawVerkey:
                self._verkey = rawToFriendly(rawVerkey)
                self.abbreviated = False
            elif verkey.startswith("~"):
                self._verkey = verkey[1:]
                self.abbreviated = True
            else:
                self._verkey = verkey
                self.abbreviated = False
        else:
            verraw = rawVerkey or friendlyToRaw(verkey)
            self._identifier = rawToFriendly(verraw[:16])
            self._verkey = rawToFriendly(verraw[16:])
            self.abbreviated = True

    @property
    def identifier(self):
        return self._identifier

    @property
    def verkey(self):
        if self._verkey is None:
            return None
        return self.abbr_prfx + self._verkey if self.abbreviated else self._verkey

    @property
    def full_verkey(self):
        if self.abbreviated:
            return rawToFriendly(friendlyToRaw(self.identifier) + friendlyToRaw(self.verkey[1:]))
        return self.verkey


class _SeedSigner:
    """What both signers share: the seed, its key pair, and signing of a serialized request."""
    ignored_keys = ()

    def _init_keys(self, seed):
        self.seed = seed if seed else randombytes(32)  # should be stored securely/privately
        self.sk = SigningKey(seed=self.seed)
        self.naclSigner = NaclSigner(self.sk)

    @property
    def alias(self):
        return self._alias

    @property
    def seedHex(self) -> bytes:
        return hexlify(self.seed)

    def serialize(self, msg) -> bytes:
        return serialize_msg_for_signing(msg, topLevelKeysToIgnore=list(self.ignored_keys))

    def sign(self, msg) -> str:
        bsig = self.naclSigner.signature(self.serialize(msg))
        return b58encode(bsig).decode("utf-8")


class DidSigner(DidIdentity, _SeedSigner):
    ignored_keys = (SIG,)

    def __init__(self, identifier=None, seed=None, alias=None):
        self._init_keys(seed)
        DidIdentity.__init__(self, identifier, rawVerkey=self.naclSigner.verraw)
        self._alias = alias

    @_SeedSigner.alias.setter
    def alias(self, value):
        self._alias = value


class SimpleSigner(_SeedSigner):
    ignored_keys = (SIG, SIGS)

    def __init__(self, identifier=None, seed=None, alias=None):
        self._init_keys(seed)
        # the public key used to verify signatures (shared with the recipient beforehand)
        self.verkey = hexToFriendly(hexlify(self.naclSigner.verraw))
        self._identifier = identifier or self.verkey
        self._alias = alias

    @property
    def identifier(self):
        return self._identifier


def sign_requests(signers, msgs):
    """``[signers[i].sign(msgs[i]) for i in ...]`` in one GPU call.

    signers: one signer for every message, or a sequence of DidSigner / SimpleSigner objects as long as
    msgs (the same object may repeat: distinct signers share one entry of the key table). Each dict is
    serialized with its signer's own rule. Returns the base58 signatures."""
    msgs = list(msgs)
    if isinstance(signers, _SeedSigner):
        signers = [signers] * len(msgs)
    signers = list(signers)
    if len(signers) != len(msgs):
        raise ValueError("sign_requests: one signer per message")
    if not msgs:
        return []
    table, sks, idx = {}, [], np.zeros(len(msgs), np.uint32)
    for i, s in enumerate(signers):
        u = table.get(id(s))
        if u is None:
            u = table[id(s)] = len(sks)
            sks.append(s.sk._signing_key)
        idx[i] = u
    blob, off = _native._blob([s.serialize(m) for s, m in zip(signers, msgs)])
    sigs = _native.sign_batch(blob, off, np.frombuffer(b"".join(sks), np.uint8), idx)
    return [b58encode(sig.tobytes()).decode("utf-8") for sig in sigs]
