"""Generate tests/golden/signing.json by running the REFERENCE's own signers.

TEST INFRASTRUCTURE, run in the build container only (the reference never ships to the GPU box):
    python tests/golden/make_signing_golden.py
The reference (swcurran/indy-plenum, checked out beside this repository) is imported, never copied;
its missing third-party modules come from tests/golden/_shims as for make_golden.py (libnacl over
libsodium 1.0.18, base58). Output (JSON, data only): for ~12 seeds the DidSigner and SimpleSigner
properties (identifier, verkey, full_verkey, seedHex), and ~40 request dicts with the base58 signature
each signer's ``sign`` returns -- including dicts with ``signature`` / ``signatures`` keys, which the
two signers ignore differently.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("PLENUM_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path[:0] = [os.path.join(HERE, "_shims"), REF, ROOT]

from plenum.common.signer_did import DidSigner  # noqa: E402
from plenum.common.signer_simple import SimpleSigner  # noqa: E402


def seed_of(i):
    if i == 0:
        return bytes(32)
    if i == 1:
        return b"\xff" * 32
    return hashlib.sha256(b"signing golden seed %d" % i).digest()


def requests():
    out = []
    for j in range(20):
        req = {"identifier": "V4SGRU86Z58d6TV7PBUe6f", "reqId": 1700000000000000 + j, "protocolVersion": 2,
               "operation": {"type": "1", "dest": "Th7MpTaRZVRYnPiabds81Y", "alias": "u%08d" % j,
                             "verkey": "~7TYfekw4GUagBnBVCqPjiC"}}
        if j % 4 == 1:
            req["signature"] = "must be ignored by both signers"
        if j % 4 == 2:
            req["signatures"] = {"someone": "ignored by SimpleSigner only"}
        if j % 4 == 3:
            req["signature"] = None
            req["signatures"] = None
            req["taaAcceptance"] = {"taaDigest": "ab" * 32, "mechanism": "service_agreement", "time": 1700000000}
        if j % 5 == 0:
            req["operation"]["raw"] = "x" * (j * 13)
        if j == 7:
            req["operation"] = {"type": "100", "data": {"ü": ["€", 10 ** 30, None, True], "nested": {"b": 2, "a": 1}}}
        out.append(req)
    out.append({})
    out.append({"signature": "only"})
    return out


def main():
    signers, cases = [], []
    objs = []
    for i in range(12):
        seed = seed_of(i)
        if i % 2 == 0:
            idr = None if i % 4 == 0 else "L5AD5g65TDQr1PPHHRoiGf"
            s = DidSigner(identifier=idr, seed=seed)
            rec = {"kind": "did", "identifier_arg": idr, "full_verkey": s.full_verkey}
        else:
            idr = None if i % 4 == 1 else "an-explicit-identifier"
            s = SimpleSigner(identifier=idr, seed=seed)
            rec = {"kind": "simple", "identifier_arg": idr}
        rec.update(seed=seed.hex(), identifier=s.identifier, verkey=s.verkey, seedHex=s.seedHex.decode(),
                   verraw=s.naclSigner.verraw.hex())
        signers.append(rec)
        objs.append(s)
    reqs = requests()
    for j, req in enumerate(reqs):
        for u in ((j % 12), ((j * 5 + 1) % 12)):
            cases.append({"signer": u, "msg": req, "sig": objs[u].sign(req)})
    with open(os.path.join(HERE, "signing.json"), "w") as f:
        json.dump({"signers": signers, "cases": cases}, f, indent=1, ensure_ascii=True)
    print("wrote signing.json: %d signers, %d cases" % (len(signers), len(cases)))


if __name__ == "__main__":
    main()
