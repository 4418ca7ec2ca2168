"""GPU parity of the device ingress front end (pv_ingress_verify): base58 decode
of every signature, DidVerifier key resolution per signer, device-side sm assembly, verification.

Expected values come from the checkers, never from the product: base58 from oracle/base58_ref.py
(the restatement pinned by the reference's KAT), key resolution from the reference's own
DidVerifier outcomes (tests/golden/didverifier.json) and from pv_resolve_verkeys (host C++, pinned
against the same goldens in test_abi.py), verdicts from libsodium 1.0.18 crypto_sign_open on
b58decode(sig) || M."""
import json
import os

import numpy as np
import pytest

from oracle.base58_ref import b58decode as ref_b58decode, b58encode as ref_b58encode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    _native.ensure_device()
    return _native


def host_key_status(native, idrs, vks):
    """pv_resolve_verkeys on the host (golden-pinned) -> (status, pk) per signer."""
    n = len(idrs)
    ib, io = native._blob(idrs)
    vb, vo = native._blob([v if v is not None else b"" for v in vks])
    has = np.array([v is not None for v in vks], np.uint8)
    pk = np.zeros((n, 32), np.uint8)
    st = np.zeros(n, np.uint8)
    native.check(native.lib().pv_resolve_verkeys(ib.ctypes.data, io.ctypes.data, vb.ctypes.data, vo.ctypes.data,
                                                 has.ctypes.data, n, pk.ctypes.data, st.ctypes.data),
                 "pv_resolve_verkeys")
    return st, pk


def expected(sodium, native, sigs, msgs, msg_idx, signer_idx, idrs, vks):
    kst, kpk = host_key_status(native, idrs, vks)
    status, verdict = [], []
    for sig, mi, si in zip(sigs, msg_idx, signer_idx):
        try:
            raw = ref_b58decode(sig)
        except ValueError:
            status.append(1)
            verdict.append(False)
            continue
        if len(raw) > 96:
            status.append(2)
            verdict.append(False)
            continue
        if kst[si]:
            status.append(16 + int(kst[si]))
            verdict.append(False)
            continue
        status.append(0)
        verdict.append(sodium.sign_open_ok(raw + msgs[mi], kpk[si].tobytes()))
    return np.array(status, np.uint8), np.array(verdict, bool)


def signer_forms(sodium, rng, count):
    """Signers in every verkey form the reference accepts: DidSigner (DID + '~' abbreviated
    verkey), cryptonym (identifier = full key, no verkey), full verkey, hex verkey."""
    out = []
    for i in range(count):
        pk, sk = sodium.seed_keypair(rng.bytes(32))
        form = i % 4
        if form == 0:
            idr, vk = ref_b58encode(pk[:16]), b"~" + ref_b58encode(pk[16:])
        elif form == 1:
            idr, vk = ref_b58encode(pk), None
        elif form == 2:
            idr, vk = ref_b58encode(pk[:16]), ref_b58encode(pk)
        else:
            idr, vk = ref_b58encode(pk[:16]), ref_b58encode(pk.hex().encode())
        out.append((idr, vk, sk))
    return out


def signature_variant(kind, sig, rng):
    """Encodings of one signature covering every b58decode / sm-assembly rule."""
    if kind == 1:
        return ref_b58encode(sig[:63])  # shifts the signature / message split point
    if kind == 2:
        return ref_b58encode(sig + b"\x07")
    if kind == 3:
        return ref_b58encode(sig)[:-1] + b"0"  # character outside the alphabet
    if kind == 4:
        return b""
    if kind == 5:
        return ref_b58encode(b"\0\0" + sig)  # leading '1's
    if kind == 6:
        return ref_b58encode(sig) + b" \t\n"  # trailing ASCII whitespace
    if kind == 7:
        return ref_b58encode(rng.bytes(97))  # decodes to more than 96 bytes
    if kind == 8:
        return ref_b58encode(sig[:1] + bytes([sig[1] ^ 4]) + sig[2:])  # one bit changed
    if kind == 9:
        return b"1" * 100  # 100 zero bytes
    if kind == 10:
        return b"\xc3\xa9" + ref_b58encode(sig)  # non-ASCII byte
    return ref_b58encode(sig)


# signer table rows whose key resolution fails in each documented way (statuses 17..20)
ODD_SIGNERS = [
    (b"99BgFBg35BehzfSADV5nM4", None), (b"99BgFBg35BehzfSADV5nM4", b""), (b"0OIl", b"~8zH9ZSyZTFPGJ4ZPL5Rvxx"),
    (b"99BgFBg35BehzfSADV5nM4", b"~0OIl"), (b"99BgFBg35BehzfSADV5nM4", b"~2"), (b"", None), (b"", b""),
    (b"", b"   "), (b"99BgFBg35BehzfSADV5nM4", b"~"), (b"  ", b"~" + ref_b58encode(bytes(range(1, 33)))),
    (b"1111111111111111", b"~1111111111111111"), (b"FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF", None)]


def test_signature_and_key_variants(native, sodium):
    rng = np.random.default_rng(21)
    signers = signer_forms(sodium, rng, 16)
    good = len(signers)
    idrs = [s[0] for s in signers] + [b[0] for b in ODD_SIGNERS]
    vks = [s[1] for s in signers] + [b[1] for b in ODD_SIGNERS]
    msgs = [rng.bytes(int(rng.integers(0, 400))) for _ in range(40)]
    sigs, msg_idx, signer_idx = [], [], []
    for j in range(600):
        mi = int(rng.integers(0, len(msgs)))
        si = int(rng.integers(0, good)) if j % 5 else int(rng.integers(0, len(idrs)))
        sig = sodium.sign_detached(msgs[mi], signers[si][2]) if si < good else rng.bytes(64)
        sigs.append(signature_variant(j % 13, sig, rng))
        msg_idx.append(mi)
        signer_idx.append(si)
    st, v = native.ingress_verify(sigs, msgs, msg_idx, signer_idx, idrs, vks)
    want_st, want_v = expected(sodium, native, sigs, msgs, msg_idx, signer_idx, idrs, vks)
    diff = np.nonzero((st != want_st) | (v != want_v))[0]
    assert len(diff) == 0, [(i, sigs[i], signer_idx[i], st[i], want_st[i], v[i], want_v[i]) for i in diff[:6]]
    assert want_v.sum() > 150 and (want_st == 0).sum() > 300
    assert set(int(x) for x in want_st) >= {0, 1, 2, 17, 18, 19, 20}


def test_key_status_matches_reference_golden(native):
    """Device key resolution vs the reference's DidVerifier outcomes (every ASCII golden case)."""
    with open(os.path.join(ROOT, "tests", "golden", "didverifier.json")) as f:
        cases = json.load(f)
    usable = [c for c in cases if all(isinstance(x, str) or x is None for x in (c["verkey"], c["identifier"]))
              and all((x or "").isascii() and (x or "") == (x or "").rstrip() for x in (c["verkey"], c["identifier"]))]
    idrs = [(c["identifier"] or "").encode() for c in usable]
    vks = [c["verkey"].encode() if c["verkey"] is not None else None for c in usable]
    n = len(usable)
    sig = ref_b58encode(b"\x01" * 64)  # decodes, so the status is 16 + the key status
    st, _ = native.ingress_verify([sig] * n, [b"m" * 10], [0] * n, list(range(n)), idrs, vks)
    for i, c in enumerate(usable):
        out = c["out"]
        k = int(st[i]) - 16 if st[i] else 0
        if "exc" in out:
            assert k in {"ValueError": (1, 4), "InvalidKey": (2,)}[out["exc"]], (c, st[i])
        elif out["value"]["raw"] is None:
            assert k == 3, c
        else:
            assert k == 0, c


def test_many_requests_multi_signature(native, sodium):
    """Three endorser signatures over one M per request (authenticate_multi), 64 signers in every
    verkey form, 49,152 verifications over many scan tiles; every verdict True except the flipped
    ones."""
    rng = np.random.default_rng(5)
    signers = signer_forms(sodium, rng, 64)
    idrs = [s[0] for s in signers]
    vks = [s[1] for s in signers]
    nreq = 1 << 14
    msgs = [b"identifier:%d|operation:dest:x|reqId:%d" % (i % 97, i) + rng.bytes(int(rng.integers(200, 300)))
            for i in range(nreq)]
    sigs, mi, si, flipped = [], [], [], []
    for r in range(nreq):
        for k in range(3):
            s = (3 * r + k) % 64
            sig = sodium.sign_detached(msgs[r], signers[s][2])
            t = (r * 3 + k) % 101 == 0
            if t:
                sig = bytes([sig[0] ^ 1]) + sig[1:]
            sigs.append(ref_b58encode(sig))
            mi.append(r)
            si.append(s)
            flipped.append(t)
    st, v = native.ingress_verify(sigs, msgs, mi, si, idrs, vks)
    assert (st == 0).all()
    assert np.array_equal(v, ~np.array(flipped))


def test_out_of_range_indices_are_errors(native):
    with pytest.raises(native.NativeError):
        native.ingress_verify([b"2"], [b"m"], [5], [0], [b"99BgFBg35BehzfSADV5nM4"], [None])
    with pytest.raises(native.NativeError):
        native.ingress_verify([b"2"], [b"m"], [0], [3], [b"99BgFBg35BehzfSADV5nM4"], [None])


# ------------------------------------------------------------------ the workspace: streams, growth

@pytest.fixture(scope="module")
def tile_pool(native, sodium):
    """64 signed requests (8 signers in every verkey form plus two that do not resolve: an identifier that is not base58, status 16 + 4; a verkey of a wrong length, 16 + 2) with
    a tampered signature, a signature by the malformed-key signer and a character outside the alphabet
    among the first 16, and what the reference path gives for each. Computed once; the tests below
    tile it through msg_idx / signer_idx and index these expectations the same way."""
    from types import SimpleNamespace
    rng = np.random.default_rng(77)
    signers = signer_forms(sodium, rng, 8)
    idrs = [s[0] for s in signers] + [ODD_SIGNERS[2][0], ODD_SIGNERS[4][0]]  # identifier not base58; key of a wrong length
    vks = [s[1] for s in signers] + [ODD_SIGNERS[2][1], ODD_SIGNERS[4][1]]
    msgs = [b"reqId:%d|" % i + rng.bytes(int(rng.integers(0, 90))) for i in range(64)]
    sigs, signer_idx = [], []
    for i in range(64):
        si = {5: 8, 9: 9}.get(i, i % 8)
        sig = sodium.sign_detached(msgs[i], signers[i % 8][2])
        sigs.append(signature_variant({3: 8, 7: 3, 11: 1}.get(i, 0), sig, rng))
        signer_idx.append(si)
    st, v = expected(sodium, native, sigs, msgs, list(range(64)), signer_idx, idrs, vks)
    assert st[5] == 20 and st[9] == 18 and st[7] == 1 and st[3] == 0 and not v[3] and v.sum() == 59, (st, v)
    p = SimpleNamespace(st=st, v=v, signer_idx=np.array(signer_idx, np.uint32))
    p.msg_blob, p.msg_off = native._blob(msgs)
    p.idr_blob, p.idr_off = native._blob(idrs)
    p.vk_blob, p.vk_off = native._blob([k if k is not None else b"" for k in vks])
    p.vk_present = np.array([k is not None for k in vks], np.uint8)
    p.sig_len = np.array([len(s) for s in sigs], np.uint64)
    p.sig_rows = np.zeros((64, int(p.sig_len.max())), np.uint8)
    for i, s in enumerate(sigs):
        p.sig_rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    return p


def tiled(p, order):
    """The pool's requests in `order` (pool indices): per-verification signature blob and offsets, the
    index arrays, the summed message bytes, and the expected status / verdict."""
    from types import SimpleNamespace
    order = np.asarray(order, np.int64)
    lens = p.sig_len[order]
    keep = np.arange(p.sig_rows.shape[1])[None, :] < lens[:, None]
    t = SimpleNamespace(n=len(order), sig_blob=p.sig_rows[order][keep], sig_off=np.zeros(len(order) + 1, np.uint64),
                        msg_idx=order.astype(np.uint32), signer_idx=p.signer_idx[order], st=p.st[order], v=p.v[order])
    np.cumsum(lens, out=t.sig_off[1:])
    t.msg_bytes = int((p.msg_off[1:] - p.msg_off[:-1])[order].sum())
    return t


def host_entry(native, p, t):
    return native.ingress_verify_arrays(t.sig_blob, t.sig_off, p.msg_blob, p.msg_off, t.msg_idx, t.signer_idx, p.idr_blob,
                                        p.idr_off, p.vk_blob, p.vk_off, p.vk_present)


def assert_as_reference(got, t, what):
    st, v = got
    diff = np.nonzero((st != t.st) | (v != t.v))[0]
    assert len(diff) == 0, (what, [(int(i), int(st[i]), int(t.st[i]), bool(v[i]), bool(t.v[i])) for i in diff[:6]])


def test_two_caller_streams_then_destroy(native, tile_pool):
    """pv_ingress_verify_device with 2^17 verifications in one order on stream s1 and in another order on
    stream s2, every buffer uploaded beforehand and nothing between the calls: each call's status bytes and verdict bits are the reference's for
    its order (the workspace is handed over, not shared). Then s2, the last user, is destroyed, and a call
    on the library stream and a host-buffer call (16 verifications each) still give the reference's."""
    import ctypes
    L, p = native.lib(), tile_pool
    n = 1 << 17
    i = np.arange(n)
    orders = [i % 64, ((i * 37 + 11) % 64)[::-1].copy()]
    bufs = []

    def dev(a, slack=0):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        a = np.concatenate([a, np.zeros(slack + 8, np.uint8)])  # the host entry stages its blobs with room to read ahead
        ptr = ctypes.c_void_p()
        native.check(L.pv_dev_alloc(ctypes.byref(ptr), a.size), "pv_dev_alloc")
        bufs.append(ptr)
        native.check(L.pv_memcpy_h2d(ptr, native._ptr(a), a.size), "pv_memcpy_h2d")
        return ptr

    def upload(t):
        """Everything one call reads and writes, on the device before any call is issued (pv_dev_alloc and
        pv_memcpy_h2d wait for the engine, so none of them may stand between the two calls)."""
        t.d_in = [dev(t.sig_blob), dev(t.sig_off), dev(t.msg_idx), dev(t.signer_idx)]
        t.d_out = dev(np.full(t.n, 0xEE, np.uint8)), dev(np.zeros((t.n + 63) // 64, np.uint64))
        return t

    def enqueue(t, stream):
        return L.pv_ingress_verify_device(*t.d_in, t.n, d_msg, d_moff, 64, t.msg_bytes, d_idr, d_ioff, d_vk, d_voff, d_vkp,
                                          len(p.vk_present), *t.d_out, stream)

    def read(t, d_st, d_words):
        st, words = np.zeros(t.n, np.uint8), np.zeros((t.n + 63) // 64, np.uint64)
        native.check(L.pv_memcpy_d2h(native._ptr(st), d_st, st.nbytes), "pv_memcpy_d2h")
        native.check(L.pv_memcpy_d2h(native._ptr(words), d_words, words.nbytes), "pv_memcpy_d2h")
        return st, np.unpackbits(words.view(np.uint8), bitorder="little")[:t.n].astype(bool)

    s1, s2 = ctypes.c_void_p(), ctypes.c_void_p()
    native.check(L.pv_stream_create(ctypes.byref(s1)), "pv_stream_create")
    native.check(L.pv_stream_create(ctypes.byref(s2)), "pv_stream_create")
    try:
        d_msg, d_moff = dev(p.msg_blob, native.PV_BLOB_SLACK), dev(p.msg_off)
        d_idr, d_ioff, d_vk, d_voff, d_vkp = dev(p.idr_blob), dev(p.idr_off), dev(p.vk_blob), dev(p.vk_off), dev(p.vk_present)
        t1, t2, t3 = upload(tiled(p, orders[0])), upload(tiled(p, orders[1])), upload(tiled(p, np.arange(16)))
        assert not np.array_equal(t1.st, t2.st) and not np.array_equal(t1.v, t2.v)
        assert t1.msg_bytes == t2.msg_bytes  # the second call finds every workspace array large enough: no allocation
        rc1 = enqueue(t1, s1)
        rc2 = enqueue(t2, s2)  # straight after the first: nothing in between, not even a status check
        native.check(rc2, "pv_ingress_verify_device on s2")
        assert rc1 == native.PV_OK
        native.check(L.pv_stream_sync(s1), "pv_stream_sync")
        native.check(L.pv_stream_sync(s2), "pv_stream_sync")
        assert_as_reference(read(t1, *t1.d_out), t1, "order 1 on s1")
        assert_as_reference(read(t2, *t2.d_out), t2, "order 2 on s2")
        native.check(L.pv_stream_destroy(s2), "pv_stream_destroy")  # the workspace's last user
        s2 = None
        native.check(enqueue(t3, None), "pv_ingress_verify_device on the library stream")
        native.check(L.pv_stream_sync(None), "pv_stream_sync")
        assert_as_reference(read(t3, *t3.d_out), t3, "16 on the library stream after the destroy")
        assert_as_reference(host_entry(native, p, t3), t3, "16 through host buffers")
        assert set(int(x) for x in t3.st) == {0, 1, 18, 20} and not t3.v[3] and t3.v.sum() == 11
    finally:
        for s in (s1, s2):
            if s is not None:
                native.check(L.pv_stream_destroy(s), "pv_stream_destroy")
        for b in bufs:
            L.pv_dev_free(b)


def test_workspace_grows_and_is_reused(native, tile_pool):
    """Host-buffer calls of 16, then 65,600 (above the floor of 2^16 verifications every per-verification
    array starts with, so each one is allocated again), then 16 verifications: all as the reference."""
    p = tile_pool
    for order in (np.arange(16), (np.arange(65600) * 7 + 3) % 64, 15 - np.arange(16)):
        t, n = tiled(p, order), len(order)
        assert_as_reference(host_entry(native, p, t), t, n)
        assert len(set(int(x) for x in t.st)) == 4 and 0 < t.v.sum() < n
