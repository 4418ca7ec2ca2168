"""GPU: table reuse (pv_table_reuse). The comb tables a keyed chunk of more than 65,536 requests
builds stay in the workspace, listed in a device-side directory, and later chunks and calls that carry
the same keys read them instead of building them again. A hit changes where a table is read from and
nothing else: the verdicts stay libsodium's, the split of a chunk stays what it is with reuse off.

Every batch mixes in tampered records and three keys that fail libsodium's key checks (small order,
non-canonical, off the curve), each with as many requests as the signers, so each gets a table (with
the failing flag, which the directory has to keep). Expected verdicts are libsodium's
(oracle.cpu_verdicts over libsodium.so.23), never the engine's.

Shapes: the smallest chunk whose tables are listed has 65,537 requests; the batches here have 64 keys
x 1,100 short-message requests. A key's 1,100 records are 110 signed messages repeated (verification
does not care, signing on the CPU does)."""
import ctypes
import threading

import numpy as np
import pytest

from vectors import BLACKLIST, P, VectorGen, pack

pytestmark = pytest.mark.gpu

PER_KEY = 1100
DISTINCT = 110  # signed messages per key
NKEYS = 64      # keys of a batch, the three bad ones included


@pytest.fixture(scope="module")
def nat():
    from plenum_amd import _native
    _native.ensure_device()
    _native.set_path(_native.PV_PATH_AUTO)
    yield _native
    _native.set_path(_native.PV_PATH_AUTO)
    _native.table_reuse(True, _native.PV_TABLE_REUSE_CAP)


@pytest.fixture()
def fresh(nat):
    """Reuse on at the default capacity, nothing kept from earlier tests."""
    nat.table_reuse(False)
    nat.table_reuse(True, nat.PV_TABLE_REUSE_CAP)
    return nat


def _bad_keys(v):
    """Variant v of (small-order, non-canonical, off-curve) keys; different v give different keys."""
    small = bytes(BLACKLIST[v % len(BLACKLIST)])
    noncanon = (P + 1 + v).to_bytes(32, "little")
    d = (-121665 * pow(121666, P - 2, P)) % P
    y = 1000 + 100000 * v
    while True:  # y with (y^2 - 1) / (d y^2 + 1) a non-square
        y += 1
        t = (y * y - 1) * pow((d * y * y + 1) % P, P - 2, P) % P
        if t != 0 and pow(t, (P - 1) // 2, P) != 1:
            break
    return [small, noncanon, y.to_bytes(32, "little")]


class _Signers:
    """Key i of the module's signer pool and its signed records, made once."""

    def __init__(self, sodium, oracle):
        self.sodium = sodium
        self.g = VectorGen(sodium, oracle, seed=77)
        self.recs = {}

    def records(self, i, distinct):
        have = self.recs.get(i)
        if have is None or len(have[1]) < distinct:
            pk, sk = self.g.key(10000 + i)
            rng = np.random.default_rng(i)
            sms = []
            for _ in range(distinct):
                m = rng.bytes(int(rng.integers(0, 48)))
                sms.append(self.sodium.sign_detached(m, sk) + m)
            have = self.recs[i] = (pk, sms)
        return have[0], have[1][:distinct]


@pytest.fixture(scope="module")
def signers(sodium, oracle):
    return _Signers(sodium, oracle)


_batches = {}


def _batch(signers, key_ids, per_key=PER_KEY, bad=0, distinct=DISTINCT, seed=0):
    """(blob, off, pks, libsodium's verdicts) of per_key requests for every signer of key_ids and for
    the three bad keys of variant `bad` (None: no bad keys), ~2 % of the records tampered, shuffled.
    Built once per shape and left unchanged."""
    from oracle.oracle import cpu_verdicts
    tag = (tuple(key_ids), per_key, bad, distinct, seed)
    if tag in _batches:
        return _batches[tag]
    rng = np.random.default_rng(1000 + seed)
    cases = []
    for i in key_ids:
        pk, sms = signers.records(i, min(distinct, per_key))
        cases += [(sms[r % len(sms)], pk) for r in range(per_key)]
    if bad is not None:
        _, sms = signers.records(key_ids[0], min(distinct, per_key))
        for pk in _bad_keys(bad):
            cases += [(sms[r % len(sms)], pk) for r in range(per_key)]
    for i in rng.choice(len(cases), len(cases) // 50, replace=False):
        sm = bytearray(cases[i][0])
        sm[int(rng.integers(0, len(sm)))] ^= 1 << int(rng.integers(0, 8))
        cases[i] = (bytes(sm), cases[i][1])
    order = rng.permutation(len(cases))
    blob, off, pks = pack([cases[i] for i in order])
    want = cpu_verdicts(blob, off, pks)
    want.setflags(write=False)
    _batches[tag] = (blob, off, pks, want)
    return _batches[tag]


K1 = list(range(0, NKEYS - 3))            # 61 signers + 3 bad keys (variant 0) = 64 comb keys
K2 = list(range(100, 100 + NKEYS - 3))    # disjoint, with bad keys of variant 1


def _run(nat, b, what=""):
    blob, off, pks, want = b
    got = nat.verify_sm_batch(blob, off, pks)
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:10])


def _delta(nat, before):
    return tuple(int(a) - int(b) for a, b in zip(nat.table_reuse_stats(), before))


def test_same_keys_twice(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    assert len(b[3]) == 70400 and 0 < (~b[3]).sum() < len(b[3])
    assert b[3].sum() > 60 * PER_KEY * 0.9  # the signers' untampered records verify
    s0 = nat.table_reuse_stats()
    _run(nat, b, "first")
    split1, path1 = nat.last_split(), nat.last_path()
    assert split1 == (NKEYS, NKEYS, 70400)
    assert _delta(nat, s0) == (0, NKEYS, 0)
    _run(nat, b, "second")
    assert _delta(nat, s0) == (NKEYS, NKEYS, 0)
    assert nat.last_split() == split1 and nat.last_path() == path1


def test_half_overlap(fresh, signers):
    nat = fresh
    _run(nat, _batch(signers, K1), "first")
    s0 = nat.table_reuse_stats()
    # 32 of the first call's keys (29 signers + its 3 bad keys) and 32 new signers
    _run(nat, _batch(signers, K1[:29] + list(range(200, 232)), seed=1), "half")
    assert _delta(nat, s0) == (32, 32, 0)


@pytest.mark.parametrize("nk,per", [(1600, 44), (2200, 32)])
def test_candidacy_unchanged(fresh, signers, nk, per):
    """Resident keys with fewer than PV_COMB_MIN_REQ requests in the chunk: 1,600 keys x 44 (at most
    2,048 keys: every key is a comb key whether reuse is on or not) and 2,200 keys x 32 (no key is)."""
    nat = fresh
    ids = K1 + list(range(1000, 1000 + nk - NKEYS))
    many = _batch(signers, ids, per_key=per, distinct=4, seed=2)
    assert len(many[3]) == 70400
    nat.table_reuse(False)
    _run(nat, many, "reuse off")
    split_off = nat.last_split()
    assert split_off == ((nk, nk, 70400) if nk <= 2048 else (nk, 0, 0))
    nat.table_reuse(True)
    _run(nat, _batch(signers, K1), "first")
    _run(nat, many, "resident keys below the threshold")
    assert nat.last_split() == split_off


def test_small_chunks_between_dense(fresh, signers):
    from test_gpu_robustness import _Dev
    nat = fresh
    dense = _batch(signers, K1)
    _run(nat, dense, "dense 1")
    s0 = nat.table_reuse_stats()
    # 8,192 requests over the 64 keys and 64 others: all-comb, its tables are not listed
    _run(nat, _batch(signers, K1 + list(range(300, 364)), per_key=64, seed=3), "8192")
    assert nat.last_split() == (128, 128, 8192)
    assert _delta(nat, s0) == (NKEYS, 64, 0)
    s1 = nat.table_reuse_stats()
    _run(nat, dense, "dense 2")
    assert _delta(nat, s1) == (NKEYS, 0, 0)
    # the device-choice size (2,049..4,096 requests of a device-buffer call): once with few keys (the
    # scan keeps the keyed path: 64 keys x 47), once with many (it hands the chunk to the latency path)
    few = _batch(signers, K1, per_key=47, seed=4)
    lots = _batch(signers, list(range(400, 1600)), per_key=2, bad=None, distinct=2, seed=5)
    for b, name in ((few, "few keys"), (lots, "many keys")):
        assert 2049 <= len(b[3]) <= 4096
        d = _Dev(nat, b[0], b[1], b[2])
        try:
            nat.check(nat.lib().pv_verify_batch_device(d.blob, d.off, d.n, d.pk, d.ver, None), "pv_verify_batch_device")
            got = d.verdicts()
        finally:
            d.free()
        assert np.array_equal(got, b[3]), (name, np.nonzero(got != b[3])[0][:10])
        assert (nat.last_path()[0] == nat.PV_PATH_LATENCY) == (name == "many keys")
        s2 = nat.table_reuse_stats()
        _run(nat, dense, "dense after " + name)
        assert _delta(nat, s2) == (NKEYS, 0, 0)


def test_reset_when_full(fresh, signers):
    nat = fresh
    a, b = _batch(signers, K1), _batch(signers, K2, bad=1, seed=6)
    try:
        nat.table_reuse(True, 96)
        s0 = nat.table_reuse_stats()
        _run(nat, a, "K1")
        assert _delta(nat, s0) == (0, NKEYS, 0)
        _run(nat, b, "K2")
        assert _delta(nat, s0) == (0, 2 * NKEYS, 1)  # 64 + 64 > 96: emptied, K2 built from slot 0
        s2 = nat.table_reuse_stats()
        _run(nat, a, "K1 again")
        hits, built, resets = _delta(nat, s2)
        assert hits == 0 or resets == 1
        assert built == NKEYS
        _run(nat, a, "K1 a third time")
    finally:
        nat.table_reuse(True, nat.PV_TABLE_REUSE_CAP)


def test_forced_comb_and_auto(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    try:
        for path in (nat.PV_PATH_COMB, nat.PV_PATH_AUTO, nat.PV_PATH_COMB):
            nat.set_path(path)
            s0 = nat.table_reuse_stats()
            _run(nat, b, ("path", path))
            _run(nat, b, ("path again", path))
            hits, built, resets = _delta(nat, s0)
            assert hits + built == 2 * NKEYS and hits >= NKEYS and resets == 0
    finally:
        nat.set_path(nat.PV_PATH_AUTO)


def test_node_cache_takes_precedence(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    cached = [signers.records(i, 1)[0] for i in K1[:32]]
    kc = nat.KeyCache
    try:
        kc.configure(128)
        kc.put(cached)
        s0 = nat.table_reuse_stats()
        _run(nat, b, "half cached")
        assert _delta(nat, s0) == (0, NKEYS - 32, 0)
        kc.put([signers.records(i, 1)[0] for i in range(500, 508)])  # a put leaves the kept tables alone
        _run(nat, b, "half cached again")
        assert _delta(nat, s0) == (NKEYS - 32, NKEYS - 32, 0)
    finally:
        kc.configure(0)
    _run(nat, b, "cache gone")


def test_pipelined_host_call_around_dense_call(fresh, signers):
    """A host call large enough for pipelined sub-batches (the dense batch eight times over: 563,200
    requests, ~50 MB of records; sub-batch 0 builds into the call's store, the later ones go through
    the allocator) before and after a dense call on the same keys."""
    nat = fresh
    blob, off, pks, want = _batch(signers, K1)
    reps = 8
    big_blob = np.tile(blob, reps)
    big_off = np.concatenate([off[:-1] + np.uint64(r * int(off[-1])) for r in range(reps)] +
                             [np.array([reps * int(off[-1])], np.uint64)])
    big = (big_blob, big_off, np.tile(pks, (reps, 1)), np.tile(want, reps))
    assert big_blob.nbytes >= 8 << 20
    _run(nat, big, "pipelined before")
    s0 = nat.table_reuse_stats()
    _run(nat, (blob, off, pks, want), "dense")
    _run(nat, big, "pipelined after")
    _run(nat, (blob, off, pks, want), "dense again")
    assert _delta(nat, s0)[2] == 0


def test_off(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    _run(nat, b, "on")
    nat.table_reuse(False)
    s0 = nat.table_reuse_stats()
    _run(nat, b, "off 1")
    _run(nat, b, "off 2")
    assert nat.last_split() == (NKEYS, NKEYS, 70400)
    assert _delta(nat, s0) == (0, 0, 0)
    nat.table_reuse(True)  # starts from an empty directory
    _run(nat, b, "on again")
    assert _delta(nat, s0) == (0, NKEYS, 0)
    _run(nat, b, "on again, warm")
    assert _delta(nat, s0) == (NKEYS, NKEYS, 0)


def test_two_threads_two_streams_same_keys(fresh, signers):
    """Modelled on test_gpu_robustness.test_two_caller_streams_back_to_back: two host threads, each
    enqueueing device-buffer calls on its own stream with no synchronisation between them, on batches
    that share their keys (the second is the first in another order with other records tampered)."""
    from test_gpu_robustness import _Dev
    nat = fresh
    L = nat.lib()
    batches = [_batch(signers, K1), _batch(signers, K1, seed=7)]
    streams = [ctypes.c_void_p() for _ in batches]
    for s in streams:
        nat.check(L.pv_stream_create(ctypes.byref(s)), "pv_stream_create")
    devs = [_Dev(nat, b[0], b[1], b[2]) for b in batches]
    errors = []

    def loop(k):
        try:
            d, s, want = devs[k], streams[k], batches[k][3]
            for rep in range(3):
                nat.check(L.pv_verify_batch_device(d.blob, d.off, d.n, d.pk, d.ver, s), "pv_verify_batch_device")
                nat.check(L.pv_stream_sync(s), "pv_stream_sync")
                got = d.verdicts()
                if not np.array_equal(got, want):
                    errors.append((k, rep, np.nonzero(got != want)[0][:5]))
        except Exception as e:  # pragma: no cover
            errors.append((k, repr(e)))

    try:
        s0 = nat.table_reuse_stats()
        ts = [threading.Thread(target=loop, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not errors, errors
        assert _delta(nat, s0) == (5 * NKEYS, NKEYS, 0)  # six calls: one builds, five read
    finally:
        for d in devs:
            d.free()
        for s in streams:
            L.pv_stream_destroy(s)
