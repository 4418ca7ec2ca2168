"""Consistency proofs and catch-up verification on the GPU (device path forced): pv_merkle_consistency_kernel
and pv_merkle_catchup_kernel against the independent restatement in tests/consistency_ref.py and the goldens
recorded from the reference. Shapes are the smallest at which a kernel can go wrong: every status mixed
inside single waves, chunks that are not whole verdict words, sizes across 2^32, replies that end one
below, on and one above a tile edge, a wave's 64 replies straddling chunks, and one reply per leaf."""
import ctypes
import os

import numpy as np
import pytest

import consistency_ref as C
import merkle_ref as R
from test_consistency_host import arrays, library_status, run_catchup
from test_gpu_merkle import DevBuf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 1024


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    _native.ensure_device(0)
    return _native


@pytest.fixture()
def dev(native):
    native.merkle_path(native.PV_MERKLE_DEVICE)
    native.merkle_chunk(0)
    yield native
    native.merkle_path(native.PV_MERKLE_AUTO)
    native.merkle_chunk(0)


@pytest.fixture(scope="module")
def golden():
    return C.load_golden(os.path.join(HERE, "golden", "merkle_consistency.json"))


@pytest.fixture(scope="module")
def pairs40():
    """All 820 pairs 0 <= a < b <= 40 of one tree (the 780 with 0 < a among them), valid and truncated by one;
    computed once."""
    rng = np.random.default_rng(51)
    tree = C.PartialTree(0, [])
    tree.extend(R.random_leaves(rng, 40, 0, 30))
    valid = [(a, b, tree.root(a), tree.root(b), tree.proof(a, b) if a else []) for b in range(1, 41) for a in range(b)]
    assert len(valid) == 820
    return valid, [(a, b, o, n, p[:-1]) for a, b, o, n, p in valid]


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_every_status_mixed_inside_single_waves(dev, golden):
    """n = 3 * 64 + 1 through the C entry, stale bytes in both outputs beforehand, verdicts bit by bit."""
    items = C.golden_items(golden)
    by_status = {}
    for _, args, out in items:
        by_status.setdefault(C.status_of(out), []).append(args)
    assert sorted(by_status) == [0, 1, 2, 3, 4, 5]
    rng = np.random.default_rng(52)
    n = 3 * 64 + 1
    kinds = [int(x) for x in rng.integers(0, 6, n)]
    kinds[:6] = [0, 1, 2, 3, 4, 5]
    cases = [by_status[k][int(rng.integers(0, len(by_status[k])))] for k in kinds]
    old, new, oroot, nroot, proof, poff = arrays(cases)
    status, bits = np.full(n + 8, 0xEE, np.uint8), np.full((n + 7) // 8 + 8, 0xFF, np.uint8)
    dev.check(dev.lib().pv_merkle_verify_consistency_batch(ptr(old), ptr(new), ptr(oroot), ptr(nroot), ptr(proof), ptr(poff), n,
                                                           ptr(status), ptr(bits)), "pv_merkle_verify_consistency_batch")
    assert status[:n].tolist() == kinds and (status[n:] == 0xEE).all()
    want = C.pack_bits([k == 0 for k in kinds])
    assert bits[:(n + 7) // 8].tolist() == want.tolist() and (bits[(n + 7) // 8:] == 0xFF).all()
    for i, k in enumerate(kinds):
        assert (bits[i >> 3] >> (i & 7)) & 1 == (k == 0), i


def test_all_pairs_up_to_40_and_their_truncations_in_one_launch(dev, pairs40):
    valid, short = pairs40
    got = library_status(dev, valid + short)
    assert got[:820] == [0] * 820
    # a proof one hash short is too short for every old size but 0, which needs no proof
    assert got[820:] == [C.check(*x) for x in short] == [2 if x[0] else 0 for x in short]


def test_giant_sizes(dev):
    giant = C.giant_cases(np.random.default_rng(53), 600)
    assert sum(1 for x in giant if x[0] < 2 ** 32 < x[1]) > 150
    bent = [(a, b, o, n, [C.flip(p[0], 9)] + p[1:]) for a, b, o, n, p in giant[:200]]
    got = library_status(dev, giant + bent)
    assert got[:600] == [0] * 600 and got[600:] == [C.check(*x) for x in bent]


def test_chunks_that_are_not_whole_verdict_words(dev, golden, pairs40):
    cases = ([x[1] for x in C.golden_items(golden)] + pairs40[0])[:1000]
    assert len(cases) == 1000
    want = [C.check(*x) for x in cases]
    assert len(set(want)) == 6
    for chunk in (0, 100, 64):
        dev.merkle_chunk(chunk)
        assert library_status(dev, cases) == want, chunk


def test_device_buffer_entry_on_a_second_stream(dev, golden):
    cases = [x[1] for x in C.golden_items(golden)][:333]
    want = [C.check(*x) for x in cases]
    n = len(cases)
    L = dev.lib()
    stream = ctypes.c_void_p()
    dev.check(L.pv_stream_create(ctypes.byref(stream)), "pv_stream_create")
    bufs = [DevBuf(dev, a) for a in arrays(cases)]
    d_status, d_words = DevBuf(dev, np.full(n + 8, 0xEE, np.uint8)), DevBuf(dev, np.full(8 * ((n + 63) // 64 + 1), 0xFF, np.uint8))
    try:
        dev.merkle_chunk(128)
        dev.check(L.pv_merkle_verify_consistency_batch_device(*[b.p for b in bufs], n, d_status.p, d_words.p, stream),
                  "pv_merkle_verify_consistency_batch_device")
        dev.check(L.pv_stream_sync(stream), "pv_stream_sync")
        status = d_status.read(n + 8)
        assert status[:n].tolist() == want and (status[n:] == 0xEE).all()
        words = d_words.read(8 * ((n + 63) // 64 + 1))
        assert words[:8 * ((n + 63) // 64)].tolist() == np.concatenate(
            [C.pack_bits([w == 0 for w in want]), np.zeros(8, np.uint8)])[:8 * ((n + 63) // 64)].tolist()
        assert (words[8 * ((n + 63) // 64):] == 0xFF).all()
    finally:
        L.pv_stream_destroy(stream)
        for b in bufs + [d_status, d_words]:
            b.free()


# --------------------------------------------------------------------------------------- catch-up

def mixed_lens(rng, s, n):
    """Reply lengths from {1, 5, 64, 400} summing to n, cut so that replies end one below, on and one above the
    next two 1,024-leaf tile edges above s (2,048 +- 1 for a small s)."""
    edge = (s // TILE + 1) * TILE
    targets = sorted(e for e in (edge - 1, edge, edge + 1, edge + TILE - 1, edge + TILE, edge + TILE + 1) if s < e <= s + n)
    ends, at = [], s
    for stop in targets + [s + n]:
        while at < stop:
            at = min(stop, at + int(rng.choice([1, 5, 64, 400])))
            ends.append(at)
    lens = list(np.diff([s] + ends))
    assert sum(lens) == n and all(x > 0 for x in lens) and set(targets) <= set(ends)
    return [int(x) for x in lens]


def check_catchup(dev, c, what, outputs=False):
    verdicts, status, res = run_catchup(dev, c, want=dev.MERKLE_OUTPUTS if outputs else ())
    assert status.tolist() == c["status"], what
    assert verdicts.tolist() == [x == 0 for x in c["status"]], what
    if outputs:
        leaves = [x for lv, _ in c["replies"] for x in lv]
        blob, off = R.pack(leaves, lead=3)
        plain = dev.merkle_append(c["s"], b"".join(c["frontier"]), blob, off)
        assert set(plain) == set(res)
        for k in plain:
            assert np.array_equal(plain[k], res[k]), (what, k)
        R.assert_batch_equals(res, R.append_all(c["s"], c["frontier"], leaves), len(leaves), what)


def assert_fails_from(c, tamper):
    first = next(r for r, e in enumerate(c["ends"]) if e - c["s"] > tamper)
    assert first > 0 and not any(c["status"][:first]) and all(c["status"][first:]) and first < len(c["status"]) - 1


@pytest.mark.parametrize("s", (0, 1, 65, 1023, 1024, 2 ** 20 - 1, 2 ** 32 - 3))
def test_catchup(dev, s):
    rng = np.random.default_rng(54 + s % 1000)
    n = 3001
    lens = mixed_lens(rng, s, n)
    c = C.make_catchup(rng, s, lens, 0)
    assert not any(c["status"])
    check_catchup(dev, c, "final_size = end", outputs=True)
    dev.merkle_chunk(1000)  # a wave's 64 replies straddle chunks
    check_catchup(dev, c, "final_size = end, chunked", outputs=True)
    c = C.make_catchup(rng, s, lens, 1, tamper=n // 2)
    assert_fails_from(c, n // 2)
    check_catchup(dev, c, "final_size = end + 1, tampered, chunked")
    c = C.make_catchup(rng, s, lens, 1000)
    assert not any(c["status"])
    check_catchup(dev, c, "final_size = end + 1000, chunked")
    dev.merkle_chunk(0)
    check_catchup(dev, c, "final_size = end + 1000")
    ones = C.make_catchup(rng, s, [1] * n, 1, tamper=n // 2)  # one reply per leaf
    assert_fails_from(ones, n // 2)
    check_catchup(dev, ones, "R = n")
    dev.merkle_chunk(1000)
    check_catchup(dev, ones, "R = n, chunked")
    one = C.make_catchup(rng, s, [700], 0)  # R = 1
    check_catchup(dev, one, "R = 1", outputs=True)
    assert one["status"] == [0]


def test_catchup_goldens_through_the_python_method(dev, golden):
    from plenum_amd.merkle import CompactMerkleTree, TreeHasher
    from test_consistency_host import check_outcome
    for c in golden["catchups"]:
        tree = CompactMerkleTree(TreeHasher(), c["start"], [bytes.fromhex(h) for h in c["hashes"]])
        replies = [([bytes.fromhex(x) for x in r["leaves"]], [bytes.fromhex(h) for h in r["proof"]]) for r in c["replies"]]
        got = tree.verify_catchup_replies(replies, c["final_size"], bytes.fromhex(c["final_root"]))
        for r, (g, rec) in enumerate(zip(got, c["replies"])):
            check_outcome(g, rec["out"], (c["start"], r))


def test_device_entry_out_of_range_ends(dev):
    """Everything in device memory on a second stream; reply ends at or below the tree size, beyond the batch
    and out of order: those get status 6 and verdict 0, the others their own status."""
    rng = np.random.default_rng(55)
    s, n = 1000, 1500
    c = C.make_catchup(rng, s, mixed_lens(rng, s, n), 3)
    R_ = len(c["ends"])
    ends, want = list(c["ends"]), list(c["status"])
    for r, bad in ((0, s), (3, 0), (R_ // 2, s + n + 1), (R_ - 1, 2 ** 48 - 1)):
        ends[r], want[r] = bad, 6
    ends[5], ends[9] = ends[9], ends[5]  # out of order, both in range: each proof now belongs to the other end
    want[5] = C.check(ends[5], c["final_size"], C_root(c, ends[5]), c["final_root"], c["replies"][5][1])
    want[9] = C.check(ends[9], c["final_size"], C_root(c, ends[9]), c["final_root"], c["replies"][9][1])
    leaves = [x for lv, _ in c["replies"] for x in lv]
    blob, off = R.pack(leaves, lead=2)
    proofs = [p for _, p in c["replies"]]
    poff = np.zeros(R_ + 1, np.uint64)
    np.cumsum([len(p) for p in proofs], out=poff[1:])
    L = dev.lib()
    stream = ctypes.c_void_p()
    dev.check(L.pv_stream_create(ctypes.byref(stream)), "pv_stream_create")
    words = (R_ + 63) // 64
    d = {"front": DevBuf(dev, np.frombuffer(b"".join(c["frontier"]), np.uint8)), "blob": DevBuf(dev, blob),
         "off": DevBuf(dev, off), "ends": DevBuf(dev, np.array(ends, np.uint64)),
         "root": DevBuf(dev, np.frombuffer(c["final_root"], np.uint8)),
         "proof": DevBuf(dev, np.frombuffer(b"".join(b"".join(p) for p in proofs), np.uint8)), "poff": DevBuf(dev, poff),
         "status": DevBuf(dev, np.full(R_ + 8, 0xEE, np.uint8)), "words": DevBuf(dev, np.full(8 * (words + 1), 0xFF, np.uint8)),
         "out_root": DevBuf(dev, np.zeros(32, np.uint8)), "out_front": DevBuf(dev, np.zeros(2048, np.uint8))}
    try:
        dev.merkle_chunk(500)
        o = dev.PvMerkleOut()
        o.root, o.frontier = d["out_root"].p, d["out_front"].p
        dev.check(L.pv_merkle_catchup_batch_device(s, d["front"].p, d["blob"].p, d["off"].p, n, d["ends"].p, R_, c["final_size"],
                                                   d["root"].p, d["proof"].p, d["poff"].p, ctypes.byref(o), d["status"].p,
                                                   d["words"].p, stream), "pv_merkle_catchup_batch_device")
        dev.check(L.pv_stream_sync(stream), "pv_stream_sync")
        status = d["status"].read(R_ + 8)
        assert status[:R_].tolist() == want and (status[R_:] == 0xEE).all()
        assert {0, 6} <= set(want)
        got = d["words"].read(8 * (words + 1))
        bits = np.unpackbits(got[:8 * words], bitorder="little")
        assert bits[:R_].tolist() == [int(w == 0) for w in want] and not bits[R_:].any()
        assert (got[8 * words:] == 0xFF).all()
        plain = R.append_all(s, c["frontier"], leaves)
        assert d["out_root"].read(32).tobytes() == plain["root"]
        assert d["out_front"].read(32 * len(plain["frontier"])).tobytes() == b"".join(plain["frontier"])
    finally:
        L.pv_stream_destroy(stream)
        for b in d.values():
            b.free()


def C_root(c, end):
    """The root of the tree of `end` leaves the replies of case c build."""
    tree = C.PartialTree(c["s"], c["frontier"])
    tree.extend([x for lv, _ in c["replies"] for x in lv])
    return tree.root(end)
