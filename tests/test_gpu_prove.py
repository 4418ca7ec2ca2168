"""Batched proof generation on the GPU (device path forced): pv_merkle_prove_kernel against the independent
restatement in tests/prove_ref.py and the goldens recorded from the reference. Shapes are the smallest at
which the kernel can go wrong: every kind mixed inside single waves, a batch that is no multiple of the wave,
heights above the 1,024-leaf tile, several chunks, slots of the wrong size, and, for the 64-bit index
arithmetic that no real store can reach, the walker itself in a kernel of its own (tests/native/provecheck.hip)
at sizes around 2^32 and 2^47."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import prove_ref as P
from test_gpu_merkle import DevBuf
from test_prove_host import (BAD_QUERIES, FILL, assert_proofs, golden, guarded, make_tree, plan, prove,  # noqa: F401
                             q_arrays, split, store_of, tree70)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
SRC = os.path.join(HERE, "native", "provecheck.hip")
LIB = os.path.join(HERE, "native", "libprovecheck.so")
U64, U32, VP = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p


def build_provecheck():
    # the product Makefile's flags: the walker as the product kernel compiles it
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-fPIC", "-shared", "-I" + CSRC,
                           SRC, "-o", LIB])


def provecheck_lib():
    """libprovecheck.so, rebuilt when older than its sources. Loading needs no GPU; pc_walk_device does."""
    srcs = [os.path.join(CSRC, "merkle_core.h"), SRC]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_provecheck()
    lib = ctypes.CDLL(LIB)
    lib.pc_words.restype = lib.pc_fold_at.restype = U32
    for f in (lib.pc_walk_host, lib.pc_walk_device):
        f.argtypes = [U64, VP, VP, VP, U32, VP]
    lib.pc_walk_host.restype = None
    return lib


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


def ptr(a):
    return a.ctypes.data_as(VP)


def test_mixed_kinds_in_one_launch(dev):
    """All 820 inclusion queries, all 820 consistency queries (a == b among them) and the 40 roots of a 40-leaf
    tree, shuffled so every wave mixes the kinds; q = 1,680 is no multiple of 64. prove() pre-fills out and
    status with stale bytes and checks the bytes behind both."""
    tree = make_tree(40, 71)
    queries = [(P.INCLUSION, a, b) for b in range(1, 41) for a in range(b)]
    queries += [(P.CONSISTENCY, a, b) for b in range(1, 41) for a in range(1, b + 1)]
    queries += [(P.ROOT, 0, b) for b in range(1, 41)]
    assert len(queries) == 820 + 820 + 40 and len(queries) % 64
    order = np.random.default_rng(72).permutation(len(queries))
    queries = [queries[i] for i in order]
    assert all(len({q[0] for q in queries[w:w + 64]}) >= 2 for w in range(0, len(queries), 64))
    flat = assert_proofs(dev, store_of(tree), queries, [tree.prove(*q) for q in queries])
    assert len(flat) > 32 * 6000


def test_heights_above_the_tile(dev):
    tree = make_tree(2051, 73)
    queries = []
    for b in (1023, 1024, 1025, 2047, 2048, 2049, 2051):
        for a in (0, 1, 1023, 1024, b - 1):
            queries += [q for q in ((P.INCLUSION, a, b), (P.CONSISTENCY, a, b), (P.CONSISTENCY, a + 1, b), (P.ROOT, 0, b))
                        if P.valid(*q, 2051)]
    assert len(queries) > 100
    assert_proofs(dev, store_of(tree), queries, [tree.prove(*q) for q in queries])


def test_chunks(dev, golden):
    store, cases = golden
    cases = [cases[i * len(cases) // 300] for i in range(300)]
    assert len(cases) == 300 and {c[0] for c in cases} == {0, 1, 2}
    one = assert_proofs(dev, store, [c[:3] for c in cases], [c[3] for c in cases])
    dev.merkle_chunk(64)  # five chunks
    assert assert_proofs(dev, store, [c[:3] for c in cases], [c[3] for c in cases]) == one


def test_status_1_and_the_room_guard(dev, tree70):
    store, queries, want = tree70
    mixed, expect = [], []
    for i, bad in enumerate(BAD_QUERIES):
        mixed += [bad, queries[37 * i]]
        expect += [[], want[37 * i]]
    off, flat, status = prove(dev, store, mixed)
    assert status.tolist() == [1, 0] * len(BAD_QUERIES) and split(off, flat) == expect
    sel = [i for i in range(len(queries)) if want[i]][::41]
    for victim in (0, 63, 64, len(sel) - 1):
        guarded(dev, store, [queries[i] for i in sel], [want[i] for i in sel], victim)


def test_round_trip_in_device_memory(dev, golden):
    """The golden cases through the device-buffer entry on a second stream, and the device buffer it filled
    handed straight to the two device-buffer checks (the proof offsets are the plan's own out_off): every
    verdict bit set, no host copy of a proof. The roots the checks compare with are the reference's recorded
    ones."""
    store, cases = golden
    root = {c[2]: c[3][0] for c in cases if c[0] == P.ROOT}
    inc = [c for c in cases if c[0] == P.INCLUSION]
    con = [c for c in cases if c[0] == P.CONSISTENCY and c[1] < c[2]]
    queries = [c[:3] for c in inc + con]
    q, n_inc, n_con = len(queries), len(inc), len(con)
    assert n_inc > 600 and n_con > 100
    off, _ = plan(dev, 300, queries)
    total = int(off[q])
    L = dev.lib()
    stream = ctypes.c_void_p()
    dev.check(L.pv_stream_create(ctypes.byref(stream)), "pv_stream_create")
    kind, a, b = q_arrays(queries)
    leaf_idx = np.array([c[1] for c in inc], np.uint64)
    u64 = lambda xs: np.array(xs, np.uint64)  # noqa: E731
    hashes = lambda xs: np.frombuffer(b"".join(xs), np.uint8)  # noqa: E731
    d = {"leaf": DevBuf(dev, store[0]), "node": DevBuf(dev, store[1]), "kind": DevBuf(dev, kind), "a": DevBuf(dev, a),
         "b": DevBuf(dev, b), "off": DevBuf(dev, off), "out": DevBuf(dev, np.full(32 * total + 64, FILL, np.uint8)),
         "status": DevBuf(dev, np.full(q + 64, FILL, np.uint8)),
         "leafs": DevBuf(dev, hashes([store[0][32 * int(i):32 * int(i) + 32].tobytes() for i in leaf_idx])),
         "idx": DevBuf(dev, leaf_idx), "size": DevBuf(dev, u64([c[2] for c in inc])),
         "inc_root": DevBuf(dev, hashes([root[c[2]] for c in inc])),
         "old": DevBuf(dev, u64([c[1] for c in con])), "new": DevBuf(dev, u64([c[2] for c in con])),
         "old_root": DevBuf(dev, hashes([root[c[1]] for c in con])), "new_root": DevBuf(dev, hashes([root[c[2]] for c in con])),
         "st": DevBuf(dev, np.full(q, FILL, np.uint8)), "words": DevBuf(dev, np.zeros(8 * ((q + 63) // 64), np.uint8))}
    try:
        dev.merkle_chunk(512)
        dev.check(L.pv_merkle_prove_batch_device(d["leaf"].p, 300, d["node"].p, d["kind"].p, d["a"].p, d["b"].p, q, d["off"].p,
                                                 d["out"].p, d["status"].p, stream), "pv_merkle_prove_batch_device")
        # inclusion: the proofs are hashes [off[0], off[n_inc]) of d_out
        dev.check(L.pv_merkle_verify_inclusion_batch_device(None, None, d["leafs"].p, d["idx"].p, d["size"].p, d["out"].p,
                                                            d["off"].p, d["inc_root"].p, n_inc, d["st"].p, d["words"].p, stream),
                  "pv_merkle_verify_inclusion_batch_device")
        dev.check(L.pv_stream_sync(stream), "pv_stream_sync")
        assert not d["st"].read(n_inc).any()
        bits = np.unpackbits(d["words"].read(8 * ((n_inc + 63) // 64)), bitorder="little")
        assert bits[:n_inc].all() and not bits[n_inc:].any()
        # consistency: the offsets from off[n_inc] on, into the same buffer
        dev.check(L.pv_merkle_verify_consistency_batch_device(d["old"].p, d["new"].p, d["old_root"].p, d["new_root"].p, d["out"].p,
                                                              d["off"].p + 8 * n_inc, n_con, d["st"].p, d["words"].p, stream),
                  "pv_merkle_verify_consistency_batch_device")
        dev.check(L.pv_stream_sync(stream), "pv_stream_sync")
        assert not d["st"].read(n_con).any()
        bits = np.unpackbits(d["words"].read(8 * ((n_con + 63) // 64)), bitorder="little")
        assert bits[:n_con].all() and not bits[n_con:].any()
        # and the bytes are the recorded ones, with nothing written behind them
        status = d["status"].read(q + 64)
        assert not status[:q].any() and (status[q:] == FILL).all()
        got = d["out"].read(32 * total + 64)
        assert (got[32 * total:] == FILL).all()
        assert split(off, got[:32 * total].tobytes()) == [c[3] for c in inc + con]
    finally:
        L.pv_stream_destroy(stream)
        for x in d.values():
            x.free()


# ------------------------------------------------------------ the walker's 64-bit arithmetic on the device

def node_pos(end, height):
    return (end - 1) - bin(end - 1).count("1") + height - 1


def aligned_ref(lo, hi):
    """The (tag, idx) of the aligned full subtree [lo, hi)."""
    n = hi - lo
    assert n & (n - 1) == 0 and lo % n == 0
    return (0, lo) if n == 1 else (1, node_pos(hi, n.bit_length() - 1))


def check_refs(query, refs, fold):
    """refs: the walker's (tag, idx) per proof hash; the restatement's ranges say what each must stand for."""
    kind, a, b = query
    want = P.ranges(kind, a, b)
    assert len(refs) == len(want), query
    for (tag, idx), (lo, hi) in zip(refs, want):
        if tag == 2:  # ragged at level idx: [b cleared below that level, b), and not a full subtree
            assert hi == b and lo == (b >> idx) << idx and lo < b, (query, idx, lo, hi)
        else:
            assert (tag, idx) == aligned_ref(lo, hi), (query, lo, hi)
    assert not any(t == 2 for t, _ in refs) or b & (b - 1) or kind == P.ROOT
    # the fold gathers the full subtrees of b from the smallest up
    parts, at = [], b
    for j in range(b.bit_length()):
        if (b >> j) & 1:
            parts.append(aligned_ref(at - (1 << j), at))
            at -= 1 << j
    assert fold == parts, query


def test_walker_on_the_device_at_giant_sizes():
    lib = provecheck_lib()
    W, F = lib.pc_words(), lib.pc_fold_at()
    queries = []
    for b in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 47 - 1, 2 ** 47, 2 ** 47 + 1, 2 ** 48 - 1):
        for a in (0, 1, 2, b // 2 - 1, b // 2, b // 2 + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, b - 2, b - 1, b):
            queries += [q for q in ((P.INCLUSION, a, b), (P.CONSISTENCY, a, b)) if P.valid(*q, 2 ** 48 - 1)]
        queries.append((P.ROOT, 0, b))
    rng = np.random.default_rng(74)
    for _ in range(300):
        b = int(rng.integers(2 ** 31, 2 ** 48))
        queries.append((int(rng.integers(0, 2)), int(rng.integers(1, b)), b))
    bad = [(P.INCLUSION, 2 ** 48 - 1, 2 ** 48 - 1), (P.CONSISTENCY, 0, 2 ** 32), (P.ROOT, 0, 2 ** 48), (7, 1, 2)]
    everything = queries + bad
    kind, a, b = q_arrays(everything)
    q = len(everything)
    assert q % 64 and q > 400
    host, devi = np.zeros(W * q, np.uint64), np.zeros(W * q, np.uint64)
    lib.pc_walk_host(2 ** 48 - 1, ptr(kind), ptr(a), ptr(b), q, ptr(host))
    assert lib.pc_walk_device(2 ** 48 - 1, ptr(kind), ptr(a), ptr(b), q, ptr(devi)) == 0
    assert np.array_equal(host, devi)
    rows = devi.reshape(q, W)
    longest = 0
    for query, w in zip(queries, rows):
        k, g = int(w[0]), int(w[F])
        assert k <= 49 and g <= 48
        check_refs(query, [(int(w[1 + 2 * j]), int(w[2 + 2 * j])) for j in range(k)],
                   [(int(w[F + 1 + 2 * j]), int(w[F + 2 + 2 * j])) for j in range(g)])
        assert not w[1 + 2 * k:F].any() and not w[F + 1 + 2 * g:].any()
        longest = max(longest, k)
    assert longest == 49
    for w in rows[len(queries):]:
        assert int(w[0]) == int(w[F]) == 2 ** 64 - 1 and not w[1:F].any() and not w[F + 1:].any()
