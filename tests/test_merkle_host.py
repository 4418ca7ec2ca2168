"""The ledger Merkle feature without a GPU: the kernels' SHA-256 and index arithmetic
(indy-plenum_amd/csrc/sha256.h, merkle_core.h) compiled for the HOST (tests/native/merklecheck.hip)
against hashlib and an independent restatement of the reference's tree (tests/merkle_ref.py); the
library's host path (pv_merkle_path(HOST)) end to end; the Python classes of plenum_amd.merkle against
goldens recorded from the reference (tests/golden/merkle.json); and the argument checks. Same source as
the GPU kernels, so a pass here means their arithmetic is right up to compilation;
tests/test_gpu_merkle.py closes that gap."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import merkle_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
LIB = os.path.join(HERE, "native", "libmerklecheck.so")
# leaf lengths where len + 1 crosses a block or padding edge
BOUNDARY_LENGTHS = (0, 1, 54, 55, 56, 62, 63, 64, 118, 119, 120, 126, 127, 128)
U64, VP = ctypes.c_uint64, ctypes.c_void_p


def build_merklecheck():
    src = os.path.join(HERE, "native", "merklecheck.hip")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-pthread", "--offload-arch=gfx950",
                           "--offload-host-only", "-I" + CSRC, src, "-o", LIB])


def merklecheck_lib():
    srcs = [os.path.join(CSRC, f) for f in ("sha256.h", "sha512.h", "fe25519.h", "merkle_core.h")]
    srcs.append(os.path.join(HERE, "native", "merklecheck.hip"))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_merklecheck()
    L = ctypes.CDLL(LIB)
    L.mkc_node_pos.restype = U64
    L.mkc_popc_sum.restype = U64
    L.mkc_verify.restype = ctypes.c_uint32
    return L


@pytest.fixture(scope="module")
def mc():
    return merklecheck_lib()


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    return _native


@pytest.fixture()
def host_path(native):
    native.merkle_path(native.PV_MERKLE_HOST)
    yield native
    native.merkle_path(native.PV_MERKLE_AUTO)
    native.merkle_chunk(0)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "merkle.json")) as f:
        return json.load(f)


def ptr(a):
    return a.ctypes.data_as(VP)


def mkc_leaf(mc, data, align=0):
    out = ctypes.create_string_buffer(32)
    mc.mkc_leaf_hash(data, U64(len(data)), align, out)
    return out.raw


def mkc_append(mc, native, s, frontier, leaves, lead=5):
    """tests/native/merklecheck.hip's serial run of the kernels' decomposition -> merkle_append's dict."""
    blob, off = R.pack(leaves, lead=lead)
    n = len(leaves)
    nn, nf, npath = native.merkle_plan(s, n)
    sizes = dict(leaf_hash=n, node_hash=nn, frontier=64, root=1, roots=n, path=npath)
    o = {k: np.zeros(max(1, x) * 32, np.uint8) for k, x in sizes.items()}
    po = np.zeros(n + 1, np.uint64)
    f = np.frombuffer(b"".join(frontier) or b"\0", np.uint8)
    mc.mkc_append(U64(s), ptr(f), ptr(blob), ptr(off), U64(n),
                  *[ptr(o[k]) for k in ("leaf_hash", "node_hash", "frontier", "root", "roots", "path")], ptr(po))
    res = {k: o[k][:32 * x] for k, x in sizes.items() if k not in ("frontier", "root")}
    res["frontier"] = o["frontier"][:32 * nf]
    res["path_off"] = po
    if s + n:
        res["root"] = o["root"]
    return res


# ------------------------------------------------------------------------------------------ SHA-256

def test_sha256_every_length_and_alignment(mc):
    rng = np.random.default_rng(11)
    out = ctypes.create_string_buffer(32)
    for n in sorted(set(range(0, 301)) | set(BOUNDARY_LENGTHS) | {1000, 5000}):
        d = rng.bytes(n) if n % 3 else (b"\x80" if n % 2 else b"\xff") * n  # also 0x80 / 0xff next to the padding
        for align in range(8):
            assert mkc_leaf(mc, d, align) == R.leaf_hash(d), (n, align)
            mc.mkc_sha256(d, U64(n), align, out)
            assert out.raw == hashlib.sha256(d).digest(), (n, align)


def test_hash_children_two_block_form(mc):
    rng = np.random.default_rng(12)
    out = ctypes.create_string_buffer(32)
    pairs = [(rng.bytes(32), rng.bytes(32)) for _ in range(300)]
    pairs += [(bytes(32), bytes(32)), (b"\xff" * 32, b"\xff" * 32), (b"\x80" * 32, bytes(31) + b"\x80")]
    for left, right in pairs:
        mc.mkc_hash_children(left, right, out)
        assert out.raw == R.node_hash(left, right)


# ---------------------------------------------------------------------------------- index arithmetic

def ref_positions(s, n):
    """(u, h) of the node writes of n appends to a tree of size s, in store order."""
    out = []
    for u in range(s + 1, s + n + 1):
        out += [(u, h) for h in range(1, (u & -u).bit_length())]
    return out


def check_arithmetic(mc, native, s, n):
    t = s + n
    nn, nf, npath = native.merkle_plan(s, n)
    a, b, c = U64(), U64(), U64()
    mc.mkc_plan(U64(s), U64(n), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    assert (a.value, b.value, c.value) == (nn, nf, npath)
    pos = ref_positions(s, n)
    assert nn == len(pos) == (t - bin(t).count("1")) - (s - bin(s).count("1"))
    assert nf == bin(t).count("1")
    assert npath == sum(bin(s + i).count("1") for i in range(n))
    base = s - bin(s).count("1")
    for k, (u, h) in enumerate(pos):
        assert mc.mkc_node_pos(U64(u), h) == base + k, (s, n, u, h)
    # the frontier lookup at every size of the batch, against the positions just checked
    index = {uh: k for k, uh in enumerate(pos)}
    kind, idx = ctypes.c_uint32(), U64()
    for tt in range(s, t + 1):
        for bit in range(tt.bit_length()):
            if not (tt >> bit) & 1:
                continue
            u = ((tt >> (bit + 1)) << (bit + 1)) + (1 << bit)
            mc.mkc_frontier_ref(U64(s), U64(tt), bit, ctypes.byref(kind), ctypes.byref(idx))
            if u <= s:  # the old frontier's entry for this bit, largest first
                assert (kind.value, idx.value) == (0, bin(s >> (bit + 1)).count("1")), (s, tt, bit)
            elif bit == 0:
                assert (kind.value, idx.value) == (1, u - 1 - s), (s, tt, bit)
            else:
                assert (kind.value, idx.value) == (2, index[(u, bit)]), (s, tt, bit)


def test_plan_positions_and_frontier_lookup_small(mc, native):
    for s in range(0, 601):
        for n in (0, 1, 2, 3, 64, 65):
            check_arithmetic(mc, native, s, n)


def test_plan_positions_and_frontier_lookup_large(mc, native):
    rng = np.random.default_rng(13)
    for centre in (2 ** 20, 2 ** 32, 2 ** 47):
        for s in [centre - 66, centre - 65, centre - 3, centre - 1, centre, centre + 1] + \
                 [centre + int(rng.integers(-1000, 1000)) for _ in range(4)]:
            for n in (0, 1, 2, 3, 64, 65):
                check_arithmetic(mc, native, s, n)


def test_kernel_decomposition_against_restatement(mc, native):
    """Leaf hashes, the tile passes over absolute indices (every height up to 40), frontier, roots and paths
    of the kernels' formulation, run serially on the host."""
    rng = np.random.default_rng(14)
    cases = [(s, n) for s in (0, 1, 3, 7, 8, 1023, 1024, 1025, 2047, 2 ** 20 - 1, 2 ** 20, 2 ** 32 - 3, 2 ** 40 - 2,
                              2 ** 47 - 5) for n in (1, 2, 3, 65, 1025)] + [(0, 2050), (1023, 3073), (2 ** 20 - 2, 2051)]
    for s, n in cases:
        frontier, leaves = R.random_frontier(rng, s), R.random_leaves(rng, n, 0, 40)
        R.assert_batch_equals(mkc_append(mc, native, s, frontier, leaves), R.append_all(s, frontier, leaves), n,
                              "s=%d n=%d" % (s, n))


def test_path_check_statuses(mc):
    rng = np.random.default_rng(15)
    leaves = R.random_leaves(rng, 37)
    t = R.RefTree()
    for d in leaves:
        t.append(d)
    ok = ctypes.c_int()

    def run(lh, index, size, proof, root):
        st = mc.mkc_verify(lh, U64(index), U64(size), b"".join(proof) or b"\0", U64(len(proof)), root, ctypes.byref(ok))
        return st, bool(ok.value)

    for size in range(1, 38):
        sub = R.append_all(0, [], leaves[:size])
        root = sub["root"]
        for i in range(size):
            # the audit path of leaf i in the tree of `size` leaves, by brute force over subtree roots
            proof = brute_force_proof(sub["leaf_hash"], i)
            assert R.check_path(sub["leaf_hash"][i], i, size, proof) == (0, root)
            assert run(sub["leaf_hash"][i], i, size, proof, root) == (0, True)
            assert run(sub["leaf_hash"][i], i, size, proof, bytes(32)) == (0, False)
            for bad in (proof[:-1], proof + [bytes(32)], proof[1:], []):
                want = R.check_path(sub["leaf_hash"][i], i, size, bad)
                got = run(sub["leaf_hash"][i], i, size, bad, root)
                assert got[0] == want[0] and got[1] == (want[0] == 0 and want[1] == root), (size, i, len(bad))
        assert run(sub["leaf_hash"][0], size, size, [], root) == (1, False)
        assert run(sub["leaf_hash"][0], size + 5, size, [], root) == (1, False)


def brute_force_proof(leaf_hashes, i):
    """RFC 6962 PATH(i, D[n]) from the definition."""
    def mth(h):
        if len(h) == 1:
            return h[0]
        k = 1 << ((len(h) - 1).bit_length() - 1)
        return R.node_hash(mth(h[:k]), mth(h[k:]))

    def path(m, h):
        if len(h) == 1:
            return []
        k = 1 << ((len(h) - 1).bit_length() - 1)
        return path(m, h[:k]) + [mth(h[k:])] if m < k else path(m - k, h[k:]) + [mth(h[:k])]

    return path(i, list(leaf_hashes))


# ----------------------------------------------------------------------------- the library's host path

def test_host_path_against_restatement(host_path):
    rng = np.random.default_rng(16)
    for s in (0, 1, 2, 3, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 32 - 3, 2 ** 47 - 2):
        for n in (0, 1, 2, 3, 64, 65, 257):
            frontier, leaves = R.random_frontier(rng, s), R.random_leaves(rng, n)
            blob, off = R.pack(leaves, lead=int(rng.integers(0, 8)))
            res = host_path.merkle_append(s, b"".join(frontier), blob, off)
            R.assert_batch_equals(res, R.append_all(s, frontier, leaves), n, "s=%d n=%d" % (s, n))


def test_host_path_optional_outputs(host_path):
    rng = np.random.default_rng(18)
    s, n = 65, 257
    frontier, leaves = R.random_frontier(rng, s), R.random_leaves(rng, n)
    blob, off = R.pack(leaves)
    want = R.append_all(s, frontier, leaves)
    full = host_path.MERKLE_OUTPUTS
    for sel in [(k,) for k in full] + [tuple(x for x in full if x != k) for k in full] + [()]:
        res = host_path.merkle_append(s, b"".join(frontier), blob, off, want=sel)
        assert set(res) == set(sel) | ({"path_off"} if "path" in sel else set())
        R.assert_batch_equals(res, want, n, str(sel))


def test_host_path_goldens(host_path, golden):
    for c in golden["appends"]:
        leaves = [bytes.fromhex(x) for x in c["leaves"]]
        blob, off = R.pack(leaves)
        res = host_path.merkle_append(c["start"], bytes.fromhex("".join(c["hashes"])), blob, off)
        assert res["leaf_hash"].tobytes().hex() == "".join(c["store_leaves"])
        assert res["node_hash"].tobytes().hex() == "".join(x[2] for x in c["store_nodes"])
        assert res["frontier"].tobytes().hex() == "".join(c["final_hashes"])
        assert res["root"].tobytes().hex() == c["final_root"]
        assert res["roots"].tobytes().hex() == "".join(c["roots"])
        assert res["path"].tobytes().hex() == "".join("".join(p) for p in c["paths"])
        assert [int(x) for x in np.diff(res["path_off"])] == [len(p) for p in c["paths"]]


def golden_status(out):
    if "exc" not in out:
        return 0
    return 1 if out["exc"] == "ValueError" else 2 if "too short" in out["msg"] else 3 if "too long" in out["msg"] else 0


def test_host_verify_against_goldens(host_path, golden):
    items = R.golden_proof_items(golden)
    args = ([x[1][1] for x in items], [x[1][4] for x in items], [x[1][2] for x in items], [x[1][3] for x in items])
    verdicts, status = host_path.merkle_verify_inclusion(*args, leaves=[x[1][0] for x in items])
    for (kind, _, out), v, st in zip(items, verdicts, status):
        assert bool(v) == (out.get("value") is True) and st == golden_status(out), (kind, out)
    v2, s2 = host_path.merkle_verify_inclusion(*args, leaf_hashes=[R.leaf_hash(x[1][0]) for x in items])
    assert np.array_equal(v2, verdicts) and np.array_equal(s2, status)


def test_empty_tree_and_no_leaves(host_path):
    res = host_path.merkle_append(0, b"", np.zeros(1, np.uint8), np.zeros(1, np.uint64))
    assert res["root"].tobytes() == hashlib.sha256(b"").digest() and res["frontier"].shape == (0, 32)
    assert res["path_off"].tolist() == [0] and res["leaf_hash"].shape == (0, 32)
    rng = np.random.default_rng(19)
    frontier = R.random_frontier(rng, 13)
    res = host_path.merkle_append(13, b"".join(frontier), np.zeros(1, np.uint8), np.zeros(1, np.uint64))
    assert res["frontier"].tobytes() == b"".join(frontier) and res["root"].tobytes() == R.fold(frontier)
    one = host_path.merkle_append(0, b"", *R.pack([b"only"]))
    assert one["root"].tobytes() == one["leaf_hash"].tobytes() == R.leaf_hash(b"only") and one["node_hash"].size == 0


def test_auto_serves_a_machine_without_a_device(native, monkeypatch):
    """AUTO never answers PV_ERR_NOT_INIT: without an initialised device the host path runs."""
    native.merkle_path(native.PV_MERKLE_AUTO)
    rng = np.random.default_rng(20)
    leaves = R.random_leaves(rng, 10)
    # a batch below the threshold does not even look for a device (no engine context for a ledger-only process)
    monkeypatch.setattr(native, "ensure_device", lambda *a: pytest.fail("a ten-leaf AUTO batch bound a device"))
    res = native.merkle_append(0, b"", *R.pack(leaves))
    R.assert_batch_equals(res, R.append_all(0, [], leaves), 10)
    want = R.append_all(0, [], leaves)
    v, st = native.merkle_verify_inclusion(list(range(10)), list(range(1, 11)), want["paths"], want["roots"], leaves=leaves)
    assert v.all() and not st.any()


def test_argument_errors(native):
    L = native.lib()
    out = native.PvMerkleOut()
    root = np.zeros(32, np.uint8)
    out.root = root.ctypes.data
    blob, off = np.zeros(16, np.uint8), np.array([0, 4, 8], np.uint64)
    ARG = native.PV_ERR_ARG
    assert L.pv_merkle_append_batch(0, None, ptr(blob), ptr(off), 2, ctypes.byref(out)) == native.PV_OK
    assert L.pv_merkle_append_batch(0, None, ptr(blob), ptr(np.array([0, 8, 4], np.uint64)), 2, ctypes.byref(out)) == ARG
    assert b"non-decreasing" in L.pv_last_error()
    assert L.pv_merkle_append_batch(5, None, ptr(blob), ptr(off), 2, ctypes.byref(out)) == ARG       # no frontier
    assert L.pv_merkle_append_batch(2 ** 48 - 1, ptr(blob), ptr(blob), ptr(off), 2, ctypes.byref(out)) == ARG
    assert L.pv_merkle_append_batch(2 ** 48, ptr(blob), ptr(blob), ptr(off), 0, ctypes.byref(out)) == ARG
    assert L.pv_merkle_append_batch(0, None, ptr(blob), ptr(off), 2, None) == ARG
    assert L.pv_merkle_append_batch(0, None, None, ptr(off), 2, ctypes.byref(out)) == ARG            # null data
    assert L.pv_merkle_append_batch(0, None, ptr(blob), None, 2, ctypes.byref(out)) == ARG           # null offsets
    bad = native.PvMerkleOut()
    bad.path = root.ctypes.data                                                                     # path without path_off
    assert L.pv_merkle_append_batch(0, None, ptr(blob), ptr(off), 2, ctypes.byref(bad)) == ARG
    assert L.pv_merkle_plan(2 ** 48 - 1, 1, None, None, None) == ARG
    assert L.pv_merkle_plan(2 ** 48 - 2, 1, None, None, None) == native.PV_OK
    assert L.pv_merkle_path(7) == ARG and L.pv_merkle_chunk(2 ** 32) == ARG
    # the proof check: both or neither of (data, off) / leaf_hash; decreasing offsets
    idx, size = np.zeros(2, np.uint64), np.ones(2, np.uint64)
    poff, st, bits = np.zeros(3, np.uint64), np.zeros(2, np.uint8), np.zeros(1, np.uint8)
    roots = np.zeros(64, np.uint8)
    args = (ptr(idx), ptr(size), ptr(roots), ptr(poff), ptr(roots), 2, ptr(st), ptr(bits))
    assert L.pv_merkle_verify_inclusion_batch(ptr(blob), ptr(off), ptr(roots), *args) == ARG
    assert L.pv_merkle_verify_inclusion_batch(None, None, None, *args) == ARG
    assert L.pv_merkle_verify_inclusion_batch(ptr(blob), ptr(np.array([0, 8, 4], np.uint64)), None, *args) == ARG
    assert L.pv_merkle_verify_inclusion_batch(ptr(blob), ptr(off), None, ptr(idx), ptr(size), ptr(roots),
                                              ptr(np.array([0, 2, 1], np.uint64)), ptr(roots), 2, ptr(st), ptr(bits)) == ARG
    assert L.pv_merkle_verify_inclusion_batch(ptr(blob), ptr(off), None, *args) == native.PV_OK
    if L.pv_device_count() == 0:
        # device buffers imply an initialised device; a forced device path without one is refused loudly
        assert L.pv_merkle_append_batch_device(0, None, ptr(blob), ptr(off), 2, ctypes.byref(out), None) == native.PV_ERR_NOT_INIT
        native.merkle_path(native.PV_MERKLE_DEVICE)
        try:
            assert L.pv_merkle_append_batch(0, None, ptr(blob), ptr(off), 2, ctypes.byref(out)) == native.PV_ERR_NO_DEVICE
        finally:
            native.merkle_path(native.PV_MERKLE_AUTO)


def assert_refusals(L, table):
    """Every row's call answers its (return code, pv_last_error()) exactly."""
    for i, (call, rc, msg) in enumerate(table):
        assert (call(), L.pv_last_error().decode()) == (rc, msg), (i, msg)


def test_argument_errors_code_and_message(native):
    """One bad call per check of pv_merkle_plan, pv_merkle_append_batch and pv_merkle_verify_inclusion_batch, and
    pairs of bad arguments for the order of the checks: the return code and the message as the library gave them
    when every entry wrote its checks out itself (they are csrc/merkle_plan.h's now). The host-buffer entries
    answer without a device. pv_merkle_verify_inclusion_batch walks both offset arrays before it looks at the
    count, so its "more than 2^32 - 1 proofs" would take arrays of 2^32 offsets to reach and has no row."""
    L, ARG = native.lib(), native.PV_ERR_ARG
    out, paths = native.PvMerkleOut(), native.PvMerkleOut()
    root = np.zeros(32, np.uint8)
    out.root = paths.path = root.ctypes.data
    blob, off, dec = np.zeros(16, np.uint8), np.array([0, 4, 8], np.uint64), np.array([0, 8, 4], np.uint64)

    def append(tree_size=0, frontier=None, data=ptr(blob), off_=ptr(off), n=2, o=ctypes.byref(out)):
        return L.pv_merkle_append_batch(tree_size, frontier, data, off_, n, o)

    idx, size = np.zeros(2, np.uint64), np.ones(2, np.uint64)
    st, bits, roots = np.zeros(2, np.uint8), np.zeros(1, np.uint8), np.zeros(64, np.uint8)
    poff = np.array([0, 1, 2], np.uint64)

    def verify(data=ptr(blob), off_=ptr(off), leaf_hash=None, index=ptr(idx), proof=ptr(roots), poff_=ptr(poff)):
        return L.pv_merkle_verify_inclusion_batch(data, off_, leaf_hash, index, ptr(size), proof, poff_, ptr(roots), 2, ptr(st),
                                                  ptr(bits))

    A, V, SIZES = "pv_merkle_append_batch: ", "pv_merkle_verify_inclusion_batch: ", "tree_size + n must stay below 2^48"
    assert append() == native.PV_OK and verify() == native.PV_OK
    assert_refusals(L, [
        (lambda: L.pv_merkle_plan(2 ** 48 - 1, 1, None, None, None), ARG, "pv_merkle_plan: " + SIZES),
        (lambda: L.pv_merkle_plan(0, 2 ** 48, None, None, None), ARG, "pv_merkle_plan: " + SIZES),
        (lambda: append(o=None), ARG, A + "null output struct"),
        (lambda: append(o=ctypes.byref(paths)), ARG, A + "path and path_off go together"),
        (lambda: append(tree_size=2 ** 48, frontier=ptr(blob), n=0), ARG, A + SIZES),
        (lambda: append(tree_size=2 ** 48 - 1, frontier=ptr(blob)), ARG, A + SIZES),
        (lambda: append(tree_size=5), ARG, A + "a tree of size > 0 needs its frontier"),
        (lambda: append(off_=None), ARG, A + "null offsets"),
        (lambda: append(off_=ptr(dec)), ARG, A + "offsets must be non-decreasing"),
        (lambda: append(data=None), ARG, A + "null data"),
        # two at once: the output struct before the sizes, the sizes before the frontier, the offsets before the data
        (lambda: append(tree_size=2 ** 48, o=None), ARG, A + "null output struct"),
        (lambda: append(tree_size=2 ** 48), ARG, A + SIZES),
        (lambda: append(tree_size=5, off_=None), ARG, A + "a tree of size > 0 needs its frontier"),
        (lambda: append(data=None, off_=ptr(dec)), ARG, A + "offsets must be non-decreasing"),
        (lambda: verify(index=None), ARG, V + "null pointer"),
        (lambda: verify(leaf_hash=ptr(roots)), ARG, V + "give either data and off, or leaf_hash"),
        (lambda: verify(data=None, off_=None), ARG, V + "give either data and off, or leaf_hash"),
        (lambda: verify(off_=ptr(dec)), ARG, V + "offsets must be non-decreasing over a data blob"),
        (lambda: verify(data=None), ARG, V + "offsets must be non-decreasing over a data blob"),
        (lambda: verify(poff_=ptr(dec)), ARG, V + "proof offsets must be non-decreasing over a proof array"),
        (lambda: verify(proof=None), ARG, V + "proof offsets must be non-decreasing over a proof array"),
        (lambda: verify(off_=ptr(dec), poff_=ptr(dec)), ARG, V + "offsets must be non-decreasing over a data blob"),
    ])
    native.merkle_path(native.PV_MERKLE_DEVICE)
    try:
        if L.pv_device_count() == 0:  # a forced device path is refused after the checks, also for no leaves
            no_dev = ": the device path is forced and no device is initialised"
            assert_refusals(L, [(lambda: append(n=0), native.PV_ERR_NO_DEVICE, A[:-2] + no_dev),
                                (lambda: append(off_=None), ARG, A + "null offsets"),
                                (verify, native.PV_ERR_NO_DEVICE, V[:-2] + no_dev)])
    finally:
        native.merkle_path(native.PV_MERKLE_AUTO)


# ------------------------------------------------------------------------------- the Python classes

def test_python_tree_against_goldens(host_path, golden):
    from plenum_amd.merkle import CompactMerkleTree, MemoryHashStore, TreeHasher
    for c in golden["appends"]:
        hashes = [bytes.fromhex(h) for h in c["hashes"]]
        leaves = [bytes.fromhex(x) for x in c["leaves"]]
        want_nodes = [bytes.fromhex(x[2]) for x in c["store_nodes"]]
        seq = CompactMerkleTree(TreeHasher(), c["start"], hashes, MemoryHashStore())
        bat = CompactMerkleTree(TreeHasher(), c["start"], hashes, MemoryHashStore())
        seq_paths = [seq.append(x) for x in leaves]
        paths, roots = bat.append_batch(leaves)
        for tree in (seq, bat):
            assert [h.hex() for h in tree.hashes] == c["final_hashes"] and tree.tree_size == c["start"] + len(leaves)
            assert tree.root_hash.hex() == c["final_root"] and len(tree) == tree.tree_size
            assert tree.hashStore.readLeafs(1, len(leaves)) == [bytes.fromhex(h) for h in c["store_leaves"]]
            assert tree.hashStore.readNodes(1, len(want_nodes)) == want_nodes
            assert tree.leafCount == len(leaves) and tree.nodeCount == len(want_nodes)
        assert [[h.hex() for h in p] for p in paths] == c["paths"] == [[h.hex() for h in p] for p in seq_paths]
        assert [r.hex() for r in roots] == c["roots"]
        ext = CompactMerkleTree(TreeHasher(), c["start"], hashes).extended_batch(leaves)
        assert [h.hex() for h in ext.hashes] == c["final_hashes"] and ext.root_hash.hex() == c["final_root"]
        assert ext.hashStore.leafCount == 0
        if c["start"] == 0:
            assert seq.extended([]).hashes == CompactMerkleTree().extended(leaves).hashes == bat.hashes
            assert bat.verify_consistency(len(leaves))


def test_python_batches_in_pieces_keep_the_store_exact(host_path):
    from plenum_amd.merkle import CompactMerkleTree
    rng = np.random.default_rng(21)
    leaves = R.random_leaves(rng, 200)
    seq, bat = CompactMerkleTree(), CompactMerkleTree()
    want_paths, want_roots = [], []
    for x in leaves:
        want_paths.append(seq.append(x))
        want_roots.append(seq.root_hash)
    got_paths, got_roots = [], []
    for lo, hi in ((0, 1), (1, 3), (3, 64), (64, 64), (64, 65), (65, 200)):
        p, r = bat.append_batch(leaves[lo:hi])
        got_paths += p
        got_roots += r
    assert got_paths == want_paths and got_roots == want_roots and bat.hashes == seq.hashes
    assert bat.hashStore.readNodes(1, bat.nodeCount) == seq.hashStore.readNodes(1, seq.nodeCount)
    assert bat.nodeCount == bat.get_expected_node_count(200) and bat.hashStore.is_consistent
    # the store-backed proofs work on the batched tree's store
    for i in (0, 1, 99, 198, 199):
        assert bat.inclusion_proof(i, 200) == seq.inclusion_proof(i, 200) == brute_force_proof(
            [R.leaf_hash(x) for x in leaves], i)
    assert bat.merkle_tree_hash(0, 200) == bat.root_hash == bat.get_tree_head()["sha256_root_hash"]
    assert bat.consistency_proof(64, 200) == seq.consistency_proof(64, 200)
    assert bat.get_tree_head(64)["sha256_root_hash"] == want_roots[63]
    bat.reset()
    assert bat.tree_size == 0 and bat.leafCount == 0 and bat.root_hash == R.EMPTY


def test_python_verifier_against_goldens(host_path, golden):
    from plenum_amd.merkle import STH, MerkleVerifier
    from plenum_amd.exceptions import ProofError
    v = MerkleVerifier()
    cases = R.golden_proof_items(golden)
    items = [(leaf, index, proof, STH(size, root)) for _, (leaf, index, proof, root, size), _ in cases]
    for (kind, _, out), item, g in zip(cases, items, v.verify_leaf_inclusion_batch(items)):
        if "exc" in out:
            assert type(g).__name__ == out["exc"] and str(g) == out["msg"], (kind, g)
            assert isinstance(g, ProofError) == (out["exc"] == "ProofError")
            with pytest.raises(type(g)):
                v.verify_leaf_inclusion(*item)
        else:
            assert g is True and v.verify_leaf_inclusion(*item) is True
    # items the library cannot represent fall back to the sequential method
    odd = v.verify_leaf_inclusion_batch([(b"x", -1, [], STH(1, bytes(32))), (b"x", 0, [b"short"], STH(2, bytes(32)))])
    assert isinstance(odd[0], ValueError) and str(odd[0]).startswith("Negative tree size or leaf index")
    assert isinstance(odd[1], ProofError) and str(odd[1]).startswith("Constructed root hash differs")


def test_hash_leaves(host_path):
    from plenum_amd.merkle import TreeHasher
    rng = np.random.default_rng(22)
    leaves = [rng.bytes(n) for n in BOUNDARY_LENGTHS] + R.random_leaves(rng, 50, 0, 400)
    h = TreeHasher()
    assert h.hash_leaves(leaves) == [h.hash_leaf(x) for x in leaves] == [R.leaf_hash(x) for x in leaves]
    assert h.hash_leaves([]) == [] and h.hash_empty() == R.EMPTY
    assert h.hash_full_tree(leaves[:5]) == R.append_all(0, [], leaves[:5])["root"]
