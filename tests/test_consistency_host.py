"""Consistency proofs and catch-up verification without a GPU: the consistency walk of
indy-plenum_amd/csrc/merkle_core.h with the kernels' SHA-256 compiled for the HOST (tests/native/conscheck.hip)
against an independent restatement (tests/consistency_ref.py); the library's host path
(pv_merkle_path(HOST)) for pv_merkle_verify_consistency_batch and pv_merkle_catchup_batch; the Python
methods of plenum_amd.merkle against goldens recorded from the reference
(tests/golden/merkle_consistency.json), class and text; and the argument checks. Same source as the GPU
kernels; tests/test_gpu_consistency.py closes the gap that compilation leaves."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as C
import merkle_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
LIB = os.path.join(HERE, "native", "libconscheck.so")
U64, VP = ctypes.c_uint64, ctypes.c_void_p


def build_conscheck():
    src = os.path.join(HERE, "native", "conscheck.hip")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "--offload-arch=gfx950",
                           "--offload-host-only", "-I" + CSRC, src, "-o", LIB])


def conscheck_lib():
    srcs = [os.path.join(CSRC, f) for f in ("sha256.h", "sha512.h", "fe25519.h", "merkle_core.h")]
    srcs.append(os.path.join(HERE, "native", "conscheck.hip"))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_conscheck()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def cc():
    return conscheck_lib()


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
    return C.load_golden(os.path.join(HERE, "golden", "merkle_consistency.json"))


@pytest.fixture(scope="module")
def small_cases():
    """Every pair 0 <= a <= b <= 70 of one tree with every variant, and the restatement's status; computed once."""
    rng = np.random.default_rng(41)
    tree = C.PartialTree(0, [])
    tree.extend(R.random_leaves(rng, 70, 0, 30))
    cases = []
    for b in range(71):
        for a in range(b + 1):
            proof = tree.proof(a, b) if 0 < a < b else []
            cases += list(C.variants(a, b, tree.root(a), tree.root(b), proof).values())
            assert C.check(*cases[-len(proof) - 9]) == 0  # "valid" comes first
    return cases, [C.check(*x) for x in cases]


@pytest.fixture(scope="module")
def giant():
    return C.giant_cases(np.random.default_rng(42), 2000)


def ptr(a):
    return a.ctypes.data_as(VP)


def arrays(cases):
    old = np.array([x[0] for x in cases], np.uint64)
    new = np.array([x[1] for x in cases], np.uint64)
    oroot = np.frombuffer(b"".join(x[2] for x in cases), np.uint8)
    nroot = np.frombuffer(b"".join(x[3] for x in cases), np.uint8)
    poff = np.zeros(len(cases) + 1, np.uint64)
    np.cumsum([len(x[4]) for x in cases], out=poff[1:])
    proof = np.frombuffer(b"".join(b"".join(x[4]) for x in cases) + bytes(32), np.uint8)
    return old, new, oroot, nroot, proof, poff


def conscheck_status(cc, cases):
    old, new, oroot, nroot, proof, poff = arrays(cases)
    status = np.full(len(cases), 99, np.uint8)
    cc.csc_check(ptr(old), ptr(new), ptr(oroot), ptr(nroot), ptr(proof), ptr(poff), U64(len(cases)), ptr(status))
    return status.tolist()


def library_status(native, cases):
    verdicts, status = native.merkle_verify_consistency([x[0] for x in cases], [x[1] for x in cases], [x[2] for x in cases],
                                                        [x[3] for x in cases], [x[4] for x in cases])
    assert [bool(v) for v in verdicts] == [s == 0 for s in status]
    return status.tolist()


# ------------------------------------------------------------------------------------ the walk itself

def test_restatement_agrees_with_the_reference_recordings(golden):
    items = C.golden_items(golden)
    assert len(items) > 2000
    for name, args, out in items:
        assert C.check(*args) == C.status_of(out), name
    kinds = {C.status_of(out) for _, _, out in items}
    assert kinds == {0, 1, 2, 3, 4, 5}
    # a wrong old root of a power-of-two old tree shows as the second root differing
    for c in golden["pairs"]:
        a, b = c["old"], c["new"]
        if 0 < a < b:
            assert C.status_of(c["out"]["wrong_old_root"]) == (3 if a & (a - 1) == 0 else 4), (a, b)
            assert C.status_of(c["out"]["truncated"]) == 2 or not c["proof"], (a, b)


def test_walk_compiled_for_the_host_all_small_pairs(cc, small_cases):
    cases, want = small_cases
    assert len(cases) > 30000 and set(want) == {0, 1, 2, 3, 4, 5}
    assert conscheck_status(cc, cases) == want


def test_walk_compiled_for_the_host_giant_sizes(cc, giant):
    assert sum(1 for x in giant if x[0] < 2 ** 32 < x[1]) > 500
    assert conscheck_status(cc, giant) == [0] * len(giant)
    short = [(a, b, o, n, p[:-1]) for a, b, o, n, p in giant]
    assert conscheck_status(cc, short) == [2] * len(giant) == [C.check(*x) for x in short]
    bent = [(a, b, o, n, [C.flip(p[0], 9)] + p[1:]) for a, b, o, n, p in giant]
    assert conscheck_status(cc, bent) == [C.check(*x) for x in bent]


def test_walk_compiled_for_the_host_goldens(cc, golden):
    items = C.golden_items(golden)
    assert conscheck_status(cc, [x[1] for x in items]) == [C.status_of(x[2]) for x in items]


# ----------------------------------------------------------------------------- the library's host path

def test_host_path_against_goldens_and_restatement(host_path, golden, small_cases, giant):
    items = C.golden_items(golden)
    assert library_status(host_path, [x[1] for x in items]) == [C.status_of(x[2]) for x in items]
    cases, want = small_cases
    assert library_status(host_path, cases) == want
    assert library_status(host_path, giant) == [0] * len(giant)
    v, st = host_path.merkle_verify_consistency([], [], [], [], [])
    assert v.shape == (0,) and st.shape == (0,)


def test_auto_serves_a_machine_without_a_device(native, golden, monkeypatch):
    native.merkle_path(native.PV_MERKLE_AUTO)
    items = C.golden_items(golden)[:40]
    monkeypatch.setattr(native, "ensure_device", lambda *a: pytest.fail("a 40-proof AUTO batch bound a device"))
    assert library_status(native, [x[1] for x in items]) == [C.status_of(x[2]) for x in items]


def run_catchup(native, c, want=()):
    leaves = [x for lv, _ in c["replies"] for x in lv]
    blob, off = R.pack(leaves, lead=3)
    return native.merkle_catchup(c["s"], b"".join(c["frontier"]), blob, off, c["ends"], c["final_size"], c["final_root"],
                                 [p for _, p in c["replies"]], want=want)


@pytest.mark.parametrize("s", (0, 1, 65, 1023, 1024, 2 ** 20 - 1, 2 ** 32 - 3))
def test_host_catchup_against_restatement(host_path, s):
    rng = np.random.default_rng(43 + s % 1000)
    lens = [int(x) for x in rng.choice([1, 5, 64, 400], 14)] + [1, 1]
    for beyond in (0, 1, 1000):
        for tamper in (None, sum(lens) // 2):
            c = C.make_catchup(rng, s, lens, beyond, tamper)
            verdicts, status, res = run_catchup(host_path, c, want=host_path.MERKLE_OUTPUTS)
            assert status.tolist() == c["status"], (s, beyond, tamper)
            assert [bool(v) for v in verdicts] == [x == 0 for x in c["status"]]
            if tamper is None:
                assert not any(c["status"])
            else:
                first = next(r for r, e in enumerate(c["ends"]) if e - s > tamper)
                assert not any(c["status"][:first]) and all(c["status"][first:])
            # every output is the plain append's
            leaves = [x for lv, _ in c["replies"] for x in lv]
            plain = host_path.merkle_append(s, b"".join(c["frontier"]), *R.pack(leaves))
            for k in plain:
                assert np.array_equal(plain[k], res[k]), k
            v2, st2, none = run_catchup(host_path, c)
            assert none == {} and np.array_equal(v2, verdicts) and np.array_equal(st2, status)


def test_host_catchup_single_replies(host_path):
    rng = np.random.default_rng(44)
    for lens in ([1], [400], [1] * 130):
        c = C.make_catchup(rng, 13, lens, 2)
        verdicts, status, _ = run_catchup(host_path, c)
        assert status.tolist() == c["status"] == [0] * len(lens) and verdicts.all()


def test_argument_errors(native, golden):
    L = native.lib()
    ARG = native.PV_ERR_ARG
    c = golden["pairs"][-1]
    case = (c["old"], c["new"], bytes.fromhex(c["old_root"]), bytes.fromhex(c["new_root"]), [bytes.fromhex(h) for h in c["proof"]])
    old, new, oroot, nroot, proof, poff = arrays([case, case])
    st, bits = np.zeros(2, np.uint8), np.zeros(8, np.uint8)
    good = [ptr(old), ptr(new), ptr(oroot), ptr(nroot), ptr(proof), ptr(poff), 2, ptr(st), ptr(bits)]
    assert L.pv_merkle_verify_consistency_batch(*good) == native.PV_OK and st.tolist() == [0, 0] and bits[0] == 3
    for k in (0, 1, 2, 3, 5, 7, 8):  # null pointers
        bad = list(good)
        bad[k] = None
        assert L.pv_merkle_verify_consistency_batch(*bad) == ARG, k
    assert b"null pointer" in L.pv_last_error()
    for k, huge in ((0, 2 ** 48), (1, 2 ** 48), (1, 2 ** 63)):
        bad = list(good)
        bad[k] = ptr(np.array([1, huge], np.uint64))
        assert L.pv_merkle_verify_consistency_batch(*bad) == ARG
        assert b"2^48" in L.pv_last_error()
    bad = list(good)
    bad[5] = ptr(np.array([0, 5, 3], np.uint64))
    assert L.pv_merkle_verify_consistency_batch(*bad) == ARG and b"non-decreasing" in L.pv_last_error()
    bad = list(good)
    bad[6] = 2 ** 32
    assert L.pv_merkle_verify_consistency_batch(*bad) == ARG and b"2^32" in L.pv_last_error()
    assert L.pv_merkle_verify_consistency_batch(*(good[:6] + [0, None, None])) == native.PV_OK  # n = 0
    # the catch-up entry: pv_merkle_append_batch's checks, and the replies'
    blob, off = np.zeros(16, np.uint8), np.array([0, 4, 8, 12], np.uint64)
    root, pf, po = np.zeros(32, np.uint8), np.zeros(64, np.uint8), np.zeros(3, np.uint64)
    st, bits = np.zeros(2, np.uint8), np.zeros(8, np.uint8)

    def catchup(ends, n_replies=2, tree_size=0, off_=off, final=3, poff_=po, out=None, **kw):
        a = dict(frontier=None, data=ptr(blob), root=ptr(root), proof=ptr(pf), status=ptr(st), bits=ptr(bits))
        a.update(kw)
        e = None if ends is None else ptr(np.array(ends, np.uint64))
        return L.pv_merkle_catchup_batch(tree_size, a["frontier"], a["data"], ptr(off_), 3, e, n_replies, final, a["root"],
                                         a["proof"], None if poff_ is None else ptr(poff_), out, a["status"], a["bits"])

    # the first reply's proof is missing; the second ends on final_size, whose root is not the zero root given
    assert catchup([1, 3]) == native.PV_OK and st.tolist() == [2, 5] and bits[0] == 0
    for ends in ([0, 3], [2, 2], [3, 2], [1, 4]):
        assert catchup(ends) == ARG and b"reply ends" in L.pv_last_error(), ends
    assert catchup([6, 7], tree_size=5) == ARG  # no frontier
    assert catchup([1, 3], off_=np.array([0, 8, 4, 12], np.uint64)) == ARG
    assert catchup([1, 3], final=2 ** 48) == ARG
    assert catchup([1, 3], poff_=np.array([0, 2, 1], np.uint64)) == ARG
    assert catchup([1, 3], n_replies=2 ** 32) == ARG
    for k in ("root", "status", "bits"):
        assert catchup([1, 3], **{k: None}) == ARG, k
    assert catchup(None) == ARG and catchup([1, 3], poff_=None) == ARG
    bad_out = native.PvMerkleOut()
    bad_out.path = root.ctypes.data
    assert catchup([1, 3], out=ctypes.byref(bad_out)) == ARG
    assert catchup(None, n_replies=0, root=None, proof=None, poff_=None, status=None, bits=None) == native.PV_OK
    if L.pv_device_count() == 0:
        assert L.pv_merkle_verify_consistency_batch_device(*good, None) == native.PV_ERR_NOT_INIT
        assert L.pv_merkle_catchup_batch_device(0, None, ptr(blob), ptr(off), 3, ptr(po), 2, 3, ptr(root), ptr(pf), ptr(po), None,
                                                ptr(st), ptr(bits), None) == native.PV_ERR_NOT_INIT
        native.merkle_path(native.PV_MERKLE_DEVICE)
        try:
            assert L.pv_merkle_verify_consistency_batch(*good) == native.PV_ERR_NO_DEVICE
            assert catchup([1, 3]) == native.PV_ERR_NO_DEVICE
        finally:
            native.merkle_path(native.PV_MERKLE_AUTO)


def test_argument_errors_code_and_message(native, golden):
    """One bad call per check of pv_merkle_verify_consistency_batch and pv_merkle_catchup_batch, and pairs of bad
    arguments for the order of the checks: the return code and the message as the library gave them when every
    entry wrote its checks out itself (they are csrc/merkle_plan.h's now). Both entries look at the count before
    they walk an array, so 2^32 is safe to pass."""
    from test_merkle_host import assert_refusals
    L, ARG = native.lib(), native.PV_ERR_ARG
    c = golden["pairs"][-1]
    case = (c["old"], c["new"], bytes.fromhex(c["old_root"]), bytes.fromhex(c["new_root"]), [bytes.fromhex(h) for h in c["proof"]])
    good = [ptr(a) for a in arrays([case, case])] + [2, ptr(np.zeros(2, np.uint8)), ptr(np.zeros(8, np.uint8))]
    dec = np.array([0, 5, 3], np.uint64)

    def cons(**kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return L.pv_merkle_verify_consistency_batch(*args)

    blob, off = np.zeros(16, np.uint8), np.array([0, 4, 8, 12], np.uint64)
    root, pf, po = np.zeros(32, np.uint8), np.zeros(64, np.uint8), np.array([0, 1, 2], np.uint64)
    st, bits = np.zeros(2, np.uint8), np.zeros(8, np.uint8)
    paths = native.PvMerkleOut()
    paths.path = root.ctypes.data

    def catchup(ends=(1, 3), tree_size=0, frontier=None, data=ptr(blob), off_=ptr(off), n_replies=2, final=3, proof=ptr(pf),
                poff_=ptr(po), out=None, status=ptr(st)):
        e = None if ends is None else ptr(np.array(ends, np.uint64))
        return L.pv_merkle_catchup_batch(tree_size, frontier, data, off_, 3, e, n_replies, final, ptr(root), proof, poff_, out,
                                         status, ptr(bits))

    V, K, SIZES = "pv_merkle_verify_consistency_batch: ", "pv_merkle_catchup_batch: ", "tree_size + n must stay below 2^48"
    POFF, ENDS = "proof offsets must be non-decreasing over a proof array", \
        "reply ends must increase strictly within (tree_size, tree_size + n]"
    assert cons() == native.PV_OK and catchup() == native.PV_OK
    assert_refusals(L, [
        (lambda: cons(a2=None), ARG, V + "null pointer"),
        (lambda: cons(a6=2 ** 32), ARG, V + "more than 2^32 - 1 proofs"),
        (lambda: cons(a5=ptr(dec)), ARG, V + POFF),
        (lambda: cons(a4=None), ARG, V + POFF),
        (lambda: cons(a1=ptr(np.array([1, 2 ** 48], np.uint64))), ARG, V + "tree sizes must stay below 2^48"),
        # two at once: a null pointer before the count, the count before the offsets, the offsets before the sizes
        (lambda: cons(a2=None, a6=2 ** 32), ARG, V + "null pointer"),
        (lambda: cons(a6=2 ** 32, a5=ptr(dec)), ARG, V + "more than 2^32 - 1 proofs"),
        (lambda: cons(a5=ptr(dec), a0=ptr(np.array([2 ** 48, 1], np.uint64))), ARG, V + POFF),
        (lambda: catchup(out=ctypes.byref(paths)), ARG, K + "path and path_off go together"),
        (lambda: catchup(tree_size=2 ** 48 - 3, frontier=ptr(blob), ends=(2 ** 48 - 2, 2 ** 48)), ARG, K + SIZES),
        (lambda: catchup(tree_size=5, ends=(6, 7)), ARG, K + "a tree of size > 0 needs its frontier"),
        (lambda: catchup(off_=None), ARG, K + "null offsets"),
        (lambda: catchup(off_=ptr(np.array([0, 8, 4, 12], np.uint64))), ARG, K + "offsets must be non-decreasing"),
        (lambda: catchup(data=None), ARG, K + "null data"),
        (lambda: catchup(final=2 ** 48), ARG, K + "final_size must stay below 2^48"),
        (lambda: catchup(n_replies=2 ** 32), ARG, K + "more than 2^32 - 1 replies"),
        (lambda: catchup(ends=None), ARG, K + "null pointer"),
        (lambda: catchup(status=None), ARG, K + "null pointer"),
        (lambda: catchup(poff_=ptr(dec)), ARG, K + POFF),
        (lambda: catchup(proof=None), ARG, K + POFF),
        (lambda: catchup(ends=(0, 3)), ARG, K + ENDS),
        (lambda: catchup(ends=(2, 2)), ARG, K + ENDS),
        (lambda: catchup(ends=(1, 4)), ARG, K + ENDS),
        # two at once, in the order of the checks
        (lambda: catchup(out=ctypes.byref(paths), tree_size=5), ARG, K + "path and path_off go together"),
        (lambda: catchup(data=None, final=2 ** 48), ARG, K + "null data"),
        (lambda: catchup(final=2 ** 48, n_replies=2 ** 32), ARG, K + "final_size must stay below 2^48"),
        (lambda: catchup(n_replies=2 ** 32, ends=None), ARG, K + "more than 2^32 - 1 replies"),
        (lambda: catchup(status=None, poff_=ptr(dec)), ARG, K + "null pointer"),
        (lambda: catchup(poff_=ptr(dec), ends=(3, 1)), ARG, K + POFF),
    ])


# ------------------------------------------------------------------------------- the Python methods

def check_outcome(got, out, what):
    if "exc" in out:
        assert type(got).__name__ == out["exc"] and str(got) == out["msg"], (what, got)
    else:
        assert got is True, (what, got)


def test_python_sequential_and_batch_against_goldens(host_path, golden):
    from plenum_amd.exceptions import ConsistencyError, ProofError, VerifyError
    from plenum_amd.merkle import MerkleVerifier
    assert issubclass(ConsistencyError, VerifyError) and not issubclass(ConsistencyError, ProofError)
    v = MerkleVerifier()
    items = C.golden_items(golden)
    for name, args, out in items:
        try:
            got = v.verify_tree_consistency(*args)
        except Exception as ex:
            got = ex
        check_outcome(got, out, name)
    batch = v.verify_tree_consistency_batch([x[1] for x in items])
    for (name, _, out), got in zip(items, batch):
        check_outcome(got, out, name)
    assert v.verify_tree_consistency_batch([]) == []
    # items the library cannot represent fall back to the sequential method
    h = hashlib.sha256(b"x").digest()
    odd = v.verify_tree_consistency_batch([(-1, 2, h, h, []), (2, -1, h, h, []), (3, 2 ** 48, h, h, []),
                                           (2, 3, h, b"short", [h]), (2 ** 48 + 1, 2 ** 48, h, h, [])])
    assert [type(x) for x in odd] == [ValueError, ValueError, ProofError, ProofError, ValueError]
    assert str(odd[0]) == str(odd[1]) == "Negative tree size" and str(odd[2]) == "Merkle proof is too short"
    assert str(odd[3]).startswith("Bad Merkle proof: second root hash does not match. Expected hash: b'73686f7274' ,")
    assert str(odd[4]).startswith("Older tree has bigger size (281474976710657 vs 281474976710656)")


def test_python_other_hasher_goes_sequential(host_path, monkeypatch):
    from plenum_amd import _native
    from plenum_amd.merkle import CompactMerkleTree, MerkleVerifier, TreeHasher
    hasher = TreeHasher(hashlib.sha512)
    tree = CompactMerkleTree(hasher)
    leaves = [b"leaf %d" % i for i in range(9)]
    for x in leaves:
        tree.append(x)
    monkeypatch.setattr(_native, "merkle_verify_consistency", lambda *a: pytest.fail("SHA-512 went to the library"))
    monkeypatch.setattr(_native, "merkle_catchup", lambda *a, **k: pytest.fail("SHA-512 went to the library"))
    v = MerkleVerifier(hasher)
    old = CompactMerkleTree(hasher).extended(leaves[:5])
    proof = tree.consistency_proof(5, 9)
    assert v.verify_tree_consistency_batch([(5, 9, old.root_hash, tree.root_hash, proof)]) == [True]
    assert old.verify_catchup_replies([(leaves[5:7], tree.consistency_proof(7, 9)), (leaves[7:], [])], 9, tree.root_hash) == \
        [True, True]


def per_reply_loop(tree, replies, final_size, final_root):
    """catchup_rep_service.py:375-426 per reply, with the sequential methods."""
    from plenum_amd.merkle import MerkleVerifier
    out, sofar = [], []
    for leaves, proof in replies:
        sofar = sofar + list(leaves)
        temp = tree.extended(sofar)
        try:
            out.append(MerkleVerifier().verify_tree_consistency(temp.tree_size, final_size, temp.root_hash, final_root, proof))
        except Exception as ex:
            out.append(ex)
    return out


def same_outcomes(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is True and w is True) or (type(g) is type(w) and str(g) == str(w)), (g, w)


def test_verify_catchup_replies_against_goldens(host_path, golden):
    from plenum_amd.merkle import CompactMerkleTree, TreeHasher
    seen = set()
    for c in golden["catchups"]:
        tree = CompactMerkleTree(TreeHasher(), c["start"], [bytes.fromhex(h) for h in c["hashes"]])
        replies = [([bytes.fromhex(x) for x in r["leaves"]], [bytes.fromhex(h) for h in r["proof"]]) for r in c["replies"]]
        final_root = bytes.fromhex(c["final_root"])
        got = tree.verify_catchup_replies(replies, c["final_size"], final_root)
        for r, (g, rec) in enumerate(zip(got, c["replies"])):
            check_outcome(g, rec["out"], (c["start"], r))
        same_outcomes(got, per_reply_loop(tree, replies, c["final_size"], final_root))
        if c["tampered"] is not None:
            first = next(r for r, g in enumerate(got) if g is not True)
            assert all(g is not True for g in got[first:]) and first > 0
            seen.add(type(got[first]).__name__)
        assert tree.tree_size == c["start"] and tree.hashStore.leafCount == 0  # untouched
    assert seen == {"ProofError", "ConsistencyError"}


def test_verify_catchup_replies_against_the_per_reply_loop(host_path):
    from plenum_amd.merkle import CompactMerkleTree
    rng = np.random.default_rng(45)
    base = R.random_leaves(rng, 37)
    for beyond in (0, 1, 50):
        for tamper in (None, 40):
            tree = CompactMerkleTree()
            tree.append_batch(base)
            store_before = (tree.leafCount, tree.nodeCount, tree.hashes)
            lens = [1, 5, 64, 3, 1, 17]
            fresh = R.random_leaves(rng, sum(lens) + beyond)
            full = tree.extended(fresh)  # consistency_proof needs a store: build one
            whole = CompactMerkleTree()
            whole.append_batch(base + fresh)
            replies, at = [], 0
            for n in lens:
                sent = [x if at + j != tamper else x + b"!" for j, x in enumerate(fresh[at:at + n])]
                at += n
                replies.append((sent, whole.consistency_proof(37 + at, whole.tree_size) if 37 + at < whole.tree_size else []))
            got = tree.verify_catchup_replies(replies, whole.tree_size, full.root_hash)
            same_outcomes(got, per_reply_loop(tree, replies, whole.tree_size, full.root_hash))
            assert [g is True for g in got] == [tamper is None or sum(lens[:r + 1]) <= tamper for r in range(len(lens))]
            assert (tree.leafCount, tree.nodeCount, tree.hashes) == store_before and tree.tree_size == 37
            # a reply without leaves: the sequential path, same answers (it repeats the tree before it)
            with_empty = replies[:2] + [([], replies[1][1])] + replies[2:]
            got2 = tree.verify_catchup_replies(with_empty, whole.tree_size, full.root_hash)
            same_outcomes(got2, per_reply_loop(tree, with_empty, whole.tree_size, full.root_hash))
    assert CompactMerkleTree().verify_catchup_replies([], 0, R.EMPTY) == []
