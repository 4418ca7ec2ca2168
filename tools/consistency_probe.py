"""Consistency-proof and catch-up probe: one JSON line, on one MI355X.

  auto        pv_merkle_verify_consistency_batch, device path forced against host path forced, interleaved
              in one process, REPS calls each (min / median / max) at 64 .. 65,536 proofs: the table
              PV_MERKLE_AUTO_MIN_CONSISTENCY comes from
  consistency 262,144 proofs PROOF(a, F) against the catch-up's final tree, F = 2 * 2^20 + 12,345 + 54,321
              leaves, for old sizes a inside the appended leaves (16,384 distinct ones, each 16 times):
              device-resident time per launch, the C++ host path on up to 16 threads, and
              MerkleVerifier.verify_tree_consistency in a Python loop on a slice
  catchup     N = 1,048,576 leaves of 300 B onto a tree of 2^20 + 12,345 leaves (random frontier), the final
              tree 54,321 leaves larger, as replies of 400 leaves and of 5 leaves:
              device-resident pv_merkle_catchup_batch_device with frontier + root only beside
              pv_merkle_append_batch_device timed in the same run (the difference is what verification
              adds), the host path, and the per-reply Python loop (temporary tree extended, then
              verify_tree_consistency) on a slice; statuses and roots compared between all of them

    python tools/consistency_probe.py [--n 1048576] [--seconds 1.0] [--python-leaves 100000] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "indy-plenum_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

LEAF_BYTES = 300
START = (1 << 20) + 12345
BEYOND = 54321
AUTO_N = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 65536)
REPS = 15
U64 = np.uint64


def popcount(x):
    x = x.astype(U64)
    x = x - ((x >> U64(1)) & U64(0x5555555555555555))
    x = (x & U64(0x3333333333333333)) + ((x >> U64(2)) & U64(0x3333333333333333))
    x = (x + (x >> U64(4))) & U64(0x0F0F0F0F0F0F0F0F)
    return (x * U64(0x0101010101010101)) >> U64(56)


class Hashes:
    """The hashes of a tree known from size s on (frontier at s, leaf hashes and nodes of the leaves appended
    since, as pv_merkle_append_batch returns them) as one table, and PROOF(e, F) for many e at once."""

    def __init__(self, s, frontier, leaf_hash, node_hash, F):
        self.s, self.F = s, F
        self.nf, self.nl = len(frontier) // 32, len(leaf_hash)
        self.table = [np.asarray(frontier, np.uint8).reshape(-1, 32), leaf_hash, node_hash]
        self.spine = {}  # level -> row of the incomplete node [j << h, F), j = (F - 1) >> h
        self.extra = []
        self.base = self.nf + self.nl + len(node_hash)

    def complete_row(self, u, h):
        """Row of the aligned node of height h completed at size u (arrays)."""
        s = U64(self.s)
        u, h = u.astype(U64), h.astype(U64)
        old = popcount(np.full(u.shape, self.s, U64) >> (h + U64(1)))
        leaf = U64(self.nf) + (u - U64(1) - s)
        node = U64(self.nf + self.nl) + (u - U64(1)) - popcount(u - U64(1)) + (h - U64(1)) - (s - popcount(np.array([s]))[0])
        return np.where(u <= s, old, np.where(h == 0, leaf, node)).astype(np.int64)

    def row_bytes(self, row):
        for t in self.table:
            if row < len(t):
                return t[row].tobytes()
            row -= len(t)
        return self.extra[row]

    def spine_row(self, h):
        """Row of the node of height h that holds leaf F - 1 (complete or not)."""
        if h in self.spine:
            return self.spine[h]
        j = (self.F - 1) >> h
        if (j + 1) << h <= self.F:  # complete
            row = int(self.complete_row(np.array([(j + 1) << h], U64), np.array([h], U64))[0])
        elif ((2 * j + 1) << (h - 1)) < self.F:  # two children
            left = int(self.complete_row(np.array([(2 * j + 1) << (h - 1)], U64), np.array([h - 1], U64))[0])
            digest = hashlib.sha256(b"\x01" + self.row_bytes(left) + self.row_bytes(self.spine_row(h - 1))).digest()
            self.extra.append(digest)
            row = self.base + len(self.extra) - 1
        else:  # only a left child: the node is its child
            row = self.spine_row(h - 1)
        self.spine[h] = row
        return row

    def proofs(self, e):
        """(proof bytes uint8[32 total], proof_off uint64[len(e) + 1]) of PROOF(e[i], F), e[i] < F, e[i] > 0."""
        e = np.asarray(e, U64)
        idx0, F1 = e - U64(1), self.F - 1
        started = np.zeros(e.shape, bool)
        who, key, rows = [], [], []
        ids = np.arange(e.shape[0])
        for h in range(F1.bit_length() + 1):
            idx, last = idx0 >> U64(h), F1 >> h
            odd = (idx & U64(1)).astype(bool)
            begin = ~started & ~odd
            first = begin & (idx != 0)  # the stripped subtree's root opens the proof
            hh = np.full(e.shape, h, U64)
            if first.any():
                who.append(ids[first]); key.append(np.full(first.sum(), 2 * h)); rows.append(self.complete_row(e[first], hh[first]))
            started |= begin
            left = started & odd
            if left.any():
                who.append(ids[left]); key.append(np.full(left.sum(), 2 * h + 1))
                rows.append(self.complete_row(idx[left] << U64(h), hh[left]))
            right = started & ~odd & (idx < U64(last))
            if right.any():
                full = ((idx + U64(2)) << U64(h)) <= U64(self.F)
                r = np.where(full[right], self.complete_row(((idx + U64(2)) << U64(h))[right], hh[right]),
                             self.spine_row(h) if (~full[right]).any() else 0)
                who.append(ids[right]); key.append(np.full(right.sum(), 2 * h + 1)); rows.append(r)
        who, key, rows = np.concatenate(who), np.concatenate(key), np.concatenate(rows)
        order = np.lexsort((key, who))
        table = np.concatenate(self.table + [np.frombuffer(b"".join(self.extra) or bytes(32), np.uint8).reshape(-1, 32)])
        off = np.zeros(e.shape[0] + 1, U64)
        np.cumsum(np.bincount(who, minlength=e.shape[0]), out=off[1:])
        return np.ascontiguousarray(table[rows[order]]).reshape(-1), off


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--python-leaves", type=int, default=100000)
    ap.add_argument("--proofs", type=int, default=262144)
    ap.add_argument("--no-device", action="store_true", help="host path and Python only (a machine without a GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n
    from plenum_amd import _native
    from plenum_amd.merkle import CompactMerkleTree, MerkleVerifier, TreeHasher
    L = _native.lib()
    rng = np.random.default_rng(9)
    total = n + BEYOND
    blob = rng.integers(0, 256, total * LEAF_BYTES, dtype=np.uint8)
    off = np.arange(total + 1, dtype=U64) * U64(LEAF_BYTES)
    frontier = rng.integers(0, 256, 32 * bin(START).count("1"), dtype=np.uint8)
    front_list = [frontier[32 * i:32 * i + 32].tobytes() for i in range(len(frontier) // 32)]
    out = {"probe": "consistency", "n": n, "leaf_bytes": LEAF_BYTES, "start_size": START, "beyond": BEYOND}
    _native.merkle_path(_native.PV_MERKLE_HOST)
    final = _native.merkle_append(START, frontier, blob, off, want=("leaf_hash", "node_hash", "root"))
    F = START + total
    final_root = final["root"].tobytes()
    hashes = Hashes(START, frontier, final["leaf_hash"], final["node_hash"], F)
    have_dev = not a.no_device
    if have_dev:
        _native.ensure_device()

    def dput(arr, slack=0):
        p = ctypes.c_void_p()
        _native.check(L.pv_dev_alloc(ctypes.byref(p), max(arr.nbytes, 32) + slack), "pv_dev_alloc")
        if arr.nbytes:
            _native.check(L.pv_memcpy_h2d(p, arr.ctypes.data, arr.nbytes), "pv_memcpy_h2d")
        return p

    def dget(p, nbytes):
        got = np.zeros(nbytes, np.uint8)
        _native.check(L.pv_memcpy_d2h(got.ctypes.data, p, nbytes), "pv_memcpy_d2h")
        return got

    def per_launch(launch, sync):
        launch(2); sync()
        t = time.perf_counter()
        launch(1); sync()
        k = max(3, int(a.seconds / max(time.perf_counter() - t, 1e-6)) + 1)
        t = time.perf_counter()
        launch(k); sync()
        return k, (time.perf_counter() - t) * 1e3 / k

    stream = ctypes.c_void_p()
    if have_dev:
        _native.check(L.pv_stream_create(ctypes.byref(stream)), "pv_stream_create")
    sync = lambda: _native.check(L.pv_stream_sync(stream), "pv_stream_sync")  # noqa: E731

    # ---- consistency proofs PROOF(a, F): old trees that end inside the appended leaves
    distinct = min(16384, a.proofs)
    olds = np.sort(rng.choice(np.arange(START + 1, F, dtype=U64), distinct, replace=False))
    pbytes, poff = hashes.proofs(olds)
    roots = np.zeros((distinct, 32), np.uint8)
    # the old roots: what the catch-up entry's host path folds, read back through a tiny catch-up per old size would
    # hash everything again; fold them here from the append's per-leaf roots of one more host call instead
    per_leaf = _native.merkle_append(START, frontier, blob, off, want=("roots",))["roots"]
    roots[:] = per_leaf[(olds - U64(START) - U64(1)).astype(np.int64)]
    del per_leaf
    reps = max(1, a.proofs // distinct)
    np_ = distinct * reps
    old_size = np.tile(olds, reps)
    new_size = np.full(np_, F, U64)
    old_root = np.ascontiguousarray(np.tile(roots, (reps, 1))).reshape(-1)
    new_root = np.ascontiguousarray(np.tile(np.frombuffer(final_root, np.uint8), np_))
    proof = np.tile(pbytes, reps)
    each = np.diff(poff)
    proof_off = np.zeros(np_ + 1, U64)
    np.cumsum(np.tile(each, reps), out=proof_off[1:])
    out["consistency_proofs"] = np_
    out["consistency_hashes_per_proof"] = float(each.mean())

    def host_entry(m, st, bits):
        _native.check(L.pv_merkle_verify_consistency_batch(old_size.ctypes.data, new_size.ctypes.data, old_root.ctypes.data,
                                                           new_root.ctypes.data, proof.ctypes.data, proof_off.ctypes.data, m,
                                                           st.ctypes.data, bits.ctypes.data), "pv_merkle_verify_consistency_batch")

    st_h, bits_h = np.full(np_, 9, np.uint8), np.zeros((np_ + 7) // 8, np.uint8)
    host_entry(np_, st_h, bits_h)
    out["consistency_hostpath_ms"] = min(timed(lambda: host_entry(np_, st_h, bits_h), 3)) * 1e3
    out["consistency_hostpath_all_true"] = bool(not st_h.any() and np.unpackbits(bits_h, count=np_, bitorder="little").all())
    out["hostpath_threads"] = min(16, len(os.sched_getaffinity(0)))
    m = min(20000, np_)
    verifier = MerkleVerifier()
    items = [(int(old_size[i]), F, old_root[32 * i:32 * i + 32].tobytes(), final_root,
              [proof[32 * j:32 * j + 32].tobytes() for j in range(int(proof_off[i]), int(proof_off[i + 1]))]) for i in range(m)]
    t = time.perf_counter()
    ok = all(verifier.verify_tree_consistency(*x) for x in items)
    out["consistency_python_proofs"] = m
    out["consistency_python_proofs_per_s"] = m / (time.perf_counter() - t)
    out["consistency_python_all_true"] = bool(ok)
    if have_dev:
        d_in = [dput(x, 32) for x in (old_size, new_size, old_root, new_root, proof, proof_off)]
        d_st, d_w = dput(np.full(np_, 9, np.uint8)), dput(np.zeros((np_ + 63) // 64, U64))

        def launch(k):
            for _ in range(k):
                _native.check(L.pv_merkle_verify_consistency_batch_device(*d_in, np_, d_st, d_w, stream),
                              "pv_merkle_verify_consistency_batch_device")

        k, ms = per_launch(launch, sync)
        out["consistency_device_launches"], out["consistency_device_ms"] = k, ms
        out["consistency_device_proofs_per_s"] = np_ / (ms / 1e3)
        out["consistency_device_equals_hostpath"] = bool(
            np.array_equal(dget(d_st, np_), st_h) and
            np.array_equal(dget(d_w, 8 * ((np_ + 63) // 64))[:bits_h.size], bits_h))
        for p in d_in + [d_st, d_w]:
            L.pv_dev_free(p)
        # the AUTO table
        table = []
        for cn in AUTO_N:
            if cn > np_:
                break
            st, bits = np.zeros(cn, np.uint8), np.zeros((cn + 7) // 8, np.uint8)
            ts = {"device": [], "host": []}
            for rep in range(REPS + 1):
                for mode, key in ((_native.PV_MERKLE_DEVICE, "device"), (_native.PV_MERKLE_HOST, "host")):
                    _native.merkle_path(mode)
                    one = timed(lambda: host_entry(cn, st, bits), 1)
                    assert not st.any()
                    if rep:  # the first round warms both up
                        ts[key] += one
            row = {"n": cn}
            for key in ("device", "host"):
                us = sorted(x * 1e6 for x in ts[key])
                row["%s_us" % key] = [round(us[0], 1), round(statistics.median(us), 1), round(us[-1], 1)]
            table.append(row)
        out["auto_us_min_median_max"] = table
    del old_size, new_size, old_root, new_root, proof, proof_off, items

    # ---- catch-up
    if have_dev:
        d_blob, d_off, d_f = dput(blob[:n * LEAF_BYTES], _native.PV_BLOB_SLACK), dput(off[:n + 1]), dput(frontier)
        d_root_in = dput(np.frombuffer(final_root, np.uint8))
        d_front, d_root = dput(np.zeros(2048, np.uint8)), dput(np.zeros(32, np.uint8))
        o = _native.PvMerkleOut()
        o.frontier, o.root = d_front.value, d_root.value

        def plain(k):
            for _ in range(k):
                _native.check(L.pv_merkle_append_batch_device(START, d_f, d_blob, d_off, n, ctypes.byref(o), stream),
                              "pv_merkle_append_batch_device")
    lean = _native.merkle_append(START, frontier, blob[:n * LEAF_BYTES + 1], off[:n + 1], want=("frontier", "root"))
    for per in (400, 5):
        ends = np.arange(START + per, START + n + 1, per, dtype=U64)
        if int(ends[-1]) != START + n:
            ends = np.append(ends, U64(START + n))
        R = ends.shape[0]
        pb, po = hashes.proofs(ends)
        tag = "catchup%d" % per
        out[tag + "_replies"] = R
        st_h, bits_h = np.full(R, 9, np.uint8), np.zeros((R + 7) // 8, np.uint8)
        root_h, front_h = np.zeros(32, np.uint8), np.zeros(2048, np.uint8)
        oh = _native.PvMerkleOut()
        oh.root, oh.frontier = root_h.ctypes.data, front_h.ctypes.data
        root_np = np.frombuffer(final_root, np.uint8)

        def host_catchup():
            _native.check(L.pv_merkle_catchup_batch(START, frontier.ctypes.data, blob.ctypes.data, off.ctypes.data, n,
                                                    ends.ctypes.data, R, F, root_np.ctypes.data, pb.ctypes.data, po.ctypes.data,
                                                    ctypes.byref(oh), st_h.ctypes.data, bits_h.ctypes.data),
                          "pv_merkle_catchup_batch")

        _native.merkle_path(_native.PV_MERKLE_HOST)
        host_catchup()
        out[tag + "_hostpath_ms"] = min(timed(host_catchup, 2)) * 1e3
        out[tag + "_hostpath_all_true"] = bool(not st_h.any() and np.unpackbits(bits_h, count=R, bitorder="little").all())
        out[tag + "_hostpath_root_equals_append"] = bool(root_h.tobytes() == lean["root"].tobytes())
        if have_dev:
            _native.merkle_path(_native.PV_MERKLE_DEVICE)
            st_e, bits_e = np.full(R, 9, np.uint8), np.zeros((R + 7) // 8, np.uint8)
            keep = (st_h, bits_h)
            st_h, bits_h = st_e, bits_e
            host_catchup()
            out[tag + "_host_entry_ms"] = min(timed(host_catchup, 2)) * 1e3
            st_h, bits_h = keep
            out[tag + "_host_entry_equals_hostpath"] = bool(np.array_equal(st_e, st_h) and np.array_equal(bits_e, bits_h))
            d_ends, d_pb, d_po = dput(ends), dput(pb, 32), dput(po)
            d_st, d_w = dput(np.full(R, 9, np.uint8)), dput(np.zeros((R + 63) // 64, U64))

            def catchup(k):
                for _ in range(k):
                    _native.check(L.pv_merkle_catchup_batch_device(START, d_f, d_blob, d_off, n, d_ends, R, F, d_root_in, d_pb,
                                                                   d_po, ctypes.byref(o), d_st, d_w, stream),
                                  "pv_merkle_catchup_batch_device")

            # plain append and catch-up alternately, three rounds: the difference is what matters
            pairs = []
            for _ in range(3):
                _, ms_plain = per_launch(plain, sync)
                _, ms_catch = per_launch(catchup, sync)
                pairs.append([round(ms_plain, 4), round(ms_catch, 4)])
            out[tag + "_device_plain_vs_catchup_ms"] = pairs
            out[tag + "_device_added_ms"] = statistics.median(c - p for p, c in pairs)
            out[tag + "_device_equals_hostpath"] = bool(
                np.array_equal(dget(d_st, R), st_h) and np.array_equal(dget(d_w, 8 * ((R + 63) // 64))[:bits_h.size], bits_h)
                and dget(d_root, 32).tobytes() == lean["root"].tobytes()
                and dget(d_front, 2048)[:lean["frontier"].size].tobytes() == lean["frontier"].tobytes())
            for p in (d_ends, d_pb, d_po, d_st, d_w):
                L.pv_dev_free(p)
        # the per-reply Python loop on a slice: temporary tree extended by the reply, then the check
        m = min(a.python_leaves, n) // per
        tree = CompactMerkleTree(TreeHasher(), START, front_list)
        verifier = MerkleVerifier()
        t = time.perf_counter()
        ok = True
        for r in range(m):
            tree.extend([blob[LEAF_BYTES * i:LEAF_BYTES * (i + 1)].tobytes() for i in range(r * per, (r + 1) * per)])
            prf = [pb[32 * j:32 * j + 32].tobytes() for j in range(int(po[r]), int(po[r + 1]))]
            ok &= verifier.verify_tree_consistency(tree.tree_size, F, tree.root_hash, final_root, prf)
        out[tag + "_python_leaves"] = m * per
        out[tag + "_python_leaves_per_s"] = m * per / (time.perf_counter() - t)
        out[tag + "_python_all_true"] = bool(ok)
    _native.merkle_path(_native.PV_MERKLE_AUTO)
    if have_dev:
        _native.check(L.pv_stream_destroy(stream), "pv_stream_destroy")
        for p in (d_blob, d_off, d_f, d_root_in, d_front, d_root):
            L.pv_dev_free(p)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
