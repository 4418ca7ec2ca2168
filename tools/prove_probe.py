"""Proof-generation probe: one JSON line, on one MI355X. The store has N = 1,048,576 leaves (built by
pv_merkle_append_batch, so it is a real tree).

  auto   pv_merkle_prove_batch (host buffers, the store uploaded by every call), device path forced against host
         path forced, alternately in one process, REPS calls each (min / median / max) at 64 .. 1,048,576
         queries of the mixed set: the table PV_MERKLE_AUTO_MIN_PROVE comes from
  sets   four query sets, each on the device path with everything resident (time per launch, beside a
         device-to-device copy of as many bytes as the proofs hold, the kernel's floor), on the device path
         from host buffers (the whole call, and the upload of the store alone), on the C++ host path, and
         through the sequential Python methods on a slice; every form's bytes compared with the host path's
           reads    262,144 audit paths of random leaves in the full tree (Ledger.auditProof)
           coarse   consistency_proof(end, N) for replies of 400 leaves (the seeder's CatchupReps)
           fine     the same for replies of 5 leaves
           mixed    262,144 queries of random kind at random sizes

    python tools/prove_probe.py [--n 1048576] [--seconds 0.5] [--python-queries 20000] [--no-device] [--out FILE]
"""
import argparse
import ctypes
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

AUTO_N = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 262144, 1048576)
REPS = 9
U64 = np.uint64
HIP_D2D = 3  # hipMemcpyDeviceToDevice


class ArrayStore:
    """The hash store interface the sequential methods read, over the two byte arrays."""

    def __init__(self, leaf, node):
        from plenum_amd.merkle import MemoryHashStore
        self.leaf, self.node = leaf.tobytes(), node.tobytes()
        self.getNodePosition = MemoryHashStore.getNodePosition

    def readLeaf(self, pos):
        return self.leaf[32 * pos - 32:32 * pos]

    def readNode(self, pos):
        return self.node[32 * pos - 32:32 * pos]

    leafCount = property(lambda self: len(self.leaf) // 32)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


def query_sets(rng, n, count):
    ends400 = np.append(np.arange(400, n, 400, dtype=U64), U64(n))
    ends5 = np.append(np.arange(5, n, 5, dtype=U64), U64(n))
    b = rng.integers(1, n + 1, count).astype(U64)
    kind = rng.integers(0, 3, count).astype(np.uint8)
    a = (rng.integers(0, 2 ** 62, count).astype(U64) % b) + (kind == 1).astype(U64)  # consistency: 1 <= a <= b
    reads = rng.choice(n, min(count, n), replace=False).astype(U64)
    return {"reads": (np.zeros(reads.size, np.uint8), reads, np.full(reads.size, n, U64)),
            "coarse": (np.ones(ends400.size, np.uint8), ends400, np.full(ends400.size, n, U64)),
            "fine": (np.ones(ends5.size, np.uint8), ends5, np.full(ends5.size, n, U64)),
            "mixed": (kind, a, b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--queries", type=int, default=262144)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--python-queries", type=int, default=20000)
    ap.add_argument("--no-device", action="store_true", help="host path and Python only (a machine without a GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n
    from plenum_amd import _native
    from plenum_amd.merkle import CompactMerkleTree, TreeHasher
    L = _native.lib()
    rng = np.random.default_rng(15)
    have_dev = not a.no_device
    if have_dev:
        _native.ensure_device()
    blob = rng.integers(0, 256, 40 * n, dtype=np.uint8)
    r = _native.merkle_append(0, b"", blob, np.arange(n + 1, dtype=U64) * U64(40), want=("leaf_hash", "node_hash"))
    leaf, node = r["leaf_hash"].reshape(-1), r["node_hash"].reshape(-1)
    del blob, r
    out = {"probe": "prove", "n_leaves": n, "store_bytes": int(leaf.nbytes + node.nbytes),
           "hostpath_threads": min(16, len(os.sched_getaffinity(0)))}
    sets = query_sets(rng, n, a.queries)

    def host_entry(kind, qa, qb, off, dst, status, q):
        _native.check(L.pv_merkle_prove_batch(leaf.ctypes.data, n, node.ctypes.data, kind.ctypes.data, qa.ctypes.data,
                                              qb.ctypes.data, q, off.ctypes.data, dst.ctypes.data, status.ctypes.data),
                      "pv_merkle_prove_batch")

    def dput(arr):
        p = ctypes.c_void_p()
        _native.check(L.pv_dev_alloc(ctypes.byref(p), max(arr.nbytes, 32)), "pv_dev_alloc")
        if arr.nbytes:
            _native.check(L.pv_memcpy_h2d(p, arr.ctypes.data, arr.nbytes), "pv_memcpy_h2d")
        return p

    stream = ctypes.c_void_p()
    if have_dev:
        _native.check(L.pv_stream_create(ctypes.byref(stream)), "pv_stream_create")
        hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        d_leaf, d_node = dput(leaf), dput(node)
        up = timed(lambda: (_native.check(L.pv_memcpy_h2d(d_leaf, leaf.ctypes.data, leaf.nbytes), "pv_memcpy_h2d"),
                            _native.check(L.pv_memcpy_h2d(d_node, node.ctypes.data, node.nbytes), "pv_memcpy_h2d")), 5)
        out["store_upload_ms"] = [round(min(up) * 1e3, 3), round(statistics.median(up) * 1e3, 3), round(max(up) * 1e3, 3)]
    sync = lambda: _native.check(L.pv_stream_sync(stream), "pv_stream_sync")  # noqa: E731

    def per_launch(launch):
        launch(2); sync()
        t = time.perf_counter()
        launch(1); sync()
        k = max(5, int(a.seconds / max(time.perf_counter() - t, 1e-6)) + 1)
        t = time.perf_counter()
        launch(k); sync()
        return k, (time.perf_counter() - t) * 1e3 / k

    seq = CompactMerkleTree(TreeHasher(), hashStore=ArrayStore(leaf, node))
    for name, (kind, qa, qb) in sets.items():
        q = kind.size
        off, status = _native.merkle_prove_plan(n, kind, qa, qb)
        assert not status.any()
        total = int(off[q])
        res = {"queries": q, "hashes": total, "bytes": 32 * total}
        want, st = np.zeros(32 * total, np.uint8), np.full(q, 9, np.uint8)
        _native.merkle_path(_native.PV_MERKLE_HOST)
        host_entry(kind, qa, qb, off, want, st, q)
        res["hostpath_ms"] = round(min(timed(lambda: host_entry(kind, qa, qb, off, want, st, q), 3)) * 1e3, 3)
        assert not st.any()
        if have_dev:
            _native.merkle_path(_native.PV_MERKLE_DEVICE)
            got, st2 = np.zeros(32 * total, np.uint8), np.full(q, 9, np.uint8)
            host_entry(kind, qa, qb, off, got, st2, q)
            res["host_entry_ms"] = round(min(timed(lambda: host_entry(kind, qa, qb, off, got, st2, q), 3)) * 1e3, 3)
            res["host_entry_equals_hostpath"] = bool(np.array_equal(got, want) and not st2.any())
            d_q = [dput(x) for x in (kind, qa, qb)]
            d_off, d_out, d_copy, d_st = dput(off), dput(np.zeros(32 * total, np.uint8)), dput(np.zeros(32 * total, np.uint8)), dput(st)

            def launch(k):
                for _ in range(k):
                    _native.check(L.pv_merkle_prove_batch_device(d_leaf, n, d_node, d_q[0], d_q[1], d_q[2], q, d_off, d_out, d_st,
                                                                 stream), "pv_merkle_prove_batch_device")

            def copy(k):
                for _ in range(k):
                    assert hip.hipMemcpyAsync(d_copy, d_out, 32 * total, HIP_D2D, stream) == 0

            rounds = [(per_launch(launch)[1], per_launch(copy)[1]) for _ in range(3)]  # alternately
            res["device_ms"] = [round(x, 4) for x, _ in rounds]
            res["copy_floor_ms"] = [round(x, 4) for _, x in rounds]
            res["device_queries_per_s"] = q / (statistics.median(x for x, _ in rounds) / 1e3)
            _native.check(L.pv_memcpy_d2h(got.ctypes.data, d_out, 32 * total), "pv_memcpy_d2h")
            res["device_equals_hostpath"] = bool(np.array_equal(got, want))
            for p in d_q + [d_off, d_out, d_copy, d_st]:
                L.pv_dev_free(p)
        m = min(a.python_queries, q)
        pick = rng.choice(q, m, replace=False)
        t = time.perf_counter()
        proofs = [seq.inclusion_proof(int(qa[i]), int(qb[i])) if kind[i] == 0 else
                  seq.consistency_proof(int(qa[i]), int(qb[i])) if kind[i] == 1 else [seq.merkle_tree_hash(0, int(qb[i]))]
                  for i in pick]
        res["python_queries"] = m
        res["python_queries_per_s"] = m / (time.perf_counter() - t)
        res["python_equals_hostpath"] = all(b"".join(p) == want[32 * int(off[i]):32 * int(off[i + 1])].tobytes()
                                            for i, p in zip(pick, proofs))
        out[name] = res

    if have_dev:  # the AUTO table, on the mixed set
        kind, qa, qb = sets["mixed"]
        reps = -(-AUTO_N[-1] // kind.size)
        kind, qa, qb = np.tile(kind, reps), np.tile(qa, reps), np.tile(qb, reps)
        table = []
        for cn in AUTO_N:
            off, _ = _native.merkle_prove_plan(n, kind[:cn], qa[:cn], qb[:cn])
            dst, st = np.zeros(32 * int(off[cn]), np.uint8), np.zeros(cn, np.uint8)
            ts = {"device": [], "host": []}
            for rep in range(REPS + 1):
                for mode, key in ((_native.PV_MERKLE_DEVICE, "device"), (_native.PV_MERKLE_HOST, "host")):
                    _native.merkle_path(mode)
                    one = timed(lambda: host_entry(kind, qa, qb, off, dst, st, cn), 1)
                    assert not st.any()
                    if rep:  # the first round warms both up
                        ts[key] += one
            row = {"n": cn}
            for key in ("device", "host"):
                us = sorted(x * 1e6 for x in ts[key])
                row["%s_us" % key] = [round(us[0], 1), round(statistics.median(us), 1), round(us[-1], 1)]
            table.append(row)
        out["auto_us_min_median_max"] = table
        _native.check(L.pv_stream_destroy(stream), "pv_stream_destroy")
        for p in (d_leaf, d_node):
            L.pv_dev_free(p)
    _native.merkle_path(_native.PV_MERKLE_AUTO)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
