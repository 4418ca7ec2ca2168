"""State-trie probe: one JSON line for N pairs (32-byte keys, 150-byte values) set into the state.

  root_of    PruningState.root_of's library call for the N pairs from empty (state rebuild, catch-up):
             pv_trie_update_batch alone on prepared arrays, device path and host path (up to 16 threads),
             and the Python time around it (packing the pairs, unpacking the nodes)
  set_batch  1,000 and 65,536 further pairs onto that trie: the fetch rounds through Python (rounds, total
             wall clock) and the final library call alone (every node it needs already fetched), device
             path and host path
  python     the sequential PruningState.set loop (the reference's per-call form, restated) on a slice from
             empty and, for the 1,000-pair batch, onto the same trie
  sha3       pv_sha3_256_batch on N records of 532 bytes (a full branch node), device path and host path
  crossover  pv_trie_update_batch from empty for n = 64 .. 65,536 pairs, the device and the host path forced
             alternately in one process, REPS calls each (min / median / max) and the number of nodes
             hashed: the table PV_TRIE_AUTO_MIN comes from

  build      the root of the N pairs from empty through the device builder: pv_trie_root from host buffers,
             pv_trie_root_device on buffers already on the device, and pv_trie_update_batch from empty (the
             call root_of made before), the three interleaved in one process, --reps rounds after a warm-up
             (min / median / max); then root_of and root_of_arrays through Python
  build_crossover  pv_trie_root for n = 64 .. 65,536 pairs, the device builder and the host structural path
             forced alternately, REPS calls each: the table PV_TRIE_BUILD_AUTO_MIN comes from

    python tools/trie_probe.py [--n 1048576] [--python-sets 20000] [--out FILE]
    python tools/trie_probe.py --build-only [--n 1048576] [--reps 5] [--out FILE]     the last two legs alone
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

KEY_BYTES, VALUE_BYTES = 32, 150
CROSSOVER_N = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 65536)
REPS = 9


class Call:
    """pv_trie_update_batch on arrays prepared once, so a timing holds the library call alone."""

    def __init__(self, N, root, known, keys, values):
        self.N, self.L = N, N.lib()
        hs = list(known)
        self.root = np.frombuffer(root, np.uint8)
        self.kb, self.ko = N._blob(keys)
        self.vb, self.vo = N._blob(values)
        self.nb, self.no = N._blob([known[h] for h in hs])
        self.nh = np.frombuffer(b"".join(hs) or bytes(32), np.uint8)
        self.k, self.n = len(hs), len(keys)
        self.size(2 * self.n + self.k + 16, int(self.nb.size + self.kb.size + self.vb.size) + 640 * self.n + 1024)

    def size(self, node_cap, blob_cap):
        self.rootbuf, self.hashes = np.zeros(32, np.uint8), np.zeros((node_cap, 32), np.uint8)
        self.blob, self.off, self.len = np.zeros(blob_cap, np.uint8), np.zeros(node_cap, np.uint64), np.zeros(node_cap, np.uint64)
        self.miss = np.zeros((16 * self.n + 16, 32), np.uint8)
        self.out = self.N.PvTrieOut(self.rootbuf.ctypes.data, self.hashes.ctypes.data, node_cap, self.blob.ctypes.data,
                                    blob_cap, self.off.ctypes.data, self.len.ctypes.data, self.miss.ctypes.data,
                                    self.miss.shape[0])

    def run(self):
        p = self.N._ptr
        rc = self.L.pv_trie_update_batch(p(self.root), p(self.nh), p(self.nb), p(self.no), self.k, p(self.kb), p(self.ko),
                                         p(self.vb), p(self.vo), self.n, ctypes.byref(self.out))
        if rc == self.N.PV_TRIE_NEED_SPACE:
            self.size(int(self.out.n_nodes), int(self.out.blob_bytes))
            return self.run()
        self.N.check(rc, "pv_trie_update_batch")
        return self.rootbuf.tobytes()


class RootCall:
    """pv_trie_root and pv_trie_root_device on arrays prepared once (raw values: the library wraps them)."""

    def __init__(self, N, keys, raw_values):
        self.N, self.L, self.n = N, N.lib(), len(keys)
        self.keys = np.frombuffer(b"".join(keys), np.uint8)
        self.vb, self.vo = N._blob(raw_values)
        self.out = N.PvTrieRootOut()
        self.dev = None

    def run(self):
        p = self.N._ptr
        self.N.check(self.L.pv_trie_root(p(self.keys), KEY_BYTES, self.n, p(self.vb), p(self.vo), self.N.PV_TRIE_ROOT_WRAP,
                                         ctypes.byref(self.out)), "pv_trie_root")
        return bytes(self.out.root)

    def upload(self):
        self.dev = [ctypes.c_void_p() for _ in range(4)]
        for d, a in zip(self.dev, (self.keys, self.vb, self.vo, np.zeros(32, np.uint8))):
            self.N.check(self.L.pv_dev_alloc(ctypes.byref(d), a.nbytes), "pv_dev_alloc")
            self.N.check(self.L.pv_memcpy_h2d(d, self.N._ptr(a), a.nbytes), "h2d")

    def run_device(self):
        d_keys, d_vb, d_vo, d_root = self.dev
        self.N.check(self.L.pv_trie_root_device(d_keys, KEY_BYTES, self.n, d_vb, d_vo, self.N.PV_TRIE_ROOT_WRAP, d_root,
                                                ctypes.byref(self.out), None), "pv_trie_root_device")
        self.N.check(self.L.pv_sync(), "pv_sync")  # the root is there

    def device_root(self):
        got = np.zeros(32, np.uint8)
        self.N.check(self.L.pv_memcpy_d2h(self.N._ptr(got), self.dev[3], 32), "d2h")
        return got.tobytes()

    def free(self):
        for d in self.dev or ():
            self.L.pv_dev_free(d)
        self.dev = None


def spread(ts, scale=1e3, digits=2):
    xs = sorted(x * scale for x in ts)
    return [round(xs[0], digits), round(statistics.median(xs), digits), round(xs[-1], digits)]


def build_legs(N, S, keys, raw, wrapped, reps, out):
    """The device builder against the call root_of made before, interleaved; then the crossover table."""
    n = len(keys)
    N.ensure_device()
    N.trie_path(N.PV_TRIE_DEVICE)
    old, new = Call(N, S.BLANK_ROOT, {}, keys, wrapped), RootCall(N, keys, raw)
    new.upload()
    legs = (("update_batch_from_empty", old.run), ("trie_root_host_buffers", new.run), ("trie_root_device_resident", new.run_device))
    ts = {name: [] for name, _ in legs}
    for rep in range(reps + 1):
        for name, fn in legs:
            one = timed(fn, 1)
            if rep:  # the first round sizes the buffers and warms up
                ts[name] += one
    roots = (old.rootbuf.tobytes(), new.run(), new.device_root())
    out["build_roots_equal"] = roots[0] == roots[1] == roots[2]
    for name, _ in legs:
        out["build_%s_ms_min_median_max" % name] = spread(ts[name])
    out["build_counts"] = {f: int(getattr(new.out, f)) for f in ("n_keys", "n_nodes", "n_records", "arena_bytes", "max_depth",
                                                                  "launches", "tail_records")}
    new.free()
    items = list(zip(keys, raw))
    t = time.perf_counter()
    r1 = S.PruningState.root_of(items)
    out["build_root_of_through_python_ms"] = (time.perf_counter() - t) * 1e3
    karr = np.frombuffer(b"".join(keys), np.uint8).reshape(n, KEY_BYTES)
    vb, vo = N._blob(raw)
    t = time.perf_counter()
    r2 = S.PruningState.root_of_arrays(karr, vb, vo)
    out["build_root_of_arrays_ms"] = (time.perf_counter() - t) * 1e3
    out["build_python_roots_equal"] = r1 == r2 == roots[0]
    table = []
    for cn in CROSSOVER_N:
        if cn > n:
            break
        call = RootCall(N, keys[:cn], raw[:cn])
        ts = {"device": [], "host": []}
        for rep in range(REPS + 1):
            for mode, key in ((N.PV_TRIE_DEVICE, "device"), (N.PV_TRIE_HOST, "host")):
                N.trie_path(mode)
                one = timed(call.run, 1)
                if rep:
                    ts[key] += one
        table.append({"n": cn, "device_us": spread(ts["device"], 1e6, 1), "host_us": spread(ts["host"], 1e6, 1)})
    N.trie_path(N.PV_TRIE_AUTO)
    out["build_crossover_us_min_median_max"] = table


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


def both_paths(N, call, reps, out, name):
    roots = {}
    for mode, key in ((N.PV_TRIE_HOST, "hostpath"), (N.PV_TRIE_DEVICE, "device")):
        N.trie_path(mode)
        roots[key] = call.run()  # sizes the buffers and the workspace
        out["%s_%s_ms" % (name, key)] = min(timed(call.run, reps)) * 1e3
    out["%s_nodes" % name] = int(call.out.n_nodes)
    out["%s_node_bytes" % name] = int(call.out.blob_bytes)
    out["%s_device_launches" % name] = int(call.out.launches)
    out["%s_device_equals_hostpath" % name] = roots["device"] == roots["hostpath"]
    return roots["device"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--python-sets", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-only", action="store_true", help="the device-builder legs alone")
    ap.add_argument("--reps", type=int, default=5, help="interleaved rounds of the build leg")
    ap.add_argument("--trace-leg", action="store_true",
                    help="pv_trie_root from host buffers --reps + 1 times and nothing else (for a kernel trace)")
    a = ap.parse_args()
    n = a.n
    from plenum_amd import _native as N
    from plenum_amd import state_trie as S
    rng = np.random.default_rng(9)

    raw_of = {}

    def pairs(m):
        kb, vb = rng.bytes(KEY_BYTES * m), rng.bytes(VALUE_BYTES * m)
        raw_of[m] = [vb[VALUE_BYTES * i:VALUE_BYTES * (i + 1)] for i in range(m)]
        return ([kb[KEY_BYTES * i:KEY_BYTES * (i + 1)] for i in range(m)], [S.rlp_encode([v]) for v in raw_of[m]])

    keys, values = pairs(n)
    out = {"probe": "trie", "n": n, "key_bytes": KEY_BYTES, "value_bytes": VALUE_BYTES,
           "hostpath_threads": min(16, len(os.sched_getaffinity(0)))}
    raw = raw_of.pop(n)
    if a.trace_leg:
        N.ensure_device()
        N.trie_path(N.PV_TRIE_DEVICE)
        call = RootCall(N, keys, raw)
        out["trace_leg_ms"] = [round(x * 1e3, 2) for x in timed(call.run, a.reps + 1)]
        print(json.dumps(out))
        return
    if a.build_only:
        build_legs(N, S, keys, raw, values, a.reps, out)
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return

    # the sequential Python loop from empty, on a slice
    m = min(a.python_sets, n)
    st = S.PruningState(S.KeyValueStorageInMemory())
    t = time.perf_counter()
    for k, v in zip(keys[:m], values[:m]):
        st._trie.update(k, v)
    out["python_sets"] = m
    out["python_sets_per_s"] = m / (time.perf_counter() - t)
    N.ensure_device()
    N.trie_path(N.PV_TRIE_HOST)
    out["python_equals_library"] = st.headHash == Call(N, S.BLANK_ROOT, {}, keys[:m], values[:m]).run()

    # root_of: the library call alone, then through Python
    root = both_paths(N, Call(N, S.BLANK_ROOT, {}, keys, values), 2, out, "root_of")
    for key in ("hostpath", "device"):
        out["root_of_%s_sets_per_s" % key] = n / (out["root_of_%s_ms" % key] / 1e3)
    N.trie_path(N.PV_TRIE_DEVICE)
    t = time.perf_counter()
    new_root, nodes = N.trie_update(S.BLANK_ROOT, None, keys, values)
    out["root_of_device_through_python_ms"] = (time.perf_counter() - t) * 1e3
    assert new_root == root
    kv = S.KeyValueStorageInMemory()
    for h, enc in nodes:
        kv.put(h, enc)
    del nodes

    # batches onto that trie
    for bn in (1000, 65536):
        bk, bv = pairs(bn)
        name = "set_batch_%d" % bn
        known = {}

        def fetch(h):
            known[h] = kv.get(h)
            return known[h]

        N.trie_path(N.PV_TRIE_DEVICE)
        t = time.perf_counter()
        want_root, _ = N.trie_update(root, fetch, bk, bv)
        out["%s_device_through_python_ms" % name] = (time.perf_counter() - t) * 1e3
        out["%s_rounds" % name] = N.trie_last["rounds"]
        out["%s_fetched" % name] = len(known)
        assert both_paths(N, Call(N, root, known, bk, bv), 5, out, name) == want_root
        if bn == 1000:
            st = S.PruningState(kv)
            st._trie.set_root_hash(root)
            t = time.perf_counter()
            for k, v in zip(bk, bv):
                st._trie.update(k, v)
            out["%s_python_ms" % name] = (time.perf_counter() - t) * 1e3
            out["%s_python_equals_library" % name] = st.headHash == want_root

    # the hash on its own
    recs = rng.integers(0, 256, 532 * n, dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(532)
    digs = {}
    for mode, key in ((N.PV_TRIE_HOST, "hostpath"), (N.PV_TRIE_DEVICE, "device")):
        N.trie_path(mode)
        digs[key] = N.sha3_256_batch(recs, off)
        out["sha3_%s_ms" % key] = min(timed(lambda: N.sha3_256_batch(recs, off), 2)) * 1e3
    out["sha3_device_equals_hostpath"] = bool(np.array_equal(digs["device"], digs["hostpath"]))

    # crossover: the device path against the host path, forced alternately in one process
    table = []
    for cn in CROSSOVER_N:
        if cn > n:
            break
        call = Call(N, S.BLANK_ROOT, {}, keys[:cn], values[:cn])
        ts = {"device": [], "host": []}
        for rep in range(REPS + 1):
            for mode, key in ((N.PV_TRIE_DEVICE, "device"), (N.PV_TRIE_HOST, "host")):
                N.trie_path(mode)
                one = timed(call.run, 1)
                if rep:  # the first round warms both up
                    ts[key] += one
        row = {"n": cn, "nodes": int(call.out.n_nodes)}
        for key in ("device", "host"):
            us = sorted(x * 1e6 for x in ts[key])
            row["%s_us" % key] = [round(us[0], 1), round(statistics.median(us), 1), round(us[-1], 1)]
        table.append(row)
    N.trie_path(N.PV_TRIE_AUTO)
    out["crossover_us_min_median_max"] = table
    build_legs(N, S, keys, raw, values, a.reps, out)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
