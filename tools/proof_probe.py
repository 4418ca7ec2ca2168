"""State-proof probe: one JSON line for P proofs out of a trie of N pairs (32-byte keys, 150-byte values).

  python     the sequential PruningState.verify_state_proof on a slice, proofs/s
  hostpath   pv_trie_verify_proofs with the host path forced (up to 16 threads)
  device     the same entry with the device path forced: staging, two launches, statuses back
  resident   pv_trie_verify_proofs_device on buffers uploaded once: host clock over back-to-back calls and one
             synchronise at the end
  sizes      records and bytes per proof
A few per cent of the proofs are corrupted (wrong value, a node dropped, a byte flipped) or prove an absence.
All paths must give identical statuses; the Python slice must agree wherever the library decides.

  --threshold  instead: the host entry for 64 .. 65,536 proof records, the device and the host path forced
               alternately in one process, REPS calls each (min / median / max): the table
               PV_TRIE_PROOF_AUTO_MIN comes from. --append adds the run to the runs already in --out.

    python tools/proof_probe.py [--n 1048576] [--proofs 262144] [--python-proofs 2000] [--out FILE]
    python tools/proof_probe.py --threshold [--append] [--out FILE]
--out defaults to profiles/r11/state_proof/probe_final.json (probe_threshold.json with --threshold).
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
THRESHOLD_NODES = (64, 128, 192, 256, 352, 512, 768, 1024, 2048, 4096, 16384, 65536)
REPS = 9


def build(N, S, n, rng):
    """A state of n random pairs, built by one library call; (state, keys, values)."""
    kb, vb = rng.bytes(KEY_BYTES * n), rng.bytes(VALUE_BYTES * n)
    keys = [kb[KEY_BYTES * i:KEY_BYTES * (i + 1)] for i in range(n)]
    values = [vb[VALUE_BYTES * i:VALUE_BYTES * (i + 1)] for i in range(n)]
    st = S.PruningState(S.KeyValueStorageInMemory())
    st.set_batch(list(zip(keys, values)))
    return st, keys, values


def proofs_for(S, st, keys):
    """Per key the proof's records (the stored RLPs on its path, the root's last) and the raw value found."""
    trie, cache, out = st._trie, {}, []
    root_enc = S.rlp_encode(trie.root_node)
    for k in keys:
        load, seen = trie._recorder(cache)
        raw = trie._get_with(trie.root_node, S.bin_to_nibbles(k), load)
        out.append((list(seen) + [root_enc], raw))
    return out


class Arrays:
    """The arrays of one PvProofIn, prepared once, so a timing holds the library call alone."""

    def __init__(self, N, root, keys, vals, proofs):
        self.N, self.L = N, N.lib()
        recs = [r for p in proofs for r in p]
        self.blob, self.off = N._blob(recs)
        self.first = np.zeros(len(proofs) + 1, np.uint64)
        np.cumsum([len(p) for p in proofs], out=self.first[1:])
        self.qp = np.arange(len(keys), dtype=np.uint32)
        self.roots = np.frombuffer(root * len(keys), np.uint8)
        self.kb, self.ko = N._blob(keys)
        self.vb, self.vo = N._blob(vals)
        self.nn, self.nq = len(recs), len(keys)
        self.status = np.zeros(self.nq, np.uint8)
        p = lambda a: a.ctypes.data  # noqa: E731
        self.arg = N.PvProofIn(p(self.blob), p(self.off), self.nn, p(self.first), len(proofs), p(self.qp), p(self.roots),
                               p(self.kb), p(self.ko), p(self.vb), p(self.vo), self.nq, None)

    def run(self):
        self.N.check(self.L.pv_trie_verify_proofs(ctypes.byref(self.arg), self.N._ptr(self.status)), "pv_trie_verify_proofs")
        return self.status.copy()

    def resident(self, reps):
        """(statuses, seconds per call) of the device-buffer entry on buffers uploaded once."""
        N, L = self.N, self.L
        host = {"blob": np.concatenate([self.blob, np.zeros(8, np.uint8)]), "off": self.off, "first": self.first, "qp": self.qp,
                "root": self.roots, "kb": self.kb, "ko": self.ko, "vb": self.vb, "vo": self.vo}
        d = {}
        try:
            for name, a in list(host.items()) + [("status", self.status), ("hash", np.zeros(32 * self.nn + 8, np.uint8))]:
                d[name] = ctypes.c_void_p()
                N.check(L.pv_dev_alloc(ctypes.byref(d[name]), max(a.nbytes, 8)), "pv_dev_alloc")
                if name in host:
                    N.check(L.pv_memcpy_h2d(d[name], N._ptr(a), a.nbytes), "h2d")
            arg = N.PvProofIn(d["blob"].value, d["off"].value, self.nn, d["first"].value, len(self.first) - 1, d["qp"].value,
                              d["root"].value, d["kb"].value, d["ko"].value, d["vb"].value, d["vo"].value, self.nq, None)
            call = lambda: N.check(L.pv_trie_verify_proofs_device(ctypes.byref(arg), d["status"], d["hash"], None),  # noqa: E731
                                   "pv_trie_verify_proofs_device")
            call()
            N.check(L.pv_sync(), "pv_sync")
            t = time.perf_counter()
            for _ in range(reps):
                call()
            N.check(L.pv_sync(), "pv_sync")
            per_call = (time.perf_counter() - t) / reps
            status = np.zeros(self.nq, np.uint8)
            N.check(L.pv_memcpy_d2h(N._ptr(status), d["status"], self.nq), "d2h")
            return status, per_call
        finally:
            for p in d.values():
                L.pv_dev_free(p)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


def corrupt(rng, S, keys, values, proofs, share):
    """(keys, stored values, records per proof): a share of the honest queries corrupted, by kind in turn."""
    vals = [raw if raw else b"" for _, raw in proofs]
    recs = [list(p) for p, _ in proofs]
    kinds = {"wrong_value": 0, "node_dropped": 0, "byte_flipped": 0}
    for i in rng.choice(len(keys), int(share * len(keys)), replace=False):
        kind = ("wrong_value", "node_dropped", "byte_flipped")[int(i) % 3]
        kinds[kind] += 1
        if kind == "wrong_value":
            vals[i] = S.rlp_encode([b"forged"])
        elif kind == "node_dropped":
            del recs[i][int(rng.integers(0, len(recs[i])))]
        else:
            j = int(rng.integers(0, len(recs[i])))
            b = bytearray(recs[i][j])
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
            recs[i][j] = bytes(b)
    return vals, recs, kinds


def threshold(N, S, a):
    rng = np.random.default_rng(12)
    st, keys, values = build(N, S, 65536, rng)
    proofs = proofs_for(S, st, keys[:16384])
    table = []
    for want in THRESHOLD_NODES:
        take, nodes = 0, 0
        while take < len(proofs) and nodes < want:
            nodes += len(proofs[take][0])
            take += 1
        arr = Arrays(N, st.headHash, keys[:take], [raw for _, raw in proofs[:take]], [p for p, _ in proofs[:take]])
        ts = {"device": [], "host": []}
        same = True
        for rep in range(REPS + 1):
            got = {}
            for mode, key in ((N.PV_TRIE_DEVICE, "device"), (N.PV_TRIE_HOST, "host")):
                N.trie_path(mode)
                t = time.perf_counter()
                got[key] = arr.run()
                if rep:  # the first round warms both up
                    ts[key].append(time.perf_counter() - t)
            same &= bool(np.array_equal(got["device"], got["host"])) and bool((got["device"] == N.PV_PROOF_ACCEPT).all())
        row = {"nodes": arr.nn, "proofs": take, "device_equals_host_all_accept": same}
        for key in ("device", "host"):
            us = sorted(x * 1e6 for x in ts[key])
            row["%s_us" % key] = [round(us[0], 1), round(statistics.median(us), 1), round(us[-1], 1)]
        table.append(row)
    N.trie_path(N.PV_TRIE_AUTO)
    return {"probe": "proof_threshold", "reps": REPS, "hostpath_threads": min(16, len(os.sched_getaffinity(0))),
            "us_min_median_max": table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--proofs", type=int, default=1 << 18)
    ap.add_argument("--python-proofs", type=int, default=2000)
    ap.add_argument("--threshold", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r11", "state_proof", "probe_threshold.json" if a.threshold else "probe_final.json")
    from plenum_amd import _native as N
    from plenum_amd import state_trie as S
    N.ensure_device()
    if a.threshold:
        out = threshold(N, S, a)
        if a.append and a.out and os.path.exists(a.out):
            with open(a.out) as f:
                out = {"runs": json.load(f).get("runs", []) + [out]}
        else:
            out = {"runs": [out]}
    else:
        rng = np.random.default_rng(11)
        t = time.perf_counter()
        N.trie_path(N.PV_TRIE_DEVICE)
        st, keys, values = build(N, S, a.n, rng)
        out = {"probe": "proof", "n": a.n, "proofs": a.proofs, "key_bytes": KEY_BYTES, "value_bytes": VALUE_BYTES,
               "hostpath_threads": min(16, len(os.sched_getaffinity(0))), "build_s": time.perf_counter() - t}
        print("built %d pairs in %.1f s" % (a.n, out["build_s"]), file=sys.stderr, flush=True)
        absent = max(1, a.proofs // 50)
        qkeys = [keys[int(i)] for i in rng.choice(a.n, a.proofs - absent, replace=False)] + [rng.bytes(KEY_BYTES) for _ in range(absent)]
        t = time.perf_counter()
        proofs = proofs_for(S, st, qkeys)
        out["generate_proofs_per_s"] = a.proofs / (time.perf_counter() - t)
        print("%d proofs generated" % a.proofs, file=sys.stderr, flush=True)
        vals, recs, kinds = corrupt(rng, S, qkeys, values, proofs, 0.03)
        out.update(absent=absent, corrupted=kinds)
        root = st.headHash
        arr = Arrays(N, root, qkeys, vals, recs)
        out.update(nodes=arr.nn, nodes_per_proof=arr.nn / a.proofs, bytes_per_proof=int(arr.blob.size) / a.proofs,
                   node_bytes=int(arr.blob.size))
        status = {}
        for mode, key, reps in ((N.PV_TRIE_HOST, "hostpath", 2), (N.PV_TRIE_DEVICE, "device", 3)):
            N.trie_path(mode)
            status[key] = arr.run()  # sizes the workspace
            ms = [x * 1e3 for x in timed(arr.run, reps)]
            out["%s_ms" % key] = min(ms)
            out["%s_proofs_per_s" % key] = a.proofs / (min(ms) / 1e3)
        status["resident"], per_call = arr.resident(5)
        out["resident_ms"] = per_call * 1e3
        out["resident_proofs_per_s"] = a.proofs / per_call
        out["statuses"] = {name: int((status["device"] == code).sum()) for name, code in
                           (("reject", N.PV_PROOF_REJECT), ("accept", N.PV_PROOF_ACCEPT), ("defer", N.PV_PROOF_DEFER))}
        out["statuses_identical"] = bool(np.array_equal(status["device"], status["hostpath"])
                                         and np.array_equal(status["device"], status["resident"]))
        # the sequential method on a slice that holds every kind of query
        m = min(a.python_proofs, a.proofs)
        pick = [int(i) for i in np.linspace(0, a.proofs - 1, m)]
        sers = [S._length_prefix(sum(len(r) for r in recs[i]), 0xC0) + b"".join(recs[i]) for i in pick]
        t = time.perf_counter()
        seq = [S.Trie.verify_spv_proof(root, qkeys[i], vals[i], ser, serialized=True) for i, ser in zip(pick, sers)]
        out["python_proofs"] = m
        out["python_proofs_per_s"] = m / (time.perf_counter() - t)
        out["python_slice_agrees"] = all(status["device"][i] == N.PV_PROOF_DEFER or status["device"][i] == int(v)
                                         for i, v in zip(pick, seq))
        # and through the package's batch call, serialized input, fallback included
        N.trie_path(N.PV_TRIE_DEVICE)
        t = time.perf_counter()
        got = S.Trie.verify_spv_proof_batch([(root, qkeys[i], vals[i], ser) for i, ser in zip(pick, sers)], serialized=True)
        out["python_batch_call_proofs_per_s"] = m / (time.perf_counter() - t)
        out["python_batch_call_equals_sequential"] = got == seq
        N.trie_path(N.PV_TRIE_AUTO)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
