"""What table reuse (pv_table_reuse) costs when nothing recurs, and what a multi-chunk call gains.

Two device-resident batches of 1,048,576 requests from disjoint sets of 1,024 signers (NYM-sized
records, 16 signed messages per signer repeated). Three loops, each timed per call by the host clock
around a sync, median of --calls calls after --warmup:

  alternate  capacity 1,024, the two batches in turn: every call finds none of its keys, empties the
             directory and builds all 1,024 tables, with the probe and the publish on top -- the price
             of the mechanism when no signer recurs (compare with the same loop on a library without
             reuse, or with PV_TABLE_REUSE=0)
  recur      default capacity, one batch again and again: the steady state of recurring signers
  multi      one call of 4 x 1,048,576 requests (four chunks of the same signers)
  twice      capacity 1,024, three batches of disjoint signers in the order A A B B C C: every set is
             built, hit once and replaced, so with affine rows on (pv_table_affine) each hit converts
             1,024 tables that are never read again -- the promotion's worst case. Reported apart: the
             calls that build (first of a pair) and the calls that hit (second); the conversion's own
             time is the second's median less the same figure with PV_TABLE_AFFINE=0
  four       capacity 1,024, three sets in the order A A A A B B B B C C C C: every table is built, hit,
             converted, and -- with wide rows on (pv_table_wide) -- widened behind the fourth call and never
             read wide: the widening's worst case. Reported per position in the group of four; the
             widening's own time is the fourth's median less the same figure with PV_TABLE_WIDE=0

Prints one JSON line; every leg reports the counters the library has (hits_built_resets,
converted_affine_reads, widened_wide_reads). A library without pv_table_reuse, pv_table_affine or
pv_table_wide (an older build) runs the same loops."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "indy-plenum_amd")]

from plenum_amd import _native  # noqa: E402
from oracle.libsodium_ref import LibSodium  # noqa: E402

N = 1 << 20
SIGNERS = 1024
DISTINCT = 16
MSG = 299


def make_batch(ls, tag, reps=1):
    rng = np.random.default_rng(tag)
    sms, pks = [], []
    for s in range(SIGNERS):
        pk, sk = ls.seed_keypair(rng.bytes(32))
        for _ in range(DISTINCT):
            m = rng.bytes(MSG)
            sms.append(ls.sign_detached(m, sk) + m)
            pks.append(pk)
    unit = len(sms)  # 16,384 records; repeated, so consecutive requests come from different signers
    k = N // unit * reps
    blob = np.frombuffer(b"".join(sms) * k, np.uint8)
    pk = np.frombuffer(b"".join(pks) * k, np.uint8)
    off = np.arange(unit * k + 1, dtype=np.uint64) * np.uint64(64 + MSG)
    return blob, off, pk


class Dev:
    def __init__(self, L, blob, off, pk):
        self.L, self.n = L, len(off) - 1
        self.blob = self._put(np.concatenate([blob, np.zeros(_native.PV_BLOB_SLACK, np.uint8)]))
        self.off, self.pk = self._put(off), self._put(pk)
        self.words = (self.n + 63) // 64
        self.ver = self._alloc(self.words * 8)

    def _alloc(self, nbytes):
        p = ctypes.c_void_p()
        _native.check(self.L.pv_dev_alloc(ctypes.byref(p), nbytes), "pv_dev_alloc")
        return p

    def _put(self, a):
        p = self._alloc(a.nbytes)
        _native.check(self.L.pv_memcpy_h2d(p, a.ctypes.data, a.nbytes), "pv_memcpy_h2d")
        return p

    def call(self):
        t0 = time.perf_counter()
        _native.check(self.L.pv_verify_batch_device(self.blob, self.off, self.n, self.pk, self.ver, None),
                      "pv_verify_batch_device")
        _native.check(self.L.pv_sync(), "pv_sync")
        return 1e3 * (time.perf_counter() - t0)

    def valid(self):
        out = np.zeros(self.words, np.uint64)
        _native.check(self.L.pv_memcpy_d2h(out.ctypes.data, self.ver, out.nbytes), "pv_memcpy_d2h")
        return int(np.unpackbits(out.view(np.uint8), bitorder="little")[:self.n].sum())


def loop(devs, calls, warmup):
    ts = []
    for i in range(warmup + calls):
        t = devs[i % len(devs)].call()
        if i >= warmup:
            ts.append(t)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def loop_pairs(devs, rounds, warmup_rounds):
    """devs in the order A A B B C C ...: medians of all calls, of the first and of the second of a pair."""
    first, second = [], []
    for r in range(warmup_rounds + rounds):
        for i, d in enumerate(devs):
            t = d.call()
            if r >= warmup_rounds:
                (second if i % 2 else first).append(t)
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    return {"median_ms": med(first + second), "first_ms": med(first), "second_ms": med(second),
            "second_min_ms": round(min(second), 4), "second_max_ms": round(max(second), 4)}


def loop_groups(devs, group, rounds, warmup_rounds):
    """devs in groups of `group` equal entries: the median per position in the group."""
    ts = [[] for _ in range(group)]
    for r in range(warmup_rounds + rounds):
        for i, d in enumerate(devs):
            t = d.call()
            if r >= warmup_rounds:
                ts[i % group].append(t)
    return {"position_ms": [round(float(np.median(v)), 4) for v in ts],
            "last_min_ms": round(min(ts[-1]), 4), "last_max_ms": round(max(ts[-1]), 4)}


class Counters:
    """The counters the loaded library has, as deltas per leg."""

    GETTERS = (("hits_built_resets", "table_reuse_stats"), ("converted_affine_reads", "table_affine_stats"),
               ("widened_wide_reads", "table_wide_stats"))

    def __init__(self):
        self.v = self._read()

    def _read(self):
        return {k: getattr(_native, f)() for k, f in self.GETTERS if hasattr(_native, f)}

    def into(self, leg):
        v = self._read()
        for k in v:
            leg[k] = [int(x - y) for x, y in zip(v[k], self.v[k])]
        self.v = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--no-multi", action="store_true")
    ap.add_argument("--no-twice", action="store_true")
    ap.add_argument("--no-four", action="store_true")
    a = ap.parse_args()
    ls = LibSodium()
    _native.ensure_device()
    L = _native.lib()
    has = hasattr(_native, "table_reuse")
    A, B = Dev(L, *make_batch(ls, 1)), Dev(L, *make_batch(ls, 2))
    out = {"lib": os.path.basename(_native.LIB_PATH), "table_reuse": has and os.environ.get("PV_TABLE_REUSE") != "0"}
    out["table_affine"] = hasattr(_native, "table_affine") and os.environ.get("PV_TABLE_AFFINE") != "0"
    out["table_wide"] = hasattr(_native, "table_wide") and os.environ.get("PV_TABLE_WIDE") != "0"
    if has:
        _native.table_reuse(out["table_reuse"], SIGNERS)
    c = Counters()
    out["alternate"] = loop([A, B], a.calls, a.warmup)
    c.into(out["alternate"])
    if has:
        _native.table_reuse(out["table_reuse"], _native.PV_TABLE_REUSE_CAP)
    out["recur"] = loop([A], a.calls, a.warmup)
    c.into(out["recur"])
    assert A.valid() == A.n and B.valid() == B.n
    if not (a.no_twice and a.no_four):
        C = Dev(L, *make_batch(ls, 3))
    if not a.no_twice:
        if has:
            _native.table_reuse(out["table_reuse"], SIGNERS)
        c = Counters()
        out["twice"] = loop_pairs([A, A, B, B, C, C], max(3, a.calls // 4), 1)
        c.into(out["twice"])
        if has:
            _native.table_reuse(out["table_reuse"], _native.PV_TABLE_REUSE_CAP)
        assert A.valid() == A.n and B.valid() == B.n and C.valid() == C.n
    if not a.no_four:
        if has:
            _native.table_reuse(out["table_reuse"], SIGNERS)
        c = Counters()
        out["four"] = loop_groups([A] * 4 + [B] * 4 + [C] * 4, 4, max(3, a.calls // 4), 1)
        c.into(out["four"])
        if has:
            _native.table_reuse(out["table_reuse"], _native.PV_TABLE_REUSE_CAP)
        assert A.valid() == A.n and B.valid() == B.n and C.valid() == C.n
    if not a.no_multi:
        M = Dev(L, *make_batch(ls, 1, reps=4))
        c = Counters()
        out["multi_4m"] = loop([M], max(5, a.calls // 2), 2)
        c.into(out["multi_4m"])
        assert M.valid() == M.n
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
