"""Signing-rate probe: one JSON line for N messages of the NYM template (tools/nym_workload.py, 299 B)
signed by the 1,024-signer pool.

  device   pv_sign_batch_device on device-resident inputs: K back-to-back launches on one stream after a
           warm-up, K chosen for about a second of timed work; timed with HIP events (through torch)
           when torch can wrap the library's stream, else with the host's clock around the K launches
           and the final stream synchronise ("device_timer" says which)
  host     pv_sign_batch on host buffers (staging, transfers and kernels), wall clock
  cpu      libsodium crypto_sign_detached in worker processes on the CPUs this process may use, in the
           same run, when libsodium is present (else null)

The batch repeats 65,536 distinct messages (rendering 1M of them in Python would take longer than
everything measured here); every message is signed on its own all the same. A sample of the GPU's
signatures is compared with libsodium's when it is present.

    python tools/sign_probe.py [--n 1048576] [--seconds 1.0]
"""
import argparse
import ctypes
import hashlib
import json
import multiprocessing as mp
import os
import struct
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "indy-plenum_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nym_workload  # noqa: E402

DISTINCT = 65536
CPU_SAMPLE = 65536


def pool_seeds():
    return [hashlib.sha512(b"plenum-bench" + struct.pack("<Q", s)).digest()[:32] for s in range(nym_workload.POOL)]


def messages(vks, count):
    pool = [{"did": nym_workload.b58(vk[:16])} for vk in vks]
    return [nym_workload.message(i, pool[i % nym_workload.POOL]) for i in range(count)]


def _cpu_worker(args):
    path, sks, msgs, idx = args
    lib = ctypes.CDLL(path)
    lib.sodium_init()
    sig = ctypes.create_string_buffer(64)
    t = time.perf_counter()
    for m, s in zip(msgs, idx):
        lib.crypto_sign_detached(sig, None, m, ctypes.c_ulonglong(len(m)), sks[s])
    return time.perf_counter() - t


def cpu_rate(path, sks, msgs, idx, workers):
    """Signatures per second of `workers` processes each signing its share of msgs (the slowest
    worker's time counts)."""
    parts = [(path, sks, msgs[w::workers], idx[w::workers]) for w in range(workers)]
    with mp.get_context("spawn").Pool(workers) as pool:
        pool.map(_cpu_worker, [(path, sks, msgs[:64], idx[:64])] * workers)  # start-up and page-in
        times = pool.map(_cpu_worker, parts)
    return len(msgs) / max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--seconds", type=float, default=1.0)
    a = ap.parse_args()
    n = a.n
    from oracle.libsodium_ref import LibSodium, find_libsodium
    seeds = pool_seeds()
    out = {"probe": "sign", "n": n, "signers": len(seeds)}
    sodium = LibSodium() if find_libsodium() else None
    distinct = min(DISTINCT, n)
    idx_small = [i % len(seeds) for i in range(distinct)]
    if sodium:  # the CPU leg first: its workers start before this process touches the GPU
        keys = [sodium.seed_keypair(s) for s in seeds]
        vks, sks = [k[0] for k in keys], [k[1] for k in keys]
        msgs = messages(vks, distinct)
        workers = min(16, len(os.sched_getaffinity(0)))
        sample = min(CPU_SAMPLE, distinct)
        out["cpu_threads"] = workers
        out["cpu_sigs_per_s"] = cpu_rate(sodium.path, sks, msgs[:sample], idx_small[:sample], workers)

    from plenum_amd import _native
    _native.ensure_device()
    L = _native.lib()
    pks_gpu, sks_gpu = _native.seed_keypairs(np.frombuffer(b"".join(seeds), np.uint8))
    if sodium:
        out["keypairs_identical_to_libsodium"] = bool(pks_gpu.tobytes() == b"".join(vks) and
                                                      sks_gpu.tobytes() == b"".join(sks))
    else:
        msgs = messages([p.tobytes() for p in pks_gpu], distinct)
        out["cpu_threads"] = out["cpu_sigs_per_s"] = None
    out["msg_bytes"] = len(msgs[0])
    reps = (n + distinct - 1) // distinct
    blob1, off1 = _native._blob(msgs)
    blob = np.tile(blob1, reps)
    lens = np.tile(np.diff(off1), reps)[:n]
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    blob = blob[: int(off[n])]
    idx = (np.arange(n, dtype=np.uint64) % np.uint64(distinct) % np.uint64(len(seeds))).astype(np.uint32)

    # host entry (the first call sizes the staging buffers)
    sigs = _native.sign_batch(blob, off, sks_gpu, idx)
    t = time.perf_counter()
    sigs = _native.sign_batch(blob, off, sks_gpu, idx)
    out["host_sigs_per_s"] = n / (time.perf_counter() - t)
    if sodium:
        pick = list(range(0, n, max(1, n // 256)))[:256]
        out["signatures_identical_to_libsodium"] = all(
            sigs[i].tobytes() == sodium.sign_detached(msgs[i % distinct], sks[int(idx[i])]) for i in pick)

    # device-resident
    def dput(arr, slack=0):
        p = ctypes.c_void_p()
        _native.check(L.pv_dev_alloc(ctypes.byref(p), arr.nbytes + slack), "pv_dev_alloc")
        _native.check(L.pv_memcpy_h2d(p, arr.ctypes.data, arr.nbytes), "pv_memcpy_h2d")
        return p

    d_msg, d_off, d_idx = dput(blob, _native.PV_BLOB_SLACK), dput(off), dput(idx)
    d_sk, d_sig = dput(np.ascontiguousarray(sks_gpu)), dput(np.zeros((n, 64), np.uint8))
    s = ctypes.c_void_p()
    _native.check(L.pv_stream_create(ctypes.byref(s)), "pv_stream_create")

    def launches(k):
        for _ in range(k):
            _native.check(L.pv_sign_batch_device(d_msg, d_off, n, d_sk, len(seeds), d_idx, d_sig, s),
                          "pv_sign_batch_device")

    launches(2)
    _native.check(L.pv_stream_sync(s), "pv_stream_sync")
    t = time.perf_counter()
    launches(1)
    _native.check(L.pv_stream_sync(s), "pv_stream_sync")
    k = max(3, int(a.seconds / max(time.perf_counter() - t, 1e-6)) + 1)
    try:
        import torch
        ts = torch.cuda.ExternalStream(s.value, device=torch.device("cuda", _native.ensure_device()))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts)
        launches(k)
        e1.record(ts)
        _native.check(L.pv_stream_sync(s), "pv_stream_sync")
        ms = e0.elapsed_time(e1)
        out["device_timer"] = "hip events"
    except (ImportError, RuntimeError):  # no torch, or it cannot wrap the stream: the host's clock
        _native.check(L.pv_stream_sync(s), "pv_stream_sync")
        t = time.perf_counter()
        launches(k)
        _native.check(L.pv_stream_sync(s), "pv_stream_sync")
        ms = (time.perf_counter() - t) * 1e3
        out["device_timer"] = "wall clock"
    out["device_launches"] = k
    out["device_ms_per_launch"] = ms / k
    out["device_sigs_per_s"] = n * k / (ms / 1e3)
    got = np.zeros((n, 64), np.uint8)
    _native.check(L.pv_memcpy_d2h(got.ctypes.data, d_sig, got.nbytes), "pv_memcpy_d2h")
    out["device_equals_host_entry"] = bool(np.array_equal(got, sigs))
    if out["cpu_sigs_per_s"]:
        out["device_over_cpu"] = out["device_sigs_per_s"] / out["cpu_sigs_per_s"]
        out["host_over_cpu"] = out["host_sigs_per_s"] / out["cpu_sigs_per_s"]
    _native.check(L.pv_stream_destroy(s), "pv_stream_destroy")
    for p in (d_msg, d_off, d_idx, d_sk, d_sig):
        L.pv_dev_free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
