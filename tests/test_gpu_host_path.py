"""GPU tests of the host-fed path (include/plenum_verify.h pv_verify_batch, pv_host_alloc /
pv_host_register, pv_verify_batch_multi_gpu) and of its failure paths:
  * every input form -- pageable numpy, all inputs in the library's pinned arena, an arena sub-range
    whose offsets do not start at 0, only the blob pinned, a numpy buffer registered in place -- gives
    libsodium 1.0.18's verdicts on a configs[2]-style batch (2 % adversarial records), at sizes that
    leave a partial verdict word. At the default PV_PIPE_SUB = 262,144 a call is cut into more than one
    sub-batch from 524,288 requests on (csrc/host_plan.h plan_pieces, tests/test_host_plan.py), so the
    400,000-request batch and its sub-ranges are ONE piece each: one DMA from pageable memory, the
    copy-stream form with a single sub-batch as soon as an input is pinned;
  * test_pipelined_form_at_pipe_sub_8192 runs the form with several sub-batches (H2D of sub-batch j on
    the copy stream beside the kernels of j - 1, the shared table store, the injected failure with
    sub-batch 0's kernels in flight) in a process of its own with PV_PIPE_SUB=8192;
  * an injected staging failure (pv_test_inject) returns an error, and the next call -- single-device
    and the multi-GPU entry -- is bit-exact;
  * pv_init_devices with a device that does not exist fails without touching the primary context;
  * released arena blocks are handed out again by size (the pinned block cache) and verify bit-exact;
  * with >= 2 GPUs (skipped on a one-GPU box): the multi-GPU entry with empty shards, a partial last
    word and a >= 8 MB blob is bit-exact."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from plenum_amd import _native
    _native.ensure_device()
    _native.set_path(_native.PV_PATH_AUTO)
    return _native


@pytest.fixture(scope="module")
def adv400k(oracle):
    """400,000 NYM requests (~145 MB of records; one piece at the default PV_PIPE_SUB, which cuts a call
    from 524,288 requests on), 2 % adversarial, and libsodium's verdicts."""
    import nym_workload
    from adversarial import inject
    from oracle.oracle import cpu_verdicts
    blob, off, pks = nym_workload.generate(0, 400000)
    blob2, pks2, _, _ = inject(blob, off, pks, 0.02, seed=5, oracle=oracle)
    return blob2, off, pks2, cpu_verdicts(blob2, off, pks2)


def _check(got, want, what):
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:10])


def test_host_forms_bit_exact(native, adv400k):
    blob, off, pks, want = adv400k
    A = native.HostArena
    # pageable
    _check(native.verify_sm_batch(blob, off, pks), want, "pageable")
    # the whole batch in the arena (offsets from 0: DMA'd as they are)
    ab, ao, ak = A.batch(blob, off, pks)
    assert A.is_pinned(ab) and A.is_pinned(ao) and A.is_pinned(ak)
    assert not A.is_pinned(blob)
    _check(native.verify_sm_batch(ab, ao, ak), want, "arena")
    # a sub-range of the arena batch whose offsets start past 0 (rebased in staging), ragged sizes
    for lo, hi in ((131072 + 64, 400000), (1, 262144 + 1 + 77), (64 * 5000 + 3, 64 * 5000 + 3 + 140000)):
        _check(native.verify_sm_batch(ab, ao[lo:hi + 1], ak[lo:hi]), want[lo:hi], ("arena range", lo, hi))
    # only the blob pinned (keys and offsets pageable)
    _check(native.verify_sm_batch(ab, np.array(ao), np.array(ak)), want, "blob pinned")
    # a numpy buffer pinned in place
    reg = np.array(blob)
    L = native.lib()
    native.check(L.pv_host_register(reg.ctypes.data, reg.nbytes), "pv_host_register")
    try:
        assert A.is_pinned(reg)
        _check(native.verify_sm_batch(reg, off, pks), want, "registered")
    finally:
        native.check(L.pv_host_unregister(reg.ctypes.data), "pv_host_unregister")
    assert not A.is_pinned(reg)
    assert L.pv_host_free(ctypes.c_void_p(reg.ctypes.data)) != 0  # not an arena block


def test_arena_blocks_reused_after_free(native, adv400k):
    """pv_host_free keeps a released block pinned for the next pv_host_alloc of a similar size (at
    most twice the request); a released block is no longer reported as the caller's pinned memory;
    a batch built in reused blocks is verified bit-exact."""
    import gc
    blob, off, pks, want = adv400k
    L = native.lib()

    def alloc(nbytes):
        p = ctypes.c_void_p()
        native.check(L.pv_host_alloc(ctypes.byref(p), nbytes), "pv_host_alloc")
        return p.value

    a = alloc(48 << 20)
    native.check(L.pv_host_free(ctypes.c_void_p(a)), "pv_host_free")
    assert L.pv_host_is_pinned(ctypes.c_void_p(a), 1) == 0
    b = alloc(40 << 20)
    assert b == a and L.pv_host_is_pinned(ctypes.c_void_p(a), 48 << 20) == 1
    c = alloc(8 << 20)  # 48 MB > 2 x 8 MB: a new block
    assert c != a
    for q in (b, c):
        native.check(L.pv_host_free(ctypes.c_void_p(q)), "pv_host_free")
    n = 300000
    o = off[:n + 1]
    first = native.HostArena.batch(blob[:int(o[-1])], o, pks[:n])
    addrs = sorted(x.ctypes.data for x in first)
    del first
    gc.collect()
    ab, ao, ak = native.HostArena.batch(blob[:int(o[-1])], o, pks[:n])
    assert sorted(x.ctypes.data for x in (ab, ao, ak)) == addrs
    _check(native.verify_sm_batch(ab, ao, ak), want[:n], "reused arena")


def test_injected_stage_failure_then_exact(native, adv400k, monkeypatch):
    monkeypatch.setenv("PV_ENABLE_TEST_HOOKS", "1")
    blob, off, pks, want = adv400k
    k = 262144 + 999
    o = off[:k + 1]
    # all three are one piece and pageable, so one DMA: 263,143 requests (below the 524,288 from which a call
    # is cut), quota-size, medium. Several sub-batches: test_pipelined_form_at_pipe_sub_8192
    for n in (k, 3000, 20000):
        on = off[:n + 1]
        native.inject_stage_failures(0, 1)
        with pytest.raises(native.NativeError, match="injected"):
            native.verify_sm_batch(blob[:int(on[-1])], on, pks[:n])
        _check(native.verify_sm_batch(blob[:int(on[-1])], on, pks[:n]), want[:n], ("after failure", n))
    # the multi-GPU entry: one shard's staging fails, the call errors, the next one is exact
    devs = native.ensure_devices([0])
    native.inject_stage_failures(devs[0], 1)
    with pytest.raises(native.NativeError, match="injected"):
        native.verify_sm_batch_multi(blob[:int(o[-1])], o, pks[:k])
    _check(native.verify_sm_batch_multi(blob[:int(o[-1])], o, pks[:k]), want[:k], "multi after failure")
    _check(native.verify_sm_batch(blob[:int(o[-1])], o, pks[:k]), want[:k], "single after multi failure")
    native.inject_stage_failures(0, 0)


def test_init_devices_bad_mask_keeps_primary(native, adv400k):
    blob, off, pks, want = adv400k
    L = native.lib()
    ndev = L.pv_device_count()
    for mask in (1 << ndev, (1 << ndev) | 1, 0, 1 << 20):
        assert L.pv_init_devices(mask) < 0, mask
    # the primary context and the multi-GPU clique built before are unaffected
    o = off[:5001]
    _check(native.verify_sm_batch(blob[:int(o[-1])], o, pks[:5000]), want[:5000], "primary after bad mask")
    assert native.ensure_devices([0]) == (0,)
    _check(native.verify_sm_batch_multi(blob[:int(o[-1])], o, pks[:5000]), want[:5000], "multi after bad mask")


def test_pipelined_shared_tables_with_one_off_keys(native, sodium):
    """A host call with more than 2,048 distinct keys (1,024 signers with ~100 requests each plus ~25k
    one-off keys). Written for sub-batches of 131,072, where the first one gave tables only to the
    signers (>= 48 requests) and published them and the later ones read them from the shared store; at
    PV_PIPE_SUB = 262,144 its 322,144 requests are ONE piece (tests/test_host_plan.py), so this checks
    a single keyed chunk: the signers on the comb path, the one-off keys on the Straus path in the same
    launch -- forced COMB too (every key a comb key up to the capacity) -- libsodium's verdicts. The
    shared store is exercised by test_pipelined_form_at_pipe_sub_8192."""
    from test_gpu_configs import _split_batch
    from oracle.oracle import cpu_verdicts
    blob, off, pks = _split_batch(sodium, 262144, 60000, seed=17)
    want = cpu_verdicts(blob, off, pks)
    assert 0 < (~want).sum() < len(want) // 50
    for path in (native.PV_PATH_AUTO, native.PV_PATH_COMB):
        native.set_path(path)
        try:
            got = native.verify_sm_batch(blob, off, pks)
        finally:
            native.set_path(native.PV_PATH_AUTO)
        _check(got, want, ("one-off keys", path))


_PIPE_SUB_8192_SCRIPT = r"""
import ctypes, json, os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "indy-plenum_amd"), os.path.join(root, "tests"), os.path.join(root, "tools")]
import numpy as np
import nym_workload, adversarial_batch
from oracle.oracle import Oracle, cpu_verdicts
from plenum_amd import _native
N = 30001
blob, off, pks = nym_workload.generate(0, N, workers=8)
blob, pks, idx, labels = adversarial_batch.inject(blob, off, pks, 0.02, seed=11, forger=Oracle())
want = cpu_verdicts(blob, off, pks)
assert int(off[-1] - off[0]) >= 8 << 20, int(off[-1] - off[0])  # below 8 MB a call is one piece
_native.ensure_device(0)
_native.set_path(_native.PV_PATH_AUTO)
L, A, kc = _native.lib(), _native.HostArena, _native.KeyCache
out = {"rejected": int((~want).sum())}

def run(name, b, o, k, w=want):
    out[name] = int((_native.verify_sm_batch(b, o, k) != w).sum())

# the piece count, once: one launch per sub-batch
L.pv_set_timing(1)
run("pageable", blob, off, pks)
ms, launches = (ctypes.c_double * 5)(), ctypes.c_int()
_native.check(L.pv_stage_times(ms, 5, ctypes.byref(launches)), "pv_stage_times")
L.pv_set_timing(0)
assert launches.value == 4, launches.value
ab, ao, ak = A.batch(blob, off, pks)
assert A.is_pinned(ab) and A.is_pinned(ao) and A.is_pinned(ak) and not A.is_pinned(blob)
run("arena", ab, ao, ak)
run("blob pinned", ab, np.array(ao), np.array(ak))
run("arena range", ab, ao[1:N + 1], ak[1:N], want[1:])
_native.set_path(_native.PV_PATH_COMB)
run("comb", blob, off, pks)
_native.set_path(_native.PV_PATH_AUTO)
keys, counts = np.unique(pks, axis=0, return_counts=True)
signers = [bytes(k) for k, c in zip(keys, counts) if c >= 20]
assert len(signers) >= 1000, len(signers)
kc.configure(2048)
kc.put(signers[::2])
assert kc.stats()[0] == len(signers[::2])
run("half cached auto", blob, off, pks)
_native.set_path(_native.PV_PATH_COMB)
run("half cached comb", blob, off, pks)
_native.set_path(_native.PV_PATH_AUTO)
kc.configure(0)
_native.inject_stage_failures(0, 1)
try:
    _native.verify_sm_batch(blob, off, pks)
    out["injected"] = "no error"
except _native.NativeError as e:
    out["injected"] = str(e)
run("after injected failure", blob, off, pks)
print(json.dumps(out))
"""


def test_pipelined_form_at_pipe_sub_8192():
    """The pipelined form with more than one sub-batch, which the default PV_PIPE_SUB = 262,144 reaches only from
    524,288 requests on: a fresh process with PV_PIPE_SUB=8192 (read once per process) verifies 30,001 NYM requests
    with 2 % adversarial records as sub-batches [0, 8192, 14976, 21760, 30001) -- a first, two middle and a ragged
    last one (tests/test_host_plan.py has the bounds; the process checks that its blob reaches the 8 MB below which
    a call is one piece, and that one call makes four launches). Sub-batch 0 fills the call's shared table store and
    publishes it, the later ones look keys up there -- after the node-side key cache when that holds half of the
    signers -- and sub-batch j + 1's copies are enqueued before sub-batch j's kernels. Pageable input, the whole
    batch in the arena, only the blob pinned, an arena sub-range whose offsets start past 0, forced COMB (every key
    a comb key: the store holds tables), half of the signers cached under AUTO and COMB, and the call after an
    injected staging failure with sub-batch 0's kernels in flight: libsodium's verdicts, bit for bit."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PV_PIPE_SUB="8192", PV_ENABLE_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, "-c", _PIPE_SUB_8192_SCRIPT, root], env=env, capture_output=True, text=True,
                       timeout=170)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["rejected"] > 300
    for name in ("pageable", "arena", "blob pinned", "arena range", "comb", "half cached auto", "half cached comb",
                 "after injected failure"):
        assert res[name] == 0, (name, res)
    assert "injected" in res["injected"], res


def test_pipelined_partly_warm_cache(native, adv400k):
    """a host call with half of its signers in the node-side key cache. Written for sub-batches
    of 131,072, where the later ones look a key up in the node cache first and in the call's shared store
    next (pv_key_cache_probe_kernel's two views); at PV_PIPE_SUB = 262,144 the 400,000 requests are ONE
    piece, so this checks one keyed chunk with a partly warm cache (the two views together:
    test_pipelined_form_at_pipe_sub_8192). Verdicts are libsodium's on AUTO and forced COMB; the call is
    no slower than with the cache empty."""
    import time
    blob, off, pks, want = adv400k
    keys, counts = np.unique(pks, axis=0, return_counts=True)
    signers = [bytes(k) for k, c in zip(keys, counts) if c >= 100]
    assert len(signers) >= 1000
    kc = native.KeyCache

    def timed_calls():
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = native.verify_sm_batch(blob, off, pks)
            ts.append(time.perf_counter() - t0)
            _check(got, want, "partly warm")
        return float(np.median(ts))

    try:
        kc.configure(2048)
        native.verify_sm_batch(blob, off, pks)  # warm: staging sized
        cold = timed_calls()
        kc.put(signers[::2])
        assert kc.stats()[0] == len(signers[::2])
        for path in (native.PV_PATH_AUTO, native.PV_PATH_COMB):
            native.set_path(path)
            try:
                _check(native.verify_sm_batch(blob, off, pks), want, ("partly warm", path))
            finally:
                native.set_path(native.PV_PATH_AUTO)
        warm = timed_calls()
        print("pipelined 400k call: cache empty %.2f ms, half the signers cached %.2f ms" % (1e3 * cold, 1e3 * warm))
        assert warm < 1.25 * cold, (warm, cold)
    finally:
        kc.configure(0)


def test_multi_gpu_two_or_more_devices(native, adv400k):
    L = native.lib()
    G = L.pv_device_count()
    if G < 2:
        pytest.skip("one GPU visible: the multi-device clique needs >= 2")
    blob, off, pks, want = adv400k
    devs = native.ensure_devices(range(G))
    assert native.multi_gpu_clique() == {"devices": list(devs), "nranks": G, "user_ranks": list(range(G))}
    for n in (1, 63, 64 * G - 1, 64 * G + 65, 100001, len(want)):  # empty shards, partial words, >= 8 MB
        o = off[:n + 1]
        _check(native.verify_sm_batch_multi(blob[:int(o[-1])], o, pks[:n], devs), want[:n], ("multi", n))
