"""ctypes binding of libplenum_verify.so (include/plenum_verify.h).

This is the only way the package reaches the verification arithmetic: there is no CPU fallback.
If the library is missing, or no gfx950 GPU is visible, verification calls raise
``NativeUnavailable`` instead of silently computing elsewhere.
"""
import ctypes
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLENUM_AMD_LIB", os.path.join(_HERE, "libplenum_verify.so"))

PV_OK = 0
PV_ERR_NO_DEVICE = -1
PV_ERR_ARG = -4
PV_ERR_NOT_INIT = -5
PV_ERR_DECODE = -7
PV_BLOB_SLACK = 256
PV_ABI_VERSION = 1
PV_SIGN_CHUNK = 262144  # messages per launch inside pv_sign_batch (csrc/pv_sign.hip PV_SIGN_CHUNK)
PV_BUILD_COMB_FUSED = 1  # pv_build_flags(): [S]B and [k](-A) of the comb path in one kernel

PV_STAGES = ("keys", "prep", "table", "msm", "encode")  # PV_STAGE_* order
PV_PATH_AUTO, PV_PATH_STRAUS, PV_PATH_COMB, PV_PATH_LATENCY = 0, 1, 2, 3
PATH_NAMES = ("straus", "comb", "latency")  # forced arithmetic paths (tests run every one)

# exported symbol -> (restype, argtypes); kept in sync with include/plenum_verify.h
_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_c_u64p = ctypes.POINTER(ctypes.c_uint64)
_c_u32p = ctypes.POINTER(ctypes.c_uint32)
SIGNATURES = {
    "pv_abi_version": (ctypes.c_int, []),
    "pv_build_flags": (ctypes.c_uint32, []),
    "pv_device_count": (ctypes.c_int, []),
    "pv_init": (ctypes.c_int, [ctypes.c_int]),
    "pv_shutdown": (None, []),
    "pv_last_error": (ctypes.c_char_p, []),
    "pv_verify_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "pv_verify_batch_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_set_timing": (ctypes.c_int, [ctypes.c_int]),
    "pv_set_path": (ctypes.c_int, [ctypes.c_int]),
    "pv_last_path": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]),
    "pv_last_split": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32)] * 3),
    "pv_stage_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "pv_kernel_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]),
    "pv_b58decode_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_b58encode": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]),
    "pv_resolve_verkeys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_ingress_verify_device": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
                                 + [ctypes.c_void_p] * 5 + [ctypes.c_uint64] + [ctypes.c_void_p] * 3),
    "pv_ingress_verify": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint64] + [ctypes.c_void_p] * 5 + [ctypes.c_uint64]
                          + [ctypes.c_void_p] * 2),
    "pv_signing_serialize_json": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                 ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_wire_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int,
                                    ctypes.c_void_p]),
    "pv_ingress_front_ms": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)]),
    "pv_comm_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "pv_comm_init": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "pv_allgather_verdicts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_comm_destroy": (None, []),
    "pv_dev_alloc": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64]),
    "pv_dev_free": (ctypes.c_int, [ctypes.c_void_p]),
    "pv_memcpy_h2d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pv_memcpy_d2h": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "pv_sync": (ctypes.c_int, []),
    "pv_key_cache_configure": (ctypes.c_int, [ctypes.c_uint32]),
    "pv_key_cache_put": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "pv_key_cache_clear": (ctypes.c_int, []),
    "pv_key_cache_enable": (ctypes.c_int, [ctypes.c_int]),
    "pv_key_cache_stats": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "pv_key_cache_contains": (ctypes.c_int, [ctypes.c_void_p]),
    "pv_key_cache_auto": (ctypes.c_int, [ctypes.c_uint32]),
    "pv_key_cache_auto_stats": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "pv_table_reuse": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32]),
    "pv_table_reuse_stats": (ctypes.c_int, [_c_u64p, _c_u64p, _c_u64p]),
    "pv_table_affine": (ctypes.c_int, [ctypes.c_int]),
    "pv_table_affine_stats": (ctypes.c_int, [_c_u64p, _c_u64p]),
    "pv_table_wide": (ctypes.c_int, [ctypes.c_uint32]),
    "pv_table_wide_stats": (ctypes.c_int, [_c_u64p, _c_u64p]),
    "pv_last_zero_copy": (ctypes.c_int, []),
    "pv_init_devices": (ctypes.c_int, [ctypes.c_uint32]),
    "pv_verify_batch_multi_gpu": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "pv_multi_gpu_devices": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "pv_multi_gpu_comm_ranks": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "pv_comm_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pv_shard_plan": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, _c_u64p, _c_u64p]),
    "pv_host_alloc": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64]),
    "pv_host_free": (ctypes.c_int, [ctypes.c_void_p]),
    "pv_host_register": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "pv_host_unregister": (ctypes.c_int, [ctypes.c_void_p]),
    "pv_host_is_pinned": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "pv_test_inject": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "pv_test_clock_stamps": (ctypes.c_int, [_c_u64p, ctypes.c_uint32]),
    "pv_stream_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p)]),
    "pv_stream_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pv_stream_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "pv_sign_seed_keypairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_sign_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_sign_batch_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_merkle_plan": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, _c_u64p, _c_u64p, _c_u64p]),
    "pv_merkle_append_batch": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.c_void_p]),
    "pv_merkle_append_batch_device": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "pv_merkle_verify_inclusion_batch": (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.c_void_p,
                                                                                ctypes.c_void_p]),
    "pv_merkle_verify_inclusion_batch_device": (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.c_void_p,
                                                                                       ctypes.c_void_p, ctypes.c_void_p]),
    "pv_merkle_verify_consistency_batch": (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_uint64, ctypes.c_void_p,
                                                                                  ctypes.c_void_p]),
    "pv_merkle_verify_consistency_batch_device": (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_uint64] +
                                                  [ctypes.c_void_p] * 3),
    "pv_merkle_catchup_batch": (ctypes.c_int, [ctypes.c_uint64] + [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_void_p] * 6),
    "pv_merkle_catchup_batch_device": (ctypes.c_int, [ctypes.c_uint64] + [ctypes.c_void_p] * 3 +
                                       [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64] +
                                       [ctypes.c_void_p] * 7),
    "pv_merkle_prove_plan": (ctypes.c_int, [ctypes.c_uint64] + [ctypes.c_void_p] * 3 + [ctypes.c_uint64] +
                             [ctypes.c_void_p] * 2),
    "pv_merkle_prove_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 4 + [ctypes.c_uint64] +
                              [ctypes.c_void_p] * 3),
    "pv_merkle_prove_batch_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 4 +
                                     [ctypes.c_uint64] + [ctypes.c_void_p] * 4),
    "pv_merkle_chunk": (ctypes.c_int, [ctypes.c_uint64]),
    "pv_merkle_path": (ctypes.c_int, [ctypes.c_int]),
    "pv_sha3_256_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "pv_sha3_256_batch_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "pv_trie_update_batch": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_uint64] + [ctypes.c_void_p] * 4
                             + [ctypes.c_uint64, ctypes.c_void_p]),
    "pv_trie_path": (ctypes.c_int, [ctypes.c_int]),
    "pv_trie_root": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_uint32, ctypes.c_void_p]),
    "pv_trie_root_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "pv_trie_verify_proofs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pv_trie_verify_proofs_device": (ctypes.c_int, [ctypes.c_void_p] * 4),
    "pv_trie_proof_split": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 3
                            + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
}


class NativeUnavailable(RuntimeError):
    """The HIP engine cannot run here (library missing or no gfx950 device)."""


class NativeError(RuntimeError):
    """An infrastructure failure inside libplenum_verify (allocation, launch, comm)."""


_lib = None
_lock = threading.Lock()
_device = None


def lib():
    """The loaded library (loading does not touch the GPU)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise NativeUnavailable(
                        "libplenum_verify.so not built at %s (run __graft_entry__.build() or make -C indy-plenum_amd)"
                        % LIB_PATH)
                L = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(L, name)
                    fn.restype = res
                    fn.argtypes = args
                if L.pv_abi_version() != PV_ABI_VERSION:
                    raise NativeUnavailable("ABI version mismatch")
                _lib = L
    return _lib


def check(rc, what):
    if rc != PV_OK:
        msg = lib().pv_last_error()
        raise NativeError("%s failed (%d): %s" % (what, rc, msg.decode(errors="replace") if msg else ""))


def ensure_device(device=None):
    """Bind this process to a GPU (once). Raises NativeUnavailable when none is visible."""
    global _device
    if _device is not None:
        return _device
    L = lib()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = L.pv_device_count()
    if ndev <= 0:
        raise NativeUnavailable("no HIP device visible: the verification engine is GPU-only")
    rc = L.pv_init(device % ndev)
    if rc != PV_OK:
        raise NativeUnavailable("pv_init failed: %s" % L.pv_last_error().decode(errors="replace"))
    _device = device % ndev
    return _device


def shutdown():
    """pv_shutdown: every device context and workspace is released, and the binding forgets what it had
    bound, so the next call that needs a GPU runs pv_init again. Path settings (set_path, merkle_path,
    trie_path) are the library's and stay."""
    global _device, _multi_devices, _merkle_no_device, _trie_no_device
    lib().pv_shutdown()
    _device = _multi_devices = None
    _merkle_no_device = _trie_no_device = False


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_U8, _U64 = np.dtype(np.uint8), np.dtype(np.uint64)
_fast = None  # the CPython binding (_fastcall) once bound to the loaded library, False if not built


def _fastcall():
    global _fast
    if _fast is None:
        if os.environ.get("PLENUM_AMD_NO_FASTCALL"):  # the ctypes path (A/B, debugging)
            _fast = False
            return _fast
        try:
            from . import _fastcall as fc
            fc.bind(ctypes.cast(lib().pv_verify_batch, ctypes.c_void_p).value)
            _fast = fc
        except ImportError:
            _fast = False
    return _fast


def verify_sm_batch(blob, offsets, pks):
    """crypto_sign_open verdicts for n concatenated (sig || msg) records.

    blob: uint8 array; offsets: uint64 array of n+1 prefix offsets into blob; pks: uint8 (n, 32).
    Returns a bool array of n verdicts (True = libnacl.crypto_sign_open would not raise)."""
    if _device is None:
        ensure_device()
    # numpy inputs of the right type and layout pass through untouched (Plenum's small calls: every
    # microsecond here is on the request's latency)
    if type(offsets) is not np.ndarray or offsets.dtype != _U64 or not offsets.flags.c_contiguous:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.shape[0] - 1
    if n <= 0:
        return np.zeros(0, dtype=bool)
    if type(blob) is not np.ndarray or blob.dtype != _U8 or not blob.flags.c_contiguous:
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    if type(pks) is not np.ndarray or pks.dtype != _U8 or not pks.flags.c_contiguous:
        pks = np.ascontiguousarray(pks, dtype=np.uint8)
    if pks.size != 32 * n:
        raise ValueError("pks must hold n x 32 key bytes")
    bits = np.zeros((n + 7) // 8, dtype=np.uint8)
    fc = _fast if _fast is not None else _fastcall()
    if fc:  # the same C ABI call without ctypes' per-array marshalling
        rc = fc.verify(blob, offsets, pks, bits)
    else:
        if int(offsets[n]) > blob.size:
            raise ValueError("verify: inconsistent blob / offsets / keys / verdict sizes")
        rc = lib().pv_verify_batch(_ptr(blob), _ptr(offsets), n, _ptr(pks), _ptr(bits))
    if rc:
        check(rc, "pv_verify_batch")
    return np.unpackbits(bits, count=n, bitorder="little").view(bool)


def verify_one(pk, sm):
    """crypto_sign_open verdict of ONE (32-byte key, sig || msg) pair: the unbatched drop-in's call
    (Verifier.verify outside an authenticate_batch), without the arrays verify_sm_batch builds."""
    if _device is None:
        ensure_device()
    fc = _fast if _fast is not None else _fastcall()
    if fc and hasattr(fc, "verify_one"):
        rc = fc.verify_one(pk, sm)
        if rc < 0:
            check(rc, "pv_verify_batch")
        return bool(rc)
    off = np.array([0, len(sm)], dtype=np.uint64)
    return bool(verify_sm_batch(np.frombuffer(bytes(sm) or b"\0", dtype=np.uint8), off,
                                np.frombuffer(bytes(pk), dtype=np.uint8))[0])


def seed_keypairs(seeds):
    """crypto_sign_seed_keypair for a batch: seeds uint8 (n, 32) (or n x 32 bytes) -> (pks (n, 32),
    sks (n, 64) = seed || pk), byte-identical to libsodium. One GPU call (pv_sign_seed_keypairs)."""
    if _device is None:
        ensure_device()
    seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1)
    if seeds.size % 32:
        raise ValueError("seeds must be 32 bytes each")
    n = seeds.size // 32
    pks, sks = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    if n:
        check(lib().pv_sign_seed_keypairs(_ptr(seeds), n, _ptr(pks), _ptr(sks)), "pv_sign_seed_keypairs")
    return pks, sks


def sign_batch(blob, off, sks, signer_idx=None):
    """crypto_sign_detached for a batch: message i = blob[off[i]:off[i+1]] signed with the 64-byte secret
    key sks[signer_idx[i]] (signer_idx None: sks[i]). Returns the signatures, uint8 (n, 64),
    byte-identical to libsodium. One GPU call (pv_sign_batch)."""
    if _device is None:
        ensure_device()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = off.shape[0] - 1
    if n <= 0:
        return np.zeros((0, 64), np.uint8)
    blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    if int(off[n]) > blob.size or int(off[0]) > int(off[n]):
        raise ValueError("sign: offsets reach past the message blob")
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    sks = np.ascontiguousarray(sks, dtype=np.uint8).reshape(-1)
    if sks.size % 64 or sks.size == 0:
        raise ValueError("secret keys must be 64 bytes each (seed || public key)")
    n_signers = sks.size // 64
    if signer_idx is None:
        if n_signers != n:
            raise ValueError("without signer_idx there must be one secret key per message")
        idx = None
    else:
        idx = np.ascontiguousarray(signer_idx, dtype=np.uint32)
        if idx.shape != (n,):
            raise ValueError("signer_idx must hold one index per message")
    sigs = np.zeros((n, 64), np.uint8)
    check(lib().pv_sign_batch(_ptr(blob), _ptr(off), n, _ptr(sks), n_signers, _ptr(idx) if idx is not None else None,
                              _ptr(sigs)), "pv_sign_batch")
    return sigs


PV_INJECT_STAGE = 1  # pv_test_inject: fail the next host-buffer stagings of a device


class HostArena:
    """numpy arrays in the library's pinned host memory (pv_host_alloc). pv_verify_batch /
    pv_verify_batch_multi_gpu DMA inputs that live there straight to HBM (no pageable -> pinned
    staging copy): a node that receives its requests into such buffers, or builds its batch there,
    feeds the GPUs at PCIe rate. The block is freed when the last array viewing it is collected."""

    @staticmethod
    def empty(shape, dtype=np.uint8):
        dtype = np.dtype(dtype)
        count = int(np.prod(shape)) if np.ndim(shape) else int(shape)
        nbytes = max(1, count * dtype.itemsize)
        p = ctypes.c_void_p()
        check(lib().pv_host_alloc(ctypes.byref(p), nbytes), "pv_host_alloc")
        buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
        weakref.finalize(buf, lib().pv_host_free, p.value)
        return np.frombuffer(buf, dtype=np.uint8, count=count * dtype.itemsize).view(dtype).reshape(shape)

    @staticmethod
    def is_pinned(arr):
        arr = np.asarray(arr)
        return bool(lib().pv_host_is_pinned(arr.ctypes.data, arr.nbytes))

    @classmethod
    def batch(cls, blob, offsets, pks):
        """(blob, offsets, pks) copied into arena arrays, offsets rebased to 0 (the form whose offsets
        are DMA'd as they are)."""
        offsets = np.asarray(offsets, dtype=np.uint64)
        base, end = int(offsets[0]), int(offsets[-1])
        b = cls.empty(max(1, end - base))
        b[:end - base] = np.asarray(blob, np.uint8)[base:end]
        o = cls.empty(offsets.shape, np.uint64)
        np.subtract(offsets, np.uint64(base), out=o)
        k = cls.empty((len(offsets) - 1, 32))
        k[:] = np.asarray(pks, np.uint8).reshape(-1, 32)
        return b, o, k


def inject_stage_failures(device, count):
    """Test hook: the next `count` host-buffer stagings on `device` fail (pv_test_inject, declared in
    include/plenum_verify_test.h; the library refuses it unless PV_ENABLE_TEST_HOOKS=1 is set)."""
    check(lib().pv_test_inject(PV_INJECT_STAGE, int(device), int(count)), "pv_test_inject")


def comb_fused():
    """True if the library computes the comb path's [S]B and [k](-A) in one kernel (pv_comb_ab_kernel)."""
    return bool(lib().pv_build_flags() & PV_BUILD_COMB_FUSED)


def last_zero_copy():
    """True if the most recent host-buffer call (pv_verify_batch) took the zero-copy form."""
    return bool(lib().pv_last_zero_copy())


def shard_plan(n, ndev):
    """(bounds uint64[ndev + 1], verdict words per shard) of pv_verify_batch_multi_gpu's split of n
    requests over ndev devices (host-only, no GPU needed)."""
    b = np.zeros(ndev + 1, np.uint64)
    w = ctypes.c_uint64()
    check(lib().pv_shard_plan(int(n), int(ndev), b.ctypes.data_as(_c_u64p), ctypes.byref(w)), "pv_shard_plan")
    return b, w.value


_multi_devices = None


def ensure_devices(devices):
    """Bind this process to several GPUs for pv_verify_batch_multi_gpu (one context and one RCCL
    communicator per device, ncclCommInitAll). Raises NativeUnavailable when they are not visible."""
    global _multi_devices
    devices = tuple(sorted(set(int(d) for d in devices)))
    if _multi_devices == devices:
        return devices
    L = lib()
    ndev = L.pv_device_count()
    if ndev <= 0:
        raise NativeUnavailable("no HIP device visible: the verification engine is GPU-only")
    if not devices or devices[-1] >= ndev or devices[0] < 0:
        raise NativeUnavailable("devices %s not visible (%d GPUs)" % (list(devices), ndev))
    mask = 0
    for d in devices:
        mask |= 1 << d
    rc = L.pv_init_devices(mask)
    if rc != PV_OK:
        raise NativeUnavailable("pv_init_devices failed: %s" % L.pv_last_error().decode(errors="replace"))
    _multi_devices = devices
    return devices


def multi_gpu_clique():
    """The in-process clique as RCCL reports it: {"devices": [...], "nranks": ncclCommCount,
    "user_ranks": [ncclCommUserRank per device]} (pv_multi_gpu_devices / pv_multi_gpu_comm_ranks)."""
    L = lib()
    devs = (ctypes.c_int * 16)()
    nd = L.pv_multi_gpu_devices(devs, 16)
    nr, ranks = ctypes.c_int(), (ctypes.c_int * 16)()
    check(L.pv_multi_gpu_comm_ranks(ctypes.byref(nr), ranks, 16), "pv_multi_gpu_comm_ranks")
    return {"devices": list(devs[:nd]), "nranks": nr.value, "user_ranks": list(ranks[:nd])}


def comm_count():
    """(nranks, rank) of this process's rank communicator as RCCL reports them (pv_comm_count)."""
    nr, rk = ctypes.c_int(), ctypes.c_int()
    check(lib().pv_comm_count(ctypes.byref(nr), ctypes.byref(rk)), "pv_comm_count")
    return nr.value, rk.value


def verify_sm_batch_multi(blob, offsets, pks, devices=None):
    """verify_sm_batch sharded over several GPUs of this process (pv_verify_batch_multi_gpu: one shard
    per device, verdict bitmaps gathered with one RCCL all-gather). devices: the GPUs to use (default:
    every visible one, or the set already bound)."""
    if devices is None:
        devices = _multi_devices or range(max(1, lib().pv_device_count()))
    ensure_devices(devices)
    L = lib()
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    if n <= 0:
        return np.zeros(0, dtype=bool)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    pks = np.ascontiguousarray(pks, dtype=np.uint8).reshape(n, 32)
    bits = np.zeros((n + 7) // 8, dtype=np.uint8)
    check(L.pv_verify_batch_multi_gpu(_ptr(blob), _ptr(offsets), n, _ptr(pks), _ptr(bits)),
          "pv_verify_batch_multi_gpu")
    return np.unpackbits(bits, bitorder="little")[:n].astype(bool)


def multi_gpu_engine(devices):
    """An engine callable (blob, off, pks) -> verdicts for authenticate_batch(engine=...) that shards
    every batch over `devices` (SURVEY.md §8b pv_verify_batch_multi_gpu)."""
    devices = tuple(devices)

    def engine(blob, off, pks):
        return verify_sm_batch_multi(blob, off, pks, devices)

    engine.devices = devices
    return engine


def set_path(mode):
    """Select the arithmetic path (PV_PATH_AUTO / PV_PATH_STRAUS / PV_PATH_COMB / PV_PATH_LATENCY);
    verdicts are identical on every path."""
    check(lib().pv_set_path(int(mode)), "pv_set_path")


def last_path():
    """(path, distinct keys) of the most recent chunk: path is PV_PATH_STRAUS or PV_PATH_COMB."""
    p, u = ctypes.c_int(), ctypes.c_uint32()
    check(lib().pv_last_path(ctypes.byref(p), ctypes.byref(u)), "pv_last_path")
    return p.value, u.value


def last_split():
    """(distinct keys, keys with a comb table, requests verified with them) of the most recent
    chunk; the remaining requests took the Straus path. Synchronises (via pv_last_path)."""
    last_path()
    v = [ctypes.c_uint32() for _ in range(3)]
    check(lib().pv_last_split(*[ctypes.byref(x) for x in v]), "pv_last_split")
    return tuple(x.value for x in v)


PV_TABLE_REUSE_CAP = 16384 - 2048  # default capacity of table reuse (csrc/pv_engine_dev.h PV_DIR_DEFAULT_CAP)


def table_reuse(on=True, capacity=0):
    """Keep the comb tables a large keyed chunk builds and read them in later chunks and calls
    (pv_table_reuse; on by default). capacity: tables the engine may keep, 0 = unchanged."""
    check(lib().pv_table_reuse(1 if on else 0, int(capacity)), "pv_table_reuse")


def table_reuse_stats():
    """(hits, built, resets) of table reuse since pv_init: tables read instead of built, tables built,
    times the kept tables were dropped to make room. Synchronises the device."""
    v = [ctypes.c_uint64() for _ in range(3)]
    check(lib().pv_table_reuse_stats(*[ctypes.byref(x) for x in v]), "pv_table_reuse_stats")
    return tuple(x.value for x in v)


def table_affine(on=True):
    """Convert the kept tables a large keyed chunk reads to affine rows for the chunks that follow
    (pv_table_affine; on by default). Switching empties the kept tables."""
    check(lib().pv_table_affine(1 if on else 0), "pv_table_affine")


def table_affine_stats():
    """(converted, affine_reads) since pv_init: kept tables converted to affine rows, and kept tables
    read in that form. Synchronises the device."""
    v = [ctypes.c_uint64() for _ in range(2)]
    check(lib().pv_table_affine_stats(*[ctypes.byref(x) for x in v]), "pv_table_affine_stats")
    return tuple(x.value for x in v)


PV_TABLE_WIDE_CAP = 2048  # default capacity of the wide-row pool (csrc/pv_engine_dev.h PV_WIDE_DEFAULT)


def table_wide(capacity=PV_TABLE_WIDE_CAP):
    """Build radix-2^11 rows for the kept tables large keyed chunks keep reading, in a pool of `capacity`
    tables (pv_table_wide; 2,048 by default, 0 = off). A change empties the kept tables."""
    check(lib().pv_table_wide(int(capacity)), "pv_table_wide")


def table_wide_stats():
    """(widened, wide_reads) since pv_init: kept tables given wide rows, and kept tables read from them
    (counted among table_affine_stats' affine reads too). Synchronises the device."""
    v = [ctypes.c_uint64() for _ in range(2)]
    check(lib().pv_table_wide_stats(*[ctypes.byref(x) for x in v]), "pv_table_wide_stats")
    return tuple(x.value for x in v)


def _blob(items):
    """Concatenate byte strings -> (uint8 blob (never empty), uint64 offsets)."""
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        np.cumsum(np.fromiter((len(x) for x in items), dtype=np.uint64, count=len(items)), out=off[1:])
    joined = b"".join(items)
    return (np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, np.uint8)), off


def ingress_verify_arrays(sig_blob, sig_off, msg_blob, msg_off, msg_idx, signer_idx, idr_blob, idr_off, vk_blob,
                          vk_off, vk_present):
    """pv_ingress_verify on packed arrays (uint8 blobs, uint64 offsets, uint32 indices, uint8 flags):
    GPU base58 decode of every signature, GPU key resolution per signer, device-side sm assembly
    and verification. Returns (status uint8[n], verdict bool[n]); status codes in
    include/plenum_verify.h."""
    ensure_device()
    n = len(sig_off) - 1
    if n <= 0:
        return np.zeros(0, np.uint8), np.zeros(0, bool)
    status = np.zeros(n, np.uint8)
    bits = np.zeros((n + 7) // 8, np.uint8)
    c = np.ascontiguousarray
    args = [c(sig_blob, np.uint8), c(sig_off, np.uint64), c(msg_idx, np.uint32), c(signer_idx, np.uint32),
            c(msg_blob, np.uint8), c(msg_off, np.uint64), c(idr_blob, np.uint8), c(idr_off, np.uint64),
            c(vk_blob, np.uint8), c(vk_off, np.uint64), c(vk_present, np.uint8)]
    sb, so, mi, si, mb, mo, ib, io, vb, vo, vp = [a if a.size else np.zeros(1, a.dtype) for a in args]
    check(lib().pv_ingress_verify(_ptr(sb), _ptr(so), _ptr(mi), _ptr(si), n, _ptr(mb), _ptr(mo), len(msg_off) - 1,
                                  _ptr(ib), _ptr(io), _ptr(vb), _ptr(vo), _ptr(vp), len(idr_off) - 1,
                                  _ptr(status), _ptr(bits)), "pv_ingress_verify")
    return status, np.unpackbits(bits, bitorder="little")[:n].astype(bool)


def ingress_verify(sigs, msgs, msg_idx, signer_idx, idrs, vks):
    """ingress_verify_arrays on Python lists: sigs (n byte strings), msgs (byte strings),
    msg_idx / signer_idx (n ints), idrs (identifier bytes per signer, b"" = None), vks (verkey
    bytes or None per signer)."""
    sig_b, sig_o = _blob(list(sigs))
    msg_b, msg_o = _blob(list(msgs))
    idr_b, idr_o = _blob(list(idrs))
    vk_b, vk_o = _blob([v if v is not None else b"" for v in vks])
    vkp = np.array([v is not None for v in vks], dtype=np.uint8)
    return ingress_verify_arrays(sig_b, sig_o, msg_b, msg_o, np.asarray(msg_idx, np.uint32),
                                 np.asarray(signer_idx, np.uint32), idr_b, idr_o, vk_b, vk_o, vkp)


class KeyCache:
    """The engine's node-side key cache (include/plenum_verify.h pv_key_cache_*): known signers'
    keys verified with 32 comb-table additions on the latency path instead of 252 doublings."""

    @staticmethod
    def configure(capacity):
        ensure_device()
        check(lib().pv_key_cache_configure(int(capacity)), "pv_key_cache_configure")

    @staticmethod
    def put(pks):
        """pks: iterable of 32-byte keys, or a uint8 array (n, 32)."""
        ensure_device()
        a = np.frombuffer(b"".join(pks), np.uint8) if not isinstance(pks, np.ndarray) else pks
        a = np.ascontiguousarray(a, np.uint8).reshape(-1)
        if a.size % 32:
            raise ValueError("keys must be 32 bytes each")
        n = a.size // 32
        check(lib().pv_key_cache_put(_ptr(a if a.size else np.zeros(32, np.uint8)), n), "pv_key_cache_put")

    @staticmethod
    def clear():
        check(lib().pv_key_cache_clear(), "pv_key_cache_clear")

    @staticmethod
    def enable(on=True):
        check(lib().pv_key_cache_enable(1 if on else 0), "pv_key_cache_enable")

    @staticmethod
    def stats():
        size, cap = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().pv_key_cache_stats(ctypes.byref(size), ctypes.byref(cap)), "pv_key_cache_stats")
        return size.value, cap.value

    @staticmethod
    def auto(min_seen):
        """Automatic admission: a key seen min_seen times in host batches of <= 4,096 requests is put
        into the cache behind that batch (0 = off)."""
        check(lib().pv_key_cache_auto(int(min_seen)), "pv_key_cache_auto")

    @staticmethod
    def auto_stats():
        a, f = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().pv_key_cache_auto_stats(ctypes.byref(a), ctypes.byref(f)), "pv_key_cache_auto_stats")
        return a.value, f.value

    @staticmethod
    def contains(pk):
        b = np.frombuffer(bytes(pk), np.uint8)
        if b.size != 32:
            raise ValueError("keys must be 32 bytes each")
        return bool(lib().pv_key_cache_contains(_ptr(b)))



# ------------------------------------------------------------------------------------------ Merkle
PV_MERKLE_AUTO, PV_MERKLE_HOST, PV_MERKLE_DEVICE = 0, 1, 2
PV_MERKLE_AUTO_MIN = 2048   # include/plenum_verify.h: AUTO takes the device path from this many leaves
PV_MERKLE_AUTO_MIN_PROOFS = 1024  # the same when per-leaf roots or audit paths are asked for
PV_MERKLE_AUTO_MIN_VERIFY = 512  # proofs from which AUTO checks on the device
PV_MERKLE_AUTO_MIN_CONSISTENCY = 256  # the same for consistency proofs
# status of a consistency check (csrc/merkle_core.h pv_merkle_consistency_check)
(PV_MK_CONSISTENT, PV_MK_OLD_LARGER, PV_MK_CONS_TOO_SHORT, PV_MK_NEW_DIFFERS, PV_MK_OLD_DIFFERS, PV_MK_SAME_SIZE,
 PV_MK_REPLY_RANGE) = range(7)
PV_MERKLE_AUTO_MIN_PROVE = 32768  # queries from which AUTO generates proofs on the device
PV_MK_Q_INCLUSION, PV_MK_Q_CONSISTENCY, PV_MK_Q_ROOT = 0, 1, 2  # kinds of a proof query
PV_MK_PROVED, PV_MK_Q_RANGE, PV_MK_Q_ROOM = 0, 1, 2  # status of a proof query
PV_MERKLE_CHUNK = 1048576
MERKLE_OUTPUTS = ("leaf_hash", "node_hash", "frontier", "root", "roots", "path")


class PvMerkleOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("leaf_hash", "node_hash", "frontier", "root", "roots", "path", "path_off")]


def merkle_plan(tree_size, n):
    """(new node hashes, frontier length after, hashes of all audit paths) of n appends to tree_size leaves."""
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(lib().pv_merkle_plan(tree_size, n, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "pv_merkle_plan")
    return a.value, b.value, c.value


def merkle_chunk(leaves=0):
    check(lib().pv_merkle_chunk(leaves), "pv_merkle_chunk")


_merkle_mode = PV_MERKLE_AUTO
_merkle_no_device = False  # a device was looked for once and none is visible


def merkle_path(mode=PV_MERKLE_AUTO):
    global _merkle_mode
    check(lib().pv_merkle_path(mode), "pv_merkle_path")
    _merkle_mode = mode


def _merkle_device_ready(n, auto_min):
    """Bind a GPU only for a call that will take the device path (mode DEVICE, or AUTO at or above its
    threshold): a process that only hashes small batches, or runs where no GPU is visible, never builds
    the verification engine's context; the library's host path serves it. The look for a device happens once."""
    global _merkle_no_device
    if _device is not None or _merkle_no_device or _merkle_mode == PV_MERKLE_HOST:
        return
    if _merkle_mode == PV_MERKLE_AUTO and n < auto_min:
        return
    try:
        ensure_device()
    except NativeUnavailable:
        _merkle_no_device = True


def merkle_append(tree_size, frontier, blob, off, want=MERKLE_OUTPUTS, _catchup=None):
    """n sequential CompactMerkleTree.append calls as one pv_merkle_append_batch: leaf i = blob[off[i]:off[i+1]]
    appended to the tree (tree_size, frontier = tree.hashes joined). Returns a dict of the outputs named in
    `want` (uint8 arrays; "path" also brings "path_off", uint64 in hash units)."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = off.shape[0] - 1
    _merkle_device_ready(n, PV_MERKLE_AUTO_MIN_PROOFS if "roots" in want or "path" in want or _catchup
                         else PV_MERKLE_AUTO_MIN)
    if n < 0:
        raise ValueError("merkle_append: offsets must hold n + 1 entries")
    blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    if int(off[n]) > blob.size:
        raise ValueError("merkle_append: offsets reach past the blob")
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    front = np.frombuffer(bytes(frontier) or b"\0", dtype=np.uint8)
    if tree_size and front.size != 32 * bin(tree_size).count("1"):
        raise ValueError("merkle_append: the frontier must hold popcount(tree_size) hashes")
    n_nodes, _, n_path = merkle_plan(tree_size, n)
    res, out = {}, PvMerkleOut()
    shapes = {"leaf_hash": (n, 32), "node_hash": (n_nodes, 32), "frontier": (64, 32), "root": (32,), "roots": (n, 32),
              "path": (n_path, 32)}
    keep = []  # an empty output still passes a non-null pointer, so it counts as wanted
    for k in want:
        res[k] = np.zeros(shapes[k], np.uint8)
        keep.append(res[k] if res[k].size else np.zeros(32, np.uint8))
        setattr(out, k, keep[-1].ctypes.data)
    if "path" in want:
        res["path_off"] = np.zeros(n + 1, np.uint64)
        out.path_off = res["path_off"].ctypes.data
    if _catchup:  # merkle_catchup: the same outputs, and the replies checked in the same call
        ends, final_size, final_root, pbuf, poff, status, bits = _catchup
        check(lib().pv_merkle_catchup_batch(tree_size, _ptr(front) if tree_size else None, _ptr(blob), _ptr(off), n,
                                            _ptr(ends), ends.shape[0], final_size, _ptr(final_root), _ptr(pbuf), _ptr(poff),
                                            ctypes.byref(out), _ptr(status), _ptr(bits)), "pv_merkle_catchup_batch")
    else:
        check(lib().pv_merkle_append_batch(tree_size, _ptr(front) if tree_size else None, _ptr(blob), _ptr(off), n,
                                           ctypes.byref(out)), "pv_merkle_append_batch")
    if "frontier" in res:
        res["frontier"] = res["frontier"][:bin(tree_size + n).count("1")]
    return res


def merkle_verify_inclusion(leaf_index, tree_size, proofs, roots, leaves=None, leaf_hashes=None):
    """MerkleVerifier.verify_leaf_inclusion (leaves) / verify_leaf_hash_inclusion (leaf_hashes) for n proofs:
    proofs[i] a list of 32-byte hashes, roots[i] 32 bytes. Returns (verdicts bool[n], status uint8[n])."""
    n = len(proofs)
    _merkle_device_ready(n, PV_MERKLE_AUTO_MIN_VERIFY)
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, np.uint8)
    if (leaves is None) == (leaf_hashes is None):
        raise ValueError("merkle_verify_inclusion: give either leaves or leaf_hashes")
    poff = np.zeros(n + 1, np.uint64)
    np.cumsum([len(p) for p in proofs], out=poff[1:])
    pbuf = np.frombuffer(b"".join(b"".join(p) for p in proofs) or bytes(32), dtype=np.uint8)
    if pbuf.size != 32 * int(poff[n]) and int(poff[n]):
        raise ValueError("merkle_verify_inclusion: proof hashes must be 32 bytes each")
    rbuf = np.frombuffer(b"".join(roots), dtype=np.uint8)
    if rbuf.size != 32 * n:
        raise ValueError("merkle_verify_inclusion: roots must be 32 bytes each")
    idx = np.ascontiguousarray(leaf_index, dtype=np.uint64)
    size = np.ascontiguousarray(tree_size, dtype=np.uint64)
    data = doff = lh = None
    if leaves is not None:
        data, doff = _blob(leaves)
        if data.size == 0:
            data = np.zeros(1, np.uint8)
    else:
        lh = np.frombuffer(b"".join(leaf_hashes), dtype=np.uint8)
        if lh.size != 32 * n:
            raise ValueError("merkle_verify_inclusion: leaf hashes must be 32 bytes each")
    status, bits = np.zeros(n, np.uint8), np.zeros((n + 7) // 8, np.uint8)
    check(lib().pv_merkle_verify_inclusion_batch(
        _ptr(data) if data is not None else None, _ptr(doff) if doff is not None else None,
        _ptr(lh) if lh is not None else None, _ptr(idx), _ptr(size), _ptr(pbuf), _ptr(poff), _ptr(rbuf), n, _ptr(status),
        _ptr(bits)), "pv_merkle_verify_inclusion_batch")
    return np.unpackbits(bits, count=n, bitorder="little").view(bool), status


def _proof_arrays(proofs, who):
    n = len(proofs)
    poff = np.zeros(n + 1, np.uint64)
    if n:
        np.cumsum([len(p) for p in proofs], out=poff[1:])
    pbuf = np.frombuffer(b"".join(b"".join(p) for p in proofs) or bytes(32), dtype=np.uint8)
    if pbuf.size != 32 * int(poff[n]) and int(poff[n]):
        raise ValueError(who + ": proof hashes must be 32 bytes each")
    return pbuf, poff


def merkle_verify_consistency(old_sizes, new_sizes, old_roots, new_roots, proofs):
    """MerkleVerifier.verify_tree_consistency for n proofs as one pv_merkle_verify_consistency_batch: proofs[i] a
    list of 32-byte hashes, the roots 32 bytes each. Returns (verdicts bool[n], status uint8[n]); status codes
    PV_MK_* above."""
    n = len(proofs)
    _merkle_device_ready(n, PV_MERKLE_AUTO_MIN_CONSISTENCY)
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, np.uint8)
    pbuf, poff = _proof_arrays(proofs, "merkle_verify_consistency")
    obuf, nbuf = np.frombuffer(b"".join(old_roots), dtype=np.uint8), np.frombuffer(b"".join(new_roots), dtype=np.uint8)
    if obuf.size != 32 * n or nbuf.size != 32 * n:
        raise ValueError("merkle_verify_consistency: roots must be 32 bytes each")
    old = np.ascontiguousarray(old_sizes, dtype=np.uint64)
    new = np.ascontiguousarray(new_sizes, dtype=np.uint64)
    if old.shape != (n,) or new.shape != (n,):
        raise ValueError("merkle_verify_consistency: one old and one new size per proof")
    status, bits = np.zeros(n, np.uint8), np.zeros((n + 7) // 8, np.uint8)
    check(lib().pv_merkle_verify_consistency_batch(_ptr(old), _ptr(new), _ptr(obuf), _ptr(nbuf), _ptr(pbuf), _ptr(poff), n,
                                                   _ptr(status), _ptr(bits)), "pv_merkle_verify_consistency_batch")
    return np.unpackbits(bits, count=n, bitorder="little").view(bool), status


def merkle_catchup(tree_size, frontier, blob, off, reply_end, final_size, final_root, proofs, want=()):
    """pv_merkle_catchup_batch: the n leaves of a chain of catch-up replies appended to the tree (tree_size,
    frontier) as merkle_append does, and reply r (ending at absolute size reply_end[r], with consistency
    proof proofs[r] towards the tree of final_size leaves and root final_root) checked in the same call.
    Returns (verdicts bool[R], status uint8[R], merkle_append's dict for `want`)."""
    ends = np.ascontiguousarray(reply_end, dtype=np.uint64)
    R = ends.shape[0]
    if len(proofs) != R:
        raise ValueError("merkle_catchup: one proof per reply")
    if len(final_root) != 32:
        raise ValueError("merkle_catchup: the final root must be 32 bytes")
    pbuf, poff = _proof_arrays(proofs, "merkle_catchup")
    status, bits = np.zeros(max(R, 1), np.uint8), np.zeros((R + 7) // 8 + 1, np.uint8)
    root = np.frombuffer(bytes(final_root), dtype=np.uint8)
    res = merkle_append(tree_size, frontier, blob, off, want=want,
                        _catchup=(ends if R else np.zeros(1, np.uint64)[:0], int(final_size), root, pbuf, poff, status, bits))
    return np.unpackbits(bits, count=R, bitorder="little").view(bool), status[:R], res


def merkle_prove_plan(n_leaves, kinds, a, b):
    """pv_merkle_prove_plan: (out_off uint64[q + 1], status uint8[q]) of q queries against a store of n_leaves."""
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    q = kinds.shape[0]
    if a.shape != (q,) or b.shape != (q,):
        raise ValueError("merkle_prove: one kind, a and b per query")
    out_off, status = np.zeros(q + 1, np.uint64), np.zeros(max(q, 1), np.uint8)
    check(lib().pv_merkle_prove_plan(n_leaves, _ptr(kinds), _ptr(a), _ptr(b), q, _ptr(out_off), _ptr(status)),
          "pv_merkle_prove_plan")
    return out_off, status[:q]


def merkle_prove(leaf_hashes, node_hashes, kinds, a, b):
    """q proofs from a hash store as one pv_merkle_prove_batch. leaf_hashes / node_hashes: the store's two
    sequences as contiguous bytes (32 per hash, anything with the buffer protocol; the node hashes of
    len(leaf_hashes) / 32 leaves). Query i is (kinds[i], a[i], b[i]): PV_MK_Q_INCLUSION inclusion_proof(a, b),
    PV_MK_Q_CONSISTENCY consistency_proof(a, b), PV_MK_Q_ROOT merkle_tree_hash(0, b). Returns (out_off uint64[q + 1],
    hashes uint8[out_off[q], 32], status uint8[q]): proof i is hashes[out_off[i]:out_off[i + 1]]; status 1 marks a
    query out of range, which has no hashes."""
    leaf = np.frombuffer(leaf_hashes, dtype=np.uint8)
    node = np.frombuffer(node_hashes, dtype=np.uint8)
    n = leaf.size // 32
    if leaf.size % 32 or node.size != 32 * (n - bin(n).count("1")):
        raise ValueError("merkle_prove: the store must hold 32 n bytes of leaf hashes and 32 (n - popcount(n)) of node hashes")
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    q = kinds.shape[0]
    _merkle_device_ready(q, PV_MERKLE_AUTO_MIN_PROVE)
    out_off, status = merkle_prove_plan(n, kinds, a, b)
    out = np.zeros((int(out_off[q]), 32), np.uint8)
    if q:
        pad = np.zeros(32, np.uint8)
        check(lib().pv_merkle_prove_batch(_ptr(leaf if leaf.size else pad), n, _ptr(node if node.size else pad), _ptr(kinds),
                                          _ptr(a), _ptr(b), q, _ptr(out_off), _ptr(out if out.size else pad), _ptr(status)),
              "pv_merkle_prove_batch")
    return out_off, out, status


# -------------------------------------------------------------------------------------- state trie
PV_TRIE_NEED_NODES, PV_TRIE_NEED_SPACE = 1, 2
PV_TRIE_AUTO, PV_TRIE_HOST, PV_TRIE_DEVICE = 0, 1, 2
PV_TRIE_AUTO_MIN = 352  # include/plenum_verify.h: records from which AUTO hashes on the device
PV_TRIE_MAX_KEY, PV_TRIE_MAX_VALUE = 65535, (1 << 24) - 1


class PvTrieOut(ctypes.Structure):
    _fields_ = [("root", ctypes.c_void_p), ("node_hash", ctypes.c_void_p), ("node_cap", ctypes.c_uint64),
                ("node_blob", ctypes.c_void_p), ("blob_cap", ctypes.c_uint64), ("node_off", ctypes.c_void_p),
                ("node_len", ctypes.c_void_p), ("missing", ctypes.c_void_p), ("missing_cap", ctypes.c_uint64),
                ("n_nodes", ctypes.c_uint64), ("blob_bytes", ctypes.c_uint64), ("n_missing", ctypes.c_uint64),
                ("launches", ctypes.c_uint64), ("tail_records", ctypes.c_uint64)]


_trie_mode = PV_TRIE_AUTO
_trie_no_device = False
# how the last trie_update or trie_root ran; built_on_device: the structure too was built by kernels (trie_root)
trie_last = {"launches": 0, "tail_records": 0, "nodes": 0, "rounds": 0, "built_on_device": False}


def trie_path(mode=PV_TRIE_AUTO):
    global _trie_mode
    check(lib().pv_trie_path(mode), "pv_trie_path")
    _trie_mode = mode


def _trie_device_ready(work, auto_min=PV_TRIE_AUTO_MIN):
    """As _merkle_device_ready: a GPU is bound only by a call that will hash on it."""
    global _trie_no_device
    if _device is not None or _trie_no_device or _trie_mode == PV_TRIE_HOST:
        return
    if _trie_mode == PV_TRIE_AUTO and work < auto_min:
        return
    try:
        ensure_device()
    except NativeUnavailable:
        _trie_no_device = True


def sha3_256_batch(blob, off):
    """SHA3-256 of the records blob[off[i]:off[i+1]] -> uint8 array (n, 32), one pv_sha3_256_batch."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = off.shape[0] - 1
    if n < 0:
        raise ValueError("sha3_256_batch: offsets must hold n + 1 entries")
    blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    if n and int(off[n]) > blob.size:
        raise ValueError("sha3_256_batch: offsets reach past the blob")
    _trie_device_ready(n)
    out = np.zeros((n, 32), np.uint8)
    if n:
        check(lib().pv_sha3_256_batch(_ptr(blob if blob.size else np.zeros(1, np.uint8)), _ptr(off), n, _ptr(out)),
              "pv_sha3_256_batch")
    return out


def trie_update_raw(root, known_hashes, known_rlps, keys, values, node_cap=None, blob_cap=None, missing_cap=None):
    """One pv_trie_update_batch. Returns (rc, root bytes, [(hash, rlp)], [missing hashes], PvTrieOut)."""
    n, k = len(keys), len(known_hashes)
    kb, ko = _blob(keys)
    vb, vo = _blob(values)
    nb, no = _blob(known_rlps)
    nh = np.frombuffer(b"".join(known_hashes) or bytes(32), np.uint8)
    if nh.size != 32 * max(k, 1):
        raise ValueError("trie_update: known hashes must be 32 bytes each")
    if node_cap is None:
        node_cap = 2 * n + k + 16
    if blob_cap is None:
        blob_cap = int(nb.size) + int(kb.size) + int(vb.size) + 640 * n + 80 * k + 1024
    if missing_cap is None:
        missing_cap = 16 * n + 16
    rootbuf = np.zeros(32, np.uint8)
    hashes = np.zeros((max(node_cap, 1), 32), np.uint8)
    nblob = np.zeros(max(blob_cap, 1), np.uint8)
    noff, nlen = np.zeros(max(node_cap, 1), np.uint64), np.zeros(max(node_cap, 1), np.uint64)
    miss = np.zeros((max(missing_cap, 1), 32), np.uint8)
    out = PvTrieOut(rootbuf.ctypes.data, hashes.ctypes.data, node_cap, nblob.ctypes.data, blob_cap, noff.ctypes.data,
                    nlen.ctypes.data, miss.ctypes.data, missing_cap)
    rc = lib().pv_trie_update_batch(bytes(root), _ptr(nh), _ptr(nb), _ptr(no), k, _ptr(kb), _ptr(ko), _ptr(vb), _ptr(vo),
                                    n, ctypes.byref(out))
    nodes, missing = [], []
    if rc == PV_OK:
        data = nblob.tobytes()
        nodes = [(hashes[i].tobytes(), data[int(noff[i]):int(noff[i]) + int(nlen[i])]) for i in range(out.n_nodes)]
    elif rc == PV_TRIE_NEED_NODES:
        missing = [miss[i].tobytes() for i in range(min(out.n_missing, missing_cap))]
    return rc, rootbuf.tobytes(), nodes, missing, out


def trie_update(root, fetch, keys, values):
    """The trie under `root` overlaid with keys[i] -> values[i] (values as the trie stores them), as one call
    chain: pv_trie_update_batch says which existing nodes it lacks, fetch(hash) -> RLP brings them, until none
    are missing. Returns (new root, [(hash, rlp)] of every new node, the root last)."""
    n = len(keys)
    _trie_device_ready(2 * n)  # at least a node per set; the library decides by the real count
    known = {}
    caps = {}
    rounds = 0
    while True:
        rounds += 1
        hs = list(known)
        rc, new_root, nodes, missing, out = trie_update_raw(root, hs, [known[h] for h in hs], keys, values, **caps)
        if rc == PV_TRIE_NEED_NODES:
            if out.n_missing > len(missing):  # more than the list held: a larger list, the same round again
                caps["missing_cap"] = int(out.n_missing)
            for h in missing:
                known[h] = bytes(fetch(h))
            continue
        if rc == PV_TRIE_NEED_SPACE:
            caps["node_cap"], caps["blob_cap"] = int(out.n_nodes), int(out.blob_bytes)
            continue
        check(rc, "pv_trie_update_batch")
        trie_last.update(launches=int(out.launches), tail_records=int(out.tail_records), nodes=len(nodes), rounds=rounds,
                         built_on_device=False)
        return new_root, nodes


PV_TRIE_BUILD_MAX_KEY, PV_TRIE_ROOT_WRAP = 64, 1
PV_TRIE_BUILD_AUTO_MIN = 512  # include/plenum_verify.h: pairs from which AUTO runs the device builder


class PvTrieRootOut(ctypes.Structure):
    _fields_ = [("root", ctypes.c_uint8 * 32), ("n_keys", ctypes.c_uint64), ("n_nodes", ctypes.c_uint64),
                ("n_records", ctypes.c_uint64), ("arena_bytes", ctypes.c_uint64), ("max_depth", ctypes.c_uint64),
                ("launches", ctypes.c_uint64), ("tail_records", ctypes.c_uint64), ("built_on_device", ctypes.c_uint64)]


def trie_root(keys, val_blob, val_off, wrap=True):
    """The root of the trie built from empty of keys[i] -> val_blob[val_off[i]:val_off[i+1]], one pv_trie_root:
    keys a (n, key_len) uint8 array with key_len 1 .. 64, wrap: the trie stores rlp([value]) as PruningState.set
    does. No per-item Python. Returns the 32 root bytes; trie_last says how the call ran."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    if keys.ndim != 2:
        raise ValueError("trie_root: keys must be a (n, key_len) array")
    n, key_len = keys.shape
    val_off = np.ascontiguousarray(val_off, dtype=np.uint64)
    val_blob = np.ascontiguousarray(val_blob, dtype=np.uint8).reshape(-1)
    if val_off.shape[0] != n + 1:
        raise ValueError("trie_root: offsets must hold n + 1 entries")
    if n and int(val_off.max()) > val_blob.size:
        raise ValueError("trie_root: offsets reach past the blob")
    _trie_device_ready(n, PV_TRIE_BUILD_AUTO_MIN)
    out = PvTrieRootOut()
    check(lib().pv_trie_root(_ptr(keys if keys.size else np.zeros(1, np.uint8)), key_len, n,
                             _ptr(val_blob if val_blob.size else np.zeros(1, np.uint8)), _ptr(val_off),
                             PV_TRIE_ROOT_WRAP if wrap else 0, ctypes.byref(out)), "pv_trie_root")
    trie_last.update(launches=int(out.launches), tail_records=int(out.tail_records), nodes=int(out.n_records), rounds=1,
                     built_on_device=bool(out.built_on_device), n_keys=int(out.n_keys), n_nodes=int(out.n_nodes),
                     max_depth=int(out.max_depth), arena_bytes=int(out.arena_bytes))
    return bytes(out.root)


# ------------------------------------------------------------------------------------- state proofs
PV_PROOF_REJECT, PV_PROOF_ACCEPT, PV_PROOF_DEFER = 0, 1, 2
PV_PROOF_MAX_NODES = 1024
PV_TRIE_PROOF_AUTO_MIN = 259  # include/plenum_verify.h: proof records from which AUTO takes the device path


class PvProofIn(ctypes.Structure):
    _fields_ = [("node_blob", ctypes.c_void_p), ("node_off", ctypes.c_void_p), ("n_nodes", ctypes.c_uint64),
                ("proof_first", ctypes.c_void_p), ("n_proofs", ctypes.c_uint64), ("query_proof", ctypes.c_void_p),
                ("root", ctypes.c_void_p), ("key_blob", ctypes.c_void_p), ("key_off", ctypes.c_void_p),
                ("val_blob", ctypes.c_void_p), ("val_off", ctypes.c_void_p), ("n_queries", ctypes.c_uint64),
                ("node_len", ctypes.c_void_p)]


# how the last trie_verify_proofs_raw ran: records hashed, queries, queries deferred, kernel launches (0: host path)
proof_last = {"nodes": 0, "queries": 0, "deferred": 0, "launches": 0}


def trie_proof_split(sers):
    """One pv_trie_proof_split over serialized proofs (each the RLP list of its nodes): (blob, proof_first,
    node_off, node_len, ok). Record i is blob[node_off[i]:node_off[i] + node_len[i]], proof p has the records
    proof_first[p] .. proof_first[p + 1]; ok[p] = 0 for a proof whose outer list is not canonical RLP."""
    n = len(sers)
    blob, off = _blob(sers)
    first, ok = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8)
    cap = max(16, int(blob.size) // 32)
    while True:
        node_off, node_len, count = np.zeros(cap + 1, np.uint64), np.zeros(cap, np.uint64), ctypes.c_uint64()
        rc = lib().pv_trie_proof_split(_ptr(blob), _ptr(off), n, _ptr(first), _ptr(node_off), _ptr(node_len), cap,
                                       ctypes.byref(count), _ptr(ok))
        if rc != PV_TRIE_NEED_SPACE:
            break
        cap = int(count.value)
    check(rc, "pv_trie_proof_split")
    k = int(count.value)
    return blob, first, node_off[:k + 1], node_len[:k], ok[:n]


def trie_verify_proofs_raw(node_blob, node_off, node_len, proof_first, query_proof, roots, key_blob, key_off, val_blob,
                           val_off):
    """One pv_trie_verify_proofs on arrays laid out as PvProofIn says (node_len None: record i ends at
    node_off[i + 1]). Returns the uint8 status per query."""
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)  # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)  # noqa: E731
    node_blob, node_off, proof_first = u8(node_blob), u64(node_off), u64(proof_first)
    node_len = u64(node_len) if node_len is not None else None
    query_proof = np.ascontiguousarray(query_proof, dtype=np.uint32)
    roots, key_blob, key_off, val_blob, val_off = u8(roots), u8(key_blob), u64(key_off), u8(val_blob), u64(val_off)
    nn, npf, nq = node_off.shape[0] - 1, proof_first.shape[0] - 1, query_proof.shape[0]
    if nn < 0 or npf < 0 or key_off.shape[0] != nq + 1 or val_off.shape[0] != nq + 1 or roots.size != 32 * nq or \
            (node_len is not None and node_len.shape[0] != nn):
        raise ValueError("trie_verify_proofs: array sizes do not fit together")
    ends = node_off[:-1] + node_len if node_len is not None else node_off[1:]
    if (nn and int(ends.max()) > node_blob.size) or (nq and (int(key_off[nq]) > key_blob.size or int(val_off[nq]) > val_blob.size)):
        raise ValueError("trie_verify_proofs: offsets reach past a blob")
    status = np.zeros(nq, np.uint8)
    if nq == 0:
        return status
    _trie_device_ready(nn, PV_TRIE_PROOF_AUTO_MIN)
    pad = lambda a: a if a.size else np.zeros(1, np.uint8)  # noqa: E731
    keep = [pad(node_blob), pad(key_blob), pad(val_blob), pad(roots)]
    arg = PvProofIn(keep[0].ctypes.data, node_off.ctypes.data, nn, proof_first.ctypes.data, npf, query_proof.ctypes.data,
                    keep[3].ctypes.data, keep[1].ctypes.data, key_off.ctypes.data, keep[2].ctypes.data, val_off.ctypes.data,
                    nq, node_len.ctypes.data if node_len is not None else None)
    check(lib().pv_trie_verify_proofs(ctypes.byref(arg), _ptr(status)), "pv_trie_verify_proofs")
    device = _device is not None and (_trie_mode == PV_TRIE_DEVICE or (_trie_mode == PV_TRIE_AUTO and nn >= PV_TRIE_PROOF_AUTO_MIN))
    proof_last.update(nodes=nn, queries=nq, deferred=int((status == PV_PROOF_DEFER).sum()),
                      launches=(2 if nn else 1) if device else 0)
    return status


def trie_verify_proofs(blob, off, lens, node_idx, proof_first, query_proof, roots, keys, values):
    """pv_trie_verify_proofs over the records node_idx picks out of (blob, off, lens): lens None means record i
    ends at off[i + 1]. proof_first indexes node_idx; roots, keys and values are lists of bytes, one per query."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint64) if lens is not None else np.diff(off)
    idx = np.ascontiguousarray(node_idx, dtype=np.int64)
    node_off = np.concatenate([off[:-1][idx], np.zeros(1, np.uint64)]) if off.size else np.zeros(1, np.uint64)
    kb, ko = _blob(keys)
    vb, vo = _blob(values)
    blob = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob
    return trie_verify_proofs_raw(blob, node_off, lens[idx], proof_first, query_proof,
                                  np.frombuffer(b"".join(roots), np.uint8), kb, ko, vb, vo)
