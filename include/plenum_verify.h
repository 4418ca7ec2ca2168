/*
 * plenum_verify.h — C ABI of the MI355X batch Ed25519 request-verification engine
 * (libplenum_verify.so). Plain pointers and sizes only; no torch/HIP types cross this boundary
 * (streams are passed as void*). All functions return 0 on success and a negative PV_ERR_* code on
 * infrastructure failure; a bad signature is NEVER an error, it is a 0 verdict bit. No exceptions
 * cross the ABI; pv_last_error() describes the last failure of the calling thread.
 *
 * What each entry point replaces in the reference (swcurran/indy-plenum):
 *   pv_verify_batch        the per-signature ctypes call chain
 *                          stp_core/crypto/nacl_wrappers.py:232-242 Verifier.verify
 *                          -> :86-108 VerifyKey.verify(signature + msg)
 *                          -> libnacl.crypto_sign_open(sm, pk) (libnacl 1.6.1, setup.py:107-108)
 *                          -> libsodium 1.0.18 crypto_sign_open, batched: request i is the byte
 *                          string sm[sm_off[i] : sm_off[i+1]] (exactly the `signature + msg`
 *                          concatenation the reference builds, so the sig/msg split point is
 *                          libsodium's: the first 64 bytes) verified against pk[32 i : 32 i + 32].
 *                          verdict bit i (LSB-first within each byte) = 1 iff crypto_sign_open
 *                          would return 0 (libnacl would not raise ValueError).
 *   pv_verify_batch_device the same on device-resident inputs (the hot path the benchmark times).
 *   pv_b58decode_batch     base58.b58decode (PyPI base58, unpinned; setup.py:98-99) as called from
 *                          plenum/server/client_authn.py:97 (signature) and
 *                          plenum/common/verifier.py:27,37,50 (identifier / verkey).
 *   pv_resolve_verkeys     plenum/common/verifier.py:24-50 DidVerifier key resolution (cryptonym,
 *                          abbreviated '~' verkey expansion, full verkey) for a batch.
 *   pv_comm_* / pv_allgather_verdicts
 *                          new: the cross-GPU gather of per-shard verdict bitmaps (one RCCL
 *                          all-gather over xGMI). The reference has no equivalent.
 *   pv_init_devices / pv_verify_batch_multi_gpu
 *                          the same batched crypto_sign_open as pv_verify_batch, sharded over several
 *                          GPUs driven from ONE process (the reference's node is one process with one
 *                          asyncio Looper, stp_core/loop/looper.py:142-213, fed from
 *                          plenum/server/node.py:1518-1527 and stp_zmq/zstack.py:606-646), the
 *                          per-shard verdict bitmaps gathered with one in-process RCCL all-gather.
 * Threading: the reference caller is the single-threaded asyncio Looper (stp_core/loop/looper.py);
 * the library is synchronous per call. It keeps one context per device: pv_init binds the primary
 * device that every single-device call uses; pv_init_devices adds contexts for the multi-GPU call.
 */
#ifndef PLENUM_VERIFY_H
#define PLENUM_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PV_OK 0
#define PV_ERR_NO_DEVICE (-1)
#define PV_ERR_ALLOC (-2)
#define PV_ERR_LAUNCH (-3)
#define PV_ERR_ARG (-4)
#define PV_ERR_NOT_INIT (-5)
#define PV_ERR_COMM (-6)
#define PV_ERR_DECODE (-7)

/* Bytes that must be readable past sm_off[n] in a device blob (SHA-512 reads whole 8-byte words). */
#define PV_BLOB_SLACK 256

/* ABI version of this header. */
#define PV_ABI_VERSION 1
int pv_abi_version(void);
/* Build configuration of the library's kernels (bit set = compiled in):
 *   PV_BUILD_COMB_FUSED  the keyed comb path computes [S]B and [k](-A) in ONE kernel
 *                        (pv_comb_ab_kernel, the MSM stage) for chunks above 262,144 requests instead
 *                        of pv_comb_b_kernel (TABLE stage) + pv_comb_a_kernel (MSM stage); smaller
 *                        chunks keep the two kernels */
#define PV_BUILD_COMB_FUSED 1u
uint32_t pv_build_flags(void);

/* Number of visible GPUs (0 when none; never an error). */
int pv_device_count(void);

/* Bind this process to `device`, build the fixed-base table, allocate the workspace. Idempotent
 * for the same device. */
int pv_init(int device);
void pv_shutdown(void);
const char* pv_last_error(void);

/* Host buffers in, host bitmap out (ceil(n/8) bytes). sm_off has n+1 entries, non-decreasing;
 * offsets need no alignment. Synchronous. Inputs in ordinary (pageable) memory are copied into the
 * library's pinned staging buffer by per-device copy threads; inputs that lie in pinned memory the
 * library allocated or registered (pv_host_alloc / pv_host_register below) are DMA'd from where they
 * are, without that copy (the offsets too when sm_off[0] == 0). Batches whose blob is >= 8 MB are
 * verified in sub-batches of 262,144 requests (the first and the last half-size) whose H2D transfers
 * (on a copy stream) overlap the previous sub-batch's kernels, so a large host batch costs about its
 * PCIe time plus one sub-batch's kernels.
 * A call of <= 2,048 requests that takes the latency path (AUTO's range for host buffers without a
 * key-repeat hint, or PV_PATH_LATENCY) and whose records are all <= 1,840 bytes is zero-copy: the
 * requests go into fixed-stride slots of the pinned staging buffer that the kernel reads over PCIe,
 * and each request's verdict byte is stored back into coherent pinned memory (no copy kernels around
 * the verification); the host returns as soon as every byte is written (a fault of such a call is
 * reported by the next call's synchronisation). With stage timing on or key-cache auto-admission
 * active the host waits on the stream as for any other call. pv_last_zero_copy() returns 1 if the
 * most recent pv_verify_batch took the zero-copy form. */
int pv_verify_batch(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk,
                    uint8_t* verdict_bits);
int pv_last_zero_copy(void);

/* Several GPUs from one process (SURVEY.md §8b pv_init(device_mask) / pv_verify_batch_multi_gpu).
 *   pv_init_devices(mask)       bit d set = use device d (d < 16); builds each missing device context
 *                               (tables, workspace, streams; in parallel) and one RCCL communicator per
 *                               device with ncclCommInitAll. A primary bound by pv_init may be in the
 *                               mask: its context is shared. Calling it again with another mask
 *                               rebuilds the communicators only.
 *   pv_verify_batch_multi_gpu   pv_verify_batch's contract (host buffers, synchronous, same verdict
 *                               bits), sharded over those devices: shard r = requests
 *                               [bounds[r], bounds[r+1]) of pv_shard_plan (contiguous, whole 64-request
 *                               verdict words), staged and verified on device r's own stream by one host
 *                               worker per device; the per-shard verdict words are gathered with ONE
 *                               ncclAllGather over the clique (group call) and copied back from the first
 *                               device. No other cross-GPU traffic.
 *   pv_multi_gpu_devices        the devices in use (up to max), returns their count (0 = none).
 *   pv_multi_gpu_comm_ranks     what RCCL itself reports for the clique: ncclCommCount of the first
 *                               device's communicator, and ncclCommUserRank of each device's (up to max).
 *   pv_shard_plan               host-only: the shard bounds (ndev + 1 entries) and the verdict words
 *                               per shard (the all-gather's count) for n requests over ndev devices. */
int pv_init_devices(uint32_t device_mask);
int pv_verify_batch_multi_gpu(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk,
                              uint8_t* verdict_bits);
int pv_multi_gpu_devices(int* devices, int max_devices);
int pv_multi_gpu_comm_ranks(int* nranks, int* ranks, int max_devices);
int pv_shard_plan(uint64_t n, int ndev, uint64_t* bounds, uint64_t* words_per_shard);

/* Library-owned pinned host memory: the host-fed path's input arena. A node that receives its
 * requests straight into such buffers (the signature + message blob, the offsets, the keys) lets
 * pv_verify_batch / pv_verify_batch_multi_gpu DMA them to HBM without a pageable -> pinned copy. The
 * blocks are portable (every device of the process can DMA from them). Any range inside a block is
 * recognised per call.
 *   pv_host_alloc(p, bytes)      allocate a pinned block (*p = its address)
 *   pv_host_free(p)              release a pv_host_alloc block (PV_ERR_ARG for any other pointer);
 *                                it stays pinned in a cache (4 GB, PV_PINNED_CACHE_MB) for the next
 *                                pv_host_alloc of a similar size, returned to the system at pv_shutdown
 *   pv_host_register(p, bytes)   pin an existing host range in place (hipHostRegister; ~50 ms per GB,
 *                                for long-lived receive buffers)
 *   pv_host_unregister(p)        undo pv_host_register (p = the registered start); a registered
 *                                range must be unregistered before its memory is freed, or the
 *                                library keeps treating that address range as pinned
 *   pv_host_is_pinned(p, bytes)  1 if [p, p + bytes) lies inside one such block or range */
int pv_host_alloc(void** p, uint64_t bytes);
int pv_host_free(void* p);
int pv_host_register(void* p, uint64_t bytes);
int pv_host_unregister(void* p);
int pv_host_is_pinned(const void* p, uint64_t bytes);

/* Device buffers in, device bitmap out. Requirements: d_sm 4-byte aligned and readable up to
 * sm_off[n] + PV_BLOB_SLACK (records themselves need no alignment), d_pk 16-byte aligned,
 * verdict_words holds ceil(n/64) 64-bit words. Enqueued on `stream` (a hipStream_t, NULL = the
 * library stream); returns without synchronising. Thread-safe: calls are serialised on a library
 * mutex, and a call on a different stream than the previous call first makes its stream wait for
 * the previous launch (the workspace is shared), so concurrent callers get correct verdicts. */
int pv_verify_batch_device(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk,
                           uint64_t* d_verdict_words, void* stream);

/* pv_set_timing(1) (re)starts timing: from then on every launch records HIP events on its own
 * stream at each stage boundary. pv_stage_times returns the device time (ms) of each stage summed
 * over all launches since then, in this order (PV_STAGE_*):
 *   KEYS    per-batch key deduplication and per-key expansion (keyed comb path only)
 *   PREP    per-request checks, SHA-512, reduction mod L, recoding (Straus path: also A's
 *           decompression and the half-size split of k, pv_split_kernel)
 *   TABLE   per-request [j](+-A) and [j](-R') multiples with R's decompression, and [k2 S]B from the
 *           wide fixed-base comb (Straus path) / comb path: [S]B from the fixed-base comb while the
 *           per-key comb tables are built on a second stream, then the join
 *   MSM     the double-scalar multiplication to projective coordinates (Straus path: ~33 windows of
 *           both half-size scalars; comb path: the [k](-A) half, 32 table additions)
 *   ENCODE  batched inversion, canonical encoding, compare with R, verdict bits
 * and the number of launches (chunks). pv_kernel_times is the coarse three-way view
 * (KEYS+PREP, TABLE, MSM+ENCODE). pv_set_timing(0) stops recording. */
#define PV_STAGE_KEYS 0
#define PV_STAGE_PREP 1
#define PV_STAGE_TABLE 2
#define PV_STAGE_MSM 3
#define PV_STAGE_ENCODE 4
#define PV_NSTAGES 5
/* Arithmetic path for subsequent launches. Every path gives bit-identical verdicts:
 *   PV_PATH_STRAUS  per request: decompress A and R (R must decode to R' with encode(R') == R, else
 *                   reject), split k = k1 / k2 (mod 8L) with |k1|, k2 < ~2^128 and k2 odd (extended
 *                   Euclid in Lehmer blocks), 9-entry tables of [j](+-A) and [j](-R'), [k2 S mod L]B
 *                   from the wide fixed-base comb (11 radix-2^24 lookups: the top entry converted +
 *                   10 niels additions), then a regular-window loop over both scalars: ~33 x (4
 *                   doublings + 2 cached additions), + [k2 S]B + R', and encode(.) == R: equal iff
 *                   [k2](SB - kA - R') = 0 iff libsodium's encode(SB - kA) == R (any A, R of the
 *                   curve: 8L kills every point, k2 is odd and below L). A lane whose split is not
 *                   settled takes (k, 1) and the full-length loop, same verdict
 *   PV_PATH_COMB    per batch: deduplicate keys; per DISTINCT key: libsodium's key checks,
 *                   decompression and a radix-256 comb table T_A[i][d] = [d 256^i](-A) (32 x 129
 *                   entries); per request: [S]B as above (10 niels additions) and [k](-A) as 32
 *                   cached table additions, no doublings (keys beyond the PV_KEY_CAP = 16,384 tables
 *                   a chunk holds take the Straus path in the same launch)
 *   PV_PATH_LATENCY per request: one workgroup with limb-parallel arithmetic, every field element
 *                   spread over 10 lanes of a 16-lane row; decompression of A and R in one chain,
 *                   the same half-size split as the Straus path, [k1](+-A) and [k2](-R') (~33 x 4
 *                   doublings + ~33 additions each) on two waves at once -- batches of <= 512
 *                   requests (PV_LAT4_MAX): four waves, each scalar cut again at 2^68 (~17 windows per wave) --
 *                   [k2 S]B from the radix-65536 fixed-base comb, and the comparison with R' without
 *                   an inversion. A key in the node-side key cache keeps the full k: [k](-A) as 32
 *                   table additions, no doublings. One kernel launch; the fastest path for small
 *                   batches (Plenum's 100 / 1,000-message quotas). In the comb kernels a cached key's
 *                   additions read the cache's affine rows (entries divided by Z: no Z1 Z2 product)
 *   PV_PATH_AUTO    (default) batches of <= 2,048 requests take the latency path. From 2,049 to
 *                   4,096 requests AUTO picks by key repeats: the keyed path with >= 3 requests per
 *                   key (and <= 2,048 keys), else the latency path; pv_verify_batch counts the keys
 *                   on the host, pv_verify_batch_device lets its dedup kernels count them and choose
 *                   on the device (the other path's kernels exit at once; no host round trip). A
 *                   non-empty key cache keeps such batches on the latency path. Larger batches, per
 *                   chunk: deduplicate keys, give a comb table to every key with >= 48 requests in
 *                   the chunk (a table costs about what ~50 requests save) -- to every key when the
 *                   chunk has <= 2,048 keys and <= 256k requests -- and verify the other requests on
 *                   the Straus path in the same launch; a tail chunk of <= 4,096 requests goes
 *                   Straus unless the key cache holds keys (then keyed). Split on the device, so
 *                   pv_verify_batch_device stays asynchronous.
 * Every path returns bit-identical verdicts. */
#define PV_PATH_AUTO 0
#define PV_PATH_STRAUS 1
#define PV_PATH_COMB 2
#define PV_PATH_LATENCY 3
int pv_set_path(int mode);
/* The path the most recent chunk took (PV_PATH_COMB if any of its requests used a comb table, else
 * PV_PATH_STRAUS) and its distinct-key count (0 when no key kernels ran). Synchronises the device. */
int pv_last_path(int* path, uint32_t* nkeys);
/* The split of the most recent chunk, as read by the last pv_last_path call: distinct keys, keys
 * given a comb table, requests verified with those tables (the rest took the Straus path). */
int pv_last_split(uint32_t* keys, uint32_t* comb_keys, uint32_t* comb_requests);
int pv_set_timing(int enable);
int pv_stage_times(double* ms, int max_stages, int* launches);
int pv_kernel_times(double* prep_ms, double* table_ms, double* msm_ms, int* launches);

/* Node-side key cache (persistent across calls). A node verifies requests from a fairly stable set
 * of signers whose verkeys it already holds (the domain ledger's NYM records,
 * plenum/server/request_handlers/utils.py:30-39). For a cached key the latency path computes [k](-A)
 * with 32 additions from the key's radix-256 comb table (660 KB of HBM per key, built once by the
 * engine's key-chain and fill kernels) instead of ~132 doublings + ~66 additions; verdicts are
 * unchanged (the table holds exact multiples of -A, and libsodium's key checks ran when it was built).
 * Above the latency path's range (AUTO: batches > 4,096 requests) a non-empty cache also makes every
 * chunk keyed, the tail chunk of a multi-chunk batch included: a cached key's requests take the comb
 * path at any request count and its table is read from the cache instead of being built (no key
 * chain / table fill for it); uncached keys are handled as without the cache. A put that fails part
 * way (an error from a build step) leaves only keys whose tables were built: every slot the call
 * assigned is dropped. The benchmark's headline never configures it.
 *   pv_key_cache_configure(capacity)  allocate room for `capacity` keys (0 = free, disabled)
 *   pv_key_cache_put(pks, n)          host keys (n x 32 B): build and insert the missing ones, refresh
 *                                     the present ones; when full, the least recently USED keys are
 *                                     evicted (every launch stamps the cache slots it reads; the stamps
 *                                     are folded into the LRU order before a put evicts). Synchronous: a
 *                                     batch of keys is built in parallel, ~0.1 ms of GPU time per key with
 *                                     the affine and radix-65536 rows (1,024 keys in 0.10-0.12 s)
 *   pv_key_cache_clear()              drop every key (capacity kept)
 *   pv_key_cache_enable(on)           whether launches consult the cache (default on)
 *   pv_key_cache_stats(size, cap)     keys held / capacity
 *   pv_key_cache_contains(pk)         1 if the 32-byte key is cached
 *   pv_key_cache_auto(min_seen)       automatic admission (0 = off, the default): once a
 *                                     pv_verify_batch call's verdicts are back, the keys of its requests
 *                                     that VERIFIED are counted (every request of calls of <= 4,096
 *                                     requests, a sample of 4,096 of larger ones: one request per block of
 *                                     ceil(n / 4,096)); a request with a failing signature never counts,
 *                                     so senders without valid signatures cannot make the node build
 *                                     tables or evict its signers (plenum/server/client_authn.py:84-118:
 *                                     every signature is untrusted input). A key verified min_seen times
 *                                     within the counting window (the last ~32k distinct keys) is put
 *                                     into the cache behind that batch on the engine stream: the call
 *                                     returns with its verdicts, the build (~0.1 ms of GPU time per key)
 *                                     overlaps the caller's next steps and the next launch is ordered
 *                                     after it. The count table is keyed by a per-process random secret
 *                                     with bounded probing (csrc/kc_admit.h); an evicted key, or one whose
 *                                     admission failed, counts from zero again and is re-admitted on its
 *                                     next min_seen verified appearances. A failed admission leaves the
 *                                     verdicts unchanged and the keys uncached. Verkeys come from NYM
 *                                     records (plenum/server/request_handlers/utils.py:30-39): signers repeat
 *   pv_key_cache_auto_stats(a, f)     keys admitted automatically / admissions that failed */
int pv_key_cache_configure(uint32_t capacity);
int pv_key_cache_put(const uint8_t* pks, uint64_t n);
int pv_key_cache_clear(void);
int pv_key_cache_enable(int enable);
int pv_key_cache_stats(uint32_t* size, uint32_t* capacity);
int pv_key_cache_contains(const uint8_t* pk);
int pv_key_cache_auto(uint32_t min_seen);
int pv_key_cache_auto_stats(uint64_t* admitted, uint64_t* failed);

/* Table reuse (on by default). The per-key comb tables a keyed chunk of more than 65,536 requests
 * builds stay where they were built, in the workspace, and are listed in a device-side directory; a
 * later chunk -- of the same call or of any later one -- that carries one of those keys reads its table
 * instead of building it again. It costs no memory beyond the workspace (the table area holds 16,384
 * tables whether they are kept or not), needs no put and no admission: a key's table is kept because a
 * chunk needed it. A hit changes only where a table is read from: which keys get a table, which path a
 * chunk takes and every verdict are what they are without it (the libsodium key checks ran when the
 * table was built, and their result is kept with it). The node-side key cache takes precedence for the
 * keys it holds. A chunk whose new tables do not fit below `capacity` empties the directory and builds
 * all its tables, as every chunk does with reuse off. Chunks of at most 65,536 requests read listed
 * tables and build the others in the scratch slots above the capacity; they list nothing.
 *   pv_table_reuse(on, capacity)   on: 0 = every chunk builds its own tables. capacity: tables the
 *                                  directory may list, clamped to [1, 16,384]; 0 keeps the current value
 *                                  (default 14,336 = 16,384 less the 2,048 comb keys a chunk that lists
 *                                  nothing can have). Turning reuse off or changing the capacity empties
 *                                  the directory. Applies to every device of the process.
 *   pv_table_reuse_stats(h, b, r)  tables read from the directory / built by chunks that went through
 *                                  it / times a chunk emptied it, since pv_init. Synchronises the
 *                                  device: for tests and tools.
 * PV_TABLE_REUSE=0 in the environment at pv_init starts with reuse off. */
int pv_table_reuse(int on, uint32_t capacity);
int pv_table_reuse_stats(uint64_t* hits, uint64_t* built, uint64_t* resets);

/* Affine rows for resident tables (on by default; it needs table reuse). A chunk of more than 65,536
 * requests that reads a listed table whose key passed libsodium's key checks, when such a chunk has read
 * it once before (the table's second hit), converts that table, after its own kernels have read it, to
 * affine rows in place: every entry divided by its Z with one inversion per 33 entries. Every later
 * chunk, of any size, then adds from it with 7 field multiplications and 128 bytes per addition instead
 * of 8 and 160. Verdicts do not change. A table that large chunks do not come back for twice is never
 * converted (converting 1,024 tables costs what ten warm 1M-request chunks save); at most 1,024 tables are converted behind one chunk, the rest on their next hit; a
 * table that is rebuilt (a reset, a control call, a key-cache put over the directory) starts in cached
 * form again.
 *   pv_table_affine(on)              0 = resident tables stay as built. Switching empties the directory.
 *                                    Applies to every device of the process.
 *   pv_table_affine_stats(c, r)      tables converted / tables read in affine form by chunks that went
 *                                    through the directory, since pv_init. Synchronises the device: for
 *                                    tests and tools.
 * PV_TABLE_AFFINE=0 in the environment at pv_init starts with it off. */
int pv_table_affine(int on);
int pv_table_affine_stats(uint64_t* converted, uint64_t* affine_reads);

/* Wide rows for resident tables (on by default; it needs table reuse and affine rows). A chunk of more
 * than 65,536 requests that reads a listed table in affine form (the table's third hit by such a chunk)
 * builds, after its own kernels, radix-2^11 affine niels rows of that key in a pool of its own: 23 rows of
 * 1,025 entries, 3.0 MB per key, beside the radix-256 table, which stays. Every later keyed chunk that
 * hits the table, of any size, computes [k](-A) as 23 additions from those rows instead of 32. Verdicts
 * do not change. At most 1,024 tables are widened behind one chunk and only while the pool has room; the
 * rest stay in affine form. The pool is allocated by the first chunk that can widen a table; when that
 * allocation fails the feature turns itself off and pv_last_error() says so. The pool empties whenever the
 * directory does.
 *   pv_table_wide(capacity)          tables the pool holds; 0 = off (default 2,048 = 6.2 GB). A change
 *                                    empties the directory. Applies to every device of the process.
 *   pv_table_wide_stats(w, r)        tables widened / tables read from wide rows, since pv_init; the
 *                                    latter are counted in pv_table_affine_stats's affine reads as well
 *                                    (they are affine rows of the same table). Synchronises the device:
 *                                    for tests and tools.
 * PV_TABLE_WIDE=0 in the environment at pv_init starts with it off. */
int pv_table_wide(uint32_t capacity);
int pv_table_wide_stats(uint64_t* widened, uint64_t* wide_reads);

/* Batched base58 decode (Bitcoin alphabet, PyPI base58 2.x b58decode semantics: trailing ASCII
 * whitespace stripped, each leading '1' -> 0x00). Input: strings concatenated in `chars` with
 * n+1 offsets. Output: out[i * out_stride ...], out_len[i] bytes, status[i] = 0 ok, 1 invalid
 * character, 2 longer than out_stride. */
int pv_b58decode_batch(const char* chars, const uint64_t* off, uint64_t n, uint8_t* out,
                       uint64_t out_stride, uint32_t* out_len, uint8_t* status);

/* base58.b58encode of data[0..len): writes min(cap, result) chars, returns the full encoded length. */
int64_t pv_b58encode(const uint8_t* data, uint64_t len, char* out, uint64_t cap);

/* Batched DidVerifier key resolution (plenum/common/verifier.py:24-50) for n (identifier, verkey)
 * string pairs (concatenated + offsets; an empty identifier means None, has_verkey[i] = 0 means
 * verkey None). pk_out receives 32-byte raw keys. status[i]:
 *   0 ok, raw 32-byte key in pk_out
 *   1 ValueError("'verkey' should be a non-empty string")
 *   2 InvalidKey (key resolution failed: bad base58, wrong length, bad hex)
 *   3 empty key: the stp_core Verifier has no key and verify() returns False
 *   4 identifier is not valid base58 (b58decode raises ValueError in DidVerifier.__init__)
 * has_verkey/pk_out/status are per request. */
int pv_resolve_verkeys(const char* idr_chars, const uint64_t* idr_off, const char* vk_chars,
                       const uint64_t* vk_off, const uint8_t* has_verkey, uint64_t n, uint8_t* pk_out,
                       uint8_t* status);

/* Device ingress front end: everything between the received strings and
 * crypto_sign_open, for a whole batch, on the GPU, then the verification itself. Replaces per
 * signature: plenum/server/client_authn.py:97 b58decode(sig), plenum/common/verifier.py:24-51
 * DidVerifier(verkey, identifier) key resolution, stp_core/crypto/nacl_wrappers.py:108
 * `signature + msg`. Inputs (device pointers, offsets relative to their blob):
 *   n verifications: sig_chars/sig_off  base58 signature strings (after str.rstrip(); non-ASCII
 *                                       bytes are invalid characters)
 *                    msg_idx[n]         message M of verification i (signing-serialized request)
 *                    signer_idx[n]      signer of verification i
 *   n_msgs messages: msg/msg_off        (readable for 8 bytes past msg_off[n_msgs];
 *                                       msg_bytes_total = sum over i of len(M[msg_idx[i]]), it
 *                                       sizes the assembly buffer; an understatement empties
 *                                       every record and reports status 3, never a fault)
 *   n_signers:       idr_chars/idr_off  identifier strings ("" = None), vk_chars/vk_off verkey
 *                                       strings as getVerkey returned them, vk_present[u] = 0 when
 *                                       the verkey is None
 * Outputs: verdict bit i (as pv_verify_batch: crypto_sign_open(b58decode(sig) || M, key) == 0) and
 * status[i]:
 *   0       verified (the verdict bit is the result)
 *   1       the signature is not base58 (InvalidSignatureFormat)
 *   2       the signature decodes to more than 96 bytes (not assembled; verdict 0)
 *   3       msg_idx / signer_idx out of range, or msg_bytes_total too small (verdict 0)
 *   16 + k  signer key resolution status k (pv_resolve_verkeys codes; k = 3: no key, verify() is
 *           False) — the verdict bit is 0
 * Enqueued on `stream` (NULL = the library stream); the workspace is the library's and is handed
 * over between streams as for pv_verify_batch_device, so calls on different streams and threads are
 * safe. pv_ingress_verify is the same on host buffers (synchronous; validates
 * offsets and indices and returns PV_ERR_ARG instead of launching on bad input).
 * pv_ingress_front_ms: device time of the most recent call's front end (decode, resolve, scan,
 * assembly), excluding the verification kernels. */
int pv_ingress_verify_device(const char* d_sig_chars, const uint64_t* d_sig_off, const uint32_t* d_msg_idx,
                             const uint32_t* d_signer_idx, uint64_t n, const uint8_t* d_msg, const uint64_t* d_msg_off,
                             uint64_t n_msgs, uint64_t msg_bytes_total, const char* d_idr_chars,
                             const uint64_t* d_idr_off, const char* d_vk_chars, const uint64_t* d_vk_off,
                             const uint8_t* d_vk_present, uint64_t n_signers, uint8_t* d_status,
                             uint64_t* d_verdict_words, void* stream);
int pv_ingress_verify(const char* sig_chars, const uint64_t* sig_off, const uint32_t* msg_idx,
                      const uint32_t* signer_idx, uint64_t n, const uint8_t* msg, const uint64_t* msg_off,
                      uint64_t n_msgs, const char* idr_chars, const uint64_t* idr_off, const char* vk_chars,
                      const uint64_t* vk_off, const uint8_t* vk_present, uint64_t n_signers, uint8_t* status,
                      uint8_t* verdict_bits);
int pv_ingress_front_ms(double* ms);

/* Batch Ed25519 signing, byte-identical to libsodium 1.0.18. Replaces the reference's per-call chain
 * stp_core/crypto/nacl_wrappers.py:141 SigningKey.__init__ -> libnacl.crypto_sign_seed_keypair and
 * :170 SigningKey.sign -> libnacl.crypto_sign -> libsodium, for a whole batch in one call. A 64-byte
 * secret key is libsodium's: seed || public key, and the public-key half is hashed AS GIVEN.
 * NOT hardened against timing or memory-access side channels (table lookups are indexed by secret
 * digits): for load generation, fixtures and test wallets, not for custody of production keys. The
 * library overwrites its own copies of seeds and derived secrets before a host-entry call returns.
 * Batches are signed in chunks of 262,144 messages inside the library.
 *   pv_sign_seed_keypairs  crypto_sign_seed_keypair for n seeds (n x 32): pk_out n x 32, sk_out n x 64
 *                          (seed || pk); either may be NULL. Synchronous, host buffers.
 *   pv_sign_batch          crypto_sign_detached: message i = msg[msg_off[i] : msg_off[i+1]] signed with
 *                          sk[64 * signer_idx[i]]; signer_idx NULL means signer i (then n_signers == n).
 *                          sig_out n x 64. Synchronous, host buffers. Validates its arguments
 *                          (non-decreasing offsets, indices < n_signers, n_signers > 0 when n > 0) and
 *                          returns PV_ERR_ARG instead of launching on bad input.
 *   pv_sign_batch_device   the same on device buffers, enqueued on `stream` (NULL = the library stream),
 *                          no synchronise. d_msg readable to msg_off[n] + PV_BLOB_SLACK, d_sk and
 *                          d_sig_out 16-byte aligned. An out-of-range signer index gives an all-zero
 *                          signature, never a fault (the convention of ingress status 3). The workspace
 *                          is handed over between streams as for pv_verify_batch_device.
 * n = 0 returns PV_OK and launches nothing; without pv_init every entry returns PV_ERR_NOT_INIT. */
int pv_sign_seed_keypairs(const uint8_t* seeds, uint64_t n, uint8_t* pk_out, uint8_t* sk_out);
int pv_sign_batch(const uint8_t* msg, const uint64_t* msg_off, uint64_t n, const uint8_t* sk,
                  uint64_t n_signers, const uint32_t* signer_idx, uint8_t* sig_out);
int pv_sign_batch_device(const uint8_t* d_msg, const uint64_t* d_msg_off, uint64_t n, const uint8_t* d_sk,
                         uint64_t n_signers, const uint32_t* d_signer_idx, uint8_t* d_sig_out, void* stream);

/* Signing serialization of received JSON requests on the host, many threads:
 * request i is the JSON text json[off[i] : off[i+1]] that ZStack.deserializeMsg decodes
 * (stp_zmq/zstack.py:881-885); the output is the signing-serialized message
 * (common/serializers/signing_serializer.py:35-92, serialization.py:27-36) of
 *   PV_SER_DICT     json.loads(text)
 *   PV_SER_AUTHN    json.loads(text) minus top-level {signature, signatures, fees}
 *                   (CoreAuthMixin.authenticate, plenum/server/client_authn.py:198,232)
 *   PV_SER_REQUEST  Request(**json.loads(text)).as_dict minus those keys (Node.verifySignature,
 *                   plenum/server/node.py:2636-2650), and digest[32 i .. 32 i + 32) =
 *                   sha256(serialize(signingState())) (plenum/common/request.py:86-121)
 * written to msg_out[msg_off[i] : msg_off[i+1]]. plugin_fields: NUL-separated names ending with an
 * empty name (PLUGIN_CLIENT_REQUEST_FIELDS, request.py:37-39), or NULL. status[i]:
 *   PV_SER_OK          serialized
 *   PV_SER_INVALID     json.loads would raise (bad UTF-8, bad JSON, control characters...)
 *   PV_SER_NOT_OBJECT  the document is not a JSON object
 *   PV_SER_DEFER       valid, but outside what is reproduced bit-for-bit here (floats, NaN/Infinity,
 *                      lone surrogates, nesting > 512, ints > 4,300 digits, a request-mode digest
 *                      whose Python evaluation raises): the caller serializes it in Python
 * Returns PV_ERR_ARG with msg_off[n] = the bytes needed when msg_cap is too small. */
#define PV_SER_DICT 0
#define PV_SER_AUTHN 1
#define PV_SER_REQUEST 2
#define PV_SER_OK 0
#define PV_SER_INVALID 1
#define PV_SER_NOT_OBJECT 2
#define PV_SER_DEFER 3
int pv_signing_serialize_json(const char* json, const uint64_t* off, uint64_t n, int mode, const char* plugin_fields,
                              int threads, uint8_t* msg_out, uint64_t msg_cap, uint64_t* msg_off, uint8_t* digest,
                              uint8_t* status);

/* Fused ingress planning (replaces the per-request Python planning of the wire
 * path: json.loads -> Request(**msg).as_dict -> CoreAuthMixin._select_signatures,
 * plenum/server/client_authn.py:240-264, node.py:1643,2636-2650). ONE parse of every received
 * request gives what pv_signing_serialize_json(PV_SER_REQUEST) gives (msg, msg_off, digest, status)
 * and its signature plan:
 *   kind[i]  PV_PLAN_SINGLE  {identifier: signature}: both non-empty strings (the first branch of
 *                            _select_signatures)
 *            PV_PLAN_MULTI   the `signatures` object (non-empty, string values, no duplicate
 *                            names) of a request without a usable identifier/signature pair and
 *                            without a `signature` value (so the verified-request cache stores None)
 *            PV_PLAN_PY      anything else: the caller runs the reference's Python path for it
 *                            (serialization status not OK, not an object, a `self` key, plugin
 *                            fields registered, operation not an object or its type not a string,
 *                            non-ASCII or escaped identifier/signature text, trailing whitespace, ...)
 *   type_id[i]      operation["type"] of a SINGLE/MULTI request, as an index into the distinct type
 *                   strings types[type_off[t] : type_off[t+1]] (first-appearance order)
 *   pair_off[i]     request i's (identifier, signature) pairs are [pair_off[i], pair_off[i+1])
 *                   (dict order); pair_name[p] indexes the distinct identifier strings
 *                   names[name_off[k] : name_off[k+1]]; sigs[sig_off[p] : sig_off[p+1]] is the
 *                   signature text (ASCII)
 * Capacities: msg_cap as pv_signing_serialize_json; sigs_cap, names_cap and types_cap are byte
 * capacities and off[n] always suffices (every string is a substring of its request); pair_cap =
 * off[n] / 6 + 1 always suffices (a pair takes at least 6 bytes of JSON). name_off holds
 * pair_cap + 1 entries (distinct names <= pairs), type_off n + 1 (distinct types <= requests).
 * Returns PV_ERR_ARG with msg_off[n] = bytes needed when msg_cap is too small. */
#define PV_PLAN_PY 0
#define PV_PLAN_SINGLE 1
#define PV_PLAN_MULTI 2
typedef struct {
    uint8_t* msg_out; /* in: buffers */
    uint64_t msg_cap;
    uint64_t* msg_off;  /* [n + 1] */
    uint8_t* digest;    /* [32 n] */
    uint8_t* status;    /* [n] PV_SER_* */
    uint8_t* kind;      /* [n] PV_PLAN_* */
    uint32_t* type_id;  /* [n] */
    uint64_t* pair_off; /* [n + 1] */
    uint32_t* pair_name; /* [pair_cap] */
    uint64_t* sig_off;   /* [pair_cap + 1] */
    uint64_t pair_cap;
    char* sigs;
    uint64_t sigs_cap;
    char* names;
    uint64_t* name_off; /* [pair_cap + 1] */
    uint64_t names_cap;
    char* types;
    uint64_t* type_off; /* [n + 1] */
    uint64_t types_cap;
    char* keys_hex;   /* [65 n] or NULL: Request.digest of request i as 64 lowercase hex digits + '\n' */
    char* sig_lines;  /* [sigs_cap + pair_cap] or NULL: every signature text followed by '\n' */
    uint64_t n_pairs; /* out */
    uint64_t n_names; /* out */
    uint64_t n_types; /* out */
} PvWirePlan;
int pv_wire_plan(const char* json, const uint64_t* off, uint64_t n, const char* plugin_fields, int threads,
                 PvWirePlan* plan);

/* Multi-GPU: one process per GPU. pv_comm_unique_id on rank 0, broadcast the 128 bytes by any
 * channel, pv_comm_init on every rank (after pv_init). pv_allgather_verdicts gathers
 * words_per_rank 64-bit verdict words from every rank into d_all (nranks * words_per_rank) with
 * one RCCL all-gather on `stream`. pv_comm_count reports what RCCL itself sees for this rank's
 * communicator (ncclCommCount / ncclCommUserRank), so a multi-GPU run can show the ranks RCCL joined
 * (plenum/server/node.py:1518-1527 is the batch feed these shards come from). */
int pv_comm_unique_id(uint8_t out[128]);
int pv_comm_init(int nranks, int rank, const uint8_t id[128]);
int pv_allgather_verdicts(const uint64_t* d_local, uint64_t words_per_rank, uint64_t* d_all, void* stream);
int pv_comm_count(int* nranks, int* rank);
void pv_comm_destroy(void);

/* Device memory helpers so hosts without a GPU framework can stage data (bench, smoke).
 * pv_memcpy_h2d / pv_memcpy_d2h are ordered after every launch enqueued before them (on any stream:
 * the copy runs on the library stream after the last launch's completion event) and return once the
 * copy is done. So pv_verify_batch_device(..., NULL) followed by pv_memcpy_d2h of its verdict words
 * needs no pv_sync, and pv_memcpy_h2d right after a launch never overwrites inputs that launch still
 * reads. pv_sync waits for all work on the calling thread's current device. */
int pv_dev_alloc(void** p, uint64_t bytes);
int pv_dev_free(void* p);
int pv_memcpy_h2d(void* dst, const void* src, uint64_t bytes);
int pv_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
int pv_sync(void);
/* Caller streams for the *_device entry points, for hosts without a GPU framework. A stream handed
 * to pv_verify_batch_device / pv_ingress_verify_device may be any stream of this device: batches
 * enqueued on DIFFERENT streams are ordered by the library (each launch waits for the previous one
 * to release the shared workspace), so they never race; pv_stream_destroy synchronises first. */
int pv_stream_create(void** stream);
int pv_stream_destroy(void* stream);
int pv_stream_sync(void* stream);

/* The ledger's SHA-256 Merkle tree (RFC 6962 hashing as ledger/tree_hasher.py:16-28), batched. A tree
 * is its size and its frontier (CompactMerkleTree.tree_size / .hashes, ledger/compact_merkle_tree.py:
 * 73-79): one 32-byte hash per set bit of the size, the largest subtree first. Frontier hashes are
 * opaque, so any size with popcount(size) hashes is a valid starting tree. Everything is byte-identical
 * with the reference; a bad proof is never an error, it is a 0 verdict bit with a status.
 *
 *   pv_merkle_plan          host-only arithmetic (like pv_shard_plan) for n leaves appended to a tree of
 *                           tree_size leaves: the node hashes the appends write to the hash store
 *                           (ledger/compact_merkle_tree.py:131-136), popcount(tree_size + n) (the new
 *                           frontier's length) and the sum of popcount(tree_size + i), i < n (the hashes
 *                           of all audit paths). NULL out-pointers are skipped.
 *   pv_merkle_append_batch  n sequential CompactMerkleTree.append calls (ledger/compact_merkle_tree.py:
 *                           155-160 over _push_subtree :95-153), as plenum/common/ledger.py:75-100
 *                           commitTxns and :129-143 treeWithAppliedTxns make them one transaction at a
 *                           time; leaf i is data[off[i] : off[i+1]]. Host buffers, synchronous. Outputs
 *                           (PvMerkleOut, every pointer may be NULL, which skips that output and its work):
 *                             leaf_hash  the writeLeaf values, in order
 *                             node_hash  the writeNode hashes, in hash-store order
 *                             frontier   tree.hashes after the batch (popcount(tree_size + n) entries of
 *                                        a 64-entry buffer, the rest zero), root = tree.root_hash
 *                             roots      tree.root_hash after each leaf (:81-88)
 *                             path       what append returned for each leaf (the frontier before it,
 *                                        smallest subtree first), leaf i's hashes at [path_off[i],
 *                                        path_off[i+1]) in 32-byte units; path and path_off go together
 *                           n = 0 returns the input tree's frontier and root (the empty tree's root is
 *                           SHA-256 of the empty string). Runs on the GPU, or in C++ on the host
 *                           (pv_merkle_path) when no device is initialised or the batch is small, so it
 *                           works without a GPU and never returns PV_ERR_NOT_INIT.
 *   pv_merkle_append_batch_device
 *                           the same on device buffers, enqueued on `stream` (NULL: the library's)
 *                           without synchronising. Needs pv_init. d_frontier and every output pointer
 *                           16-byte aligned; d_data readable to d_off[n] + PV_BLOB_SLACK, and from the
 *                           4-byte boundary at or below d_data + d_off[0] (records are read as aligned
 *                           32-bit words, so up to 3 bytes before the first record are touched; their
 *                           values do not matter). n = 0 fills frontier, root and path_off[0] only.
 *   pv_merkle_verify_inclusion_batch
 *                           MerkleVerifier.verify_leaf_inclusion / verify_leaf_hash_inclusion
 *                           (ledger/merkle_verifier.py:195-266 over :155-181) for n proofs: give either
 *                           data and off (leaf i = data[off[i] : off[i+1]]) or leaf_hash[32 n]. Proof i is
 *                           proof[32 proof_off[i] : 32 proof_off[i+1]], checked against root[32 i] for a
 *                           tree of tree_size[i] leaves at leaf_index[i]. Verdict bit i (LSB-first) = 1 iff
 *                           the reference returns True. status[i]: 0 compared, 1 tree_size <= leaf_index
 *                           (the reference's ValueError), 2 proof too short, 3 proof too long.
 *   pv_merkle_verify_inclusion_batch_device
 *                           the same on device buffers (16-byte aligned hash arrays); verdicts as
 *                           ceil(n / 64) 64-bit words like pv_verify_batch_device.
 *   pv_merkle_verify_consistency_batch
 *                           MerkleVerifier.verify_tree_consistency (ledger/merkle_verifier.py:23-153) for n
 *                           proofs: proof i is proof[32 proof_off[i] : 32 proof_off[i+1]], for the trees of
 *                           old_size[i] and new_size[i] leaves with roots old_root[32 i] and new_root[32 i].
 *                           Host buffers, synchronous, GPU or C++ host path (pv_merkle_path; AUTO from
 *                           PV_MERKLE_AUTO_MIN_CONSISTENCY proofs); works without a device. Verdict bit i
 *                           (LSB-first) = 1 iff the reference returns True. status[i]:
 *                             0 consistent; equal sizes with equal roots and old_size 0 ignore the proof
 *                             1 old_size > new_size (the reference's ValueError)
 *                             2 proof too short: a hash the walk needs is missing (ProofError); hashes
 *                               left over are accepted
 *                             3 the second (new) root differs (ProofError); also a wrong old root when
 *                               old_size is a power of two, as the new chain starts from it
 *                             4 the new root matches, the first (old) one differs (ConsistencyError)
 *                             5 equal sizes, different roots (ConsistencyError)
 *   pv_merkle_verify_consistency_batch_device
 *                           the same on device buffers (16-byte aligned hash arrays), enqueued on `stream`
 *                           without synchronising, no workspace; verdicts as ceil(n / 64) 64-bit words.
 *   pv_merkle_catchup_batch what plenum/server/catchup/catchup_rep_service.py:375-426
 *                           (_has_valid_catchup_replies) does per CatchupRep, for a whole chain of replies:
 *                           pv_merkle_append_batch's arguments (the ledger's tree and the n leaves of all
 *                           replies) and outputs (every PvMerkleOut pointer, or `out` itself, may be NULL;
 *                           what is asked for is filled exactly as pv_merkle_append_batch fills it, so one
 *                           pass over the leaves also yields what a commit needs), plus the replies: reply r
 *                           is leaves [reply_end[r-1], reply_end[r]) in absolute sizes, reply_end[-1] =
 *                           tree_size, and proof[32 proof_off[r] : 32 proof_off[r+1]] is its consistency
 *                           proof between the tree of reply_end[r] leaves (the temporary tree of plenum/
 *                           common/ledger.py:129-143 treeWithAppliedTxns, whose root the call computes) and
 *                           the tree of final_size leaves with root final_root[32]. status[r] as above,
 *                           verdict bit r = 1 iff status[r] = 0. reply_end must increase strictly within
 *                           (tree_size, tree_size + n]. GPU or host path by n as an append with per-leaf
 *                           outputs (PV_MERKLE_AUTO_MIN_PROOFS).
 *   pv_merkle_catchup_batch_device
 *                           the same with everything in device memory, enqueued on `stream` without a host
 *                           round trip (alignment and readability as pv_merkle_append_batch_device;
 *                           d_final_root and d_proof 16-byte aligned). A reply whose end is not in
 *                           (tree_size, tree_size + n] gets status 6 and verdict 0.
 *   pv_merkle_prove_plan    host-only arithmetic for q proof queries against a hash store of n_leaves leaves.
 *                           Query i is (kind[i], a[i], b[i]):
 *                             PV_MK_Q_INCLUSION 0    CompactMerkleTree.inclusion_proof(a, b) (ledger/
 *                                                    compact_merkle_tree.py:217-219 over _path :237-249), the
 *                                                    audit path of leaf a in the tree of b leaves that
 *                                                    Ledger.merkleInfo / auditProof (ledger/ledger.py:196-217)
 *                                                    send with a read reply; 0 <= a < b <= n_leaves
 *                             PV_MK_Q_CONSISTENCY 1  consistency_proof(a, b) (:213-215 over _subproof :221-235),
 *                                                    what plenum/server/catchup/seeder_service.py:85-150 builds
 *                                                    per CatchupReq and LedgerStatus; 1 <= a <= b <= n_leaves,
 *                                                    empty when a == b
 *                             PV_MK_Q_ROOT 2         merkle_tree_hash(0, b) (:198-211), one hash; 1 <= b <=
 *                                                    n_leaves, a ignored
 *                           out_off[q + 1] receives the prefix sum of the proofs' lengths in 32-byte units
 *                           (out_off[0] = 0; a proof has at most 49 hashes), status[i] (may be NULL) 0, or 1
 *                           for a query outside those ranges or of an unknown kind, whose length is 0.
 *   pv_merkle_prove_batch   the q proofs themselves, byte for byte what the reference's methods return: proof
 *                           i at out[32 out_off[i] : 32 out_off[i+1]], out holding out_off[q] hashes. The store
 *                           is leaf_hash[32 n_leaves] (the writeLeaf values by 0-based leaf index) and
 *                           node_hash[32 (n_leaves - popcount(n_leaves))] (the writeNode hashes in hash-store
 *                           order), exactly what pv_merkle_append_batch writes. Host buffers, synchronous, GPU
 *                           or C++ host path (pv_merkle_path; AUTO from PV_MERKLE_AUTO_MIN_PROVE queries); works
 *                           without a device and never returns PV_ERR_NOT_INIT. status[i]: 0 written, 1 out of
 *                           range (nothing written), 2 the query's own length differs from the room of its
 *                           slot, out_off[i+1] - out_off[i], or the slot ends beyond out_off[q]: nothing is
 *                           written, so a wrong out_off never makes a write land outside out.
 *   pv_merkle_prove_batch_device
 *                           the same on device buffers (16-byte aligned hash arrays), enqueued on `stream`
 *                           without synchronising, no workspace: a device-resident ledger appends, proves and
 *                           verifies without a hash leaving device memory. d_out_off is the plan's.
 *   pv_merkle_chunk         leaves (or proofs) per device pass; larger batches are chained chunk by
 *                           chunk through the frontier. 0 restores the default, 1,048,576; at most
 *                           PV_MERKLE_CHUNK_MAX (the upper levels of a chunk run in one workgroup).
 *   pv_merkle_path          PV_MERKLE_AUTO, PV_MERKLE_HOST, PV_MERKLE_DEVICE, for the two host-buffer entries.
 *                           AUTO takes the host path without a device and below PV_MERKLE_AUTO_MIN leaves
 *                           (PV_MERKLE_AUTO_MIN_PROOFS when per-leaf roots or paths are asked for,
 *                           PV_MERKLE_AUTO_MIN_VERIFY proofs for the check): the smallest measured sizes
 *                           at which the device path won by more than the run-to-run spread on one
 *                           MI355X; PV_MERKLE_AUTO_MIN_CONSISTENCY proofs for the consistency
 *                           check and PV_MERKLE_AUTO_MIN_PROVE queries for proof generation, measured the
 *                           same way.
 * Bad arguments (decreasing offsets, a store of 2^48 or more leaves, 2^32 or more queries, tree_size + n >= 2^48, a tree size >= 2^48, no frontier for tree_size
 * > 0, path without path_off, 2^32 or more proofs or replies, reply ends out of order or range) return
 * PV_ERR_ARG before anything is launched. */
#define PV_MERKLE_AUTO 0
#define PV_MERKLE_HOST 1
#define PV_MERKLE_DEVICE 2
#define PV_MERKLE_AUTO_MIN 2048        /* appends: frontier / root / leaf and node hashes only */
#define PV_MERKLE_AUTO_MIN_PROOFS 1024 /* appends with per-leaf roots or audit paths */
#define PV_MERKLE_AUTO_MIN_VERIFY 512  /* the proof check */
#define PV_MERKLE_AUTO_MIN_CONSISTENCY 256 /* the consistency check */
#define PV_MERKLE_AUTO_MIN_PROVE 32768 /* proof generation: the host-buffer call uploads the whole store */
#define PV_MERKLE_CHUNK 1048576
#define PV_MERKLE_CHUNK_MAX 16777216 /* 2^24: the largest chunk pv_merkle_chunk accepts */
typedef struct {
    uint8_t* leaf_hash;  /* [32 n] */
    uint8_t* node_hash;  /* [32 n_nodes] */
    uint8_t* frontier;   /* [32 * 64] */
    uint8_t* root;       /* [32] */
    uint8_t* roots;      /* [32 n] */
    uint8_t* path;       /* [32 path_hashes] */
    uint64_t* path_off;  /* [n + 1] */
} PvMerkleOut;
int pv_merkle_plan(uint64_t tree_size, uint64_t n, uint64_t* n_nodes, uint64_t* n_frontier, uint64_t* path_hashes);
int pv_merkle_append_batch(uint64_t tree_size, const uint8_t* frontier, const uint8_t* data, const uint64_t* off,
                           uint64_t n, const PvMerkleOut* out);
int pv_merkle_append_batch_device(uint64_t tree_size, const uint8_t* d_frontier, const uint8_t* d_data,
                                  const uint64_t* d_off, uint64_t n, const PvMerkleOut* d_out, void* stream);
int pv_merkle_verify_inclusion_batch(const uint8_t* data, const uint64_t* off, const uint8_t* leaf_hash,
                                     const uint64_t* leaf_index, const uint64_t* tree_size, const uint8_t* proof,
                                     const uint64_t* proof_off, const uint8_t* root, uint64_t n, uint8_t* status,
                                     uint8_t* verdict_bits);
int pv_merkle_verify_inclusion_batch_device(const uint8_t* d_data, const uint64_t* d_off, const uint8_t* d_leaf_hash,
                                            const uint64_t* d_leaf_index, const uint64_t* d_tree_size,
                                            const uint8_t* d_proof, const uint64_t* d_proof_off, const uint8_t* d_root,
                                            uint64_t n, uint8_t* d_status, uint64_t* d_verdict_words, void* stream);
int pv_merkle_verify_consistency_batch(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_root,
                                       const uint8_t* new_root, const uint8_t* proof, const uint64_t* proof_off,
                                       uint64_t n, uint8_t* status, uint8_t* verdict_bits);
int pv_merkle_verify_consistency_batch_device(const uint64_t* d_old_size, const uint64_t* d_new_size,
                                              const uint8_t* d_old_root, const uint8_t* d_new_root, const uint8_t* d_proof,
                                              const uint64_t* d_proof_off, uint64_t n, uint8_t* d_status,
                                              uint64_t* d_verdict_words, void* stream);
int pv_merkle_catchup_batch(uint64_t tree_size, const uint8_t* frontier, const uint8_t* data, const uint64_t* off, uint64_t n,
                            const uint64_t* reply_end, uint64_t n_replies, uint64_t final_size, const uint8_t* final_root,
                            const uint8_t* proof, const uint64_t* proof_off, const PvMerkleOut* out, uint8_t* status,
                            uint8_t* verdict_bits);
int pv_merkle_catchup_batch_device(uint64_t tree_size, const uint8_t* d_frontier, const uint8_t* d_data,
                                   const uint64_t* d_off, uint64_t n, const uint64_t* d_reply_end, uint64_t n_replies,
                                   uint64_t final_size, const uint8_t* d_final_root, const uint8_t* d_proof,
                                   const uint64_t* d_proof_off, const PvMerkleOut* d_out, uint8_t* d_status,
                                   uint64_t* d_verdict_words, void* stream);
#ifndef PV_MK_Q_INCLUSION
#define PV_MK_Q_INCLUSION 0
#define PV_MK_Q_CONSISTENCY 1
#define PV_MK_Q_ROOT 2
#endif
int pv_merkle_prove_plan(uint64_t n_leaves, const uint8_t* kind, const uint64_t* a, const uint64_t* b, uint64_t q,
                         uint64_t* out_off, uint8_t* status);
int pv_merkle_prove_batch(const uint8_t* leaf_hash, uint64_t n_leaves, const uint8_t* node_hash, const uint8_t* kind,
                          const uint64_t* a, const uint64_t* b, uint64_t q, const uint64_t* out_off, uint8_t* out,
                          uint8_t* status);
int pv_merkle_prove_batch_device(const uint8_t* d_leaf_hash, uint64_t n_leaves, const uint8_t* d_node_hash,
                                 const uint8_t* d_kind, const uint64_t* d_a, const uint64_t* d_b, uint64_t q,
                                 const uint64_t* d_out_off, uint8_t* d_out, uint8_t* d_status, void* stream);
int pv_merkle_chunk(uint64_t leaves);
int pv_merkle_path(int mode);

/* ---- The state trie: batched PruningState.set with SHA3-256 node hashing ----
 * The state's Patricia trie (state/trie/pruning_trie.py) is canonical and its store content-addressed
 * and never pruned (state/db/persistent_db.py:26-30), so n sequential Trie.update calls
 * (pruning_trie.py:1006-1027) equal one pass that builds the final trie and hashes every new node once.
 *   pv_sha3_256_batch        SHA3-256 of n records data[off[i] .. off[i + 1]) -> out[32 i]. Host buffers;
 *                            on the device or the host path as pv_trie_path says.
 *   pv_sha3_256_batch_device the same on device buffers, enqueued on `stream` (null = the library's), no
 *                            synchronise: d_data readable to d_off[n] rounded up to 8 bytes, d_out 8-byte
 *                            aligned. PV_ERR_NOT_INIT without pv_init.
 *   pv_trie_update_batch     the trie under `root` (32 bytes; the blank root = the empty trie) overlaid
 *                            with n sets key i -> value i (values as the trie stores them: PruningState
 *                            passes rlp([value])), a later entry of a key winning. `known` holds the
 *                            existing nodes the caller has fetched: known_hash[32 k] and their RLP
 *                            known_blob[known_off[k] .. known_off[k + 1]). Returns
 *                              PV_OK                out->root, and the new nodes (every node on a touched
 *                                                   path, deepest first, the root last): node i has hash
 *                                                   node_hash[32 i] and RLP node_blob[node_off[i] ..
 *                                                   + node_len[i]); n_nodes and blob_bytes say how many;
 *                              PV_TRIE_NEED_NODES   the update reaches existing nodes that `known` lacks:
 *                                                   out->n_missing hashes in out->missing (as many as
 *                                                   missing_cap holds); fetch them, add them to `known`
 *                                                   and call again. Nothing is called back and no caller
 *                                                   pointer is kept;
 *                              PV_TRIE_NEED_SPACE   node_cap or blob_cap is too small: n_nodes and
 *                                                   blob_bytes hold what is needed;
 *                              PV_ERR_DECODE        a known node is not a well-formed trie node;
 *                              PV_ERR_ARG           null pointers, decreasing offsets, a key above 65,535
 *                                                   bytes, a value that is empty or not below 2^24 bytes.
 *                            n = 0 returns the input root and no nodes. out->launches and
 *                            out->tail_records report how the device path ran (0 on the host path).
 *   pv_trie_path             PV_TRIE_AUTO, PV_TRIE_HOST, PV_TRIE_DEVICE for the two host-buffer entries.
 *                            AUTO hashes on the host without a device and below PV_TRIE_AUTO_MIN records;
 *                            DEVICE without an initialised device returns PV_ERR_NO_DEVICE. */
#define PV_TRIE_NEED_NODES 1
#define PV_TRIE_NEED_SPACE 2
#define PV_TRIE_AUTO 0
#define PV_TRIE_HOST 1
#define PV_TRIE_DEVICE 2
#define PV_TRIE_AUTO_MIN 352 /* records (nodes to hash) from which AUTO takes the device path */
typedef struct {
    uint8_t* root;       /* [32] */
    uint8_t* node_hash;  /* [32 node_cap] */
    uint64_t node_cap;
    uint8_t* node_blob;  /* [blob_cap] */
    uint64_t blob_cap;
    uint64_t* node_off;  /* [node_cap] */
    uint64_t* node_len;  /* [node_cap] */
    uint8_t* missing;    /* [32 missing_cap] */
    uint64_t missing_cap;
    uint64_t n_nodes;    /* written */
    uint64_t blob_bytes;
    uint64_t n_missing;
    uint64_t launches;
    uint64_t tail_records;
} PvTrieOut;
int pv_sha3_256_batch(const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* out);
int pv_sha3_256_batch_device(const uint8_t* d_data, const uint64_t* d_off, uint64_t n, uint8_t* d_out, void* stream);
int pv_trie_update_batch(const uint8_t* root, const uint8_t* known_hash, const uint8_t* known_blob,
                         const uint64_t* known_off, uint64_t n_known, const uint8_t* key_blob, const uint64_t* key_off,
                         const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, PvTrieOut* out);
int pv_trie_path(int mode);

/* ---- The state trie built from empty: the root of n key-value pairs ("Device builder") ----
 * What PruningState.root_of answers, for keys of one length: on the device path the structural half runs as
 * kernels too (sort, deduplicate, structure, sizes, emit), so nothing proportional to n crosses to the host.
 *   pv_trie_root         host buffers. Key i is the key_len bytes at keys + i * key_len, key_len 1 ..
 *                        PV_TRIE_BUILD_MAX_KEY: one length for all, so no key is a prefix of another (mixed
 *                        lengths, the empty key and longer keys stay with pv_trie_update_batch). Value i is
 *                        val_blob[val_off[i] .. val_off[i + 1]). flags & PV_TRIE_ROOT_WRAP: the trie stores
 *                        rlp([value]), as PruningState.set does, wrapped on the device while the leaf is
 *                        written; a value may then be empty. Without it a value is stored as given and has at
 *                        least one byte. Either way the stored length stays below 2^24. A later entry of a key
 *                        wins. n = 0 gives the blank root; n is below 2^31. The root comes in out->root.
 *                        On the device or the host path as pv_trie_path says: PV_TRIE_HOST packs the arguments
 *                        for the structural half of pv_trie_update_batch from the blank root, PV_TRIE_DEVICE
 *                        runs the builder (PV_ERR_NO_DEVICE without a device, never the host path instead),
 *                        PV_TRIE_AUTO the builder from PV_TRIE_BUILD_AUTO_MIN pairs on.
 *                        PV_ERR_ARG: null pointers, key_len out of range, decreasing offsets, a value outside
 *                        the limits. PV_ERR_ALLOC: the builder's workspace (about 300 bytes per pair, plus the
 *                        nodes) does not fit the device.
 *   pv_trie_root_device  the same on device buffers, on `stream` (null = the library's); d_root: 32 bytes on the
 *                        device. The sizes of the second phase depend on the data, so the call synchronises
 *                        `stream` ONCE, between its two phases, to read a few hundred bytes (counts, arena
 *                        bytes, the error word, the per-depth record counts); the hashing and the copy of the
 *                        root to d_root are enqueued and not waited for. Nothing the host cannot see is
 *                        validated before that: the kernels set an error word for decreasing offsets and
 *                        values outside the limits, no kernel uses such an offset, and the call returns
 *                        PV_ERR_ARG after the read. d_val_blob must be readable up to d_val_off[n].
 *                        PV_ERR_NOT_INIT without pv_init.
 * PvTrieRootOut reports how the call ran. The device builder fills every field: n_nodes counts leaves, branches
 * and extensions, embedded ones included; max_depth is the greatest node depth, the root being 0; launches and
 * tail_records are the hashing's, as in PvTrieOut. The host path fills n_records and arena_bytes and leaves the
 * rest 0. The new nodes themselves are not returned. */
#define PV_TRIE_BUILD_MAX_KEY 64
#define PV_TRIE_ROOT_WRAP 1u
#define PV_TRIE_BUILD_AUTO_MIN 512 /* pairs from which AUTO runs the device builder */
typedef struct {
    uint8_t root[32];    /* pv_trie_root; pv_trie_root_device leaves it zero (the root goes to d_root) */
    uint64_t n_keys;     /* distinct keys */
    uint64_t n_nodes;
    uint64_t n_records;  /* nodes hashed: RLP of 32 bytes and more, and the root */
    uint64_t arena_bytes;
    uint64_t max_depth;
    uint64_t launches;
    uint64_t tail_records;
    uint64_t built_on_device; /* 1: the device builder ran */
} PvTrieRootOut;
int pv_trie_root(const uint8_t* keys, uint32_t key_len, uint64_t n, const uint8_t* val_blob, const uint64_t* val_off,
                 uint32_t flags, PvTrieRootOut* out);
int pv_trie_root_device(const uint8_t* d_keys, uint32_t key_len, uint64_t n, const uint8_t* d_val_blob,
                        const uint64_t* d_val_off, uint32_t flags, uint8_t* d_root, PvTrieRootOut* out, void* stream);

/* ---- State proofs: batched verification with SHA3-256 proof-node hashing ----
 * PruningState.verify_state_proof (state/pruning_state.py:113-122 over pruning_trie.py:1100-1119) for many
 * queries at once. A proof is a pool of node records (each one node's RLP); a query names its proof, a root,
 * a key and the value expected as the trie stores it (PruningState passes rlp([value])), length 0 expecting
 * the key's absence. Several queries may share one proof (verify_state_proof_multi, prefix proofs).
 *   pv_trie_verify_proofs         host buffers; one status byte per query:
 *                                   PV_PROOF_ACCEPT / PV_PROOF_REJECT   what the reference's call returns;
 *                                   PV_PROOF_DEFER    the library does not decide: a record of the query's
 *                                                     proof is not canonical RLP (the reference decodes
 *                                                     leniently and hashes its own re-encoding), or a node
 *                                                     the walk visits is not a well-formed trie node. The
 *                                                     caller runs its sequential method.
 *                                 On the device or the host path as pv_trie_path says; AUTO takes the device
 *                                 from PV_TRIE_PROOF_AUTO_MIN records on. PV_ERR_ARG: a null pointer,
 *                                 decreasing offsets, query_proof[i] >= n_proofs, a proof of more than
 *                                 PV_PROOF_MAX_NODES records, a key above 65,535 bytes, a value not below 2^24.
 *   pv_trie_verify_proofs_device  the same on device buffers (d_in is a host struct of device pointers),
 *                                 two launches enqueued on `stream` (null = the library's), no synchronise.
 *                                 d_node_hash: 32 n_nodes bytes of scratch, 8-byte aligned; node_blob readable
 *                                 to its last record's end rounded up to 8 bytes. Nothing the host cannot see
 *                                 is validated: a query whose indices or sizes are out of range gets
 *                                 PV_PROOF_DEFER and reads nothing. PV_ERR_NOT_INIT without pv_init.
 *   pv_trie_proof_split           host only: n_proofs serialized proofs ser[ser_off[p] .. ser_off[p + 1]), each
 *                                 the RLP list of its nodes, split into records in place: node i is
 *                                 ser[node_off[i] .. + node_len[i]), proof p has the records proof_first[p] ..
 *                                 proof_first[p + 1]. The list prefixes lie between the records, hence the
 *                                 lengths. proof_ok[p] = 0 (and no records) for a proof whose outer list is not
 *                                 canonical RLP: the caller defers it. node_off holds node_cap + 1 entries
 *                                 (the last one closes the array, as PvProofIn's), node_len node_cap.
 *                                 *n_nodes is the count needed; records beyond node_cap are not written
 *                                 (PV_TRIE_NEED_SPACE). */
#define PV_PROOF_REJECT 0
#define PV_PROOF_ACCEPT 1
#define PV_PROOF_DEFER 2
#define PV_PROOF_MAX_NODES 1024   /* records per proof */
#define PV_TRIE_PROOF_AUTO_MIN 259 /* proof records from which AUTO takes the device path */
typedef struct {
    const uint8_t* node_blob;
    const uint64_t* node_off;    /* n_nodes + 1: record i starts at node_off[i] */
    uint64_t n_nodes;
    const uint64_t* proof_first; /* n_proofs + 1: first record of proof p */
    uint64_t n_proofs;
    const uint32_t* query_proof; /* n_queries: which proof */
    const uint8_t* root;         /* 32 n_queries */
    const uint8_t* key_blob;
    const uint64_t* key_off;     /* n_queries + 1 */
    const uint8_t* val_blob;
    const uint64_t* val_off;     /* n_queries + 1; length 0 = expect absence */
    uint64_t n_queries;
    const uint64_t* node_len;    /* null: record i ends at node_off[i + 1]; else n_nodes lengths (records
                                    with bytes between them, as pv_trie_proof_split leaves them) */
} PvProofIn;
int pv_trie_verify_proofs(const PvProofIn* in, uint8_t* status);
int pv_trie_verify_proofs_device(const PvProofIn* d_in, uint8_t* d_status, uint8_t* d_node_hash, void* stream);
int pv_trie_proof_split(const uint8_t* ser, const uint64_t* ser_off, uint64_t n_proofs, uint64_t* proof_first,
                        uint64_t* node_off, uint64_t* node_len, uint64_t node_cap, uint64_t* n_nodes, uint8_t* proof_ok);

#ifdef __cplusplus
}
#endif
#endif /* PLENUM_VERIFY_H */
