// Host state of the verification engine shared by its translation units: the device context Ctx
// (pv_engine.hip builds, frees and launches the kernels of its kern_*.h headers on it; pv_sign.hip, pv_host.hip and pv_multi.hip work on it
// under its mutex), the calling thread's error string, the kernel-launch helpers, and the functions
// that cross a file boundary. Everything declared here is internal to libplenum_verify.so (hidden).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "copy_pool.h"
#include "kc_admit.h"
#include "kc_index.h"
#include "keycache.h"
#include "pv_engine_dev.h"
#include "pv_internal.h"
#include "../../include/plenum_verify.h"

typedef struct ncclComm* ncclComm_t;  // <rccl/rccl.h>'s, for Ctx::comm: only pv_multi.hip and ctx_free call RCCL

#pragma GCC visibility push(hidden)

// an integer from the environment (A/B knobs read once at first use), or dflt
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

// Node-side key cache (keycache.h): the device arrays and the host index over their slots.
struct KeyCache {
    PvOwner own;  // the device and pinned blocks below: they live from one configure call to the next
    uint32_t cap = 0;
    uint32_t* d_htab = nullptr;
    uint32_t* d_keys = nullptr;
    uint32_t* d_flags = nullptr;
    uint4* d_tab = nullptr;
    uint4* d_ntab = nullptr;      // the tables with every entry divided by its Z (comb path), or null
    uint4* d_wtab = nullptr;      // radix-65536 niels rows of slots < wcap (comb.h PV_KW_*), or null
    uint32_t wcap = 0;
    uint32_t* d_wscr = nullptr;   // Z products of one group of wide-row builds
    uint8_t* d_put_pk = nullptr;  // keys of one put batch
    uint32_t* d_put_slot = nullptr;
    uint32_t hmask = 0, seed = 0;
    bool enabled = true;  // consulted by the latency path
    pvhost::KcIndex index;  // which slot holds which key, the LRU, the free slots (kc_index.h)
    bool broken = false;  // a failed hash-table upload left the device table stale: not consulted
    // automatic admission (pv_key_cache_auto): a key is put on its auto_min-th VERIFIED appearance
    // in pv_verify_batch calls (every request of calls of <= PV_KC_AUTO_MAX_BATCH requests, a
    // sample of larger ones). Appearances are counted in a table of full keys hashed by NH +
    // multiply-shift under a per-process secret, with bounded probing (kc_admit.h); an evicted key is
    // forgotten there, so it can be re-admitted
    uint32_t auto_min = 0;
    pvhost::AdmitTable seen;
    uint64_t auto_admitted = 0, auto_failed = 0;
    // LRU refresh on use: every launch that consults the cache stamps the slots it reads with its
    // epoch (d_stamp, pv_kc_lookup); before a put evicts, the slots stamped since the last fold
    // move to the front of the host LRU (kc_fold_hits)
    uint32_t* d_stamp = nullptr;
    uint32_t epoch = 1, fold_epoch = 1;
    // pinned staging of an asynchronous put (keys, slots, hash table), reused once ev_async is done
    uint8_t* h_async = nullptr;
    uint64_t h_async_cap = 0;
    hipEvent_t ev_async = nullptr;  // the context's (Ctx::own): it outlives a reconfigure
    bool async_pending = false;
};

struct Ctx {
    int device = -1;
    int cus = 0;
    // Everything the context creates once and keeps until pv_shutdown (workspace.h): the streams and
    // events below, the blocks of work / kw / xt, the fixed-base tables, h_zc_verdict, kc.ev_async. The
    // fields are what the code reads; ctx_free releases through `own` alone.
    PvOwner own;
    hipStream_t stream = nullptr;
    hipStream_t kstream = nullptr;           // per-key pipeline (chain + table fill), overlapped
    hipEvent_t ev_keys_ready = nullptr;      // dedup done (main -> Straus side stream)
    hipEvent_t ev_scan_done = nullptr;       // comb keys chosen (main -> kstream, before the scatter)
    hipEvent_t ev_tables_ready = nullptr;    // comb tables done (fstream -> main)
    hipStream_t fstream = nullptr;           // table fill of a chunk that may fill sparsely
    hipEvent_t ev_chain = nullptr;           // chain done (kstream -> fstream)
    hipEvent_t ev_prep_done = nullptr;        // comb_prep done: need masks ready (main -> fstream)
    hipStream_t sstream = nullptr;           // Straus-path slots of a split chunk, overlapped
    hipEvent_t ev_straus_done = nullptr;     // their q / flags written (sstream -> main)
    // Workspace hand-over between callers' streams (workspace.h): every launch ends by recording it on
    // its stream, and a launch on a DIFFERENT stream first makes its stream wait for it.
    PvHandover hand;
    uint32_t* d_btab = nullptr;
    Work work{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr};
    KeyWork kw{};
    bool last_keyed = false;  // the most recent chunk ran the dedup / split kernels
    bool slots_dirty = true;  // the key hash table / need masks may hold entries (cleared before use)
    // resident-table directory (KeyWork::dir_*): on/off, the slots it may list, and whether it has to be
    // emptied before the next keyed chunk (first use, a control call, an enqueue failure in a keyed chunk)
    bool dir_on = true;
    uint32_t dir_cap = PV_DIR_DEFAULT_CAP;
    bool dir_dirty = true;
    bool aff_on = true;  // dense chunks convert the resident tables they hit to affine rows (pv_table_affine)
    // radix-2^11 rows of resident tables (pv_table_wide): the pool's capacity in tables (0: off), the pool
    // and its builder's scratch (allocated by the first chunk that can widen), dense chunks seen until then
    uint32_t wide_cap = PV_WIDE_DEFAULT;
    bool wide_failed = false;  // the pool's allocation failed: off until pv_table_wide names a capacity again
    uint32_t wide_dense = 0;
    PvDevBuf d_wide, d_wide_scr;
    bool last_latency = false;  // the most recent launch took the latency path
    bool verdict_zeroed = false;  // the caller's verdict words are already 0 (pv_verify_batch)
    bool keyed_hint = false;      // pv_verify_batch saw few distinct keys: keyed path below PV_LATENCY_MAX
    bool hint_set = false;        // pv_verify_batch decided keyed_hint on the host (no device-side choice)
    bool last_dev_choice = false; // the last launch let its dedup pick latency vs keyed
    uint32_t last_split[3] = {0, 0, 0};  // PV_SPLIT_* of it, read back by pv_last_path
    uint4* d_bcomb = nullptr;  // fixed-base comb T_B (radix 65536; latency path)
    uint4* d_bc2 = nullptr;    // wide fixed-base comb T_B2 (radix 2^W; comb path's [S]B)
    int bc2_w = PV_BC2_W;      // its radix: PV_BC2_W, or 16 when d_bc2 aliases d_bcomb (fallback)
    uint32_t prep_lds_pad = PV_PREP_LDS_PAD;  // dynamic LDS per comb_prep workgroup (occupancy cap)
    int path = PV_PATH_AUTO;
    // host-entry staging
    PvPinnedBuf h_stage;
    PvDevBuf d_stage;
    PvPinnedBuf h_ver;  // verdict words of the pipelined host-buffer form
    // pipelined host-buffer form: H2D of sub-batch j on cstream, its kernels on `stream` after ev_copy[j]
    hipStream_t cstream = nullptr;
    hipEvent_t ev_cstart = nullptr;  // the engine stream's work so far (cstream waits: staging reuse)
    std::vector<hipEvent_t> ev_copy;
    int inject_stage = 0;  // pv_test_inject(PV_INJECT_STAGE): host-buffer stagings left to fail
    // the comb tables one pipelined host call's sub-batches share (pv_xtab_publish_kernel): room for
    // PV_XT_KEYS keys, allocated on first use; xt_fill: the next chunk builds its tables here and
    // publishes them; xt_use: the next chunks look keys up here (as in the node-side key cache)
    struct {
        uint32_t* htab = nullptr;
        uint32_t* keys = nullptr;
        uint32_t* flags = nullptr;
        uint4* tab = nullptr;
        bool failed = false;  // allocation failed once: the call's sub-batches build their own tables
    } xt;
    bool xt_fill = false, xt_use = false;
    bool timing = false;
    // PV_NSTAGES + 1 events per chunk launched since pv_set_timing(1) (stage boundaries, see
    // pv_stage_times); unused stages record back-to-back events
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    KeyCache kc;  // node-side key cache (pv_keycache.hip)
    // zero-copy verdict bytes (pinned, coherent: the host reads them while the kernel runs)
    uint8_t* h_zc_verdict = nullptr;
    bool last_zero_copy = false;  // the most recent pv_verify_batch took the zero-copy form
    // pv_verify_batch_multi_gpu: this device's gathered verdict words (device) and their host copy
    PvDevBuf d_mg;
    PvPinnedBuf h_mg;
    const uint32_t* last_nkeys = nullptr;  // split counters of the most recent keyed chunk
    // Signing workspace (pv_sign_*), its own: the expanded keys (a mod L || prefix, 64 B per signer), the
    // host entries' copy of the secret keys (pinned and device) and their pinned chunk stage, which also
    // carries pv_sign_seed_keypairs' seeds. Handed over between callers' streams like the verification
    // workspace. The secret parts are overwritten before a call returns (device entry: behind its
    // kernels, on its stream).
    struct {
        PvDevBuf d_keys;
        PvDevBuf d_sk;
        PvPinnedBuf h_sk;
        PvStage stage;
        PvHandover hand;
    } sg;
};

// One context per device. The single-device ABI (pv_init, pv_verify_batch, ...) works on the device
// pv_init bound (the primary); pv_init_devices adds contexts for more devices of the same process,
// which pv_verify_batch_multi_gpu drives from one worker thread per device. g_ctx / g_mu name the
// calling thread's context: a multi-GPU worker's device (t_dev), else the primary.
constexpr int PV_MAX_DEV = 16;
extern Ctx g_ctxs[PV_MAX_DEV];
extern std::mutex g_mus[PV_MAX_DEV];
extern std::atomic<int> g_primary;
extern __attribute__((require_constant_initialization)) thread_local int t_dev;
inline int pv_cur_dev() {
    if (t_dev >= 0) return t_dev;
    const int p = g_primary.load(std::memory_order_acquire);
    return p >= 0 ? p : 0;
}
#define g_ctx (g_ctxs[pv_cur_dev()])
#define g_mu (g_mus[pv_cur_dev()])
// Makes `dev` the calling thread's context for the scope (multi-GPU workers, per-device init).
struct DevScope {
    int prev;
    explicit DevScope(int dev) : prev(t_dev) { t_dev = dev; }
    ~DevScope() { t_dev = prev; }
};
extern thread_local std::string g_err;

int fail(int code, const std::string& msg);

// PV_LAUNCH (workspace.h) for a kernel instantiated per wide-comb radix (Bc2<W>), launched for the radix
// pv_init chose.
#define PV_LAUNCH_BC2(k, ...)                                                                      \
    do {                                                                                           \
        if (g_ctx.bc2_w == 16) hipLaunchKernelGGL(k<16>, __VA_ARGS__);                             \
        else hipLaunchKernelGGL(k<PV_BC2_W>, __VA_ARGS__);                                          \
        PV_HIP(hipGetLastError(), PV_ERR_LAUNCH);                                                  \
    } while (0)

// pv_engine.hip
int kc_build_tables(const pvhost::KcIndex::Assigned& put, bool async);
int launch(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk, uint64_t* d_verdict,
           hipStream_t stream);
int check_device_index(int device, const char* who);
int ctx_init(int device);
// pv_keycache.hip
void kc_free();
PvKeyCacheView kc_view();
int kc_put_locked(const uint8_t* pks, uint64_t n, bool async);
// pv_host.hip
void pinned_cache_drain();
bool offsets_nondecreasing(const uint64_t* off, uint64_t n);
int stage_and_launch(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk, uint64_t* d_out,
                     uint64_t** dver_out, uint64_t** hver_out);
// pv_multi.hip
extern std::mutex g_mg_mu;
void mg_destroy_comms();

#pragma GCC visibility pop
