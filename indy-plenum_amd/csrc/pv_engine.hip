// libplenum_verify: MI355X batch Ed25519 verification engine: the unit of the verification kernels (one
// kern_*.h header per stage, included below and nowhere else), the device context (pv_ctx.h Ctx: lifecycle,
// launch, control and statistics entries), the table build of a key-cache put and the device-buffer entry.
// No __global__ or __device__ function is written in this file. The rest of the engine lives beside it: signing in
// pv_sign.hip, the host-buffer entries in pv_host.hip, the key cache's host side in pv_keycache.hip, RCCL
// and in-process multi-GPU in pv_multi.hip, the latency path in pv_latency.hip; the device types they
// share are pv_engine_dev.h. What a launch decides on the host (path, lookup views, KeyWork scalars, launch
// shape, grids) is chunk_plan.h, with the thresholds those rules read; launch_chunk applies it.
//
// One lane per request, 256-thread workgroups, two workgroups per CU (2 waves/SIMD: measured
// v_mad_u64_u32 throughput saturates at >= 2 waves/SIMD, profiles/r01_isa_rates.jsonl). The grid is
// a fixed number of workgroups that stride over the batch, so the per-lane HBM table of [j](-A)
// (9 cached points x 160 B) is sized by resident lanes, not by the batch.
//
// Replaces (per request) stp_core/crypto/nacl_wrappers.py:108 libnacl.crypto_sign_open(sm, pk);
// see include/plenum_verify.h for the ABI contract and verify_core.h for the arithmetic.
//
// The #ifndef switches in the kern_*.h headers are numeric tuning constants (microbench/build_variants.sh
// varies them) and diagnostic builds. The kernel forms, priorities and stream layouts that lost their A/B are
// not in the source any more: DESIGN.md, "Variants tried and retired", has each one's result.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <atomic>
#include <random>
#include <functional>
#include <thread>
#include <string>
#include <vector>

#include "btable.h"
#include "comb.h"
#include "keycache.h"
#include "lp25519.h"
#include "verify_core.h"
#include "pv_engine_dev.h"
#include "pv_ctx.h"
#include "pv_internal.h"
#include "../../include/plenum_verify.h"
#include "../../include/plenum_verify_test.h"

// The verification kernels, one header per stage, in launch order but for the wide-row builders. Only this
// unit includes them: their non-template __global__ functions have external linkage.
#include "kern_access.h"
#include "kern_straus.h"
#include "kern_keys.h"
#include "kern_tables.h"
#include "kern_wide.h"
#include "kern_comb.h"
#include "kern_encode.h"

// ------------------------------------------------------------------------------------------ host

// The device contexts and the calling thread's error string (pv_ctx.h).
Ctx g_ctxs[PV_MAX_DEV];
std::mutex g_mus[PV_MAX_DEV];
std::atomic<int> g_primary{-1};
thread_local int t_dev = -1;
thread_local std::string g_err;

namespace {

int ensure_events(int count) {
    while ((int)g_ctx.ev.size() < count) {
        hipEvent_t e;
        if (int rc = g_ctx.own.event(e, hipEventDefault)) return rc;
        g_ctx.ev.push_back(e);
    }
    return PV_OK;
}

static_assert(PV_FILL_ITEMS_PER_KEY == PV_COMB_POS * PV_COMB_BLOCKS, "chunk_plan.h: fill work items per key");
// bytes of one table's radix-2^11 rows in the wide pool
constexpr uint64_t PV_WIDE_TABLE_BYTES = (uint64_t)PV_KR_POS * PV_KR_ENT * PV_BCOMB_STRIDE * 4;

// One chunk's launch sequence: what its stages share. Every decision is in `p` (chunk_plan.h); the stages
// below enqueue what it names, record and wait on events, and keep the dirty flags in step with the enqueues.
struct ChunkLaunch {
    const pvhost::ChunkPlan& p;
    const KeyWork& kw;  // the context's, with the plan applied (apply_plan)
    Gate gate;
    const uint8_t* d_sm;
    const uint64_t* d_off;  // the chunk's first offset
    uint64_t m;
    const uint8_t* d_pk;  // the chunk's first key
    uint64_t* d_verdict;  // the chunk's first verdict word
    hipStream_t stream;
    hipEvent_t* e;  // the chunk's PV_NSTAGES + 1 timing events, or null
    int mark(int k) const {
        if (e) PV_HIP(hipEventRecord(e[k], stream), PV_ERR_LAUNCH);
        return PV_OK;
    }
};

// The plan's scalars into the chunk's KeyWork, and the pointers its lookup arrangement names: kcv / xtv are
// the probe's first and second view, kc_flags the flags of the first.
void apply_plan(const pvhost::ChunkPlan& p, KeyWork& kw, PvKeyCacheView& kcv, PvKeyCacheView& xtv,
                const uint32_t*& kc_flags) {
    const PvKeyCacheView xv{g_ctx.xt.htab, g_ctx.xt.keys, g_ctx.xt.flags, g_ctx.xt.tab, PV_XT_HASH - 1, g_ctx.kw.seed};
    const bool xt_only = p.lookup == pvhost::LOOKUP_XT_ONLY, xt_second = p.lookup == pvhost::LOOKUP_NODE_THEN_XT;
    xtv = xt_second ? xv : PvKeyCacheView{nullptr, nullptr, nullptr, nullptr, 0u, 0u};
    if (xt_only) kcv = xv;
    kc_flags = xt_only ? g_ctx.xt.flags : g_ctx.kc.d_flags;
    kw.kc_tab = xt_only ? g_ctx.xt.tab : g_ctx.kc.d_tab;
    kw.kc_ntab = xt_only ? nullptr : g_ctx.kc.d_ntab;
    kw.kc_wtab = xt_only ? nullptr : g_ctx.kc.d_wtab;
    kw.xt_flags = xt_second ? g_ctx.xt.flags : nullptr;
    kw.xt_tab = xt_second ? g_ctx.xt.tab : nullptr;
    kw.wide_tab = g_ctx.d_wide.as<uint4>();
    kw.wide_scr = g_ctx.d_wide_scr.as<uint32_t>();
    if (p.dense_only) kw.ctab = g_ctx.xt.tab;  // sub-batch 0 of a pipelined host call builds into the shared store
    kw.min_req = p.min_req;
    kw.kc_on = p.kc_on;
    kw.kc_wcap = p.kc_wcap;
    kw.dir_on = p.dir_on;
    kw.dir_cap = p.dir_cap;
    kw.dir_pub = p.dir_pub;
    kw.aff_conv = p.aff_conv;
    kw.wide_cap = p.wide_cap;
    kw.wide_conv = p.wide_conv;
    kw.chunk_n = p.chunk_n;
    kw.seg_cap = p.seg_cap;
    kw.lat_choice = p.lat_choice;
    kw.dense_only = p.dense_only;
    kw.kcap = p.kcap;
}

// The wide pool's allocation, when plan_wide_pool asks for it. A failure turns the feature off and is
// reported once through the error string; the chunk goes on without wide rows.
void wide_pool_attempt(uint64_t wide_want) {
    if (g_ctx.d_wide.grow(wide_want) != PV_OK ||
        g_ctx.d_wide_scr.grow((uint64_t)PV_WIDE_GRID * PV_KR_RUN * 10 * PV_WIDE_THREADS * 4) != PV_OK) {
        (void)hipGetLastError();  // clear the failed allocation's sticky error
        g_ctx.d_wide.release();
        g_ctx.d_wide_scr.release();
        g_ctx.wide_failed = true;
        (void)fail(PV_ERR_ALLOC, "wide rows of resident tables: no memory for the pool, the feature is off");
    }
}

// Key stage of a keyed chunk: the clears the dirty flags force, dedup (seed, insert, assign), the probe of
// the lookup views, the scan, the scatter on the main stream and the chain and fill on the key stream.
int launch_key_stage(const ChunkLaunch& L, const PvKeyCacheView& kcv, const PvKeyCacheView& xtv,
                     const uint32_t* kc_flags) {
    const pvhost::ChunkPlan& p = L.p;
    const KeyWork& kw = L.kw;
    hipStream_t stream = L.stream;
    if (p.clear_slots) {
        PV_HIP(hipMemsetAsync(kw.slot, 0xFF, (uint64_t)(kw.hmask + 1) * 4, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.slot_cnt, 0, (uint64_t)(kw.hmask + 1) * 4 * PV_RANK_SUB, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.need, 0, (uint64_t)PV_ALLCOMB_KEYS * PV_COMB_POS * 5 * 4, stream), PV_ERR_LAUNCH);
    }
    g_ctx.slots_dirty = true;  // until this chunk's unpermute kernel is enqueued
    if (p.clear_dir) {
        PV_HIP(hipMemsetAsync(kw.dir_htab, 0xFF, (uint64_t)PV_DIR_HASH * 4, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.dir_cnt, 0, 2 * 4, stream), PV_ERR_LAUNCH);
        PV_HIP(hipMemsetAsync(kw.wide_cnt, 0, 2 * 4, stream), PV_ERR_LAUNCH);  // the pool empties with it
    }
    if (p.mark_dir_dirty) g_ctx.dir_dirty = true;  // until the chunk is enqueued whole
    // kw.nkeys is cleared by pv_key_insert_lds_kernel (m >= 1 here: the grid has a thread 0)
    if (p.seed_reqs) {
        PV_LAUNCH(pv_key_seed_kernel, dim3(pvhost::block_grid(p.seed_reqs)), dim3(PV_BLOCK), 0, stream, L.d_pk,
                  p.seed_reqs, kw);
    }
    PV_LAUNCH(pv_key_insert_lds_kernel, dim3(p.ins_grid), dim3(PV_INS_THREADS), 0, stream, L.d_pk, L.m, kw);
    PV_LAUNCH(pv_key_assign_kernel, dim3(p.req_grid), dim3(PV_BLOCK), 0, stream, L.m, kw);
    if (p.run_probe) {
        PvKeyCacheView dirv{kw.dir_htab, kw.dir_keys, kw.dir_flags, kw.ctab, p.dir_use ? PV_DIR_HASH - 1 : 0u, kw.seed};
        PV_LAUNCH(pv_key_cache_probe_kernel, dim3(p.probe_grid), dim3(PV_BLOCK), 0, stream, L.d_pk, kw, kcv, xtv, dirv);
    }
    // key-sorted slot order: comb keys' requests first, then the Straus requests
    PV_LAUNCH(pv_key_scan_kernel, dim3(1), dim3(PV_SCAN_THREADS), 0, stream, kw, kc_flags);
    // the per-key chain (few, long-latency lanes) and the table fill run on kstream, overlapped
    // with the scatter and the per-request prep on the main stream: the chain needs only the
    // scan's comb-key list (comb_key, comb_cslot), so kstream forks before the scatter
    PV_HIP(hipEventRecord(g_ctx.ev_scan_done, stream), PV_ERR_LAUNCH);
    PV_HIP(hipStreamWaitEvent(g_ctx.kstream, g_ctx.ev_scan_done, 0), PV_ERR_LAUNCH);
    PV_LAUNCH(pv_key_scatter_kernel, dim3(p.req_grid), dim3(PV_BLOCK), 0, stream, L.m, kw);
    PV_HIP(hipEventRecord(g_ctx.ev_keys_ready, stream), PV_ERR_LAUNCH);
    // one chain launch over all positions, then the fill. direct_fill: back to back on kstream
    // and the tables-ready event right after the fill (no event hop to fstream, no gated
    // sparse-fill launch in the dependency chain of the comb kernel). Otherwise the fill runs on
    // fstream, where the sparse fill follows it (launch_comb_stage).
    hipStream_t fs = p.direct_fill ? g_ctx.kstream : g_ctx.fstream;
    PV_LAUNCH(pv_key_chain_lp_kernel, dim3(p.chain_blocks), dim3(64), 0, g_ctx.kstream, L.d_pk, kw, L.gate, 0,
              PV_COMB_POS);
    if (!p.direct_fill) {
        PV_HIP(hipEventRecord(g_ctx.ev_chain, g_ctx.kstream), PV_ERR_LAUNCH);
        PV_HIP(hipStreamWaitEvent(fs, g_ctx.ev_chain, 0), PV_ERR_LAUNCH);
    }
    PV_LAUNCH(pv_key_fill_kernel, dim3(p.fill_grid), dim3(PV_BLOCK), 0, fs, kw, L.gate, 0, PV_COMB_POS);
    if (p.direct_fill) PV_HIP(hipEventRecord(g_ctx.ev_tables_ready, g_ctx.kstream), PV_ERR_LAUNCH);
    return PV_OK;
}

// The Straus-path slots of a split chunk (keys without a table: usually a few thousand one-off requests)
// run on their own stream beside the comb kernels: their waves take ~1 ms from start to end however few
// they are, which on the main stream would delay the whole comb path. Their blocks are dispatched from
// the END of the slot range (where the Straus slots are), and blocks of comb slots exit at once.
int launch_straus_side(const ChunkLaunch& L) {
    hipStream_t ss = g_ctx.sstream;
    const dim3 grid(L.p.side_grid), block(PV_BLOCK);
    PV_HIP(hipStreamWaitEvent(ss, g_ctx.ev_keys_ready, 0), PV_ERR_LAUNCH);
    PV_LAUNCH_BC2(pv_prep_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    PV_LAUNCH_BC2(pv_split_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, g_ctx.work, L.gate);
    PV_LAUNCH(pv_table_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    PV_LAUNCH_BC2(pv_msm_kernel, grid, block, 0, ss, L.d_sm, L.d_off, L.m, g_ctx.d_btab, g_ctx.work, g_ctx.d_bc2,
                  L.gate);
    PV_HIP(hipEventRecord(g_ctx.ev_straus_done, ss), PV_ERR_LAUNCH);
    return PV_OK;
}

// Comb stage of a keyed chunk on the main stream: the per-request prep and digits while the key stream
// builds the tables, then [S]B + [k](-A) once they are ready, then the join with the Straus side.
int launch_comb_stage(const ChunkLaunch& L) {
    const pvhost::ChunkPlan& p = L.p;
    const KeyWork& kw = L.kw;
    hipStream_t stream = L.stream;
    const dim3 grid(p.req_grid), block(PV_BLOCK);
    int rc;
    PV_LAUNCH_BC2(pv_comb_prep_req_kernel, grid, block, g_ctx.prep_lds_pad, stream, L.d_sm, L.d_off, L.m, L.d_pk,
                  g_ctx.work, kw, L.gate);
    if (!p.direct_fill) {
        // a small chunk's sparse table fill (needs the chain's bases and the need masks comb_prep
        // writes) runs on fstream after the full fill; for a large chunk it exits at once
        PV_HIP(hipEventRecord(g_ctx.ev_prep_done, stream), PV_ERR_LAUNCH);
        PV_HIP(hipStreamWaitEvent(g_ctx.fstream, g_ctx.ev_prep_done, 0), PV_ERR_LAUNCH);
        PV_LAUNCH(pv_key_fill_sparse_kernel, dim3(PV_ALLCOMB_KEYS * PV_COMB_POS / PV_BLOCK), block, 0, g_ctx.fstream,
                  kw, L.gate);
        PV_HIP(hipEventRecord(g_ctx.ev_tables_ready, g_ctx.fstream), PV_ERR_LAUNCH);
    }
    // the per-request results to slot-ordered rows, while the key stream finishes the tables
    PV_LAUNCH_BC2(pv_comb_digits_kernel, grid, block, 0, stream, g_ctx.work, kw, L.gate);
    if ((rc = L.mark(PV_STAGE_TABLE))) return rc;
    if (!p.fused)  // [S]B while the key stream finishes the tables, then join
        PV_LAUNCH_BC2(pv_comb_b_kernel, grid, block, 0, stream, L.m, g_ctx.work, kw, g_ctx.d_bc2, L.gate);
    PV_HIP(hipStreamWaitEvent(stream, g_ctx.ev_tables_ready, 0), PV_ERR_LAUNCH);
    if ((rc = L.mark(PV_STAGE_MSM))) return rc;
    if (p.fused)  // [S]B + [k](-A) in one kernel as soon as the tables are built
        PV_LAUNCH_BC2(pv_comb_ab_kernel, grid, block, 0, stream, L.m, g_ctx.work, kw, g_ctx.d_bc2, L.gate);
    else
        PV_LAUNCH(pv_comb_a_kernel, grid, block, 0, stream, L.m, g_ctx.work, kw, L.gate);
    PV_HIP(hipStreamWaitEvent(stream, g_ctx.ev_straus_done, 0), PV_ERR_LAUNCH);
    return PV_OK;
}

// A chunk with no key kernels: every request on the Straus path, on the main stream.
int launch_straus_only(const ChunkLaunch& L) {
    hipStream_t stream = L.stream;
    const dim3 grid(L.p.req_grid), block(PV_BLOCK);
    int rc;
    PV_LAUNCH_BC2(pv_prep_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    PV_LAUNCH_BC2(pv_split_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, g_ctx.work, L.gate);
    if ((rc = L.mark(PV_STAGE_TABLE))) return rc;
    PV_LAUNCH(pv_table_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.work, L.gate);
    if ((rc = L.mark(PV_STAGE_MSM))) return rc;
    PV_LAUNCH_BC2(pv_msm_kernel, grid, block, 0, stream, L.d_sm, L.d_off, L.m, g_ctx.d_btab, g_ctx.work, g_ctx.d_bc2,
                  L.gate);
    return PV_OK;
}

// Epilogue: the encode; for a keyed chunk the verdicts back to request order, the publishes and conversions
// for the chunks that follow, and the latency launch of a device-side choice.
int launch_epilogue(const ChunkLaunch& L) {
    const pvhost::ChunkPlan& p = L.p;
    const KeyWork& kw = L.kw;
    hipStream_t stream = L.stream;
    if (p.enc16)
        PV_LAUNCH(pv_encode_kernel<16>, dim3(p.enc_grid), dim3(PV_BLOCK), 0, stream, L.d_sm, L.d_off, L.m, g_ctx.work,
                  L.d_verdict, kw, L.gate);
    else
        PV_LAUNCH(pv_encode_kernel<PV_ENC_SMALL_B>, dim3(p.enc_grid), dim3(PV_BLOCK), 0, stream, L.d_sm, L.d_off, L.m,
                  g_ctx.work, L.d_verdict, kw, L.gate);
    if (!p.keyed) return PV_OK;
    PV_LAUNCH(pv_unpermute_kernel, dim3(p.req_grid), dim3(PV_BLOCK), 0, stream, L.m, kw, L.d_verdict, L.gate);
    g_ctx.slots_dirty = false;
    if (p.run_xtab_publish)
        PV_LAUNCH(pv_xtab_publish_kernel, dim3(PV_XT_KEYS / PV_BLOCK), dim3(PV_BLOCK), 0, stream, L.d_pk, kw,
                  g_ctx.xt.htab, PV_XT_HASH - 1, g_ctx.kw.seed, g_ctx.xt.keys, g_ctx.xt.flags);
    if (p.run_dir_publish)
        PV_LAUNCH(pv_dir_publish_kernel, dim3(p.pub_grid), dim3(PV_BLOCK), 0, stream, L.d_pk, kw);
    if (p.run_affine) PV_LAUNCH(pv_dir_affine_kernel, dim3(PV_AFF_CAP), dim3(PV_AFF_THREADS), 0, stream, kw);
    if (p.run_widen) PV_LAUNCH(pv_dir_widen_kernel, dim3(PV_WIDE_GRID), dim3(PV_WIDE_THREADS), 0, stream, kw);
    if (p.dir_use) g_ctx.dir_dirty = false;
    if (p.run_dev_latency)  // the words were zeroed by the unpermute kernel
        return pv_latency_launch(L.d_sm, L.d_off, L.m, L.d_pk, g_ctx.d_bcomb, kc_view(), L.d_verdict, true, stream,
                                 kw.nkeys + PV_SPLIT_LAT);
    return PV_OK;
}

// Chunk c of the batch on `stream` (the workspace is the context's; key / fill / side streams join it):
// plan (chunk_plan.h), apply, launch.
int launch_chunk(int c, uint64_t n, const uint8_t* d_sm, const uint64_t* d_off, const uint8_t* d_pk,
                 uint64_t* d_verdict, hipStream_t stream, const pvhost::BatchPlan& batch, int evb) {
    constexpr int NE = PV_NSTAGES + 1;
    const uint64_t cap = g_ctx.work.stride;
    const uint64_t c0 = (uint64_t)c * cap;
    const uint64_t m = std::min<uint64_t>(cap, n - c0);
    pvhost::ChunkPlan p;
    KeyWork kw = g_ctx.kw;
    ChunkLaunch L{p, kw, Gate{nullptr, nullptr}, d_sm, d_off + c0, m, d_pk + 32 * c0, d_verdict + c0 / 64, stream,
                  g_ctx.timing ? &g_ctx.ev[evb + NE * c] : nullptr};
    int rc = L.mark(PV_STAGE_KEYS);
    if (rc) return rc;
    if (batch.latency) {
        // one kernel: every stage of the verification inside it (timed as MSM)
        g_ctx.last_keyed = false;
        for (int k = PV_STAGE_PREP; k <= PV_STAGE_MSM; k++)
            if ((rc = L.mark(k))) return rc;
        rc = pv_latency_launch(d_sm, L.d_off, m, L.d_pk, g_ctx.d_bcomb, kc_view(), L.d_verdict, g_ctx.verdict_zeroed,
                               stream, nullptr);
        if (rc) return rc;
        if ((rc = L.mark(PV_STAGE_ENCODE)) || (rc = L.mark(PV_NSTAGES))) return rc;
        return PV_OK;
    }
    PvKeyCacheView kcv = kc_view(), xtv;
    pvhost::ChunkFacts f{};
    f.m = m;
    f.path = g_ctx.path;
    f.keyed_hint = g_ctx.keyed_hint;
    f.node_kc = kcv.hmask != 0;
    f.kc_wcap = g_ctx.kc.wcap;
    f.xt_use = g_ctx.xt_use;
    f.xt_fill = g_ctx.xt_fill;
    f.dir_on = g_ctx.dir_on;
    f.dir_cap = g_ctx.dir_cap;
    f.aff_on = g_ctx.aff_on;
    f.wide_cap = g_ctx.wide_cap;
    f.kcap = g_ctx.kw.kcap;
    f.cus = g_ctx.cus;
    f.slots_dirty = g_ctx.slots_dirty;
    f.dir_dirty = g_ctx.dir_dirty;
    const bool keyed = pvhost::chunk_keyed(batch, f);
    g_ctx.last_keyed = keyed;
    if (keyed) g_ctx.last_nkeys = g_ctx.kw.nkeys;
    const uint64_t wide_want = (uint64_t)g_ctx.wide_cap * PV_WIDE_TABLE_BYTES;
    const pvhost::WideTrigger wt = pvhost::plan_wide_pool(keyed, pvhost::chunk_dir_pub(f), g_ctx.wide_failed,
                                                         g_ctx.d_wide.cap, wide_want, g_ctx.wide_dense);
    g_ctx.wide_dense = wt.dense;
    if (wt.attempt) wide_pool_attempt(wide_want);
    f.wide_have = g_ctx.d_wide.cap / PV_WIDE_TABLE_BYTES;
    p = pvhost::plan_chunk(batch, f);
    const uint32_t* kc_flags;
    apply_plan(p, kw, kcv, xtv, kc_flags);
    if (p.keyed) {
        L.gate = Gate{kw.nkeys, kw.slot_req};
        if ((rc = launch_key_stage(L, kcv, xtv, kc_flags))) return rc;
    }
    if ((rc = L.mark(PV_STAGE_PREP))) return rc;
    if (p.keyed) {
        if ((rc = launch_straus_side(L)) || (rc = launch_comb_stage(L))) return rc;
    } else {
        if ((rc = launch_straus_only(L))) return rc;
    }
    if ((rc = L.mark(PV_STAGE_ENCODE))) return rc;
    if ((rc = launch_epilogue(L))) return rc;
    return L.mark(PV_NSTAGES);
}

int launch_chunks(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk, uint64_t* d_verdict,
                  hipStream_t stream) {
    const uint64_t cap = g_ctx.work.stride;
    const int nchunks = (int)((n + cap - 1) / cap);
    constexpr int NE = PV_NSTAGES + 1;
    const pvhost::BatchPlan batch =
        pvhost::plan_batch({g_ctx.path, n, g_ctx.hint_set, g_ctx.keyed_hint, kc_view().hmask != 0});
    g_ctx.last_latency = batch.latency;
    g_ctx.last_dev_choice = batch.dev_choice;
    int evb = 0;
    if (g_ctx.timing) {
        evb = g_ctx.ev_used;
        int rc = ensure_events(evb + NE * nchunks);
        if (rc) return rc;
        g_ctx.ev_used = evb + NE * nchunks;
    }
    int rc = PV_OK;
    for (int c = 0; c < nchunks && rc == PV_OK; c++)
        rc = launch_chunk(c, n, d_sm, d_off, d_pk, d_verdict, stream, batch, evb);
    return rc;
}

// The per-lane workspace: per-request rows (Work) and the keyed path's tables (KeyWork), ~15 GB, owned
// by the context (Work::qb is never allocated: it only keeps the kernel-argument layout).
int lane_alloc_buffers(Work& w, KeyWork& kw) {
    PvOwner& own = g_ctx.own;
    const uint64_t S = PV_CHUNK;
    w.stride = S;
    if (int rc = own.dev(w.atab, S * PV_ATAB_ENT * 160)) return rc;
    if (int rc = own.dev(w.digits, S * PV_DIGIT_ROWS * 4)) return rc;
    if (int rc = own.dev(w.flags, S * 4)) return rc;
    if (int rc = own.dev(w.q, S * 40 * 4)) return rc;
    if (int rc = own.dev(w.aos, S * PV_PREP_AOS_QMAX * 16)) return rc;
    const uint64_t H = 2 * S;
    kw.hmask = (uint32_t)(H - 1);
    kw.kcap = PV_KEY_CAP;
    kw.seed = (uint32_t)std::random_device{}() | 1u;
    if (int rc = own.dev(kw.slot, H * 4)) return rc;
    if (int rc = own.dev(kw.slot_id, H * 4)) return rc;
    if (int rc = own.dev(kw.slot_cnt, H * 4 * PV_RANK_SUB)) return rc;
    if (int rc = own.dev(kw.req_key, S * 4)) return rc;
    if (int rc = own.dev(kw.req_rank, S * 4)) return rc;
    if (int rc = own.dev(kw.nkeys, PV_SPLIT_ALLOC_WORDS * 4)) return rc;
    if (int rc = own.dev(kw.key_owner, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.key_cid, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.comb_key, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.key_flag, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.bases, (uint64_t)kw.kcap * PV_COMB_POS * PV_COMB_PTS * 160)) return rc;
    if (int rc = own.dev(kw.ctab, (uint64_t)kw.kcap * PV_COMB_POS * PV_COMB_ENT * 160)) return rc;
    if (int rc = own.dev(kw.key_count, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.key_cursor, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.slot_req, S * 4)) return rc;
    if (int rc = own.dev(kw.req_pos, S * 4)) return rc;
    if (int rc = own.dev(kw.skey, S * 4)) return rc;
    if (int rc = own.dev(kw.sverdict, S / 64 * 8)) return rc;
    if (int rc = own.dev(kw.key_cslot, (S + 64 * PV_NSEG) * 4)) return rc;  // key ids: segment-major
    if (int rc = own.dev(kw.comb_cslot, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.need, (uint64_t)PV_ALLCOMB_KEYS * PV_COMB_POS * 5 * 4)) return rc;
    PV_HIP(hipMemset(kw.comb_cslot, 0xFF, (uint64_t)kw.kcap * 4), PV_ERR_ALLOC);
    if (int rc = own.dev(kw.comb_tslot, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.dir_htab, (uint64_t)PV_DIR_HASH * 4)) return rc;
    if (int rc = own.dev(kw.dir_keys, (uint64_t)kw.kcap * 32)) return rc;
    if (int rc = own.dev(kw.dir_flags, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.dir_cnt, 2 * 4)) return rc;
    if (int rc = own.dev(kw.dir_stat, PV_DIR_STATS * 8)) return rc;
    if (int rc = own.dev(kw.aff_list, (uint64_t)PV_AFF_CAP * 4)) return rc;
    if (int rc = own.dev(kw.aff_cnt, 4)) return rc;
    if (int rc = own.dev(kw.wide_list, (uint64_t)PV_WIDE_CAP * 2 * 4)) return rc;
    if (int rc = own.dev(kw.wide_cnt, 2 * 4)) return rc;
    if (int rc = own.dev(kw.dir_wslot, (uint64_t)kw.kcap * 4)) return rc;
    if (int rc = own.dev(kw.comb_wslot, (uint64_t)kw.kcap * 4)) return rc;
    PV_HIP(hipMemset(kw.wide_cnt, 0, 2 * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.comb_wslot, 0xFF, (uint64_t)kw.kcap * 4), PV_ERR_ALLOC);
    if (int rc = own.dev(kw.aff_scr, (uint64_t)PV_AFF_CAP * PV_AFF_SEG * 10 * PV_AFF_THREADS * 4)) return rc;
    PV_HIP(hipMemset(kw.aff_cnt, 0, 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.comb_tslot, 0, (uint64_t)kw.kcap * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.dir_htab, 0xFF, (uint64_t)PV_DIR_HASH * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.dir_cnt, 0, 2 * 4), PV_ERR_ALLOC);
    PV_HIP(hipMemset(kw.dir_stat, 0, PV_DIR_STATS * 8), PV_ERR_ALLOC);
    return PV_OK;
}

// Builds g_ctxs[device] (caller: g_mus[device] held, DevScope(device) active, context not built yet):
// streams and events, the fixed-base tables, the workspace. Sets the calling thread's HIP device.
bool env_flag_devscope() {
    const char* e = getenv("PV_EVENT_DEVSCOPE");
    return !(e && *e == '0');
}

int ctx_init_parts(int device) {
    PV_HIP(hipSetDevice(device), PV_ERR_NO_DEVICE);
    hipDeviceProp_t prop;
    PV_HIP(hipGetDeviceProperties(&prop, device), PV_ERR_NO_DEVICE);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PV_ERR_NO_DEVICE, std::string("pv_init: built for gfx950, device is ") + prop.gcnArchName);
    g_ctx.cus = prop.multiProcessorCount;
    PvOwner& own = g_ctx.own;
    if (int rc = own.stream(g_ctx.stream, hipStreamNonBlocking)) return rc;
    if (int rc = own.stream(g_ctx.kstream, hipStreamNonBlocking)) return rc;
    // stream-to-stream hand-overs inside the engine (one device, never read by the host) are recorded with
    // a device-scope release instead of the default system-scope fence: headline step 2.612-2.618 against
    // 2.620-2.624 ms interleaved (profiles/r05/ab_event_devscope.txt); PV_EVENT_DEVSCOPE=0 restores it
    const unsigned evf = hipEventDisableTiming | (env_flag_devscope() ? hipEventReleaseToDevice : 0u);
    if (int rc = own.event(g_ctx.ev_keys_ready, evf)) return rc;
    if (int rc = own.event(g_ctx.ev_scan_done, evf)) return rc;
    if (int rc = own.event(g_ctx.ev_tables_ready, evf)) return rc;
    if (int rc = own.stream(g_ctx.fstream, hipStreamNonBlocking)) return rc;
    if (int rc = own.event(g_ctx.ev_chain, evf)) return rc;
    if (int rc = own.event(g_ctx.ev_prep_done, evf)) return rc;
    if (int rc = own.stream(g_ctx.sstream, hipStreamNonBlocking)) return rc;
    if (int rc = own.event(g_ctx.ev_straus_done, evf)) return rc;
    if (int rc = g_ctx.hand.ensure()) return rc;
    {
        // the host path's copy stream at the greatest priority: the runtime keeps such streams on hardware
        // queues of their own instead of round-robin over GPU_MAX_HW_QUEUES (4) with the engine's streams,
        // where a copy sat behind the key stream's table fill (profiles/r05/host_path)
        int least = 0, greatest = 0;
        PV_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest), PV_ERR_NO_DEVICE);
        const char* pe = getenv("PV_CSTREAM_PRIO");  // A/B knob: 0 = normal priority
        const bool hi = !(pe && *pe == '0');
        if (int rc = own.stream(g_ctx.cstream, hipStreamNonBlocking, hi ? greatest : least)) return rc;
    }
    if (int rc = own.event(g_ctx.ev_cstart, hipEventDisableTiming)) return rc;
    std::vector<uint32_t> bt(PV_BTAB_ENTRIES * PV_BTAB_STRIDE);
    pv_build_b_table(bt.data());
    if (int rc = own.dev(g_ctx.d_btab, bt.size() * 4)) return rc;
    PV_HIP(hipMemcpy(g_ctx.d_btab, bt.data(), bt.size() * 4, hipMemcpyHostToDevice), PV_ERR_ALLOC);
    {
        if (int rc = lane_alloc_buffers(g_ctx.work, g_ctx.kw)) return rc;
        std::vector<uint32_t> bc((size_t)PV_BCOMB_POS * PV_BCOMB_ENT * PV_BCOMB_STRIDE);
        {
            ge_p3 base[PV_BCOMB_POS];
            pv_bcomb_bases(base);
            std::vector<std::thread> th;
            for (int j = 0; j < PV_BCOMB_POS; j++)
                th.emplace_back(pv_bcomb_build_position, bc.data() + (size_t)j * PV_BCOMB_ENT * PV_BCOMB_STRIDE,
                                std::cref(base[j]));
            for (auto& t : th) t.join();
        }
        if (int rc = own.dev(g_ctx.d_bcomb, bc.size() * 4)) return rc;
        PV_HIP(hipMemcpy(g_ctx.d_bcomb, bc.data(), bc.size() * 4, hipMemcpyHostToDevice), PV_ERR_ALLOC);
        // the wide fixed-base comb, built on the device row by row (one scratch row of Z products)
        {
            const uint64_t rows_ent = (uint64_t)(PV_BC2_POS - 1) * PV_BC2_ENT + PV_BC2_TOP_ENT;
            // not enough HBM for the wide table (a smaller part, several processes on one GPU) or
            // PV_FORCE_BCOMB16 set: [S]B from the radix-65536 comb T_B instead (16 lookups instead of
            // 11, same verdicts; profiles/r02/ab_bcomb_radix.txt: ~2 % slower per step)
            const char* force16 = getenv("PV_FORCE_BCOMB16");
            if (PV_BC2_W == 16 || (force16 && *force16 && *force16 != '0') ||
                own.dev(g_ctx.d_bc2, rows_ent * PV_BCOMB_STRIDE * 4) != PV_OK) {
                (void)hipGetLastError();  // clear a failed allocation's sticky error
                g_ctx.d_bc2 = g_ctx.d_bcomb;  // an alias: the owner holds the one block
                g_ctx.bc2_w = 16;
            }
        }
        if (g_ctx.bc2_w != 16) {
            uint32_t* scratch = nullptr;
            PV_HIP(hipMalloc((void**)&scratch, (uint64_t)PV_BC2_ENT * 40), PV_ERR_ALLOC);
            ge_p3 negB, P;
            ge_frombytes_negate(negB, PV_B_ENC);
            P = negB;
            fe z;
            fe_0(z);
            fe_sub(P.X, z, negB.X);
            fe_carry(P.X, P.X);
            fe_sub(P.T, z, negB.T);
            fe_carry(P.T, P.T);
            int rc = PV_OK;
            for (int j = 0; j < PV_BC2_POS && rc == PV_OK; j++) {
                PvPoint40 arg;
                ge_p3_store_words(arg.w, P);
                const uint32_t ent = j + 1 < PV_BC2_POS ? PV_BC2_ENT : PV_BC2_TOP_ENT;
                const uint32_t threads = (ent + PV_BC2_RUN - 1) / PV_BC2_RUN;
                hipLaunchKernelGGL(pv_bc2_build_kernel, dim3((threads + PV_BLOCK - 1) / PV_BLOCK), dim3(PV_BLOCK), 0,
                                   g_ctx.stream, g_ctx.d_bc2 + (uint64_t)j * PV_BC2_ENT * (PV_BCOMB_STRIDE / 4), ent,
                                   arg, scratch);
                if (hipGetLastError() != hipSuccess || hipStreamSynchronize(g_ctx.stream) != hipSuccess)
                    rc = fail(PV_ERR_LAUNCH, "pv_init: wide fixed-base comb build failed");
                for (int r = 0; r < PV_BC2_W; r++) {  // next row's base: 2^W P
                    ge_p1p1 t;
                    ge_p2_dbl(t, P.X, P.Y, P.Z);
                    ge_p1p1_to_p3(P, t);
                }
            }
            (void)hipFree(scratch);
            if (rc != PV_OK) return rc;
        }
    }
    if (int rc = own.pinned(g_ctx.h_zc_verdict, PV_ZC_MAX_REQ, hipHostMallocCoherent | hipHostMallocPortable)) return rc;
    if (const char* pad = getenv("PV_PREP_LDS_PAD")) g_ctx.prep_lds_pad = (uint32_t)atoi(pad);  // A/B knob
    {  // PV_TABLE_REUSE=0: start with table reuse off (pv_table_reuse), every keyed chunk builds its tables
        const char* tr = getenv("PV_TABLE_REUSE");
        g_ctx.dir_on = !(tr && *tr == '0');
        g_ctx.dir_cap = PV_DIR_DEFAULT_CAP;
        g_ctx.dir_dirty = true;
        const char* ta = getenv("PV_TABLE_AFFINE");  // PV_TABLE_AFFINE=0: resident tables stay in cached form
        g_ctx.aff_on = !(ta && *ta == '0');
        const char* tw = getenv("PV_TABLE_WIDE");  // PV_TABLE_WIDE=0: resident tables get no radix-2^11 rows
        g_ctx.wide_cap = tw && *tw == '0' ? 0u : PV_WIDE_DEFAULT;
    }
    g_ctx.device = device;
    return PV_OK;
}

// Frees g_ctxs[t_dev or primary] (caller holds its mutex).
void ctx_free() {
    if (g_ctx.device < 0) return;
    (void)hipSetDevice(g_ctx.device);
    if (g_ctx.comm) ncclCommDestroy(g_ctx.comm);
    kc_free();  // first: it waits for a pending asynchronous put
    for (PvDevBuf* b : {&g_ctx.d_mg, &g_ctx.d_stage, &g_ctx.sg.d_keys, &g_ctx.sg.d_sk, &g_ctx.d_wide, &g_ctx.d_wide_scr})
        b->release();
    for (PvPinnedBuf* b : {&g_ctx.h_mg, &g_ctx.h_stage, &g_ctx.h_ver, &g_ctx.sg.h_sk}) b->release();
    g_ctx.sg.stage.release();
    g_ctx.hand.destroy();
    g_ctx.sg.hand.destroy();
    g_ctx.own.release_all();
    g_ctx = Ctx();
}

}  // namespace

// What the engine's other translation units call (declared in pv_ctx.h).

// Builds the tables of a put's fresh keys (slot PV_KC_EMPTY = evicted again within the same put) into
// their cache slots, in batches of the workspace's comb capacity. async: one batch only (the caller caps
// the keys), staged through the pinned h_async area and left running on the engine stream (the
// next launch is stream-ordered after it). PV_TEST_FAIL_KC_PUT_BATCH=b (tests only) reports a
// failure after batch b has been enqueued, to exercise the rollback.
int kc_build_tables(const pvhost::KcIndex::Assigned& put, bool async) {
    auto& k = g_ctx.kc;
    hipStream_t s = g_ctx.stream;
    if (int rc = g_ctx.hand.begin(s)) return rc;
    const char* fail_env = getenv("PV_TEST_FAIL_KC_PUT_BATCH");
    const long fail_batch = fail_env ? atol(fail_env) : -1;
    KeyWork kw = g_ctx.kw;
    // the put builds comb index j's table in slot j of a scratch area: the part of ctab above the slots
    // the resident-table directory may list when the batch fits there, else over the directory
    constexpr uint64_t tab_q = (uint64_t)PV_COMB_POS * PV_COMB_ENT * 10;  // uint4 per table
    uint4* const scratch_tab = g_ctx.kw.ctab + g_ctx.dir_cap * tab_q;
    const uint32_t scratch_keys = kw.kcap - g_ctx.dir_cap;
    std::vector<uint8_t> lpk;
    std::vector<uint32_t> lslot;
    long batch = 0;
    for (size_t f0 = 0; f0 < put.fresh.size();) {
        uint8_t* bpk;
        uint32_t* bslot;
        if (async) {  // pinned: keys [kcap][32], then slots [kcap]
            bpk = k.h_async;
            bslot = reinterpret_cast<uint32_t*>(k.h_async + (uint64_t)kw.kcap * 32);
        } else {
            lpk.resize((uint64_t)kw.kcap * 32);
            lslot.resize(kw.kcap);
            bpk = lpk.data();
            bslot = lslot.data();
        }
        uint32_t m;
        f0 = pvhost::KcIndex::pack(put, f0, kw.kcap, bpk, bslot, m);
        if (m == 0) continue;
        if (async && f0 < put.fresh.size()) return fail(PV_ERR_ARG, "kc_build_tables: asynchronous put above one batch");
        if (g_ctx.dir_on && m <= scratch_keys) {
            kw.ctab = scratch_tab;
        } else {
            kw.ctab = g_ctx.kw.ctab;
            g_ctx.dir_dirty = true;
        }
        PV_HIP(hipMemcpyAsync(k.d_put_pk, bpk, 32ull * m, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
        PV_HIP(hipMemcpyAsync(k.d_put_slot, bslot, (uint64_t)m * 4, hipMemcpyHostToDevice, s), PV_ERR_LAUNCH);
        PV_LAUNCH(pv_kc_put_prep_kernel, dim3((m + PV_BLOCK - 1) / PV_BLOCK), dim3(PV_BLOCK), 0, s, kw, m);
        const Gate gate{kw.nkeys, kw.slot_req};
        PV_LAUNCH(pv_key_chain_lp_kernel, dim3(pvhost::chain_blocks(m)), dim3(64), 0, s, k.d_put_pk, kw, gate, 0,
                  PV_COMB_POS);
        PV_LAUNCH(pv_key_fill_kernel, dim3(pvhost::fill_grid(m)), dim3(PV_BLOCK), 0, s, kw, gate, 0, PV_COMB_POS);
        PV_LAUNCH(pv_kc_scatter_kernel, dim3(64, m), dim3(PV_BLOCK), 0, s, kw.ctab, kw.key_flag, k.d_put_pk,
                  k.d_put_slot, m, k.d_tab, k.d_flags, k.d_keys);
        if (k.d_ntab) {
            PV_LAUNCH(pv_kc_affine_kernel, dim3((m * PV_COMB_POS + 63) / 64), dim3(64), 0, s, k.d_tab,
                      k.d_put_slot, m, k.d_ntab);
        }
        if (k.d_wtab) {
            bool any = false;
            for (uint32_t j = 0; j < m && !any; j++) any = bslot[j] < k.wcap;
            for (uint32_t j0 = 0; any && j0 < m; j0 += PV_KW_GROUP) {
                const uint32_t g = std::min<uint32_t>(PV_KW_GROUP, m - j0);
                const uint64_t threads = (uint64_t)g * PV_KW_POS * PV_KW_RUNS;
                PV_LAUNCH(pv_kc_wide_kernel, dim3((unsigned)((threads + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK),
                          0, s, kw, k.d_put_slot, j0, g, k.wcap, k.d_wtab, k.d_wscr);
            }
        }
        if (!async) PV_HIP(hipStreamSynchronize(s), PV_ERR_LAUNCH);  // bpk / bslot are host locals
        if (batch++ == fail_batch) return fail(PV_ERR_LAUNCH, "pv_key_cache_put: injected failure (PV_TEST_FAIL_KC_PUT_BATCH)");
    }
    return PV_OK;
}

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// One batch on `stream` (caller holds g_mu). Chunks of at most work.stride requests (a multiple of
// 64, so verdict words never straddle).
int launch(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk, uint64_t* d_verdict,
           hipStream_t stream) {
    if (n == 0) return PV_OK;
    int rc = g_ctx.hand.begin(stream);
    if (rc) return rc;
    rc = launch_chunks(d_sm, d_off, n, d_pk, d_verdict, stream);
    // recorded even after a failed enqueue: whatever did get enqueued is covered
    if (int rc2 = g_ctx.hand.end(stream)) return rc2;
    return rc;
}

int check_device_index(int device, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(PV_ERR_NO_DEVICE, std::string(who) + ": no HIP device visible");
    if (device < 0 || device >= ndev || device >= PV_MAX_DEV)
        return fail(PV_ERR_ARG, std::string(who) + ": device index out of range");
    return PV_OK;
}

// ctx_init_parts, and on failure everything it had built is released (streams, events, the workspace,
// the tables): a retry of pv_init / pv_init_devices starts from an empty context instead of allocating
// ~25 GB on top of a half-built one.
int ctx_init(int device) {
    const int rc = ctx_init_parts(device);
    if (rc != PV_OK) {
        const std::string err = g_err;
        g_ctx.device = device;  // ctx_free releases a context of a known device
        ctx_free();
        g_err = err;
    }
    return rc;
}

hipStream_t pv_engine_stream() { return g_ctx.stream; }
int pv_fail(int code, const std::string& msg) { return fail(code, msg); }

extern "C" {

int pv_abi_version(void) { return PV_ABI_VERSION; }
uint32_t pv_build_flags(void) { return PV_BUILD_COMB_FUSED; }

int pv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* pv_last_error(void) { return g_err.c_str(); }

int pv_init(int device) {
    const int p = g_primary.load();
    if (p == device) {
        PV_HIP(hipSetDevice(device), PV_ERR_NO_DEVICE);  // this thread's device as well
        return PV_OK;
    }
    if (p >= 0) return fail(PV_ERR_ARG, "pv_init: already bound to another device");
    int rc = check_device_index(device, "pv_init");
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mus[device]);
        DevScope ds(device);
        if (g_ctx.device != device && (rc = ctx_init(device)) != PV_OK) return rc;
    }
    PV_HIP(hipSetDevice(device), PV_ERR_NO_DEVICE);
    g_primary.store(device);
    return PV_OK;
}

void pv_shutdown(void) {
    pinned_cache_drain();  // freed pv_host_alloc blocks back to the system (live ones stay the caller's)
    pv_ingress_shutdown();
    pv_merkle_shutdown();
    pv_trie_shutdown();
    {
        std::lock_guard<std::mutex> lk(g_mg_mu);
        mg_destroy_comms();
    }
    for (int d = 0; d < PV_MAX_DEV; d++) {
        std::lock_guard<std::mutex> lk(g_mus[d]);
        DevScope ds(d);
        ctx_free();
    }
    const int p = g_primary.exchange(-1);
    if (p >= 0) (void)hipSetDevice(p);
}

int pv_last_path(int* path, uint32_t* nkeys) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_last_path: call pv_init first");
    uint32_t u[PV_SPLIT_WORDS] = {};
    if (g_ctx.last_keyed) {
        PV_HIP(hipStreamSynchronize(g_ctx.stream), PV_ERR_LAUNCH);
        PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
        PV_HIP(hipMemcpy(u, g_ctx.last_nkeys ? g_ctx.last_nkeys : g_ctx.kw.nkeys, sizeof(u), hipMemcpyDeviceToHost),
               PV_ERR_LAUNCH);
    }
    if (nkeys) *nkeys = u[PV_SPLIT_KEYS];
    const bool lat = g_ctx.last_latency || (g_ctx.last_keyed && u[PV_SPLIT_LAT] != 0);
    if (path) *path = lat ? PV_PATH_LATENCY : u[PV_SPLIT_SLOTS] > 0 ? PV_PATH_COMB : PV_PATH_STRAUS;
    g_ctx.last_split[0] = u[PV_SPLIT_KEYS];
    g_ctx.last_split[1] = u[PV_SPLIT_COMB_KEYS];
    g_ctx.last_split[2] = u[PV_SPLIT_SLOTS];
    return PV_OK;
}

int pv_last_split(uint32_t* keys, uint32_t* comb_keys, uint32_t* comb_requests) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_last_split: call pv_init first");
    if (keys) *keys = g_ctx.last_split[0];
    if (comb_keys) *comb_keys = g_ctx.last_split[1];
    if (comb_requests) *comb_requests = g_ctx.last_split[2];
    return PV_OK;
}

int pv_set_path(int mode) {
    if (mode != PV_PATH_AUTO && mode != PV_PATH_STRAUS && mode != PV_PATH_COMB && mode != PV_PATH_LATENCY)
        return fail(PV_ERR_ARG, "pv_set_path: unknown mode");
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        g_ctxs[d].path = mode;
    }
    return PV_OK;
}

int pv_table_reuse(int on, uint32_t capacity) {
    const uint32_t cap = std::min<uint32_t>(capacity, PV_KEY_CAP);
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        Ctx& c = g_ctxs[d];
        const bool want = on != 0;
        if (want != c.dir_on || (cap && cap != c.dir_cap)) c.dir_dirty = true;  // emptied before its next use
        c.dir_on = want;
        if (cap) c.dir_cap = cap;
    }
    return PV_OK;
}

int pv_table_reuse_stats(uint64_t* hits, uint64_t* built, uint64_t* resets) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_table_reuse_stats: call pv_init first");
    unsigned long long u[3] = {0, 0, 0};
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpy(u, g_ctx.kw.dir_stat, sizeof(u), hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    if (hits) *hits = u[0];
    if (built) *built = u[1];
    if (resets) *resets = u[2];
    return PV_OK;
}

int pv_table_affine(int on) {
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        Ctx& c = g_ctxs[d];
        const bool want = on != 0;
        if (want != c.aff_on) c.dir_dirty = true;  // emptied before its next use: never half in one regime
        c.aff_on = want;
    }
    return PV_OK;
}

int pv_table_affine_stats(uint64_t* converted, uint64_t* affine_reads) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_table_affine_stats: call pv_init first");
    unsigned long long u[5] = {0, 0, 0, 0, 0};
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpy(u, g_ctx.kw.dir_stat, sizeof(u), hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    if (converted) *converted = u[3];
    if (affine_reads) *affine_reads = u[4];
    return PV_OK;
}

int pv_table_wide(uint32_t capacity) {
    for (int d = 0; d < PV_MAX_DEV; d++) {  // every device context of the process
        std::lock_guard<std::mutex> lk(g_mus[d]);
        Ctx& c = g_ctxs[d];
        if (capacity != c.wide_cap) c.dir_dirty = true;  // emptied before its next use, and the pool with it
        c.wide_cap = capacity;
        if (capacity) c.wide_failed = false;  // a new capacity may fit where the last one did not
    }
    return PV_OK;
}

int pv_table_wide_stats(uint64_t* widened, uint64_t* wide_reads) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_table_wide_stats: call pv_init first");
    unsigned long long u[PV_DIR_STATS] = {};
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpy(u, g_ctx.kw.dir_stat, sizeof(u), hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    if (widened) *widened = u[5];
    if (wide_reads) *wide_reads = u[6];
    return PV_OK;
}

int pv_set_timing(int enable) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_ctx.timing = enable != 0;
    g_ctx.ev_used = 0;
    return PV_OK;
}

int pv_stage_times(double* ms, int max_stages, int* launches) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_stage_times: call pv_init first");
    constexpr int NE = PV_NSTAGES + 1;
    double acc[PV_NSTAGES] = {0};
    const int nq = g_ctx.ev_used / NE;
    for (int c = 0; c < nq; c++) {
        hipEvent_t* e = &g_ctx.ev[NE * c];
        PV_HIP(hipEventSynchronize(e[PV_NSTAGES]), PV_ERR_LAUNCH);
        for (int k = 0; k < PV_NSTAGES; k++) {
            float t = 0;
            PV_HIP(hipEventElapsedTime(&t, e[k], e[k + 1]), PV_ERR_LAUNCH);
            acc[k] += t;
        }
    }
    for (int k = 0; k < max_stages && k < PV_NSTAGES; k++) ms[k] = acc[k];
    if (launches) *launches = nq;
    return PV_OK;
}

int pv_kernel_times(double* prep_ms, double* table_ms, double* msm_ms, int* launches) {
    double t[PV_NSTAGES];
    const int rc = pv_stage_times(t, PV_NSTAGES, launches);
    if (rc) return rc;
    if (prep_ms) *prep_ms = t[PV_STAGE_KEYS] + t[PV_STAGE_PREP];
    if (table_ms) *table_ms = t[PV_STAGE_TABLE];
    if (msm_ms) *msm_ms = t[PV_STAGE_MSM] + t[PV_STAGE_ENCODE];
    return PV_OK;
}

int pv_verify_batch_device(const uint8_t* d_sm, const uint64_t* d_off, uint64_t n, const uint8_t* d_pk,
                           uint64_t* d_verdict_words, void* stream) {
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_verify_batch_device: call pv_init first");
    if (n > 0 && (!d_sm || !d_off || !d_pk || !d_verdict_words)) return fail(PV_ERR_ARG, "null pointer");
    std::lock_guard<std::mutex> lk(g_mu);
    return launch(d_sm, d_off, n, d_pk, d_verdict_words, stream ? (hipStream_t)stream : g_ctx.stream);
}

int pv_test_clock_stamps(uint64_t* out, uint32_t max_blocks) {
#if PV_CLOCK_PROBE
    const uint32_t k = std::min<uint32_t>(max_blocks, PV_CLOCK_SLOTS);
    if (!out || k == 0) return (int)PV_CLOCK_SLOTS;
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    PV_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(pv_clock_stamps), (size_t)k * 32, 0, hipMemcpyDeviceToHost), PV_ERR_LAUNCH);
    return (int)k;
#else
    (void)out;
    (void)max_blocks;
    return 0;
#endif
}

int pv_sync(void) {
    PV_HIP(hipDeviceSynchronize(), PV_ERR_LAUNCH);
    return PV_OK;
}

int pv_stream_create(void** stream) {
    if (!stream) return fail(PV_ERR_ARG, "pv_stream_create: null pointer");
    hipStream_t s = nullptr;
    PV_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), PV_ERR_NO_DEVICE);
    *stream = (void*)s;
    return PV_OK;
}
int pv_stream_destroy(void* stream) {
    if (!stream) return PV_OK;
    PV_HIP(hipStreamSynchronize((hipStream_t)stream), PV_ERR_LAUNCH);
    {
        // a later launch must not wait on an event of a destroyed stream
        std::lock_guard<std::mutex> lk(g_mu);
        g_ctx.hand.forget((hipStream_t)stream);
        g_ctx.sg.hand.forget((hipStream_t)stream);
    }
    pv_ingress_forget_stream(stream);
    pv_merkle_forget_stream(stream);
    pv_trie_forget_stream(stream);
    PV_HIP(hipStreamDestroy((hipStream_t)stream), PV_ERR_LAUNCH);
    return PV_OK;
}
int pv_stream_sync(void* stream) {
    PV_HIP(hipStreamSynchronize(stream ? (hipStream_t)stream : g_ctx.stream), PV_ERR_LAUNCH);
    return PV_OK;
}

}  // extern "C"
