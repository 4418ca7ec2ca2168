// libplenum_verify: RCCL and in-process multi-GPU entries. pv_comm_* gathers verdict words between the
// ranks of a multi-process run; pv_init_devices builds one device context per GPU of this process
// (pv_engine.hip ctx_init) and pv_verify_batch_multi_gpu shards a host-buffer batch over them (pv_host.hip
// stage_and_launch on each), one all-gather bringing the verdict words together. No kernel is defined here.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pv_ctx.h"
#include "../../include/plenum_verify.h"

namespace {

// In-process multi-GPU state (pv_init_devices): the devices in mask order and one RCCL communicator
// per device from ncclCommInitAll (a single-process clique).
struct MultiGpu {
    std::vector<int> devs;
    std::vector<ncclComm_t> comms;
};
MultiGpu g_mg;

}  // namespace

// pv_shutdown (pv_engine.hip) destroys the communicators too (declared in pv_ctx.h).
std::mutex g_mg_mu;

void mg_destroy_comms() {
    for (ncclComm_t c : g_mg.comms)
        if (c) ncclCommDestroy(c);
    g_mg.comms.clear();
    g_mg.devs.clear();
}

extern "C" {

int pv_comm_unique_id(uint8_t out[128]) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return fail(PV_ERR_COMM, "ncclGetUniqueId failed");
    static_assert(sizeof(id.internal) == 128, "ncclUniqueId size");
    memcpy(out, id.internal, 128);
    return PV_OK;
}

int pv_comm_init(int nranks, int rank, const uint8_t id_bytes[128]) {
    if (g_ctx.device < 0) return fail(PV_ERR_NOT_INIT, "pv_comm_init: call pv_init first");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PV_ERR_ARG, "pv_comm_init: bad rank");
    ncclUniqueId id;
    memcpy(id.internal, id_bytes, 128);
    ncclResult_t r = ncclCommInitRank(&g_ctx.comm, nranks, id, rank);
    if (r != ncclSuccess) return fail(PV_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    g_ctx.nranks = nranks;
    g_ctx.rank = rank;
    return PV_OK;
}

int pv_allgather_verdicts(const uint64_t* d_local, uint64_t words_per_rank, uint64_t* d_all, void* stream) {
    if (!g_ctx.comm) return fail(PV_ERR_NOT_INIT, "pv_allgather_verdicts: call pv_comm_init first");
    ncclResult_t r = ncclAllGather(d_local, d_all, words_per_rank, ncclUint64, g_ctx.comm,
                                   stream ? (hipStream_t)stream : g_ctx.stream);
    if (r != ncclSuccess) return fail(PV_ERR_COMM, std::string("ncclAllGather: ") + ncclGetErrorString(r));
    return PV_OK;
}

int pv_comm_count(int* nranks, int* rank) {
    if (!g_ctx.comm) return fail(PV_ERR_NOT_INIT, "pv_comm_count: call pv_comm_init first");
    int c = 0, r = -1;
    ncclResult_t e = ncclCommCount(g_ctx.comm, &c);
    if (e == ncclSuccess) e = ncclCommUserRank(g_ctx.comm, &r);
    if (e != ncclSuccess) return fail(PV_ERR_COMM, std::string("ncclCommCount / ncclCommUserRank: ") + ncclGetErrorString(e));
    if (nranks) *nranks = c;
    if (rank) *rank = r;
    return PV_OK;
}

void pv_comm_destroy(void) {
    if (g_ctx.comm) ncclCommDestroy(g_ctx.comm);
    g_ctx.comm = nullptr;
}

int pv_shard_plan(uint64_t n, int ndev, uint64_t* bounds, uint64_t* words_per_shard) {
    if (ndev < 1 || ndev > PV_MAX_DEV || !bounds || !words_per_shard) return fail(PV_ERR_ARG, "pv_shard_plan: bad arguments");
    // whole 64-request verdict words per shard (sharding.py shard_bounds): word ranges
    // [words r / G, words (r + 1) / G), so every shard but the last is a multiple of 64 requests
    const uint64_t words = (n + 63) / 64;
    uint64_t wmax = 0;
    for (int r = 0; r <= ndev; r++) bounds[r] = std::min<uint64_t>(n, 64 * (words * (uint64_t)r / (uint64_t)ndev));
    for (int r = 0; r < ndev; r++)
        wmax = std::max<uint64_t>(wmax, words * (uint64_t)(r + 1) / ndev - words * (uint64_t)r / ndev);
    *words_per_shard = wmax;
    return PV_OK;
}

int pv_init_devices(uint32_t device_mask) {
    std::vector<int> devs;
    for (int d = 0; d < PV_MAX_DEV; d++)
        if ((device_mask >> d) & 1u) devs.push_back(d);
    if (devs.empty() || (device_mask >> PV_MAX_DEV) != 0) return fail(PV_ERR_ARG, "pv_init_devices: bad device mask");
    for (int d : devs) {
        const int rc = check_device_index(d, "pv_init_devices");
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> mg(g_mg_mu);
    // the missing contexts are built in parallel, one host thread per device (tables built on each GPU)
    std::vector<int> rcs(devs.size(), PV_OK);
    std::vector<std::string> errs(devs.size());
    {
        std::vector<std::thread> th;
        for (size_t i = 0; i < devs.size(); i++)
            th.emplace_back([&, i] {
                const int d = devs[i];
                std::lock_guard<std::mutex> lk(g_mus[d]);
                DevScope ds(d);
                if (g_ctx.device != d && (rcs[i] = ctx_init(d)) != PV_OK) errs[i] = g_err;
            });
        for (auto& t : th) t.join();
    }
    for (size_t i = 0; i < devs.size(); i++)
        if (rcs[i]) return fail(rcs[i], "pv_init_devices: device " + std::to_string(devs[i]) + ": " + errs[i]);
    if (g_mg.devs != devs) {
        mg_destroy_comms();
        int cur = 0;
        (void)hipGetDevice(&cur);
        std::vector<ncclComm_t> comms(devs.size(), nullptr);
        const ncclResult_t r = ncclCommInitAll(comms.data(), (int)devs.size(), devs.data());
        (void)hipSetDevice(cur);  // the caller's current device is unchanged
        if (r != ncclSuccess) return fail(PV_ERR_COMM, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
        g_mg.comms = comms;
        g_mg.devs = devs;
    }
    return PV_OK;
}

int pv_multi_gpu_devices(int* devices, int max_devices) {
    std::lock_guard<std::mutex> mg(g_mg_mu);
    for (int i = 0; i < (int)g_mg.devs.size() && i < max_devices && devices; i++) devices[i] = g_mg.devs[i];
    return (int)g_mg.devs.size();
}

int pv_multi_gpu_comm_ranks(int* nranks, int* ranks, int max_devices) {
    std::lock_guard<std::mutex> mg(g_mg_mu);
    if (g_mg.comms.empty()) return fail(PV_ERR_NOT_INIT, "pv_multi_gpu_comm_ranks: call pv_init_devices first");
    int c = 0;
    ncclResult_t e = ncclCommCount(g_mg.comms[0], &c);
    for (int i = 0; e == ncclSuccess && i < (int)g_mg.comms.size() && i < max_devices && ranks; i++)
        e = ncclCommUserRank(g_mg.comms[i], &ranks[i]);
    if (e != ncclSuccess) return fail(PV_ERR_COMM, std::string("ncclCommCount / ncclCommUserRank: ") + ncclGetErrorString(e));
    if (nranks) *nranks = c;
    return PV_OK;
}

int pv_verify_batch_multi_gpu(const uint8_t* sm, const uint64_t* sm_off, uint64_t n, const uint8_t* pk,
                              uint8_t* verdict_bits) {
    if (n == 0) return PV_OK;
    if (!sm || !sm_off || !pk || !verdict_bits) return fail(PV_ERR_ARG, "null pointer");
    if (!offsets_nondecreasing(sm_off, n)) return fail(PV_ERR_ARG, "sm_off must be non-decreasing");
    std::lock_guard<std::mutex> mg(g_mg_mu);
    const int G = (int)g_mg.devs.size();
    if (G == 0) return fail(PV_ERR_NOT_INIT, "pv_verify_batch_multi_gpu: call pv_init_devices first");
    std::vector<uint64_t> b(G + 1);
    uint64_t wpr = 0;
    int rc = pv_shard_plan(n, G, b.data(), &wpr);
    if (rc) return rc;
    // every device's context for the whole call (ascending device order: no lock-order inversion)
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int d : g_mg.devs) locks.emplace_back(g_mus[d]);
    // one worker per device: stage its shard (host -> pinned -> HBM, its own stream) and enqueue the
    // shard's verification with the verdict words landing in its slot of the gather buffer
    std::vector<int> rcs(G, PV_OK);
    std::vector<std::string> errs(G);
    {
        std::vector<std::thread> th;
        for (int r = 0; r < G; r++)
            th.emplace_back([&, r] {
                const int d = g_mg.devs[r];
                DevScope ds(d);
                auto run = [&]() -> int {
                    PV_HIP(hipSetDevice(d), PV_ERR_NO_DEVICE);
                    Ctx& c = g_ctx;
                    int rc;
                    if ((rc = c.d_mg.grow((uint64_t)G * wpr * 8)) || (rc = c.hand.begin(c.stream))) return rc;
                    uint64_t* slot = c.d_mg.as<uint64_t>() + (uint64_t)r * wpr;
                    PV_HIP(hipMemsetAsync(slot, 0, wpr * 8, c.stream), PV_ERR_LAUNCH);
                    const uint64_t lo = b[r], hi = b[r + 1];
                    if (hi == lo) return PV_OK;
                    uint64_t *dv = nullptr, *hv = nullptr;
                    return stage_and_launch(sm, sm_off + lo, hi - lo, pk + 32 * lo, slot, &dv, &hv);
                };
                if ((rcs[r] = run()) != PV_OK) errs[r] = g_err;
            });
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < G; r++)
        if (rcs[r]) {
            for (int d : g_mg.devs) (void)hipStreamSynchronize(g_ctxs[d].stream);  // no DMA still reads staging
            return fail(rcs[r], "pv_verify_batch_multi_gpu: device " + std::to_string(g_mg.devs[r]) + ": " + errs[r]);
        }
    // ONE all-gather of the per-shard verdict words over the devices' RCCL clique (in place: shard r
    // sits at r * wpr on every device), then the gathered words come back from the first device
    ncclResult_t nr = ncclGroupStart();
    for (int r = 0; r < G && nr == ncclSuccess; r++) {
        Ctx& c = g_ctxs[g_mg.devs[r]];
        nr = ncclAllGather(c.d_mg.as<uint64_t>() + (uint64_t)r * wpr, c.d_mg.p, wpr, ncclUint64, g_mg.comms[r], c.stream);
    }
    const ncclResult_t ne = ncclGroupEnd();
    if (nr == ncclSuccess) nr = ne;
    Ctx& c0 = g_ctxs[g_mg.devs[0]];
    int cur = 0;
    (void)hipGetDevice(&cur);
    rc = PV_OK;
    if (nr != ncclSuccess) rc = fail(PV_ERR_COMM, std::string("ncclAllGather: ") + ncclGetErrorString(nr));
    const uint64_t gbytes = (uint64_t)G * wpr * 8;
    if (rc == PV_OK && c0.h_mg.cap < gbytes &&
        (hipSetDevice(c0.device) != hipSuccess || c0.h_mg.grow(gbytes, hipHostMallocPortable) != PV_OK))
        rc = fail(PV_ERR_ALLOC, "pv_verify_batch_multi_gpu: pinned verdict buffer");
    if (rc == PV_OK && hipMemcpyAsync(c0.h_mg.p, c0.d_mg.p, gbytes, hipMemcpyDeviceToHost, c0.stream) != hipSuccess)
        rc = fail(PV_ERR_LAUNCH, "pv_verify_batch_multi_gpu: verdict copy");
    for (int r = 0; r < G; r++) {
        Ctx& c = g_ctxs[g_mg.devs[r]];
        const hipError_t e = hipStreamSynchronize(c.stream);
        if (e != hipSuccess && rc == PV_OK)
            rc = fail(PV_ERR_LAUNCH, std::string("pv_verify_batch_multi_gpu: ") + hipGetErrorString(e));
    }
    (void)hipSetDevice(cur);
    if (rc) return rc;
    for (int r = 0; r < G; r++) {  // shard r's words start at bit b[r] (a multiple of 64)
        const uint64_t lo = b[r], hi = b[r + 1];
        if (hi > lo) memcpy(verdict_bits + lo / 8, c0.h_mg.p + (uint64_t)r * wpr * 8, (hi - lo + 7) / 8);
    }
    return PV_OK;
}

}  // extern "C"
