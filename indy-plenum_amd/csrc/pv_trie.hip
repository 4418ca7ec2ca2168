// The hashing half of the batched state-trie update on the GPU: SHA3-256 (keccak.h) of every new node,
// one lane per node, depth by depth. The structural half (trie_host.cpp) lays every node's RLP out in an
// arena with a 32-byte hole per hashed child; a node's lane absorbs its record, then stores the digest
// into its parent's hole and into the output hash array. A depth's nodes only need the depths below, so:
//   pv_sha3_batch_kernel  one launch per depth, deepest first, while that depth and everything above it
//                         hold more than TR_TAIL_MAX nodes;
//   pv_sha3_tail_kernel   one workgroup for all remaining depths in a single launch, a fence and a
//                         barrier between depths (as pv_merkle_upper_kernel for the upper Merkle
//                         levels): a long, thin top of the trie costs no launches.
// and pv_sha3_blob_kernel, the primitive on its own: records in a blob plus offsets, at any alignment.
// Further down, the read path: pv_proof_node_kernel and pv_proof_walk_kernel verify batches of state proofs.
// And the structural half itself for a trie built from empty (pv_trie_root): the passes of trie_build.h as the
// kernels of kern_trie_build.h, with rocPRIM's radix sort and scan between them, driven by tb_build below.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <string>
#include <vector>

#include "../../include/plenum_verify.h"
#include "keccak.h"
#include "pv_internal.h"
#include "trie_core.h"
#include "trie_host.h"

namespace {

constexpr int TR_BLOCK = 256;
constexpr uint64_t TR_TAIL_MAX = 256;  // records the single-workgroup tail takes: one per lane

__device__ __forceinline__ void tr_hash_record(uint8_t* arena, const PvTrieRec& r, uint64_t* out) {
    uint64_t d[4];
    sha3_256(d, r.len, PvKeccakWords(arena + r.off, r.len));
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = d[k];
    if (r.hole != PV_TRIE_NO_HOLE) {  // the hole lies at any byte offset of the parent's record
        uint8_t* h = arena + r.hole;
#pragma unroll
        for (int k = 0; k < 32; k++) h[k] = (uint8_t)(d[k >> 3] >> (8 * (k & 7)));
    }
}

// records [first, first + count): one depth
__global__ __launch_bounds__(TR_BLOCK) void pv_sha3_batch_kernel(uint8_t* arena, const PvTrieRec* __restrict__ recs,
                                                                 uint32_t first, uint32_t count, uint64_t* hashes) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= count) return;
    tr_hash_record(arena, recs[first + i], hashes + 4 * (uint64_t)(first + i));
}

// records [first, n): every remaining depth, one workgroup
__global__ __launch_bounds__(TR_BLOCK) void pv_sha3_tail_kernel(uint8_t* arena, const PvTrieRec* __restrict__ recs,
                                                                uint32_t first, uint32_t n, uint64_t* hashes) {
    for (uint32_t i0 = first; i0 < n;) {
        const uint32_t i1 = recs[i0].next;  // uniform
        for (uint32_t i = i0 + threadIdx.x; i < i1; i += TR_BLOCK) tr_hash_record(arena, recs[i], hashes + 4 * (uint64_t)i);
        __threadfence();  // the next depth reads this depth's digests
        __syncthreads();
        i0 = i1;
    }
}

__global__ __launch_bounds__(TR_BLOCK) void pv_sha3_blob_kernel(const uint8_t* __restrict__ data,
                                                                const uint64_t* __restrict__ off, uint64_t n,
                                                                uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], len = off[i + 1] - a;
    uint64_t d[4];
    sha3_256(d, len, PvKeccakWords(data + a, len));
#pragma unroll
    for (int k = 0; k < 4; k++) out[4 * i + k] = d[k];
}

// State proofs: two launches on one stream, ordered by the stream alone.
//   pv_proof_node_kernel  one lane per proof record: its SHA3-256, absorbed as pv_sha3_blob_kernel absorbs
//                         it, and one flag byte, 1 when the record is not canonical RLP all the way down
//                         (tr_rlp_canonical: byte loads inside the record, four named list ends, no stack);
//   pv_proof_walk_kernel  one lane per query: PV_PROOF_DEFER when a record of its proof is flagged, else
//                         tr_proof_walk on the RLP bytes in place, the node behind a reference found by a
//                         linear scan of the proof's digests.
// Neither trusts an index it reads from device memory: a record whose offsets decrease is flagged, a query
// whose proof, record range or key and value offsets are out of range is deferred without a read.
__global__ __launch_bounds__(TR_BLOCK) void pv_proof_node_kernel(const uint8_t* __restrict__ blob,
                                                                 const uint64_t* __restrict__ off,
                                                                 const uint64_t* __restrict__ lens, uint64_t n,
                                                                 uint64_t* __restrict__ digest, uint8_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i];
    uint64_t len;
    bool bad = false;
    if (lens) {
        len = lens[i];
    } else {
        const uint64_t b = off[i + 1];
        bad = b < a;
        len = bad ? 0 : b - a;
    }
    uint64_t d[4];
    sha3_256(d, len, PvKeccakWords(blob + a, len));
#pragma unroll
    for (int k = 0; k < 4; k++) digest[4 * i + k] = d[k];
    flag[i] = bad || !tr_rlp_canonical(blob + a, len) ? 1 : 0;
}

__global__ __launch_bounds__(TR_BLOCK) void pv_proof_walk_kernel(const PvProofIn in, const uint64_t* __restrict__ digest,
                                                                 const uint8_t* __restrict__ flag,
                                                                 uint8_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= in.n_queries) return;
    uint8_t st = PV_PROOF_DEFER;
    const uint64_t p = in.query_proof[i];
    if (p < in.n_proofs) {
        const uint64_t first = in.proof_first[p], last = in.proof_first[p + 1];
        const uint64_t ka = in.key_off[i], kb = in.key_off[i + 1], va = in.val_off[i], vb = in.val_off[i + 1];
        if (first <= last && last <= in.n_nodes && last - first <= PV_PROOF_MAX_NODES && ka <= kb && va <= vb) {
            bool clean = true;
            for (uint64_t j = first; j < last; j++) clean &= flag[j] == 0;
            if (clean)
                st = (uint8_t)tr_proof_walk(in.node_blob, in.node_off, in.node_len, digest, first, last - first,
                                            in.root + 32 * i, in.key_blob + ka, kb - ka, in.val_blob + va, vb - va);
        }
    }
    status[i] = st;
}

#include "kern_trie_build.h"

// --------------------------------------------------------------------------------------------- host

// The trie code's own workspace: allocated on first use (an engine that never touches a trie holds
// nothing), freed by pv_shutdown, handed over between caller streams by an event (workspace.h).
// Launches are serialised on g_tr_mu.
struct TrWork {
    PvStage stage;  // in: the arena and its records, a blob and its offsets, or proofs; out: digests, flags, statuses
    PvHandover hand;
    PvDevBuf build;  // the device builder's arrays (tb_build), and what its second phase writes and hashes
    PvDevBuf built;
};
TrWork g_tr;
std::mutex g_tr_mu;
int g_tr_path = PV_TRIE_AUTO;

// The launches for nr records on device buffers; next(i0) is the end of the depth that starts at record i0,
// asked once per depth in order. Caller holds g_tr_mu.
template <class Next>
int tr_enqueue_runs(uint8_t* d_arena, const PvTrieRec* d_recs, uint64_t nr, uint64_t* d_hashes, hipStream_t st,
                    uint64_t* launches, uint64_t* tail_records, const Next& next) {
    for (uint64_t i0 = 0; i0 < nr;) {
        if (nr - i0 <= TR_TAIL_MAX) {
            PV_LAUNCH(pv_sha3_tail_kernel, dim3(1), dim3(TR_BLOCK), 0, st, d_arena, d_recs, (uint32_t)i0,
                      (uint32_t)nr, d_hashes);
            ++*launches;
            *tail_records = nr - i0;
            break;
        }
        const uint64_t i1 = next(i0), count = i1 - i0;
        PV_LAUNCH(pv_sha3_batch_kernel, dim3((unsigned)((count + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0, st,
                  d_arena, d_recs, (uint32_t)i0, (uint32_t)count, d_hashes);
        ++*launches;
        i0 = i1;
    }
    return PV_OK;
}

// ... with the depth boundaries read from a host copy of the records
int tr_enqueue(uint8_t* d_arena, const PvTrieRec* d_recs, const PvTrieRec* recs, uint64_t nr, uint64_t* d_hashes,
               hipStream_t st, uint64_t* launches, uint64_t* tail_records) {
    return tr_enqueue_runs(d_arena, d_recs, nr, d_hashes, st, launches, tail_records,
                           [&](uint64_t i0) { return (uint64_t)recs[i0].next; });
}
// ... and from a small host array: ends[k] is the end of the k-th depth, deepest first
int tr_enqueue_bounds(uint8_t* d_arena, const PvTrieRec* d_recs, const std::vector<uint32_t>& ends, uint64_t nr,
                      uint64_t* d_hashes, hipStream_t st, uint64_t* launches, uint64_t* tail_records) {
    size_t k = 0;
    return tr_enqueue_runs(d_arena, d_recs, nr, d_hashes, st, launches, tail_records,
                           [&](uint64_t) { return (uint64_t)ends[k++]; });
}

// arena and records staged whole, hashed, copied back: arena -> blob, digests -> hashes
int tr_device_hash(PvTriePlan& plan, uint8_t* blob, uint8_t* hashes, uint64_t* launches, uint64_t* tail_records) {
    const hipStream_t st = pv_engine_stream();
    return g_tr.hand.run(st, [&]() -> int {
        PvStage& g = g_tr.stage;
        int rc = g.reset(st, false);
        if (rc) return rc;
        const uint64_t nr = plan.recs.size();
        const int arena = g.inout(plan.arena.data(), blob, plan.arena_bytes),
                  recs = g.in(plan.recs.data(), nr * sizeof(PvTrieRec)), digest = g.out(hashes, 32 * nr);
        if ((rc = g.upload()) || (rc = tr_enqueue(g.dev<uint8_t>(arena), g.dev<const PvTrieRec>(recs), plan.recs.data(), nr,
                                                  g.dev<uint64_t>(digest), st, launches, tail_records)))
            return rc;
        return g.download();
    });
}

// The path of entry `who` with `work` records under pv_trie_path's mode. Caller holds g_tr_mu.
int tr_choose(uint64_t work, uint64_t auto_min, const char* who, bool* device) {
    return pv_choose_path(g_tr_path, pv_engine_stream() != nullptr, work, auto_min, who, device);
}

// Both proof launches for device buffers. Caller holds g_tr_mu.
int tr_proof_enqueue(const PvProofIn& d, uint64_t* d_digest, uint8_t* d_flag, uint8_t* d_status, hipStream_t st) {
    if (d.n_nodes) {
        PV_LAUNCH(pv_proof_node_kernel, dim3((unsigned)((d.n_nodes + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0,
                  st, d.node_blob, d.node_off, d.node_len, d.n_nodes, d_digest, d_flag);
    }
    PV_LAUNCH(pv_proof_walk_kernel, dim3((unsigned)((d.n_queries + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0, st,
              d, (const uint64_t*)d_digest, (const uint8_t*)d_flag, d_status);
    return PV_OK;
}

// The host-buffer entry's device path: every array staged into the workspace, offsets rebased to the
// bytes that are copied, statuses copied back. Caller holds g_tr_mu and has validated `in`.
int tr_proof_device(const PvProofIn& in, uint8_t* status) {
    const hipStream_t st = pv_engine_stream();
    return g_tr.hand.run(st, [&]() -> int {
        const uint64_t nn = in.n_nodes, np = in.n_proofs, nq = in.n_queries;
        uint64_t lo = ~0ull, hi = 0;  // the span of the node blob the records lie in
        for (uint64_t i = 0; i < nn; i++) {
            const uint64_t len = in.node_len ? in.node_len[i] : in.node_off[i + 1] - in.node_off[i];
            lo = std::min(lo, in.node_off[i]);
            hi = std::max(hi, in.node_off[i] + len);
        }
        if (nn == 0) lo = hi = 0;
        PvStage& g = g_tr.stage;
        int rc = g.reset(st, false), i_noff;
        if (rc) return rc;
        uint64_t* noff = g.in_u64(nn + 1, &i_noff);  // records need not lie in order: moved to the span's start
        for (uint64_t i = 0; i < nn; i++) noff[i] = in.node_off[i] - lo;
        noff[nn] = in.node_len ? hi - lo : in.node_off[nn] - lo;
        const int i_nlen = in.node_len ? g.in(in.node_len, 8 * nn) : -1, i_pf = g.in(in.proof_first, 8 * (np + 1)),
                  i_koff = g.in_offsets(in.key_off, nq), i_voff = g.in_offsets(in.val_off, nq),
                  i_qp = g.in(in.query_proof, 4 * nq), i_root = g.in(in.root, 32 * nq),
                  i_key = g.in(in.key_blob + in.key_off[0], in.key_off[nq] - in.key_off[0]),
                  i_val = g.in(in.val_blob + in.val_off[0], in.val_off[nq] - in.val_off[0]),
                  i_blob = g.in(in.node_blob + lo, hi - lo, 8),  // the hash reads to a whole word
                  o_digest = g.out(nullptr, 32 * nn + 1), o_flag = g.out(nullptr, nn + 1), o_status = g.out(status, nq);
        if ((rc = g.upload())) return rc;
        const PvProofIn d{g.dev<const uint8_t>(i_blob), g.dev<const uint64_t>(i_noff), nn,
                          g.dev<const uint64_t>(i_pf),  np,                             g.dev<const uint32_t>(i_qp),
                          g.dev<const uint8_t>(i_root), g.dev<const uint8_t>(i_key),    g.dev<const uint64_t>(i_koff),
                          g.dev<const uint8_t>(i_val),  g.dev<const uint64_t>(i_voff),  nq,
                          g.dev<const uint64_t>(i_nlen)};
        if ((rc = tr_proof_enqueue(d, g.dev<uint64_t>(o_digest), g.dev<uint8_t>(o_flag), g.dev<uint8_t>(o_status), st)))
            return rc;
        return g.download();
    });
}

// The device builder on device buffers: phase one (sort, deduplicate, structure, sizes, record order), one
// read of the header, phase two (emit, hash), the root copied to d_root on the device. Caller holds g_tr_mu
// and is inside the workspace's hand-over on `st`.
int tb_build(const uint8_t* d_keys, uint32_t key_len, uint64_t n64, const uint8_t* d_val, const uint64_t* d_voff,
             uint32_t flags, uint8_t* d_root, PvTrieRootOut* out, hipStream_t st) {
    // node ids are 32-bit and there are 3 n of them; that many pairs need more device memory than there is
    if ((3 * n64) >> 32) return pv_fail(PV_ERR_ALLOC, "pv_trie_root: the device builder's workspace for n pairs does not fit");
    const uint32_t n = (uint32_t)n64, n3 = 3 * n, W = (key_len + 7) / 8;
    size_t t_sort = 0, t_scan = 0, t_scan64 = 0, t_dsort = 0;
    PV_HIP(rocprim::radix_sort_keys(nullptr, t_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 64, st), PV_ERR_LAUNCH);
    PV_HIP(rocprim::exclusive_scan(nullptr, t_scan, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), st),
           PV_ERR_LAUNCH);
    PV_HIP(rocprim::exclusive_scan(nullptr, t_scan64, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n3,
                                   rocprim::plus<uint64_t>(), st), PV_ERR_LAUNCH);
    PV_HIP(rocprim::radix_sort_pairs(nullptr, t_dsort, (uint8_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr,
                                     (uint32_t*)nullptr, n3, 0, 8, st), PV_ERR_LAUNCH);
    const size_t t_bytes = std::max(std::max(t_sort, t_scan), std::max(t_scan64, t_dsort));
    PvLayout lay;
    const uint64_t o_hdr = lay.add(sizeof(TbHdr)), o_idx = lay.add(4ull * n), o_idx2 = lay.add(4ull * n),
                   o_wk = lay.add(8ull * n), o_wk2 = lay.add(8ull * n), o_keep = lay.add(4ull * n), o_pos = lay.add(4ull * n),
                   o_sidx = lay.add(4ull * n), o_skey = lay.add(8ull * n * W), o_h = lay.add(n), o_isrep = lay.add(n),
                   o_ct = lay.add(64ull * n), o_lpar = lay.add(4ull * n), o_bpar = lay.add(4ull * n), o_lsz = lay.add(4ull * n),
                   o_bsmall = lay.add(4ull * n), o_bsz = lay.add(4ull * n), o_esz = lay.add(4ull * n),
                   o_rlen8 = lay.add(8ull * n3), o_roff = lay.add(8ull * n3), o_dkey = lay.add(n3), o_ndepth = lay.add(n3),
                   o_nid = lay.add(4ull * n3), o_dkey_s = lay.add(n3), o_order = lay.add(4ull * n3),
                   o_rank = lay.add(4ull * n3), o_temp = lay.add(t_bytes);
    PvDevBuf& b = g_tr.build;
    if (int rc = b.grow(lay.at)) return rc;
    auto at = [&](uint64_t o) { return b.p + o; };
    TbCtx c{};
    c.keys = d_keys;
    c.val = d_val;
    c.voff = d_voff;
    c.key_len = key_len;
    c.n = n;
    c.wrap = (flags & PV_TRIE_ROOT_WRAP) ? 1 : 0;
    c.W = W;
    c.hdr = (TbHdr*)at(o_hdr);
    c.idx = (uint32_t*)at(o_idx);
    c.keep = (uint32_t*)at(o_keep);
    c.pos = (uint32_t*)at(o_pos);
    c.sidx = (uint32_t*)at(o_sidx);
    c.skey = (uint64_t*)at(o_skey);
    c.h = at(o_h);
    c.isrep = at(o_isrep);
    c.ct = (uint32_t*)at(o_ct);
    c.lpar = (uint32_t*)at(o_lpar);
    c.bpar = (uint32_t*)at(o_bpar);
    c.lsz = (uint32_t*)at(o_lsz);
    c.bsmall = (uint32_t*)at(o_bsmall);
    c.bsz = (uint32_t*)at(o_bsz);
    c.esz = (uint32_t*)at(o_esz);
    c.rlen8 = (uint64_t*)at(o_rlen8);
    c.roff = (uint64_t*)at(o_roff);
    c.dkey = at(o_dkey);
    c.ndepth = at(o_ndepth);
    c.nid = (uint32_t*)at(o_nid);
    c.dkey_s = at(o_dkey_s);
    c.order = (uint32_t*)at(o_order);
    c.rank = (uint32_t*)at(o_rank);
    void* temp = at(o_temp);
    uint64_t *wk = (uint64_t*)at(o_wk), *wk2 = (uint64_t*)at(o_wk2);
    uint32_t* idx2 = (uint32_t*)at(o_idx2);
    const dim3 blk(TR_BLOCK), gn((n + TR_BLOCK - 1) / TR_BLOCK), gn3((unsigned)(((uint64_t)n3 + TR_BLOCK - 1) / TR_BLOCK));

    PV_HIP(hipMemsetAsync(c.hdr, 0, sizeof(TbHdr), st), PV_ERR_LAUNCH);
    PV_LAUNCH(pv_tb_init_kernel, gn, blk, 0, st, c, n);
    // LSD sort of the entry indices by big-endian 32-bit key parts, the least significant part first. A pass
    // sorts (part, position) keys, all distinct, so entries of one key keep the order they were given in
    // whatever the sort does with equal keys; the entry indices follow by a gather.
    for (uint32_t w = (key_len + 3) / 4; w-- > 0;) {
        size_t tb = t_bytes;
        PV_LAUNCH(pv_tb_word_kernel, gn, blk, 0, st, c, n, w, wk);
        PV_HIP(rocprim::radix_sort_keys(temp, tb, wk, wk2, n, 0, 64, st), PV_ERR_LAUNCH);
        PV_LAUNCH(pv_tb_gather_kernel, gn, blk, 0, st, c, n, (const uint64_t*)wk2, idx2);
        std::swap(c.idx, idx2);
    }
    PV_LAUNCH(pv_tb_keep_kernel, gn, blk, 0, st, c, n);
    {
        size_t tb = t_bytes;
        PV_HIP(rocprim::exclusive_scan(temp, tb, c.keep, c.pos, 0u, n, rocprim::plus<uint32_t>(), st), PV_ERR_LAUNCH);
    }
    PV_LAUNCH(pv_tb_compact_kernel, gn, blk, 0, st, c, n);
    PV_LAUNCH(pv_tb_lcp_kernel, gn, blk, 0, st, c, n);
    PV_LAUNCH(pv_tb_branch_kernel, gn, blk, 0, st, c, n);
    PV_LAUNCH(pv_tb_leaf_size_kernel, gn, blk, 0, st, c, n);
    PV_LAUNCH(pv_tb_small_kernel, gn, blk, 0, st, c, n);
    PV_LAUNCH(pv_tb_size_kernel, gn, blk, 0, st, c, n);
    PV_LAUNCH(pv_tb_mark_kernel, gn3, blk, 0, st, c, n3);
    {
        size_t tb = t_bytes;
        PV_HIP(rocprim::exclusive_scan(temp, tb, c.rlen8, c.roff, (uint64_t)0, n3, rocprim::plus<uint64_t>(), st), PV_ERR_LAUNCH);
        tb = t_bytes;
        PV_HIP(rocprim::radix_sort_pairs(temp, tb, c.dkey, c.dkey_s, c.nid, c.order, n3, 0, 8, st), PV_ERR_LAUNCH);
    }
    PV_LAUNCH(pv_tb_bounds_kernel, gn3, blk, 0, st, c, n3);
    // the one read between the phases: counts, arena bytes, the error word, the per-depth record ranges
    TbHdr hdr;
    PV_HIP(hipMemcpyAsync(&hdr, c.hdr, sizeof(TbHdr), hipMemcpyDeviceToHost, st), PV_ERR_LAUNCH);
    PV_HIP(hipStreamSynchronize(st), PV_ERR_LAUNCH);
    if (hdr.err)
        return pv_fail(PV_ERR_ARG, "pv_trie_root: value offsets decrease, or a value is empty without PV_TRIE_ROOT_WRAP or not below 2^24 bytes stored");
    std::vector<uint32_t> ends;
    for (uint32_t d = TB_DEPTHS; d-- > 0;)
        if (hdr.dend[d] > hdr.dstart[d]) ends.push_back(hdr.dend[d]);
    const uint64_t nr = hdr.dend[0];  // the root is the last record
    if (nr == 0 || ends.empty() || ends.back() != nr) return pv_fail(PV_ERR_LAUNCH, "pv_trie_root: the builder left no root record");
    PvLayout la;
    const uint64_t o_arena = la.add(hdr.arena_bytes + 8), o_recs = la.add(sizeof(PvTrieRec) * nr), o_hash = la.add(32 * nr);
    PvDevBuf& a = g_tr.built;
    if (int rc = a.grow(la.at)) return rc;
    c.arena = a.p + o_arena;
    c.recs = (PvTrieRec*)(a.p + o_recs);
    uint64_t* d_hashes = (uint64_t*)(a.p + o_hash);
    PV_LAUNCH(pv_tb_emit_kernel, dim3((unsigned)((nr + TR_BLOCK - 1) / TR_BLOCK)), blk, 0, st, c, (uint32_t)nr);
    out->launches = out->tail_records = 0;
    if (int rc = tr_enqueue_bounds(c.arena, c.recs, ends, nr, d_hashes, st, &out->launches, &out->tail_records)) return rc;
    PV_HIP(hipMemcpyAsync(d_root, d_hashes + 4 * (nr - 1), 32, hipMemcpyDeviceToDevice, st), PV_ERR_LAUNCH);
    out->n_keys = hdr.m;
    out->n_nodes = (uint64_t)hdr.m + hdr.n_branch + hdr.n_ext;
    out->n_records = nr;
    out->arena_bytes = hdr.arena_bytes;
    out->max_depth = hdr.max_depth;
    return PV_OK;
}

// PV_OK or PV_ERR_ARG: the stored length of a value of `len` bytes (first byte b0) is within the limits
bool tb_value_ok(uint64_t len, uint32_t flags) {
    if (!(flags & PV_TRIE_ROOT_WRAP)) return len >= 1 && len <= PV_TRIE_MAX_VALUE;
    const uint64_t s = len == 1 ? 2 : tr_prefix_size(len) + len;
    return tr_list_size(s) <= PV_TRIE_MAX_VALUE;
}

void tb_out_clear(PvTrieRootOut* out) {
    out->n_keys = out->n_nodes = out->n_records = out->arena_bytes = out->max_depth = out->launches = out->tail_records = 0;
    out->built_on_device = 0;
    memset(out->root, 0, 32);
}

}  // namespace

void pv_trie_forget_stream(void* stream) {
    std::lock_guard<std::mutex> lk(g_tr_mu);
    g_tr.hand.forget((hipStream_t)stream);
}

void pv_trie_shutdown() {
    std::lock_guard<std::mutex> lk(g_tr_mu);
    g_tr.stage.release();
    g_tr.build.release();
    g_tr.built.release();
    g_tr.hand.destroy();
}

extern "C" {

int pv_trie_path(int mode) {
    std::lock_guard<std::mutex> lk(g_tr_mu);
    if (mode != PV_TRIE_AUTO && mode != PV_TRIE_HOST && mode != PV_TRIE_DEVICE)
        return pv_fail(PV_ERR_ARG, "pv_trie_path: unknown mode");
    g_tr_path = mode;
    return PV_OK;
}

int pv_sha3_256_batch(const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* out) {
    if (n == 0) return PV_OK;
    if (!off || !out) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: null pointer");
    if (!pv_offsets_monotone(off, n)) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: offsets must be non-decreasing");
    if (!data && off[n] != off[0]) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: null data");
    if (n >> 31) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch: more than 2^31 - 1 records");
    std::unique_lock<std::mutex> lk(g_tr_mu);
    bool device;
    int rc = tr_choose(n, PV_TRIE_AUTO_MIN, "pv_sha3_256_batch", &device);
    if (rc) return rc;
    if (!device) {
        lk.unlock();  // the host path shares no workspace
        pv_sha3_host_batch(data, off, n, out);
        return PV_OK;
    }
    const hipStream_t st = pv_engine_stream();
    return g_tr.hand.run(st, [&]() -> int {
        PvStage& g = g_tr.stage;
        int rc = g.reset(st, false);
        if (rc) return rc;
        // staged whole; the hash reads to a whole word
        const int i_off = g.in_offsets(off, n), i_data = g.in(data + off[0], off[n] - off[0], 8), o_digest = g.out(out, 32 * n);
        if ((rc = g.upload())) return rc;
        PV_LAUNCH(pv_sha3_blob_kernel, dim3((unsigned)((n + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0, st,
                  g.dev<const uint8_t>(i_data), g.dev<const uint64_t>(i_off), n, g.dev<uint64_t>(o_digest));
        return g.download();
    });
}

int pv_sha3_256_batch_device(const uint8_t* d_data, const uint64_t* d_off, uint64_t n, uint8_t* d_out, void* stream) {
    if (!pv_engine_stream()) return pv_fail(PV_ERR_NOT_INIT, "pv_sha3_256_batch_device: call pv_init first");
    if (n == 0) return PV_OK;
    if (!d_data || !d_off || !d_out) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch_device: null pointer");
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch_device: d_out must be 8-byte aligned");
    if (n >> 31) return pv_fail(PV_ERR_ARG, "pv_sha3_256_batch_device: more than 2^31 - 1 records");
    PV_LAUNCH(pv_sha3_blob_kernel, dim3((unsigned)((n + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0,
              stream ? (hipStream_t)stream : pv_engine_stream(), d_data, d_off, n, reinterpret_cast<uint64_t*>(d_out));
    return PV_OK;
}

int pv_trie_update_batch(const uint8_t* root, const uint8_t* known_hash, const uint8_t* known_blob,
                         const uint64_t* known_off, uint64_t n_known, const uint8_t* key_blob, const uint64_t* key_off,
                         const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, PvTrieOut* out) {
    if (!root || !out || !out->root) return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: null root or output struct");
    out->n_nodes = out->blob_bytes = out->n_missing = out->launches = out->tail_records = 0;
    if (n == 0) {
        memcpy(out->root, root, 32);
        return PV_OK;
    }
    if (!key_off || !val_off || !val_blob) return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: null keys or values");
    if (!pv_offsets_monotone(key_off, n) || !pv_offsets_monotone(val_off, n))
        return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: offsets must be non-decreasing");
    if (!key_blob && key_off[n] != key_off[0]) return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: null key blob");
    if (n_known && (!known_hash || !known_blob || !known_off || !pv_offsets_monotone(known_off, n_known)))
        return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: known nodes need hashes, a blob and non-decreasing offsets");
    if ((out->node_cap && (!out->node_hash || !out->node_off || !out->node_len)) || (out->blob_cap && !out->node_blob) ||
        (out->missing_cap && !out->missing))
        return pv_fail(PV_ERR_ARG, "pv_trie_update_batch: a capacity without its array");
    bool device;
    {  // a forced device path without a device fails before the build
        std::lock_guard<std::mutex> lk(g_tr_mu);
        if (int rc = tr_choose(0, 0, "pv_trie_update_batch", &device)) return rc;
    }
    const PvTrieIn in{root, known_hash, known_blob, known_off, n_known, key_blob, key_off, val_blob, val_off, n};
    PvTriePlan plan;
    std::string err;
    int rc = pv_trie_host_build(in, &plan, &err);
    if (rc == PV_TRIE_NEED_NODES) {
        out->n_missing = plan.missing.size() / 32;
        if (out->missing_cap) memcpy(out->missing, plan.missing.data(), 32 * std::min(out->n_missing, out->missing_cap));
        return rc;
    }
    if (rc) return pv_fail(rc, "pv_trie_update_batch: " + err);
    const uint64_t nr = plan.recs.size();
    out->n_nodes = nr;
    out->blob_bytes = plan.arena_bytes;
    if (nr == 0) {  // nothing to set
        memcpy(out->root, root, 32);
        return PV_OK;
    }
    if (nr > out->node_cap || plan.arena_bytes > out->blob_cap) return PV_TRIE_NEED_SPACE;
    std::unique_lock<std::mutex> lk(g_tr_mu);
    if ((rc = tr_choose(nr, PV_TRIE_AUTO_MIN, "pv_trie_update_batch", &device))) return rc;
    if (device) {
        if ((rc = tr_device_hash(plan, out->node_blob, out->node_hash, &out->launches, &out->tail_records))) return rc;
    } else {
        lk.unlock();  // the host path shares no workspace; it hashes in the plan's own (aligned) arena
        pv_trie_host_hash(reinterpret_cast<uint8_t*>(plan.arena.data()), plan.recs.data(), nr, out->node_hash);
        memcpy(out->node_blob, plan.arena.data(), plan.arena_bytes);
    }
    for (uint64_t i = 0; i < nr; i++) {
        out->node_off[i] = plan.recs[i].off;
        out->node_len[i] = plan.recs[i].len;
    }
    memcpy(out->root, out->node_hash + 32 * (nr - 1), 32);  // the root is the last record
    return PV_OK;
}

int pv_trie_root(const uint8_t* keys, uint32_t key_len, uint64_t n, const uint8_t* val_blob, const uint64_t* val_off,
                 uint32_t flags, PvTrieRootOut* out) {
    if (!out) return pv_fail(PV_ERR_ARG, "pv_trie_root: null output struct");
    tb_out_clear(out);
    uint8_t* root = out->root;
    if (key_len < 1 || key_len > PV_TRIE_BUILD_MAX_KEY) return pv_fail(PV_ERR_ARG, "pv_trie_root: key_len must be 1 .. 64");
    if (n >> 31) return pv_fail(PV_ERR_ARG, "pv_trie_root: more than 2^31 - 1 pairs");
    if (n == 0) {
        memcpy(root, PV_TRIE_BLANK_ROOT, 32);
        return PV_OK;
    }
    if (!keys || !val_off) return pv_fail(PV_ERR_ARG, "pv_trie_root: null keys or offsets");
    if (!pv_offsets_monotone(val_off, n)) return pv_fail(PV_ERR_ARG, "pv_trie_root: offsets must be non-decreasing");
    if (!val_blob && val_off[n] != val_off[0]) return pv_fail(PV_ERR_ARG, "pv_trie_root: null value blob");
    bool ok = true;
    for (uint64_t i = 0; i < n; i++) ok &= tb_value_ok(val_off[i + 1] - val_off[i], flags);
    if (!ok)
        return pv_fail(PV_ERR_ARG, "pv_trie_root: a value is empty without PV_TRIE_ROOT_WRAP or not below 2^24 bytes stored");
    std::unique_lock<std::mutex> lk(g_tr_mu);
    bool device;
    if (int rc = tr_choose(n, PV_TRIE_BUILD_AUTO_MIN, "pv_trie_root", &device)) return rc;
    if (device) {
        const hipStream_t st = pv_engine_stream();
        return g_tr.hand.run(st, [&]() -> int {
            PvStage& g = g_tr.stage;
            int rc = g.reset(st, false);
            if (rc) return rc;
            const int i_keys = g.in(keys, n * key_len), i_off = g.in_offsets(val_off, n),
                      i_val = g.in(val_blob ? val_blob + val_off[0] : nullptr, val_off[n] - val_off[0]), o_root = g.out(root, 32);
            if ((rc = g.upload()) || (rc = tb_build(g.dev<const uint8_t>(i_keys), key_len, n, g.dev<const uint8_t>(i_val),
                                                    g.dev<const uint64_t>(i_off), flags, g.dev<uint8_t>(o_root), out, st)))
                return rc;
            out->built_on_device = 1;
            return g.download();
        });
    }
    lk.unlock();  // the host path shares no workspace: the arguments packed for the structural half of pv_trie_update_batch
    std::vector<uint64_t> key_off(n + 1), woff;
    for (uint64_t i = 0; i <= n; i++) key_off[i] = i * key_len;
    std::vector<uint8_t> wrapped;
    const uint8_t* vb = val_blob;
    const uint64_t* vo = val_off;
    if (flags & PV_TRIE_ROOT_WRAP) {  // rlp([value]) of every value
        woff.resize(n + 1);
        wrapped.resize(val_off[n] - val_off[0] + 8 * n + 8);
        uint64_t at = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint8_t* p = val_blob + val_off[i];
            const uint64_t len = val_off[i + 1] - val_off[i];
            woff[i] = at;
            at += tr_put_prefix(wrapped.data() + at, tr_str_size(p, len), 0xc0);
            at += tr_put_str(wrapped.data() + at, p, len);
        }
        woff[n] = at;
        vb = wrapped.data();
        vo = woff.data();
    }
    const PvTrieIn in{PV_TRIE_BLANK_ROOT, nullptr, nullptr, nullptr, 0, keys, key_off.data(), vb, vo, n};
    PvTriePlan plan;
    std::string err;
    if (int rc = pv_trie_host_build(in, &plan, &err)) return pv_fail(rc, "pv_trie_root: " + err);
    const uint64_t nr = plan.recs.size();
    if (nr == 0) return pv_fail(PV_ERR_ARG, "pv_trie_root: the host path built no node");
    std::vector<uint8_t> hashes(32 * nr);
    pv_trie_host_hash(reinterpret_cast<uint8_t*>(plan.arena.data()), plan.recs.data(), nr, hashes.data());
    memcpy(root, hashes.data() + 32 * (nr - 1), 32);
    out->n_records = nr;
    out->arena_bytes = plan.arena_bytes;
    return PV_OK;
}

int pv_trie_root_device(const uint8_t* d_keys, uint32_t key_len, uint64_t n, const uint8_t* d_val_blob,
                        const uint64_t* d_val_off, uint32_t flags, uint8_t* d_root, PvTrieRootOut* out, void* stream) {
    if (!pv_engine_stream()) return pv_fail(PV_ERR_NOT_INIT, "pv_trie_root_device: call pv_init first");
    if (!d_root || !out) return pv_fail(PV_ERR_ARG, "pv_trie_root_device: null root or output struct");
    tb_out_clear(out);
    if (key_len < 1 || key_len > PV_TRIE_BUILD_MAX_KEY) return pv_fail(PV_ERR_ARG, "pv_trie_root_device: key_len must be 1 .. 64");
    if (n >> 31) return pv_fail(PV_ERR_ARG, "pv_trie_root_device: more than 2^31 - 1 pairs");
    const hipStream_t st = stream ? (hipStream_t)stream : pv_engine_stream();
    if (n == 0) {
        PV_HIP(hipMemcpyAsync(d_root, PV_TRIE_BLANK_ROOT, 32, hipMemcpyHostToDevice, st), PV_ERR_LAUNCH);
        return PV_OK;
    }
    if (!d_keys || !d_val_off || !d_val_blob) return pv_fail(PV_ERR_ARG, "pv_trie_root_device: null pointer");
    std::lock_guard<std::mutex> lk(g_tr_mu);
    return g_tr.hand.run(st, [&]() -> int {
        if (int rc = tb_build(d_keys, key_len, n, d_val_blob, d_val_off, flags, d_root, out, st)) return rc;
        out->built_on_device = 1;
        return PV_OK;
    });
}

int pv_trie_verify_proofs(const PvProofIn* in, uint8_t* status) {
    if (!in) return pv_fail(PV_ERR_ARG, "pv_trie_verify_proofs: null input struct");
    if (in->n_queries == 0) return PV_OK;
    if (!status) return pv_fail(PV_ERR_ARG, "pv_trie_verify_proofs: null status");
    const char* why = nullptr;
    if (pv_proof_check_args(*in, &why)) return pv_fail(PV_ERR_ARG, std::string("pv_trie_verify_proofs: ") + why);
    std::unique_lock<std::mutex> lk(g_tr_mu);
    bool device;
    if (int rc = tr_choose(in->n_nodes, PV_TRIE_PROOF_AUTO_MIN, "pv_trie_verify_proofs", &device)) return rc;
    if (device) return tr_proof_device(*in, status);
    lk.unlock();  // the host path shares no workspace
    pv_proof_host(*in, status);
    return PV_OK;
}

int pv_trie_verify_proofs_device(const PvProofIn* d_in, uint8_t* d_status, uint8_t* d_node_hash, void* stream) {
    if (!pv_engine_stream()) return pv_fail(PV_ERR_NOT_INIT, "pv_trie_verify_proofs_device: call pv_init first");
    if (!d_in) return pv_fail(PV_ERR_ARG, "pv_trie_verify_proofs_device: null input struct");
    if (d_in->n_queries == 0) return PV_OK;
    if (!d_status || !d_in->proof_first || !d_in->query_proof || !d_in->root || !d_in->key_off || !d_in->val_off ||
        !d_in->key_blob || !d_in->val_blob || (d_in->n_nodes && (!d_in->node_off || !d_in->node_blob || !d_node_hash)))
        return pv_fail(PV_ERR_ARG, "pv_trie_verify_proofs_device: null pointer");
    if (reinterpret_cast<uintptr_t>(d_node_hash) & 7u)
        return pv_fail(PV_ERR_ARG, "pv_trie_verify_proofs_device: d_node_hash must be 8-byte aligned");
    if ((d_in->n_nodes >> 31) || (d_in->n_queries >> 31) || (d_in->n_proofs >> 31))
        return pv_fail(PV_ERR_ARG, "pv_trie_verify_proofs_device: more than 2^31 - 1 records, proofs or queries");
    const hipStream_t st = stream ? (hipStream_t)stream : pv_engine_stream();
    std::lock_guard<std::mutex> lk(g_tr_mu);
    return g_tr.hand.run(st, [&]() -> int {  // the flags live in the workspace: handed over from the stream that used it last
        PvDevBuf& flag = g_tr.stage.d_out;
        if (int rc = flag.grow(pv_up256(d_in->n_nodes + 1))) return rc;
        return tr_proof_enqueue(*d_in, reinterpret_cast<uint64_t*>(d_node_hash), flag.p, d_status, st);
    });
}

int pv_trie_proof_split(const uint8_t* ser, const uint64_t* ser_off, uint64_t n_proofs, uint64_t* proof_first,
                        uint64_t* node_off, uint64_t* node_len, uint64_t node_cap, uint64_t* n_nodes, uint8_t* proof_ok) {
    if (!proof_first || !n_nodes) return pv_fail(PV_ERR_ARG, "pv_trie_proof_split: null pointer");
    if (n_proofs && (!ser_off || !proof_ok || !pv_offsets_monotone(ser_off, n_proofs)))
        return pv_fail(PV_ERR_ARG, "pv_trie_proof_split: null pointer or decreasing offsets");
    if (n_proofs && !ser && ser_off[n_proofs] != ser_off[0]) return pv_fail(PV_ERR_ARG, "pv_trie_proof_split: null proofs");
    if (!node_off || (node_cap && !node_len)) return pv_fail(PV_ERR_ARG, "pv_trie_proof_split: a capacity without its array");
    return pv_proof_split_host(ser, ser_off, n_proofs, proof_first, node_off, node_len, node_cap, n_nodes, proof_ok);
}

}  // extern "C"
