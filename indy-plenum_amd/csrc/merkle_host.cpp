// Host path of the batched Merkle append, the audit-proof and consistency-proof checks and the catch-up
// entry: the same contract as the kernels of
// pv_merkle.hip, in C++ over merkle_core.h (one source for the index arithmetic) and the host SHA-256
// of signing_json.cpp. pv_merkle_append_batch takes it for small batches (a 3PC batch of ten
// transactions must not pay kernel launches) and when no device is initialised.
#include "merkle_host.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "merkle_core.h"
#include "sha256_host.h"

namespace {

struct H32 {
    uint8_t b[32];
};

constexpr unsigned MK_THREADS = 16;
constexpr uint64_t MK_PER_THREAD = 2048;  // below this much work a thread is not worth starting

// f(lo, hi) over [0, n) split over up to MK_THREADS threads
template <class F>
void parallel_for(uint64_t n, const F& f, unsigned max_threads = MK_THREADS) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const uint64_t t = std::min<uint64_t>(std::min(max_threads, hw), (n + MK_PER_THREAD - 1) / MK_PER_THREAD);
    if (t <= 1) {
        if (n) f(0, n);
        return;
    }
    std::vector<std::thread> th;
    for (uint64_t k = 0; k < t; k++) th.emplace_back([&f, n, t, k] { f(n * k / t, n * (k + 1) / t); });
    for (auto& x : th) x.join();
}

void hash_leaf(H32& out, const uint8_t* p, uint64_t len, std::vector<uint8_t>& buf) {
    buf.resize(len + 1);
    buf[0] = 0;
    if (len) memcpy(buf.data() + 1, p, len);
    pv_sha256_host(buf.data(), len + 1, out.b);
}

void hash_children(H32& out, const H32& l, const H32& r) {
    uint8_t m[65];
    m[0] = 1;
    memcpy(m + 1, l.b, 32);
    memcpy(m + 33, r.b, 32);
    pv_sha256_host(m, 65, out.b);
}

}  // namespace

void pv_merkle_host_append(uint64_t s, const uint8_t* frontier, const uint8_t* data, const uint64_t* off, uint64_t n,
                           const PvMerkleOut* out) {
    const H32* oldf = reinterpret_cast<const H32*>(frontier);
    uint64_t n_nodes, n_front, n_path;
    pv_merkle_plan_core(s, n, &n_nodes, &n_front, &n_path);
    std::vector<H32> leaf_own, node_own;
    H32* leaf = reinterpret_cast<H32*>(out->leaf_hash);
    H32* node = reinterpret_cast<H32*>(out->node_hash);
    if (!leaf) {
        leaf_own.resize(n);
        leaf = leaf_own.data();
    }
    if (!node) {
        node_own.resize(n_nodes);
        node = node_own.data();
    }
    auto get = [&](const PvMerkleRef& r, H32& o) {
        o = r.kind == PV_MK_OLD ? oldf[r.idx] : r.kind == PV_MK_LEAF ? leaf[r.idx] : node[r.idx];
    };
    auto hash = [](H32& o, const H32& l, const H32& r) { hash_children(o, l, r); };

    parallel_for(n, [&](uint64_t lo, uint64_t hi) {
        std::vector<uint8_t> buf;
        for (uint64_t i = lo; i < hi; i++) hash_leaf(leaf[i], data + off[i], off[i + 1] - off[i], buf);
    });
    // level h from level h - 1; the nodes of one level are independent
    for (uint32_t h = 1; h <= PV_MERKLE_MAX_BITS && ((s + n) >> h) != (s >> h); h++) {
        const uint64_t first = (s >> h) + 1, count = ((s + n) >> h) - (s >> h);
        parallel_for(count, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t k = lo; k < hi; k++) {
                const uint64_t u = (first + k) << h;
                H32 l, r;
                get(pv_merkle_node_ref(s, u - (1ull << (h - 1)), h - 1), l);
                get(pv_merkle_node_ref(s, u, h - 1), r);
                hash_children(node[pv_merkle_node_pos(u, h) - pv_merkle_node_count(s)], l, r);
            }
        });
    }
    const uint64_t t = s + n;
    if (out->frontier) {
        memset(out->frontier, 0, 32 * 64);
        uint32_t k = pv_popc64(t);
        for (uint64_t rest = t; rest; rest &= rest - 1)  // ascending bits fill from the back
            get(pv_merkle_frontier_ref(s, t, (uint32_t)__builtin_ctzll(rest)), reinterpret_cast<H32*>(out->frontier)[--k]);
    }
    if (out->root) {
        H32 acc;
        if (t == 0) pv_sha256_host(acc.b, 0, acc.b);  // the empty string
        else pv_merkle_fold_root(acc, s, t, get, hash);
        memcpy(out->root, acc.b, 32);
    }
    if (out->path) {
        const uint64_t base = pv_merkle_popc_sum(s);
        parallel_for(n, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; i++) {
                const uint64_t at = pv_merkle_popc_sum(s + i) - base;
                out->path_off[i] = at;
                H32* dst = reinterpret_cast<H32*>(out->path) + at;
                pv_merkle_audit_path(s, s + i, [&](uint32_t k, const PvMerkleRef& r) { get(r, dst[k]); });
            }
        });
        out->path_off[n] = n_path;
    }
    if (out->roots)
        parallel_for(n, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; i++)
                pv_merkle_fold_root(reinterpret_cast<H32*>(out->roots)[i], s, s + i + 1, get, hash);
        });
}

void pv_merkle_host_verify(const uint8_t* data, const uint64_t* off, const uint8_t* leaf_hash,
                           const uint64_t* leaf_index, const uint64_t* tree_size, const uint8_t* proof,
                           const uint64_t* proof_off, const uint8_t* root, uint64_t n, uint8_t* status,
                           uint8_t* verdict_bits) {
    std::vector<uint8_t> ok(n);
    parallel_for(n, [&](uint64_t lo, uint64_t hi) {
        std::vector<uint8_t> buf;
        for (uint64_t i = lo; i < hi; i++) {
            H32 acc;
            if (leaf_hash) memcpy(acc.b, leaf_hash + 32 * i, 32);
            else hash_leaf(acc, data + off[i], off[i + 1] - off[i], buf);
            const H32* p = reinterpret_cast<const H32*>(proof) + proof_off[i];
            const uint32_t st = pv_merkle_path_check(
                acc, leaf_index[i], tree_size[i], proof_off[i + 1] - proof_off[i],
                [&](uint64_t k, H32& o) { o = p[k]; }, [](H32& o, const H32& l, const H32& r) { hash_children(o, l, r); });
            status[i] = (uint8_t)st;
            ok[i] = st == PV_MK_COMPARED && memcmp(acc.b, root + 32 * i, 32) == 0;
        }
    });
    memset(verdict_bits, 0, (n + 7) / 8);
    for (uint64_t i = 0; i < n; i++)
        if (ok[i]) verdict_bits[i >> 3] |= (uint8_t)(1u << (i & 7));
}

namespace {

uint32_t consistency_walk(uint64_t old_size, uint64_t new_size, const H32& old_root, const H32& new_root, const H32* p,
                          uint64_t plen) {
    return pv_merkle_consistency_check(
        old_size, new_size, old_root, new_root, plen, [&](uint64_t k, H32& o) { o = p[k]; },
        [](H32& o, const H32& l, const H32& r) { hash_children(o, l, r); },
        [](const H32& a, const H32& b) { return memcmp(a.b, b.b, 32) == 0; });
}

void pack_verdicts(const std::vector<uint8_t>& ok, uint8_t* verdict_bits) {
    const uint64_t n = ok.size();
    memset(verdict_bits, 0, (n + 7) / 8);
    for (uint64_t i = 0; i < n; i++)
        if (ok[i]) verdict_bits[i >> 3] |= (uint8_t)(1u << (i & 7));
}

}  // namespace

void pv_merkle_host_consistency(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_root,
                                const uint8_t* new_root, const uint8_t* proof, const uint64_t* proof_off, uint64_t n,
                                uint8_t* status, uint8_t* verdict_bits) {
    std::vector<uint8_t> ok(n);
    const H32* oldr = reinterpret_cast<const H32*>(old_root);
    const H32* newr = reinterpret_cast<const H32*>(new_root);
    parallel_for(n, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const uint32_t st = consistency_walk(old_size[i], new_size[i], oldr[i], newr[i],
                                                 reinterpret_cast<const H32*>(proof) + proof_off[i],
                                                 proof_off[i + 1] - proof_off[i]);
            status[i] = (uint8_t)st;
            ok[i] = st == PV_MK_CONSISTENT;
        }
    });
    pack_verdicts(ok, verdict_bits);
}

void pv_merkle_host_catchup(uint64_t s, const uint8_t* frontier, const uint8_t* data, const uint64_t* off, uint64_t n,
                            const uint64_t* reply_end, uint64_t n_replies, uint64_t final_size, const uint8_t* final_root,
                            const uint8_t* proof, const uint64_t* proof_off, const PvMerkleOut* out, uint8_t* status,
                            uint8_t* verdict_bits) {
    // the append keeps its leaf hashes and nodes here when the caller does not take them: the replies' roots fold from them
    uint64_t n_nodes, n_front, n_path;
    pv_merkle_plan_core(s, n, &n_nodes, &n_front, &n_path);
    std::vector<H32> leaf_own, node_own;
    PvMerkleOut o = *out;
    if (!o.leaf_hash && n_replies) {
        leaf_own.resize(n + 1);
        o.leaf_hash = leaf_own[0].b;
    }
    if (!o.node_hash && n_replies) {
        node_own.resize(n_nodes + 1);
        o.node_hash = node_own[0].b;
    }
    pv_merkle_host_append(s, frontier, data, off, n, &o);
    if (!n_replies) return;
    const H32* oldf = reinterpret_cast<const H32*>(frontier);
    const H32* leaf = reinterpret_cast<const H32*>(o.leaf_hash);
    const H32* node = reinterpret_cast<const H32*>(o.node_hash);
    auto get = [&](const PvMerkleRef& r, H32& h) {
        h = r.kind == PV_MK_OLD ? oldf[r.idx] : r.kind == PV_MK_LEAF ? leaf[r.idx] : node[r.idx];
    };
    auto hash = [](H32& h, const H32& l, const H32& r) { hash_children(h, l, r); };
    H32 new_root;
    memcpy(new_root.b, final_root, 32);
    std::vector<uint8_t> ok(n_replies);
    parallel_for(n_replies, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t r = lo; r < hi; r++) {
            H32 old_root;
            pv_merkle_fold_root(old_root, s, reply_end[r], get, hash);
            const uint32_t st = consistency_walk(reply_end[r], final_size, old_root, new_root,
                                                 reinterpret_cast<const H32*>(proof) + proof_off[r],
                                                 proof_off[r + 1] - proof_off[r]);
            status[r] = (uint8_t)st;
            ok[r] = st == PV_MK_CONSISTENT;
        }
    });
    pack_verdicts(ok, verdict_bits);
}

// One query at a time: the walker of merkle_core.h gathers aligned subtrees from the store, one fold follows
// for the ragged ones. A query whose length is not its slot's room writes nothing (status 2).
void pv_merkle_host_prove(const uint8_t* leaf_hash, uint64_t n_leaves, const uint8_t* node_hash, const uint8_t* kind,
                          const uint64_t* a, const uint64_t* b, uint64_t q, const uint64_t* out_off, uint8_t* out,
                          uint8_t* status, unsigned threads) {
    const H32* leaf = reinterpret_cast<const H32*>(leaf_hash);
    const H32* node = reinterpret_cast<const H32*>(node_hash);
    const uint64_t out_end = out_off[q];
    auto get = [&](const PvMerkleElem& e, H32& o) { o = e.tag == PV_MK_E_LEAF ? leaf[e.idx] : node[e.idx]; };
    auto hash = [](H32& o, const H32& l, const H32& r) { hash_children(o, l, r); };
    parallel_for(q, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            if (!pv_merkle_query_valid(kind[i], a[i], b[i], n_leaves)) {
                status[i] = PV_MK_Q_RANGE;
                continue;
            }
            if (out_off[i + 1] - out_off[i] != pv_merkle_prove_len(kind[i], a[i], b[i]) || out_off[i + 1] > out_end) {
                status[i] = PV_MK_Q_ROOM;
                continue;
            }
            H32* dst = reinterpret_cast<H32*>(out) + out_off[i];
            pv_merkle_prove<H32>(
                kind[i], a[i], b[i], [&](uint32_t k, const PvMerkleElem& e) { get(e, dst[k]); }, get, hash,
                [&](uint32_t k, const H32& acc) { dst[k] = acc; });
            status[i] = PV_MK_PROVED;
        }
    }, threads ? threads : MK_THREADS);
}

uint64_t pv_merkle_host_prove_unwritten(uint64_t n_leaves, const uint8_t* kind, const uint64_t* a, const uint64_t* b, uint64_t q,
                                        const uint64_t* out_off) {
    std::atomic<uint64_t> bad{0};
    parallel_for(q, [&](uint64_t lo, uint64_t hi) {
        uint64_t n = 0;
        for (uint64_t i = lo; i < hi; i++)
            n += !pv_merkle_query_valid(kind[i], a[i], b[i], n_leaves) ||
                 out_off[i + 1] - out_off[i] != pv_merkle_prove_len(kind[i], a[i], b[i]);
        bad += n;
    });
    return bad.load();
}
