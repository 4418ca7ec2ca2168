// Host-only check library over indy-plenum_amd/csrc/sha256.h and merkle_core.h: the Merkle kernels'
// hashing (the record loader, the prefixed leaf hash, the two-block hash_children) and their index
// arithmetic (store positions, frontier lookup, tiling, the audit-path walk) compiled for the CPU, so
// tests/test_merkle_host.py can hold them against hashlib and a restatement of the reference's tree
// without a GPU. Built with --offload-host-only like signcheck.hip.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "merkle_core.h"
#include "sha256.h"

namespace {

struct H {
    uint32_t w[8];  // digest words
};
H load(const uint8_t* p) {
    uint32_t le[8];
    memcpy(le, p, 32);
    H h;
    sha256_words_from_le(h.w, le);
    return h;
}
void store(uint8_t* p, const H& h) {
    for (int k = 0; k < 8; k++) {
        const uint32_t le = pv_bswap32(h.w[k]);
        memcpy(p + 4 * k, &le, 4);
    }
}
H children(const H& l, const H& r) {
    H o;
    sha256_hash_children(o.w, l.w, r.w);
    return o;
}
// the record at byte alignment `align` (0..7) of an 8-byte aligned buffer with room before and after
H leaf_hash(const uint8_t* data, uint64_t len, uint32_t align) {
    std::vector<uint64_t> buf((len + 8 + 16) / 8 + 2, 0xA5A5A5A5A5A5A5A5ull);  // noise around the record
    uint8_t* p = reinterpret_cast<uint8_t*>(buf.data()) + 8 + (align & 7);
    if (len) memcpy(p, data, len);
    H h;
    const PvRecordWords words(p, len);
    sha256_prefixed<1>(h.w, 0u, len, words);
    return h;
}

}  // namespace

extern "C" {

void mkc_leaf_hash(const uint8_t* data, uint64_t len, uint32_t align, uint8_t out[32]) { store(out, leaf_hash(data, len, align)); }

// SHA-256 of the bare message (no prefix byte)
void mkc_sha256(const uint8_t* data, uint64_t len, uint32_t align, uint8_t out[32]) {
    std::vector<uint64_t> buf((len + 8 + 16) / 8 + 2, 0x5A5A5A5A5A5A5A5Aull);
    uint8_t* p = reinterpret_cast<uint8_t*>(buf.data()) + 8 + (align & 7);
    if (len) memcpy(p, data, len);
    H h;
    const PvRecordWords words(p, len);
    sha256_prefixed<0>(h.w, 0u, len, words);
    store(out, h);
}

void mkc_hash_children(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]) { store(out, children(load(l), load(r))); }

void mkc_plan(uint64_t s, uint64_t n, uint64_t* nodes, uint64_t* front, uint64_t* paths) {
    pv_merkle_plan_core(s, n, nodes, front, paths);
}
uint64_t mkc_node_pos(uint64_t u, uint32_t h) { return pv_merkle_node_pos(u, h); }
uint64_t mkc_popc_sum(uint64_t x) { return pv_merkle_popc_sum(x); }
void mkc_node_ref(uint64_t s, uint64_t u, uint32_t h, uint32_t* kind, uint64_t* idx) {
    const PvMerkleRef r = pv_merkle_node_ref(s, u, h);
    *kind = r.kind;
    *idx = r.idx;
}
void mkc_frontier_ref(uint64_t s, uint64_t t, uint32_t b, uint32_t* kind, uint64_t* idx) {
    const PvMerkleRef r = pv_merkle_frontier_ref(s, t, b);
    *kind = r.kind;
    *idx = r.idx;
}
void mkc_tiles(uint64_t s, uint64_t n, uint32_t h0, uint64_t* first, uint64_t* count) { pv_merkle_tiles(s, n, h0, first, count); }
int mkc_any_above(uint64_t s, uint64_t n, uint32_t h) { return pv_merkle_any_above(s, n, h) ? 1 : 0; }

// The batch append with the kernels' decomposition, serially: leaf hashes, then the tile passes of
// merkle_core.h (each tile's levels in a local array standing for the workgroup's LDS), then the
// frontier, the root and the per-leaf outputs. Any output pointer may be null.
void mkc_append(uint64_t s, const uint8_t* frontier, const uint8_t* data, const uint64_t* off, uint64_t n,
                uint8_t* leaf_out, uint8_t* node_out, uint8_t* frontier_out, uint8_t* root_out, uint8_t* roots_out,
                uint8_t* path_out, uint64_t* path_off) {
    uint64_t n_nodes, n_front, n_path;
    pv_merkle_plan_core(s, n, &n_nodes, &n_front, &n_path);
    std::vector<uint8_t> leaf(32 * n + 32), node(32 * n_nodes + 32);
    auto at = [&](const PvMerkleRef& r) -> const uint8_t* {
        return (r.kind == PV_MK_OLD ? frontier : r.kind == PV_MK_LEAF ? leaf.data() : node.data()) + 32 * r.idx;
    };
    for (uint64_t i = 0; i < n; i++) store(leaf.data() + 32 * i, leaf_hash(data + off[i], off[i + 1] - off[i], (uint32_t)(off[i] & 7)));
    const uint64_t base = pv_merkle_node_count(s);
    std::vector<H> lds(PV_MERKLE_TILE);
    for (uint32_t h0 = 0; h0 < PV_MERKLE_MAX_BITS && (h0 == 0 ? n_nodes > 0 : pv_merkle_any_above(s, n, h0)); h0 += PV_MERKLE_TILE_LOG) {
        uint64_t first, count;
        pv_merkle_tiles(s, n, h0, &first, &count);
        for (uint64_t k = first; k < first + count; k++) {
            for (uint32_t e = 0; e < PV_MERKLE_TILE; e++) {
                const uint64_t u = ((k << PV_MERKLE_TILE_LOG) + e + 1) << h0;
                if (pv_merkle_is_new(s, n, u)) lds[e] = load(at(pv_merkle_node_ref(s, u, h0)));
            }
            for (uint32_t l = 1; l <= PV_MERKLE_TILE_LOG && h0 + l <= PV_MERKLE_MAX_BITS; l++) {
                const uint32_t h = h0 + l;
                for (uint32_t q = 0; q < (PV_MERKLE_TILE >> l); q++) {
                    const uint64_t u = ((k << PV_MERKLE_TILE_LOG) + ((uint64_t)(q + 1) << l)) << h0;
                    if (!pv_merkle_is_new(s, n, u)) continue;
                    const uint32_t ls = (2 * q) << (l - 1), rs = (2 * q + 1) << (l - 1);
                    const bool left_new = u - (1ull << (h - 1)) > s;
                    const H left = left_new ? lds[ls] : load(frontier + 32 * pv_popc64(s >> h));
                    lds[ls] = children(left, lds[rs]);
                    store(node.data() + 32 * (pv_merkle_node_pos(u, h) - base), lds[ls]);
                }
            }
        }
    }
    auto get = [&](const PvMerkleRef& r, H& o) { o = load(at(r)); };
    auto hash = [](H& o, const H& l, const H& r) { o = children(l, r); };
    const uint64_t t = s + n;
    if (leaf_out) memcpy(leaf_out, leaf.data(), 32 * n);
    if (node_out) memcpy(node_out, node.data(), 32 * n_nodes);
    if (frontier_out) {
        memset(frontier_out, 0, 32 * 64);
        uint32_t k = pv_popc64(t);
        for (uint64_t rest = t; rest; rest &= rest - 1)
            memcpy(frontier_out + 32 * --k, at(pv_merkle_frontier_ref(s, t, (uint32_t)__builtin_ctzll(rest))), 32);
    }
    if (root_out && t) {
        H acc;
        pv_merkle_fold_root(acc, s, t, get, hash);
        store(root_out, acc);
    }
    for (uint64_t i = 0; i < n; i++) {
        if (path_out) {
            const uint64_t o = pv_merkle_popc_sum(s + i) - pv_merkle_popc_sum(s);
            path_off[i] = o;
            path_off[i + 1] = o + pv_merkle_audit_path(s, s + i, [&](uint32_t k, const PvMerkleRef& r) { memcpy(path_out + 32 * (o + k), at(r), 32); });
        }
        if (roots_out) {
            H acc;
            pv_merkle_fold_root(acc, s, s + i + 1, get, hash);
            store(roots_out + 32 * i, acc);
        }
    }
}

// status of the audit-path walk; *ok = 1 iff it ends on `root`
uint32_t mkc_verify(const uint8_t leaf_hash_in[32], uint64_t index, uint64_t size, const uint8_t* proof, uint64_t plen,
                    const uint8_t root[32], int* ok) {
    H acc = load(leaf_hash_in);
    const uint32_t st = pv_merkle_path_check(
        acc, index, size, plen, [&](uint64_t k, H& o) { o = load(proof + 32 * k); },
        [](H& o, const H& l, const H& r) { o = children(l, r); });
    uint8_t got[32];
    store(got, acc);
    *ok = st == PV_MK_COMPARED && memcmp(got, root, 32) == 0;
    return st;
}

}  // extern "C"
