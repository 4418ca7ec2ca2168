// Host side of the batched state-trie update: n sequential PruningState.set calls
// (state/pruning_state.py:60-61 over state/trie/pruning_trie.py:1006-1027) as one pass.
//
// The trie is canonical (its shape depends on the key -> value mapping alone), so the batch is sorted
// by key and pushed down the existing trie as whole groups: at a branch the group splits by its next
// nibble, at an extension it either passes through or splits the path where its first and last key
// leave it, at a leaf the leaf's own entry joins the group, and below any blank slot the group's
// subtrie is built fresh from its common prefixes. Only nodes a group reaches are decoded; every other
// child stays the 32-byte reference (or the embedded RLP) its parent already holds. Existing nodes come
// from the caller: one that is needed and absent is reported, not fetched (no callback crosses the ABI).
//
// The RLP length of every new node is known before any hash is: a child is 33 bytes when its own RLP
// has 32 bytes or more, and its RLP itself below that (pruning_trie.py:339-340). So every node to hash
// is laid out in one arena, 64-bit aligned, with a 32-byte hole where each hashed child's digest goes,
// and the hashing (keccak.h here, pv_trie.hip on the device) runs depth by depth, deepest first.
//
// At the end of the file, the host side of state-proof verification: splitting serialized proofs into
// records, the argument checks of the host-buffer entry, and the host path of the two stages.
#include "trie_host.h"

#include <string.h>

#include <algorithm>
#include <deque>
#include <memory>
#include <stdexcept>
#include <thread>
#include <unordered_map>
#include <unordered_set>

#include "../../include/plenum_verify.h"
#include "keccak.h"
#include "trie_core.h"

const uint8_t PV_TRIE_BLANK_ROOT[32] = {0xbc, 0x20, 0x71, 0xa4, 0xde, 0x84, 0x6f, 0x28, 0x57, 0x02, 0x44,
                                        0x7f, 0x25, 0x89, 0xdd, 0x16, 0x36, 0x78, 0xe0, 0x97, 0x2a, 0x8a,
                                        0x1b, 0x0d, 0x28, 0xb0, 0x4e, 0xd5, 0xc0, 0x94, 0x54, 0x7f};  // SHA3-256(0x80)

namespace {

constexpr unsigned TR_THREADS = 16;
constexpr uint64_t TR_PER_THREAD = 128;  // records below which a thread is not worth starting

template <class F>
void parallel_for(uint64_t n, const F& f) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const uint64_t t = std::min<uint64_t>(std::min(TR_THREADS, hw), (n + TR_PER_THREAD - 1) / TR_PER_THREAD);
    if (t <= 1) {
        if (n) f(0, n);
        return;
    }
    std::vector<std::thread> th;
    for (uint64_t k = 0; k < t; k++) th.emplace_back([&f, n, t, k] { f(n * k / t, n * (k + 1) / t); });
    for (auto& x : th) x.join();
}

struct DecodeError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

struct H32 {
    uint8_t b[32];
    bool operator==(const H32& o) const { return memcmp(b, o.b, 32) == 0; }
};
struct H32Hash {
    size_t operator()(const H32& h) const {
        uint64_t x;
        memcpy(&x, h.b, 8);  // the keys are digests already
        return (size_t)x;
    }
};

struct Node;
struct Ref {
    uint8_t kind = TR_BLANK;  // TR_BLANK, TR_HASH (p: 32 bytes), TR_RAW (p: an embedded node's RLP), TR_NEW (node)
    const uint8_t* p = nullptr;
    uint64_t len = 0;
    Node* node = nullptr;
};
struct Node {
    int kind = 0;
    const uint8_t* path = nullptr;  // leaf / extension: nibbles
    uint32_t plen = 0;
    const uint8_t* val = nullptr;  // leaf: value; branch: value slot (vlen 0 = none)
    uint64_t vlen = 0;
    Ref* child = nullptr;  // branch: 16; extension: 1
    uint64_t pay = 0, enc = 0;  // RLP payload and whole length
};
// A batch entry, or an existing leaf's entry joining a group: nib[i] is valid from the depth at which
// the entry is looked at.
struct Item {
    const uint8_t* nib;
    uint32_t nlen;
    const uint8_t* val;
    uint64_t vlen;
};

struct Builder {
    std::unordered_map<H32, std::pair<const uint8_t*, uint64_t>, H32Hash> known;
    std::unordered_set<H32, H32Hash> missing_seen;
    std::vector<uint8_t>* missing;
    std::deque<Node> nodes;
    std::deque<std::unique_ptr<Ref[]>> kids;
    std::deque<std::unique_ptr<uint8_t[]>> nibs;

    Node* node(int kind) {
        nodes.emplace_back();
        nodes.back().kind = kind;
        return &nodes.back();
    }
    Ref* children(uint32_t n) {
        kids.emplace_back(new Ref[n]);
        return kids.back().get();
    }
    uint8_t* nibbles(uint64_t n) {
        nibs.emplace_back(new uint8_t[n ? n : 1]);
        return nibs.back().get();
    }
    static Ref fresh_ref(Node* n) {
        Ref r;
        r.kind = TR_NEW;
        r.node = n;
        return r;
    }
    Node* leaf(const uint8_t* path, uint32_t plen, const uint8_t* val, uint64_t vlen) {
        Node* n = node(TR_LEAF);
        n->path = path;
        n->plen = plen;
        n->val = val;
        n->vlen = vlen;
        return n;
    }
    Node* ext(const uint8_t* path, uint32_t plen, const Ref& child) {
        Node* n = node(TR_EXT);
        n->path = path;
        n->plen = plen;
        n->child = children(1);
        n->child[0] = child;
        return n;
    }
    Node* branch() {
        Node* n = node(TR_BRANCH);
        n->child = children(16);
        return n;
    }

    // The existing node behind a hash or an embedded RLP, decoded; null when it was not given.
    Node* load(const Ref& r) {
        const uint8_t* p = r.p;
        uint64_t len = r.len;
        if (r.kind == TR_HASH) {
            H32 h;
            memcpy(h.b, r.p, 32);
            auto it = known.find(h);
            if (it == known.end()) {
                if (missing_seen.insert(h).second) missing->insert(missing->end(), h.b, h.b + 32);
                return nullptr;
            }
            p = it->second.first;
            len = it->second.second;
        }
        TrDecoded d;
        if (!tr_decode_node(p, len, &d)) throw DecodeError("an existing node is not a well-formed trie node");
        auto conv = [](const TrChild& c) {
            Ref o;
            o.kind = c.kind;
            o.p = c.p;
            o.len = c.len;
            return o;
        };
        if (d.kind == TR_BRANCH) {
            Node* n = branch();
            for (int i = 0; i < 16; i++) n->child[i] = conv(d.child[i]);
            n->val = d.value;
            n->vlen = d.value_len;
            return n;
        }
        uint8_t* nib = nibbles(d.nibbles);
        tr_hp_unpack(nib, d.hp, d.hp_len);
        if (d.kind == TR_LEAF) return leaf(nib, d.nibbles, d.value, d.value_len);
        return ext(nib, d.nibbles, conv(d.child[0]));
    }

    static uint32_t lcp(const uint8_t* a, uint32_t an, const uint8_t* b, uint32_t bn) {
        const uint32_t m = std::min(an, bn);
        uint32_t i = 0;
        while (i < m && a[i] == b[i]) i++;
        return i;
    }
    // order of two entries from nibble `off` on: a shorter key before its extensions
    static int cmp(const Item& a, const Item& b, uint32_t off) {
        const uint32_t m = std::min(a.nlen, b.nlen);
        for (uint32_t i = off; i < m; i++)
            if (a.nib[i] != b.nib[i]) return a.nib[i] < b.nib[i] ? -1 : 1;
        return a.nlen == b.nlen ? 0 : a.nlen < b.nlen ? -1 : 1;
    }

    // The group (sorted, distinct keys, all equal on nibbles [0, off)) into the branch b at depth off.
    Node* branch_apply(Node* b, const Item* it, size_t n, uint32_t off) {
        size_t i = 0;
        if (n && it[0].nlen == off) {
            b->val = it[0].val;
            b->vlen = it[0].vlen;
            i = 1;
        }
        while (i < n) {
            const uint8_t nb = it[i].nib[off];
            size_t j = i + 1;
            while (j < n && it[j].nib[off] == nb) j++;
            b->child[nb] = update(b->child[nb], it + i, j - i, off + 1);
            i = j;
        }
        return b;
    }

    // The subtrie of a group below a blank slot.
    Ref fresh(const Item* it, size_t n, uint32_t off) {
        if (n == 1) return fresh_ref(leaf(it[0].nib + off, it[0].nlen - off, it[0].val, it[0].vlen));
        const uint32_t m = lcp(it[0].nib + off, it[0].nlen - off, it[n - 1].nib + off, it[n - 1].nlen - off);
        Node* b = branch_apply(branch(), it, n, off + m);
        return fresh_ref(m ? ext(it[0].nib + off, m, fresh_ref(b)) : b);
    }

    Ref update(const Ref& r, const Item* it, size_t n, uint32_t off) {
        if (n == 0) return r;
        if (r.kind == TR_BLANK) return fresh(it, n, off);
        Node* nd = r.kind == TR_NEW ? r.node : load(r);
        if (!nd) return r;  // reported missing: the caller comes back with it
        if (nd->kind == TR_BRANCH) return fresh_ref(branch_apply(nd, it, n, off));
        if (nd->kind == TR_LEAF) {
            // the leaf's own entry joins the group unless the group overwrites it
            uint8_t* nib = nibbles((uint64_t)off + nd->plen);
            if (nd->plen) memcpy(nib + off, nd->path, nd->plen);
            const Item own{nib, off + nd->plen, nd->val, nd->vlen};
            std::vector<Item> all;
            all.reserve(n + 1);
            size_t i = 0;
            int c = 1;
            while (i < n && (c = cmp(it[i], own, off)) < 0) all.push_back(it[i++]);
            if (c != 0) all.push_back(own);
            all.insert(all.end(), it + i, it + n);
            return fresh(all.data(), all.size(), off);
        }
        // extension: the group passes through, or leaves the path at its smallest common prefix with it
        const uint32_t m = std::min(lcp(it[0].nib + off, it[0].nlen - off, nd->path, nd->plen),
                                    lcp(it[n - 1].nib + off, it[n - 1].nlen - off, nd->path, nd->plen));
        if (m == nd->plen) {
            nd->child[0] = update(nd->child[0], it, n, off + m);
            return fresh_ref(nd);
        }
        Node* b = branch();
        const uint32_t rest = nd->plen - m - 1;
        b->child[nd->path[m]] = rest ? fresh_ref(ext(nd->path + m + 1, rest, nd->child[0])) : nd->child[0];
        branch_apply(b, it, n, off + m);
        return fresh_ref(m ? ext(nd->path, m, fresh_ref(b)) : b);
    }

    // ---------------------------------------------------------------------------- sizes and layout
    uint64_t n_hashed = 0, arena_bytes = 0;

    static uint64_t hp_str_size(uint32_t plen) {
        const uint64_t b = tr_hp_size(plen);
        return b == 1 ? 1 : tr_prefix_size(b) + b;  // a one-byte path is below 0x40: its own encoding
    }
    uint64_t child_size(const Ref& r) {
        if (r.kind == TR_BLANK) return 1;
        if (r.kind == TR_HASH) return 33;
        if (r.kind == TR_RAW) return r.len;
        const uint64_t s = size(r.node);
        if (s < 32) return s;
        n_hashed++;
        arena_bytes += (s + 7) & ~7ull;
        return 33;
    }
    uint64_t payload(const Node* n) {
        if (n->kind == TR_LEAF) return hp_str_size(n->plen) + tr_str_size(n->val, n->vlen);
        if (n->kind == TR_EXT) return hp_str_size(n->plen) + child_size(n->child[0]);
        uint64_t s = n->vlen ? tr_str_size(n->val, n->vlen) : 1;
        for (int i = 0; i < 16; i++) s += child_size(n->child[i]);
        return s;
    }
    uint64_t size(Node* n) {
        n->pay = payload(n);
        n->enc = tr_list_size(n->pay);
        return n->enc;
    }

    uint8_t* arena = nullptr;
    uint64_t cur = 0;
    std::vector<PvTrieRec>* recs = nullptr;

    void put_hp(uint8_t*& d, const Node* n) {
        const uint32_t b = tr_hp_size(n->plen);
        if (b > 1) d += tr_put_prefix(d, b, 0x80);
        tr_hp_pack(d, n->path, n->plen, n->kind == TR_LEAF);
        d += b;
    }
    void put_child(uint8_t*& d, const Ref& r, uint32_t depth) {
        if (r.kind == TR_BLANK) {
            *d++ = 0x80;
        } else if (r.kind == TR_HASH) {
            *d++ = 0xa0;
            memcpy(d, r.p, 32);
            d += 32;
        } else if (r.kind == TR_RAW) {
            memcpy(d, r.p, r.len);
            d += r.len;
        } else if (r.node->enc < 32) {
            put_node(d, r.node, depth);  // embedded: it holds no hash reference, written whole
        } else {
            *d++ = 0xa0;
            memset(d, 0, 32);
            record(r.node, depth + 1, (uint64_t)(d - arena));
            d += 32;
        }
    }
    void put_node(uint8_t*& d, const Node* n, uint32_t depth) {
        d += tr_put_prefix(d, n->pay, 0xc0);
        if (n->kind == TR_LEAF) {
            put_hp(d, n);
            d += tr_put_str(d, n->val, n->vlen);
        } else if (n->kind == TR_EXT) {
            put_hp(d, n);
            put_child(d, n->child[0], depth);
        } else {
            for (int i = 0; i < 16; i++) put_child(d, n->child[i], depth);
            if (n->vlen) d += tr_put_str(d, n->val, n->vlen);
            else *d++ = 0x80;
        }
    }
    void record(const Node* n, uint32_t depth, uint64_t hole) {
        PvTrieRec r;
        r.off = cur;
        r.hole = hole;
        r.len = (uint32_t)n->enc;
        r.depth = depth;
        r.next = 0;
        r.pad = 0;
        cur += (n->enc + 7) & ~7ull;
        recs->push_back(r);
        uint8_t* d = arena + r.off;
        put_node(d, n, depth);
    }
};

}  // namespace

int pv_trie_host_build(const PvTrieIn& in, PvTriePlan* plan, std::string* err) {
    plan->recs.clear();
    plan->missing.clear();
    plan->arena_bytes = 0;
    plan->blank = false;
    uint64_t nib_total = 0;
    for (uint64_t i = 0; i < in.n; i++) {
        const uint64_t kl = in.key_off[i + 1] - in.key_off[i], vl = in.val_off[i + 1] - in.val_off[i];
        if (kl > PV_TRIE_MAX_KEY) {
            *err = "a key is longer than 65,535 bytes";
            return PV_ERR_ARG;
        }
        if (vl == 0 || vl > PV_TRIE_MAX_VALUE) {
            *err = "a value is empty or not below 2^24 bytes";
            return PV_ERR_ARG;
        }
        nib_total += 2 * kl;
    }
    if ((in.n >> 32) || (in.n_known >> 32)) {
        *err = "more than 2^32 - 1 entries";
        return PV_ERR_ARG;
    }
    try {
        Builder b;
        b.missing = &plan->missing;
        b.known.reserve(in.n_known);
        for (uint64_t i = 0; i < in.n_known; i++) {
            H32 h;
            memcpy(h.b, in.known_hash + 32 * i, 32);
            b.known[h] = {in.known_blob + in.known_off[i], in.known_off[i + 1] - in.known_off[i]};
        }
        // the batch in key order, the last entry of a key only
        std::vector<uint32_t> order(in.n);
        for (uint64_t i = 0; i < in.n; i++) order[i] = (uint32_t)i;
        auto key = [&](uint32_t i, uint64_t* len) {
            *len = in.key_off[i + 1] - in.key_off[i];
            return in.key_blob + in.key_off[i];
        };
        auto kcmp = [&](uint32_t x, uint32_t y) {
            uint64_t xl, yl;
            const uint8_t* xp = key(x, &xl);
            const uint8_t* yp = key(y, &yl);
            const uint64_t m = std::min(xl, yl);
            const int c = m ? memcmp(xp, yp, m) : 0;
            return c ? c : xl == yl ? 0 : xl < yl ? -1 : 1;
        };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return kcmp(x, y) < 0; });
        std::vector<uint8_t> nib(nib_total ? nib_total : 1);
        std::vector<Item> items;
        items.reserve(in.n);
        uint64_t at = 0;
        for (uint64_t k = 0; k < in.n; k++) {
            if (k + 1 < in.n && kcmp(order[k], order[k + 1]) == 0) continue;  // a later entry for the key wins
            uint64_t kl;
            const uint8_t* kp = key(order[k], &kl);
            uint8_t* dst = nib.data() + at;
            for (uint64_t i = 0; i < kl; i++) {
                dst[2 * i] = kp[i] >> 4;
                dst[2 * i + 1] = kp[i] & 15;
            }
            at += 2 * kl;
            const uint32_t j = order[k];
            items.push_back(Item{dst, (uint32_t)(2 * kl), in.val_blob + in.val_off[j], in.val_off[j + 1] - in.val_off[j]});
        }
        Ref root;
        if (memcmp(in.root, PV_TRIE_BLANK_ROOT, 32) != 0) {
            root.kind = TR_HASH;
            root.p = in.root;
            root.len = 32;
        }
        const Ref out = b.update(root, items.data(), items.size(), 0);
        if (!plan->missing.empty()) return PV_TRIE_NEED_NODES;
        if (out.kind != TR_NEW) {  // nothing was set
            plan->blank = out.kind == TR_BLANK;
            return PV_OK;
        }
        const uint64_t s = b.size(out.node);
        b.n_hashed++;  // the root is always hashed
        b.arena_bytes += (s + 7) & ~7ull;
        if (b.n_hashed >> 32) {
            *err = "more than 2^32 - 1 nodes";
            return PV_ERR_ARG;
        }
        plan->arena.assign(b.arena_bytes / 8 + 1, 0);
        plan->arena_bytes = b.arena_bytes;
        plan->recs.reserve(b.n_hashed);
        b.arena = reinterpret_cast<uint8_t*>(plan->arena.data());
        b.recs = &plan->recs;
        b.record(out.node, 0, PV_TRIE_NO_HOLE);
        std::stable_sort(plan->recs.begin(), plan->recs.end(),
                         [](const PvTrieRec& x, const PvTrieRec& y) { return x.depth > y.depth; });
        const uint64_t nr = plan->recs.size();
        for (uint64_t i = nr; i-- > 0;)
            plan->recs[i].next = i + 1 < nr && plan->recs[i + 1].depth == plan->recs[i].depth ? plan->recs[i + 1].next
                                                                                           : (uint32_t)(i + 1);
        return PV_OK;
    } catch (const DecodeError& e) {
        *err = e.what();
        return PV_ERR_DECODE;
    } catch (const std::bad_alloc&) {
        *err = "out of memory";
        return PV_ERR_ALLOC;
    }
}

void pv_trie_host_hash(uint8_t* arena, const PvTrieRec* recs, uint64_t n, uint8_t* hashes) {
    for (uint64_t i0 = 0; i0 < n;) {
        const uint64_t i1 = recs[i0].next;
        parallel_for(i1 - i0, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = i0 + lo; i < i0 + hi; i++) {
                uint64_t d[4];
                sha3_256(d, recs[i].len, PvKeccakWords(arena + recs[i].off, recs[i].len));
                memcpy(hashes + 32 * i, d, 32);
                if (recs[i].hole != PV_TRIE_NO_HOLE) memcpy(arena + recs[i].hole, d, 32);
            }
        });
        i0 = i1;
    }
}

// ---------------------------------------------------------------------------------- state proofs

int pv_proof_check_args(const PvProofIn& in, const char** err) {
    auto bad = [&](const char* why) {
        *err = why;
        return PV_ERR_ARG;
    };
    auto monotone = [](const uint64_t* o, uint64_t k) {
        for (uint64_t i = 0; i < k; i++)
            if (o[i + 1] < o[i]) return false;
        return true;
    };
    if (!in.proof_first || !in.query_proof || !in.root || !in.key_off || !in.val_off || !in.node_off)
        return bad("null pointer");
    if ((in.n_nodes >> 31) || (in.n_queries >> 31) || (in.n_proofs >> 31)) return bad("more than 2^31 - 1 records, proofs or queries");
    if (!monotone(in.proof_first, in.n_proofs) || !monotone(in.key_off, in.n_queries) || !monotone(in.val_off, in.n_queries) ||
        (!in.node_len && !monotone(in.node_off, in.n_nodes)))
        return bad("offsets must be non-decreasing");
    if (in.proof_first[in.n_proofs] > in.n_nodes) return bad("proof_first reaches past the records");
    for (uint64_t p = 0; p < in.n_proofs; p++)
        if (in.proof_first[p + 1] - in.proof_first[p] > PV_PROOF_MAX_NODES) return bad("a proof of more than 1,024 records");
    bool bytes = false;
    for (uint64_t i = 0; i < in.n_nodes && !bytes; i++) bytes = in.node_len ? in.node_len[i] != 0 : in.node_off[i + 1] != in.node_off[i];
    if (bytes && !in.node_blob) return bad("null node blob");
    if ((!in.key_blob && in.key_off[in.n_queries] != in.key_off[0]) || (!in.val_blob && in.val_off[in.n_queries] != in.val_off[0]))
        return bad("null key or value blob");
    for (uint64_t i = 0; i < in.n_queries; i++) {
        if (in.query_proof[i] >= in.n_proofs) return bad("a query names a proof that is not there");
        if (in.key_off[i + 1] - in.key_off[i] > PV_TRIE_MAX_KEY) return bad("a key is longer than 65,535 bytes");
        if (in.val_off[i + 1] - in.val_off[i] > PV_TRIE_MAX_VALUE) return bad("a value is not below 2^24 bytes");
    }
    return PV_OK;
}

void pv_proof_host(const PvProofIn& in, uint8_t* status) {
    std::vector<uint64_t> digest(4 * in.n_nodes + 1);
    std::vector<uint8_t> flag(in.n_nodes + 1);  // 1: the record is not canonical RLP
    parallel_for(in.n_nodes, [&](uint64_t lo, uint64_t hi) {
        std::vector<uint64_t> buf;
        for (uint64_t i = lo; i < hi; i++) {
            const uint64_t len = in.node_len ? in.node_len[i] : in.node_off[i + 1] - in.node_off[i];
            const uint8_t* p = in.node_blob + in.node_off[i];
            buf.assign(len / 8 + 1, 0);  // aligned and whole words: what the word reader loads
            if (len) memcpy(buf.data(), p, len);
            sha3_256(&digest[4 * i], len, PvKeccakWords(reinterpret_cast<const uint8_t*>(buf.data()), len));
            flag[i] = tr_rlp_canonical(p, len) ? 0 : 1;
        }
    });
    // queries are cheap next to records: a thread per 128 of them as well
    parallel_for(in.n_queries, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const uint64_t first = in.proof_first[in.query_proof[i]], count = in.proof_first[in.query_proof[i] + 1] - first;
            bool clean = true;
            for (uint64_t j = first; j < first + count; j++) clean &= flag[j] == 0;
            status[i] = !clean ? (uint8_t)TR_PROOF_DEFER
                               : (uint8_t)tr_proof_walk(in.node_blob, in.node_off, in.node_len, digest.data(), first, count,
                                                        in.root + 32 * i, in.key_blob + in.key_off[i],
                                                        in.key_off[i + 1] - in.key_off[i], in.val_blob + in.val_off[i],
                                                        in.val_off[i + 1] - in.val_off[i]);
        }
    });
}

int pv_proof_split_host(const uint8_t* ser, const uint64_t* ser_off, uint64_t n_proofs, uint64_t* proof_first,
                        uint64_t* node_off, uint64_t* node_len, uint64_t node_cap, uint64_t* n_nodes, uint8_t* proof_ok) {
    uint64_t n = 0;
    for (uint64_t p = 0; p < n_proofs; p++) {
        proof_first[p] = n;
        proof_ok[p] = 0;
        const uint8_t* a = ser + ser_off[p];
        const uint8_t* b = ser + ser_off[p + 1];
        TrItem top, it;
        if (!tr_rlp_item(a, b, &top) || !top.list || top.raw + top.raw_len != b) continue;
        bool ok = true;
        uint64_t k = 0;
        for (const uint8_t* q = top.p; q < b; q += it.raw_len, k++)
            if (!(ok = tr_rlp_item(q, b, &it))) break;
        if (!ok) continue;
        proof_ok[p] = 1;
        for (const uint8_t* q = top.p; q < b; q += it.raw_len, n++) {
            tr_rlp_item(q, b, &it);
            if (n < node_cap) {
                node_off[n] = (uint64_t)(q - ser);
                node_len[n] = it.raw_len;
            }
        }
    }
    proof_first[n_proofs] = n;
    *n_nodes = n;
    if (n > node_cap) return PV_TRIE_NEED_SPACE;
    node_off[n] = n_proofs ? ser_off[n_proofs] : 0;  // n + 1 entries, as PvProofIn's
    return PV_OK;
}

void pv_sha3_host_batch(const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* out) {
    parallel_for(n, [&](uint64_t lo, uint64_t hi) {
        std::vector<uint64_t> buf;
        for (uint64_t i = lo; i < hi; i++) {
            // an aligned private copy: the word reader loads whole aligned words, which must not leave the caller's buffer
            const uint64_t len = off[i + 1] - off[i];
            buf.assign(len / 8 + 1, 0);
            if (len) memcpy(buf.data(), data + off[i], len);
            uint64_t d[4];
            sha3_256(d, len, PvKeccakWords(reinterpret_cast<const uint8_t*>(buf.data()), len));
            memcpy(out + 32 * i, d, 32);
        }
    });
}
