// The state trie's node format (state/trie/pruning_trie.py in the reference): RLP of byte strings and
// lists, hex-prefix packing of nibble paths, and the three node kinds
//   leaf       [hp(path + terminator), value]
//   extension  [hp(path), child]
//   branch     [child 0 .. child 15, value]
// where a child is the empty string (blank), a 32-byte string (the SHA3-256 of the child's RLP) or, for
// a child whose RLP is shorter than 32 bytes, that RLP itself as a nested list (pruning_trie.py:334-344).
//
// Plain C++, no allocation, every read bounded by the record: node bytes come from a database, so
// decoding rejects whatever an encoder would not have written (truncated or oversized length prefixes,
// non-minimal lengths, lists that are not 2 or 17 items long, children of any other length) instead of
// reading on. Shared by the host path (trie_host.cpp), the host-compiled check libraries
// (tests/native/triecheck.hip, proofcheck.hip) and, for the PV_HD functions (the item parser and the state-proof
// canonical check and walk at the end of this file), the kernels of pv_trie.hip.
#ifndef PV_TRIE_CORE_H
#define PV_TRIE_CORE_H

#include <stdint.h>
#include <string.h>

#ifndef PV_HD
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define PV_HD __host__ __device__ __forceinline__
#else
#define PV_HD inline
#endif
#endif

static constexpr uint32_t PV_TRIE_MAX_KEY = 65535;          // key bytes
static constexpr uint64_t PV_TRIE_MAX_VALUE = (1ull << 24) - 1;  // value bytes (a three-byte RLP length)

// ------------------------------------------------------------------------------------------- RLP

// bytes of the length prefix of a payload of `len` bytes (strings of one byte below 0x80 have none)
PV_HD uint32_t tr_prefix_size(uint64_t len) {
    if (len < 56) return 1;
    uint32_t ll = 0;
    for (uint64_t x = len; x; x >>= 8) ll++;
    return 1 + ll;
}
inline uint64_t tr_str_size(const uint8_t* p, uint64_t len) {
    return len == 1 && p[0] < 0x80 ? 1 : tr_prefix_size(len) + len;
}
PV_HD uint64_t tr_list_size(uint64_t payload) { return tr_prefix_size(payload) + payload; }

// writes the prefix (base 0x80 string, 0xc0 list), returns the bytes written
PV_HD uint32_t tr_put_prefix(uint8_t* dst, uint64_t len, uint8_t base) {
    if (len < 56) {
        dst[0] = (uint8_t)(base + len);
        return 1;
    }
    const uint32_t ll = tr_prefix_size(len) - 1;
    dst[0] = (uint8_t)(base + 55 + ll);
    for (uint32_t i = 0; i < ll; i++) dst[1 + i] = (uint8_t)(len >> (8 * (ll - 1 - i)));
    return 1 + ll;
}
inline uint64_t tr_put_str(uint8_t* dst, const uint8_t* p, uint64_t len) {
    if (len == 1 && p[0] < 0x80) {
        dst[0] = p[0];
        return 1;
    }
    const uint32_t h = tr_put_prefix(dst, len, 0x80);
    if (len) memcpy(dst + h, p, len);
    return h + len;
}

struct TrItem {
    const uint8_t* raw;  // the item with its prefix
    uint64_t raw_len;
    const uint8_t* p;    // the payload
    uint64_t len;
    bool list;
};

// The item at p, which must end at or before `end`. False on malformed input.
PV_HD bool tr_rlp_item(const uint8_t* p, const uint8_t* end, TrItem* it) {
    if (p >= end) return false;
    const uint64_t avail = (uint64_t)(end - p);
    const uint8_t b0 = p[0];
    uint64_t head = 1, len;
    bool list = b0 >= 0xc0;
    if (b0 < 0x80) {
        head = 0;
        len = 1;
    } else {
        const uint8_t v = (uint8_t)(b0 - (list ? 0xc0 : 0x80));
        if (v < 56) {
            len = v;
        } else {
            const uint32_t ll = v - 55;  // 1 .. 8
            if (ll > avail - 1) return false;  // truncated length prefix
            if (p[1] == 0) return false;       // leading zero
            len = 0;
            for (uint32_t i = 0; i < ll; i++) len = (len << 8) | p[1 + i];
            if (len < 56) return false;  // non-minimal
            head = 1 + ll;
        }
    }
    if (len > avail - head) return false;  // runs past the buffer
    if (!list && len == 1 && head == 1 && p[1] < 0x80) return false;  // a single byte is its own encoding
    it->raw = p;
    it->raw_len = head + len;
    it->p = p + head;
    it->len = len;
    it->list = list;
    return true;
}

// ------------------------------------------------------------------------------------ hex prefix

// hp(nibbles[0..n), terminator): n / 2 + 1 bytes to dst
PV_HD uint32_t tr_hp_size(uint32_t n) { return n / 2 + 1; }
inline void tr_hp_pack(uint8_t* dst, const uint8_t* nib, uint32_t n, bool term) {
    const uint8_t flags = (uint8_t)((term ? 2 : 0) | (n & 1));
    uint32_t i = 0;
    if (n & 1) dst[0] = (uint8_t)(16 * flags + nib[i++]);
    else dst[0] = (uint8_t)(16 * flags);
    for (uint32_t o = 1; i < n; i += 2, o++) dst[o] = (uint8_t)(16 * nib[i] + nib[i + 1]);
}
// nibble count of a packed path, or -1 when it is malformed (empty, flags above 3, padding nibble set)
PV_HD int64_t tr_hp_nibbles(const uint8_t* p, uint64_t len, bool* term) {
    if (len == 0 || len > (uint64_t)PV_TRIE_MAX_KEY + 1) return -1;
    const uint8_t flags = p[0] >> 4;
    if (flags > 3) return -1;
    if (!(flags & 1) && (p[0] & 15)) return -1;
    *term = (flags & 2) != 0;
    return (int64_t)(2 * (len - 1) + (flags & 1));
}
inline void tr_hp_unpack(uint8_t* nib, const uint8_t* p, uint64_t len) {
    uint32_t o = 0;
    if ((p[0] >> 4) & 1) nib[o++] = p[0] & 15;
    for (uint64_t i = 1; i < len; i++) {
        nib[o++] = p[i] >> 4;
        nib[o++] = p[i] & 15;
    }
}

// ----------------------------------------------------------------------------------------- nodes

enum { TR_BLANK = 0, TR_HASH = 1, TR_RAW = 2, TR_NEW = 3 };  // what a child slot holds
enum { TR_LEAF = 1, TR_EXT = 2, TR_BRANCH = 3 };

struct TrChild {
    uint8_t kind;       // TR_BLANK, TR_HASH (p = 32 bytes), TR_RAW (p = an embedded node's RLP, len bytes)
    const uint8_t* p;
    uint64_t len;
};

struct TrDecoded {
    int kind;            // TR_LEAF, TR_EXT, TR_BRANCH
    const uint8_t* hp;   // leaf / extension: the packed path
    uint64_t hp_len;
    uint32_t nibbles;
    const uint8_t* value;  // leaf: the value; branch: the value slot (len 0 = none)
    uint64_t value_len;
    TrChild child[16];     // extension: child[0]
};

PV_HD bool tr_child(const TrItem& it, TrChild* c, bool may_be_blank) {
    if (it.list) {
        c->kind = TR_RAW;
        c->p = it.raw;
        c->len = it.raw_len;
        return true;
    }
    if (it.len == 32) {
        c->kind = TR_HASH;
        c->p = it.p;
        c->len = 32;
        return true;
    }
    if (it.len == 0 && may_be_blank) {
        c->kind = TR_BLANK;
        c->p = nullptr;
        c->len = 0;
        return true;
    }
    return false;
}

// One node from exactly the bytes [p, p + len). False on malformed input.
inline bool tr_decode_node(const uint8_t* p, uint64_t len, TrDecoded* d) {
    TrItem top;
    if (!tr_rlp_item(p, p + len, &top) || !top.list || top.raw_len != len) return false;
    const uint8_t* q = top.p;
    const uint8_t* end = top.p + top.len;
    TrItem it[17];
    uint32_t n = 0;
    while (q < end) {
        if (n == 17 || !tr_rlp_item(q, end, &it[n])) return false;
        q += it[n].raw_len;
        n++;
    }
    if (n == 2) {
        bool term;
        if (it[0].list) return false;
        const int64_t nib = tr_hp_nibbles(it[0].p, it[0].len, &term);
        if (nib < 0) return false;
        d->hp = it[0].p;
        d->hp_len = it[0].len;
        d->nibbles = (uint32_t)nib;
        if (term) {
            if (it[1].list || it[1].len == 0 || it[1].len > PV_TRIE_MAX_VALUE) return false;
            d->kind = TR_LEAF;
            d->value = it[1].p;
            d->value_len = it[1].len;
            return true;
        }
        if (nib == 0) return false;  // an extension has a path
        d->kind = TR_EXT;
        return tr_child(it[1], &d->child[0], false);
    }
    if (n != 17) return false;
    d->kind = TR_BRANCH;
    for (uint32_t i = 0; i < 16; i++)
        if (!tr_child(it[i], &d->child[i], true)) return false;
    if (it[16].list || it[16].len > PV_TRIE_MAX_VALUE) return false;
    d->value = it[16].p;
    d->value_len = it[16].len;
    return true;
}

// ---------------------------------------------------------------------------------- state proofs
//
// A proof is a pool of node records; a query (root, key, expected value) is answered by walking from the
// record whose SHA3-256 is the root (pruning_trie.py:1100-1119). Two stages, the same source on the
// device (pv_trie.hip), on host threads (trie_host.cpp) and in the host-compiled check library
// (tests/native/proofcheck.hip): per record a digest and tr_rlp_canonical, per query tr_proof_walk.

static constexpr uint32_t TR_PROOF_MAX_NODES = 1024;  // records per proof: the walk scans their digests linearly
enum { TR_PROOF_REJECT = 0, TR_PROOF_ACCEPT = 1, TR_PROOF_DEFER = 2 };

// Lists below the record's own that tr_rlp_canonical follows. An honest record nests at most four lists:
// the node, an embedded extension in one of its slots, that extension's embedded branch, an embedded leaf
// in the branch. An embedded node is under 32 bytes; a branch is 18 bytes at least, so an embedded
// extension (2 bytes of prefix and path) leaves its branch 29 bytes, that is 11 bytes beyond its 17 empty
// slots and prefix: room for one embedded leaf (3 bytes or more), for no further extension (20 or more)
// and no branch (18 or more). A leaf holds no list.
static constexpr int TR_PROOF_MAX_NEST = 4;

// Deep canonical form: [p, p + len) is exactly one item by the rules of tr_rlp_item, and so is every
// nested item, each list exactly tiled by its items. A list nested deeper than TR_PROOF_MAX_NEST makes
// the record not canonical. The open lists' ends are four named pointers, no indexed stack.
PV_HD bool tr_rlp_canonical(const uint8_t* p, uint64_t len) {
    TrItem it;
    if (!tr_rlp_item(p, p + len, &it) || it.raw_len != len) return false;
    if (!it.list) return true;
    const uint8_t* q = it.p;
    const uint8_t *e0 = it.p + it.len, *e1 = e0, *e2 = e0, *e3 = e0;
    int depth = 0;  // open lists below the record's own
    for (;;) {
        const uint8_t* e = depth == 0 ? e0 : depth == 1 ? e1 : depth == 2 ? e2 : e3;
        if (q == e) {  // this list is tiled: its parent goes on behind it
            if (depth == 0) return true;
            depth--;
            continue;
        }
        if (!tr_rlp_item(q, e, &it)) return false;
        if (!it.list) {
            q += it.raw_len;
            continue;
        }
        if (depth == TR_PROOF_MAX_NEST - 1) return false;
        depth++;
        const uint8_t* ne = it.p + it.len;
        if (depth == 1) e1 = ne;
        else if (depth == 2) e2 = ne;
        else e3 = ne;
        q = it.p;
    }
}

// nibble i of a packed path (i below tr_hp_nibbles)
PV_HD uint8_t tr_hp_nibble(const uint8_t* hp, uint32_t i) {
    const uint32_t k = i + (((hp[0] >> 4) & 1) ? 1 : 2);
    return (k & 1) ? (uint8_t)(hp[k >> 1] & 15) : (uint8_t)(hp[k >> 1] >> 4);
}
PV_HD uint8_t tr_key_nibble(const uint8_t* key, uint32_t i) {
    return (i & 1) ? (uint8_t)(key[i >> 1] & 15) : (uint8_t)(key[i >> 1] >> 4);
}
PV_HD uint64_t tr_load_le64(const uint8_t* p) {
    uint64_t x = 0;
    for (int k = 7; k >= 0; k--) x = (x << 8) | p[k];
    return x;
}

// One query against the records [first, first + count) of its proof: record j is
// blob[node_off[j] .. + node_len(j)) with node_len(j) = node_len ? node_len[j] : node_off[j + 1] - node_off[j],
// digest[4 j .. 4 j + 3] its SHA3-256 as keccak.h leaves it. The caller has checked that every one of them
// is canonical (tr_rlp_canonical); the walk still bounds every read by the record it is in. It reads the
// RLP in place: per node one pass over its items that counts them and keeps the two or three it needs.
// TR_PROOF_DEFER when a node it visits is not what tr_decode_node accepts there; a node it never visits
// is not looked at. val_len 0 expects the key's absence.
PV_HD int tr_proof_walk(const uint8_t* blob, const uint64_t* node_off, const uint64_t* node_len, const uint64_t* digest,
                        uint64_t first, uint64_t count, const uint8_t* root, const uint8_t* key, uint64_t key_len,
                        const uint8_t* val, uint64_t val_len) {
    if (key_len > PV_TRIE_MAX_KEY || val_len > PV_TRIE_MAX_VALUE || count > TR_PROOF_MAX_NODES) return TR_PROOF_DEFER;
    const uint32_t nibs = (uint32_t)(2 * key_len);
    uint32_t pos = 0;
    const uint8_t* ref = root;  // 32 bytes: the root, then a child slot inside a record
    const uint8_t* found = nullptr;
    uint64_t found_len = 0;
    bool done = false;
    // every node consumes a nibble or ends the walk: nibs + 1 nodes at most
    for (uint32_t step = 0; !done; step++) {
        if (step > nibs + 1) return TR_PROOF_DEFER;
        const uint8_t* p;
        uint64_t len;
        if (ref) {
            const uint64_t r0 = tr_load_le64(ref);
            uint64_t j = first;
            for (; j < first + count; j++) {
                if (digest[4 * j] != r0) continue;
                if (digest[4 * j + 1] == tr_load_le64(ref + 8) && digest[4 * j + 2] == tr_load_le64(ref + 16) &&
                    digest[4 * j + 3] == tr_load_le64(ref + 24))
                    break;
            }
            if (j == first + count) return TR_PROOF_REJECT;  // no record hashes to the reference
            p = blob + node_off[j];
            len = node_len ? node_len[j] : node_off[j + 1] - node_off[j];
        } else {  // an embedded child: the walk goes on inside the same record
            p = found;
            len = found_len;
        }
        TrItem top, it, it0, it1, sel;
        if (!tr_rlp_item(p, p + len, &top) || !top.list || top.raw_len != len) return TR_PROOF_DEFER;
        const uint32_t want = pos < nibs ? tr_key_nibble(key, pos) : 16;  // the slot a branch is asked for
        const uint8_t* q = top.p;
        const uint8_t* end = top.p + top.len;
        uint32_t n = 0;
        bool kids_ok = true, last_is_list = false;
        it0 = it1 = sel = top;
        while (q < end) {
            if (n == 17 || !tr_rlp_item(q, end, &it)) return TR_PROOF_DEFER;
            if (n == 0) it0 = it;
            if (n == 1) it1 = it;
            if (n == want) sel = it;
            if (n < 16 && !it.list && it.len != 32 && it.len != 0) kids_ok = false;
            last_is_list = it.list || it.len > PV_TRIE_MAX_VALUE;  // what a branch's value slot must not be
            q += it.raw_len;
            n++;
        }
        TrItem child;
        if (n == 2) {
            bool term;
            if (it0.list) return TR_PROOF_DEFER;
            const int64_t hn = tr_hp_nibbles(it0.p, it0.len, &term);
            if (hn < 0) return TR_PROOF_DEFER;
            if (term) {
                if (it1.list || it1.len == 0 || it1.len > PV_TRIE_MAX_VALUE) return TR_PROOF_DEFER;
                bool same = (uint64_t)hn == (uint64_t)(nibs - pos);
                for (uint32_t i = 0; same && i < (uint32_t)hn; i++) same = tr_hp_nibble(it0.p, i) == tr_key_nibble(key, pos + i);
                found = same ? it1.p : nullptr;
                found_len = same ? it1.len : 0;
                break;
            }
            if (hn == 0) return TR_PROOF_DEFER;  // an extension has a path
            if (!it1.list && it1.len != 32) return TR_PROOF_DEFER;
            bool pre = (uint64_t)hn <= (uint64_t)(nibs - pos);
            for (uint32_t i = 0; pre && i < (uint32_t)hn; i++) pre = tr_hp_nibble(it0.p, i) == tr_key_nibble(key, pos + i);
            if (!pre) {
                found = nullptr;
                found_len = 0;
                break;
            }
            pos += (uint32_t)hn;
            child = it1;
        } else if (n == 17) {
            if (!kids_ok || last_is_list) return TR_PROOF_DEFER;
            if (want == 16) {
                found = sel.len ? sel.p : nullptr;
                found_len = sel.len;
                break;
            }
            pos++;
            child = sel;
        } else {
            return TR_PROOF_DEFER;
        }
        if (child.list) {
            ref = nullptr;
            found = child.raw;
            found_len = child.raw_len;
        } else if (child.len == 32) {
            ref = child.p;
        } else {  // blank
            found = nullptr;
            found_len = 0;
            done = true;
        }
    }
    if (found_len != val_len) return TR_PROOF_REJECT;
    for (uint64_t i = 0; i < val_len; i++)
        if (found[i] != val[i]) return TR_PROOF_REJECT;
    return TR_PROOF_ACCEPT;
}

#endif  // PV_TRIE_CORE_H
