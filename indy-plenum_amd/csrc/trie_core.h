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
// reading on. Shared by the host path (trie_host.cpp) and the host-compiled check library
// (tests/native/triecheck.hip).
#ifndef PV_TRIE_CORE_H
#define PV_TRIE_CORE_H

#include <stdint.h>
#include <string.h>

static constexpr uint32_t PV_TRIE_MAX_KEY = 65535;          // key bytes
static constexpr uint64_t PV_TRIE_MAX_VALUE = (1ull << 24) - 1;  // value bytes (a three-byte RLP length)

// ------------------------------------------------------------------------------------------- RLP

// bytes of the length prefix of a payload of `len` bytes (strings of one byte below 0x80 have none)
inline uint32_t tr_prefix_size(uint64_t len) {
    if (len < 56) return 1;
    uint32_t ll = 0;
    for (uint64_t x = len; x; x >>= 8) ll++;
    return 1 + ll;
}
inline uint64_t tr_str_size(const uint8_t* p, uint64_t len) {
    return len == 1 && p[0] < 0x80 ? 1 : tr_prefix_size(len) + len;
}
inline uint64_t tr_list_size(uint64_t payload) { return tr_prefix_size(payload) + payload; }

// writes the prefix (base 0x80 string, 0xc0 list), returns the bytes written
inline uint32_t tr_put_prefix(uint8_t* dst, uint64_t len, uint8_t base) {
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
inline bool tr_rlp_item(const uint8_t* p, const uint8_t* end, TrItem* it) {
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
inline uint32_t tr_hp_size(uint32_t n) { return n / 2 + 1; }
inline void tr_hp_pack(uint8_t* dst, const uint8_t* nib, uint32_t n, bool term) {
    const uint8_t flags = (uint8_t)((term ? 2 : 0) | (n & 1));
    uint32_t i = 0;
    if (n & 1) dst[0] = (uint8_t)(16 * flags + nib[i++]);
    else dst[0] = (uint8_t)(16 * flags);
    for (uint32_t o = 1; i < n; i += 2, o++) dst[o] = (uint8_t)(16 * nib[i] + nib[i + 1]);
}
// nibble count of a packed path, or -1 when it is malformed (empty, flags above 3, padding nibble set)
inline int64_t tr_hp_nibbles(const uint8_t* p, uint64_t len, bool* term) {
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

inline bool tr_child(const TrItem& it, TrChild* c, bool may_be_blank) {
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

#endif  // PV_TRIE_CORE_H
