// The structural half of a state trie built from empty, as per-item functions ("Device builder"):
// every pass of pv_trie_root is one of these functions over an index range, run one lane per index by the
// kernels of kern_trie_build.h and in plain loops by tests/native/trie_build_check.cpp. Plain C++, no
// allocation, no pass reads what the same pass writes: a pass reads what earlier passes wrote.
//
// Keys have one length of 1 .. 64 bytes, so no key is a prefix of another and no branch carries a value. The
// m distinct keys are sorted; h[i] is the number of nibbles key i and key i + 1 share (a "gap"). A branch is a
// maximal range [l, r] of keys that share d nibbles and not d + 1; it is named by its first gap with h == d,
// which is the end of its first child (its "rep"). The pass tb_branch finds, for every gap, whether it is a
// rep (two galloping binary searches over whole keys, O(log m) key comparisons whatever the keys are), and a
// rep lists its up to 16 children (one search per child on a single nibble), telling every child who its
// parent is. A child range of one key is a leaf; a longer one is a branch at the depth its first and last key
// share, with the nibbles in between as an extension that the child owns. The root branch at depth above 0
// owns an extension from nibble 0.
//
// The sizing argument. A child is referenced by hash (33 bytes) when its RLP has 32 bytes or more, else it is
// embedded as its RLP (pruning_trie.py:339-340). A leaf has at least 3 bytes (prefix, one path byte, one value
// byte), an empty slot 1 byte, so a branch of k embedded leaves has at least 1 + (16 - k) + 3 k + 1 = 18 + 2 k
// bytes: below 32 only for k <= 6, and a branch that holds anything but leaves holds a node of at least 22
// bytes (a branch of two leaves) and has at least 1 + 15 + 22 + 1 = 39. An extension adds at least 2 bytes to
// its branch, so it can be below 32 only over such a branch of leaves. Hence three passes, none recursive:
// tb_leaf_size (every leaf), tb_small (every branch of leaves only: its size when below 32), tb_size (every
// branch and its extension exactly: a child branch is either small, with its size stored, or 33 bytes). The
// emitter writes embedded nodes with the same functions that write records.
//
// Node ids: leaf k is k, the branch of gap i is n + i, its extension 2 n + i (n the number of entries given).
#ifndef PV_TRIE_BUILD_H
#define PV_TRIE_BUILD_H

#include <stdint.h>

#include "trie_core.h"
#include "trie_host.h"

static constexpr uint32_t TB_MAX_KEY = 64;               // PV_TRIE_BUILD_MAX_KEY
static constexpr uint32_t TB_DEPTHS = 2 * TB_MAX_KEY + 2;  // node depths 0 .. 2 key_len + 1
static constexpr uint32_t TB_NONE = 0xffffffffu;
static constexpr uint32_t TB_IS_BRANCH = 0x80000000u;  // in a child table: the rest is a gap, else a key
static constexpr uint8_t TB_NO_RECORD = 255;           // depth key of a node that is not hashed
static constexpr uint8_t TB_KEY_OF_ROOT = 200;         // depth key of a record: 200 - depth, deepest first

// What the host reads between the two phases.
struct TbHdr {
    uint32_t err;        // non-zero: an offset pair decreases or a value is outside the limits
    uint32_t m;          // distinct keys
    uint32_t n_branch;
    uint32_t n_ext;
    uint32_t max_depth;  // greatest node depth, the root being 0
    uint32_t root;       // the root branch's gap; TB_NONE: the trie is one leaf
    uint64_t arena_bytes;
    uint32_t dstart[TB_DEPTHS], dend[TB_DEPTHS];  // records of depth d: [dstart[d], dend[d])
};

struct TbCtx {
    const uint8_t* keys;   // n keys of key_len bytes
    const uint8_t* val;
    const uint64_t* voff;  // n + 1
    uint32_t key_len, n, wrap, W;  // W: 64-bit words per key
    TbHdr* hdr;
    uint32_t* idx;    // n: entry indices, sorted by key, entries of one key in the order given
    uint32_t* keep;   // n: 1 for the last entry of a run of equal keys
    uint32_t* pos;    // n: exclusive scan of keep
    uint32_t* sidx;   // m: the entry of distinct key k
    uint64_t* skey;   // m W: distinct key k as big-endian words, zero padded
    uint8_t* h;       // m - 1
    uint8_t* isrep;   // m - 1
    uint32_t* ct;     // 16 per gap: a rep's children
    uint32_t* lpar;   // m: the gap of a leaf's branch
    uint32_t* bpar;   // m - 1: the gap of a branch's parent branch
    uint32_t* lsz;    // m: a leaf's RLP length
    uint32_t* bsmall;  // m - 1: a branch's RLP length when it is below 32, else 0
    uint32_t* bsz;    // m - 1: a branch's RLP length
    uint32_t* esz;    // m - 1: its extension's, 0 without one
    uint64_t* rlen8;  // 3 n: a record's length rounded up to 8, 0 for what is not hashed
    uint64_t* roff;   // 3 n: exclusive scan of rlen8: where the record lies in the arena
    uint8_t* dkey;    // 3 n: depth key
    uint8_t* ndepth;  // 3 n
    uint32_t* nid;    // 3 n: node ids, the values of the depth sort
    uint8_t* dkey_s;  // 3 n: dkey sorted (stable)
    uint32_t* order;  // 3 n: node of record r
    uint32_t* rank;   // 3 n: record of a hashed node
    uint8_t* arena;   // phase two
    PvTrieRec* recs;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define TB_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define TB_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

// ------------------------------------------------------------------------------------------ keys

PV_HD uint64_t tb_key_word(const uint8_t* key, uint32_t key_len, uint32_t w) {
    uint64_t x = 0;
    for (uint32_t b = 0; b < 8; b++) {
        const uint32_t p = 8 * w + b;
        x = (x << 8) | (p < key_len ? key[p] : 0);
    }
    return x;
}
// nibbles distinct keys a and b share
PV_HD uint32_t tb_nlcp(const TbCtx& c, uint32_t a, uint32_t b) {
    for (uint32_t w = 0; w < c.W; w++) {
        const uint64_t x = c.skey[(uint64_t)a * c.W + w] ^ c.skey[(uint64_t)b * c.W + w];
        if (x) return 16 * w + (uint32_t)__builtin_clzll(x) / 4;
    }
    return 2 * c.key_len;
}
PV_HD uint32_t tb_nib(const TbCtx& c, uint32_t k, uint32_t p) {
    return (uint32_t)(c.skey[(uint64_t)k * c.W + (p >> 4)] >> (60 - 4 * (p & 15))) & 15;
}

// The largest j in [t, end] with p(j), p true at t and monotone; the smallest j in [0, t] likewise. Galloping
// from t, then bisection: O(log distance) calls.
template <class P>
PV_HD uint32_t tb_last_true(uint32_t t, uint32_t end, const P& p) {
    uint32_t f = TB_NONE, step = 1;
    while (t < end) {
        const uint32_t j = end - t > step ? t + step : end;
        if (p(j)) {
            t = j;
            step <<= 1;
        } else {
            f = j;
            break;
        }
    }
    if (f != TB_NONE)
        while (f - t > 1) {
            const uint32_t mid = t + (f - t) / 2;
            if (p(mid)) t = mid;
            else f = mid;
        }
    return t;
}
template <class P>
PV_HD uint32_t tb_first_true(uint32_t t, const P& p) {
    uint32_t f = TB_NONE, step = 1;
    while (t > 0) {
        const uint32_t j = t > step ? t - step : 0;
        if (p(j)) {
            t = j;
            step <<= 1;
        } else {
            f = j;
            break;
        }
    }
    if (f != TB_NONE)
        while (t - f > 1) {
            const uint32_t mid = f + (t - f) / 2;
            if (p(mid)) t = mid;
            else f = mid;
        }
    return t;
}

// ----------------------------------------------------------------------------------------- sizes

PV_HD uint32_t tb_hp_str_size(uint32_t plen) {
    const uint32_t b = tr_hp_size(plen);
    return b == 1 ? 1 : tr_prefix_size(b) + b;  // a one-byte path is below 0x40: its own encoding
}
// the value of entry e as a string item, and with `wrap` the string item of rlp([value])
PV_HD uint64_t tb_str_size(const TbCtx& c, uint32_t e) {
    const uint64_t a = c.voff[e], len = c.voff[e + 1] - a;
    return len == 1 && c.val[a] < 0x80 ? 1 : tr_prefix_size(len) + len;
}
PV_HD uint64_t tb_value_size(const TbCtx& c, uint32_t e) {
    const uint64_t s = tb_str_size(c, e);
    if (!c.wrap) return s;
    const uint64_t stored = tr_list_size(s);  // two bytes at least: never its own encoding
    return tr_prefix_size(stored) + stored;
}
// the payload of a list of `total` bytes
PV_HD uint64_t tb_payload_of(uint64_t total) {
    for (uint32_t p = 1; p < 9; p++)
        if (tr_prefix_size(total - p) == p) return total - p;
    return 0;
}
PV_HD uint32_t tb_ref_size(uint32_t size) { return size < 32 ? size : 33; }
PV_HD uint32_t tb_ext_size(uint32_t elen, uint32_t branch_size) {
    return (uint32_t)tr_list_size(tb_hp_str_size(elen) + tb_ref_size(branch_size));
}
// nibbles of the extension the branch of gap i owns
PV_HD uint32_t tb_elen(const TbCtx& c, uint32_t i) {
    const uint32_t p = c.bpar[i];
    return p == TB_NONE ? c.h[i] : (uint32_t)c.h[i] - c.h[p] - 1;
}
// nibbles above leaf k's path
PV_HD uint32_t tb_leaf_start(const TbCtx& c, uint32_t k) {
    const uint32_t p = c.lpar[k];
    return p == TB_NONE ? 0 : (uint32_t)c.h[p] + 1;
}

// ---------------------------------------------------------------------------------------- passes

// i < n: the identity to sort, and the checks the host cannot make on device offsets
PV_HD void tb_init(const TbCtx& c, uint32_t i) {
    c.idx[i] = i;
    const uint64_t a = c.voff[i], b = c.voff[i + 1];
    bool bad = b < a;
    if (!bad) {
        const uint64_t len = b - a;
        if (c.wrap) {  // a single byte adds 1 or 2: within the limit either way, and not read here
            const uint64_t s = len == 1 ? 2 : tr_prefix_size(len) + len;
            bad = tr_list_size(s) > PV_TRIE_MAX_VALUE;
        } else {
            bad = len == 0 || len > PV_TRIE_MAX_VALUE;
        }
    }
    if (bad) TB_ATOMIC_OR(&c.hdr->err, 1u);
}

// j < n: the key of one pass of the LSD sort (least significant part first): the big-endian 32-bit part `w` of
// the key at position j above the position itself. Every sort key is distinct, so the order of a pass does not
// depend on the sort being stable; tb_gather moves the entry indices after it.
PV_HD uint64_t tb_sort_word(const TbCtx& c, uint32_t j, uint32_t w) {
    const uint8_t* key = c.keys + (uint64_t)c.idx[j] * c.key_len;
    uint64_t x = 0;
    for (uint32_t b = 0; b < 4; b++) {
        const uint32_t p = 4 * w + b;
        x = (x << 8) | (p < c.key_len ? key[p] : 0);
    }
    return (x << 32) | j;
}
// r < n: the entry that the sorted key at r came from
PV_HD uint32_t tb_gather(const TbCtx& c, uint32_t r, const uint64_t* sorted) { return c.idx[(uint32_t)sorted[r]]; }

// j < n: the last entry of a key wins
PV_HD void tb_keep(const TbCtx& c, uint32_t j) {
    uint32_t keep = 1;
    if (j + 1 < c.n) {
        const uint8_t* x = c.keys + (uint64_t)c.idx[j] * c.key_len;
        const uint8_t* y = c.keys + (uint64_t)c.idx[j + 1] * c.key_len;
        bool same = true;
        for (uint32_t b = 0; b < c.key_len; b++) same &= x[b] == y[b];
        keep = same ? 0 : 1;
    }
    c.keep[j] = keep;
}

// j < n
PV_HD void tb_compact(const TbCtx& c, uint32_t j) {
    const uint32_t p = c.pos[j];
    if (c.keep[j]) {
        c.sidx[p] = c.idx[j];
        for (uint32_t w = 0; w < c.W; w++)
            c.skey[(uint64_t)p * c.W + w] = tb_key_word(c.keys + (uint64_t)c.idx[j] * c.key_len, c.key_len, w);
    }
    if (j == c.n - 1) c.hdr->m = p + 1;  // the last entry is always kept
}

// i < n
PV_HD void tb_lcp(const TbCtx& c, uint32_t i) {
    if (i + 1 < c.hdr->m) c.h[i] = (uint8_t)tb_nlcp(c, i, i + 1);
}

// i < n: is gap i the rep of its branch, and if so its children
PV_HD void tb_branch(const TbCtx& c, uint32_t i) {
    const uint32_t m = c.hdr->m;
    if (m == 1 && i == 0) {
        c.lpar[0] = TB_NONE;
        c.hdr->root = TB_NONE;
    }
    if (i + 1 >= m) return;
    const uint32_t d = c.h[i];
    const uint32_t l = tb_first_true(i, [&](uint32_t j) { return tb_nlcp(c, j, i) >= d; });
    const bool rep = l == i || tb_nib(c, l, d) == tb_nib(c, i, d);
    c.isrep[i] = rep ? 1 : 0;
    if (!rep) return;
    const uint32_t r = tb_last_true(i + 1, m - 1, [&](uint32_t j) { return tb_nlcp(c, i, j) >= d; });
    if (l == 0 && r == m - 1) {
        c.hdr->root = i;
        c.bpar[i] = TB_NONE;
    }
    uint32_t* ct = c.ct + 16 * (uint64_t)i;
    for (uint32_t s = 0; s < 16; s++) ct[s] = TB_NONE;
    for (uint32_t a = l; a <= r;) {
        const uint32_t nb = tb_nib(c, a, d);
        const uint32_t b = tb_last_true(a, r, [&](uint32_t j) { return tb_nib(c, j, d) == nb; });
        if (a == b) {
            ct[nb] = a;
            c.lpar[a] = i;
        } else {  // a branch at the depth its ends share; its rep is the end of its first child
            const uint32_t d2 = tb_nlcp(c, a, b), nb2 = tb_nib(c, a, d2);
            const uint32_t j = tb_last_true(a, b, [&](uint32_t k) { return tb_nib(c, k, d2) == nb2; });
            ct[nb] = TB_IS_BRANCH | j;
            c.bpar[j] = i;
        }
        a = b + 1;
    }
}

// k < n
PV_HD void tb_leaf_size(const TbCtx& c, uint32_t k) {
    if (k >= c.hdr->m) return;
    const uint32_t plen = 2 * c.key_len - tb_leaf_start(c, k);
    c.lsz[k] = (uint32_t)tr_list_size(tb_hp_str_size(plen) + tb_value_size(c, c.sidx[k]));
}

// i < n: a branch of leaves only that is below 32 bytes
PV_HD void tb_small(const TbCtx& c, uint32_t i) {
    if (i + 1 >= c.hdr->m || !c.isrep[i]) return;
    const uint32_t* ct = c.ct + 16 * (uint64_t)i;
    uint32_t pay = 1;  // the value slot
    bool leaves = true;
    for (uint32_t s = 0; s < 16; s++) {
        const uint32_t e = ct[s];
        if (e == TB_NONE) pay += 1;
        else if (e & TB_IS_BRANCH) leaves = false;
        else pay += tb_ref_size(c.lsz[e]);
    }
    const uint32_t size = (uint32_t)tr_list_size(pay);
    c.bsmall[i] = leaves && size < 32 ? size : 0;
}

// i < n: a branch and its extension exactly
PV_HD void tb_size(const TbCtx& c, uint32_t i) {
    if (i + 1 >= c.hdr->m || !c.isrep[i]) return;
    const uint32_t* ct = c.ct + 16 * (uint64_t)i;
    uint32_t pay = 1;
    for (uint32_t s = 0; s < 16; s++) {
        const uint32_t e = ct[s];
        if (e == TB_NONE) {
            pay += 1;
        } else if (e & TB_IS_BRANCH) {
            const uint32_t j = e & ~TB_IS_BRANCH, bs = c.bsmall[j] ? c.bsmall[j] : 32, el = (uint32_t)c.h[j] - c.h[i] - 1;
            pay += tb_ref_size(el ? tb_ext_size(el, bs) : bs);
        } else {
            pay += tb_ref_size(c.lsz[e]);
        }
    }
    const uint32_t size = (uint32_t)tr_list_size(pay), el = tb_elen(c, i);
    c.bsz[i] = size;
    c.esz[i] = el ? tb_ext_size(el, size) : 0;
}

// node depth of the branch of gap i, the root node being 0: at most 2 key_len steps up
PV_HD uint32_t tb_branch_depth(const TbCtx& c, uint32_t i) {
    uint32_t dep = 0;
    for (uint32_t g = i;;) {
        const uint32_t p = c.bpar[g];
        dep += tb_elen(c, g) ? 1 : 0;
        if (p == TB_NONE) return dep;
        dep += 1;
        g = p;
    }
}

// t < 3 n: is node t there, is it hashed, how deep is it. Returns bit 0: a branch, bit 1: an extension,
// bits 8 and up: its depth (0 when there is no such node).
PV_HD uint32_t tb_mark(const TbCtx& c, uint32_t t) {
    const uint32_t m = c.hdr->m, kind = t / c.n, x = t - kind * c.n;
    c.nid[t] = t;
    bool there, root;
    uint32_t size = 0, depth = 0;
    if (kind == 0) {
        there = x < m;
        if (there) {
            root = c.lpar[x] == TB_NONE;
            size = c.lsz[x];
            depth = root ? 0 : tb_branch_depth(c, c.lpar[x]) + 1;
        }
    } else {
        there = x + 1 < m && c.isrep[x] && (kind == 1 || c.esz[x]);
        if (there) {
            const uint32_t bd = tb_branch_depth(c, x);
            size = kind == 1 ? c.bsz[x] : c.esz[x];
            depth = kind == 1 ? bd : bd - 1;
            root = depth == 0;
        }
    }
    if (!there) {
        c.rlen8[t] = 0;
        c.dkey[t] = TB_NO_RECORD;
        c.ndepth[t] = 0;
        return 0;
    }
    const bool rec = size >= 32 || root;  // the root is always hashed
    c.rlen8[t] = rec ? ((uint64_t)size + 7) & ~7ull : 0;
    c.dkey[t] = rec ? (uint8_t)(TB_KEY_OF_ROOT - depth) : TB_NO_RECORD;
    c.ndepth[t] = (uint8_t)depth;
    return (kind == 1 ? 1u : 0u) | (kind == 2 ? 2u : 0u) | (depth << 8);
}

// r < 3 n, after the stable sort by depth key: where each depth's records lie, and each node's record
PV_HD void tb_bounds(const TbCtx& c, uint32_t r) {
    const uint32_t last = 3 * c.n - 1;
    if (r == last) c.hdr->arena_bytes = c.roff[last] + c.rlen8[last];
    const uint8_t k = c.dkey_s[r];
    if (k == TB_NO_RECORD) return;
    const uint32_t d = TB_KEY_OF_ROOT - k;
    if (r == 0 || c.dkey_s[r - 1] != k) c.hdr->dstart[d] = r;
    if (r == last || c.dkey_s[r + 1] != k) c.hdr->dend[d] = r + 1;
    c.rank[c.order[r]] = r;
}

// ----------------------------------------------------------------------------------------- emit

PV_HD uint32_t tb_put_hp(uint8_t* d, const TbCtx& c, uint32_t k, uint32_t start, uint32_t plen, bool term) {
    const uint32_t b = tr_hp_size(plen), flags = (term ? 2u : 0u) | (plen & 1);
    uint32_t o = b > 1 ? tr_put_prefix(d, b, 0x80) : 0, i = start;
    d[o++] = (uint8_t)(16 * flags + ((plen & 1) ? tb_nib(c, k, i++) : 0));
    for (; i < start + plen; i += 2) d[o++] = (uint8_t)(16 * tb_nib(c, k, i) + tb_nib(c, k, i + 1));
    return o;
}
PV_HD uint64_t tb_put_value(uint8_t* d, const TbCtx& c, uint32_t e) {
    const uint64_t a = c.voff[e], len = c.voff[e + 1] - a, s = tb_str_size(c, e);
    const uint8_t* p = c.val + a;
    uint64_t o = 0;
    if (c.wrap) {
        o += tr_put_prefix(d + o, tr_list_size(s), 0x80);
        o += tr_put_prefix(d + o, s, 0xc0);
    }
    if (len == 1 && s == 1) {  // its own encoding (an empty value has s == 1 too: 0x80, below)
        d[o++] = p[0];
        return o;
    }
    o += tr_put_prefix(d + o, len, 0x80);
    for (uint64_t i = 0; i < len; i++) d[o + i] = p[i];
    return o + len;
}
PV_HD uint64_t tb_put_leaf(uint8_t* d, const TbCtx& c, uint32_t k) {
    const uint32_t start = tb_leaf_start(c, k);
    uint64_t o = tr_put_prefix(d, tb_payload_of(c.lsz[k]), 0xc0);
    o += tb_put_hp(d + o, c, k, start, 2 * c.key_len - start, true);
    return o + tb_put_value(d + o, c, c.sidx[k]);
}
// A hashed child's slot: 0xa0 and a hole the child's digest goes to. The child's record is told where.
PV_HD uint32_t tb_put_hole(uint8_t* d, const TbCtx& c, uint32_t node, uint64_t at) {
    d[0] = 0xa0;
    for (uint32_t i = 1; i < 33; i++) d[i] = 0;
    c.recs[c.rank[node]].hole = at + 1;
    return 33;
}
// the branch of gap i at arena offset `at`: embedded children whole, hashed ones as holes
PV_HD uint32_t tb_put_branch(uint8_t* d, const TbCtx& c, uint32_t i, uint64_t at);
PV_HD uint32_t tb_put_ext(uint8_t* d, const TbCtx& c, uint32_t i, uint64_t at);

// a branch below 32 bytes: leaves and empty slots
PV_HD uint32_t tb_put_small_branch(uint8_t* d, const TbCtx& c, uint32_t i) {
    const uint32_t* ct = c.ct + 16 * (uint64_t)i;
    uint32_t o = tr_put_prefix(d, c.bsz[i] - 1, 0xc0);
    for (uint32_t s = 0; s < 16; s++) {
        if (ct[s] == TB_NONE) d[o++] = 0x80;
        else o += (uint32_t)tb_put_leaf(d + o, c, ct[s]);
    }
    d[o++] = 0x80;
    return o;
}
PV_HD uint32_t tb_put_ext(uint8_t* d, const TbCtx& c, uint32_t i, uint64_t at) {
    const uint32_t p = c.bpar[i], start = p == TB_NONE ? 0 : (uint32_t)c.h[p] + 1;
    uint32_t o = tr_put_prefix(d, tb_payload_of(c.esz[i]), 0xc0);
    o += tb_put_hp(d + o, c, i, start, tb_elen(c, i), false);
    if (c.bsz[i] < 32) return o + tb_put_small_branch(d + o, c, i);
    return o + tb_put_hole(d + o, c, c.n + i, at + o);
}
PV_HD uint32_t tb_put_branch(uint8_t* d, const TbCtx& c, uint32_t i, uint64_t at) {
    if (c.bsz[i] < 32) return tb_put_small_branch(d, c, i);
    const uint32_t* ct = c.ct + 16 * (uint64_t)i;
    uint32_t o = tr_put_prefix(d, tb_payload_of(c.bsz[i]), 0xc0);
    for (uint32_t s = 0; s < 16; s++) {
        const uint32_t e = ct[s];
        if (e == TB_NONE) {
            d[o++] = 0x80;
        } else if (e & TB_IS_BRANCH) {
            const uint32_t j = e & ~TB_IS_BRANCH;
            if (c.esz[j]) o += c.esz[j] < 32 ? tb_put_ext(d + o, c, j, 0) : tb_put_hole(d + o, c, 2 * c.n + j, at + o);
            else o += c.bsz[j] < 32 ? tb_put_small_branch(d + o, c, j) : tb_put_hole(d + o, c, c.n + j, at + o);
        } else {
            o += c.lsz[e] < 32 ? (uint32_t)tb_put_leaf(d + o, c, e) : tb_put_hole(d + o, c, e, at + o);
        }
    }
    d[o++] = 0x80;
    return o;
}

// r < records: record r's RLP into the arena and everything of its PvTrieRec but the hole, which its parent's
// lane writes (the root's own lane writes that it has none)
PV_HD void tb_emit(const TbCtx& c, uint32_t r) {
    const uint32_t t = c.order[r], kind = t / c.n, x = t - kind * c.n, depth = c.ndepth[t];
    const uint64_t at = c.roff[t];
    uint8_t* d = c.arena + at;
    const uint64_t len = kind == 0 ? tb_put_leaf(d, c, x) : kind == 1 ? tb_put_branch(d, c, x, at) : tb_put_ext(d, c, x, at);
    for (uint64_t i = len; i < c.rlen8[t]; i++) d[i] = 0;  // the hash reads whole words
    PvTrieRec& rec = c.recs[r];
    rec.off = at;
    rec.len = (uint32_t)len;
    rec.depth = depth;
    rec.next = c.hdr->dend[depth];
    rec.pad = 0;
    if (depth == 0) rec.hole = PV_TRIE_NO_HOLE;
}

#endif  // PV_TRIE_BUILD_H
