// The device trie builder's per-item functions (indy-plenum_amd/csrc/trie_build.h) run on the CPU: every pass
// that the kernels of kern_trie_build.h run one lane per item is one plain loop here, over arrays of exactly
// the sizes the driver gives them (AddressSanitizer guards their ends), with std::sort (the sort keys are distinct) and a serial
// scan where the driver calls rocPRIM. For every case of the job file: the builder's root, the root of
// pv_trie_host_build + pv_trie_host_hash from the blank root, the counts of both, and the sizing bound (the
// most leaves a node below 32 bytes holds). Stand-alone, built with -fsanitize=address,undefined by
// tests/test_trie_build_host.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../indy-plenum_amd/csrc/trie_build.h"

namespace {

struct Case {
    uint32_t key_len, n, wrap;
    std::vector<uint8_t> keys, val;
    std::vector<uint64_t> voff;
};

struct Built {
    bool err = false;
    uint8_t root[32] = {};
    uint64_t n_keys = 0, n_nodes = 0, n_records = 0, arena_bytes = 0, max_depth = 0, depths = 0;
    uint32_t small_leaves = 0;  // the most leaves inside one node below 32 bytes
};

std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

Built build(const Case& k) {
    Built out;
    const uint32_t n = k.n, n3 = 3 * n, W = (k.key_len + 7) / 8;
    TbHdr hdr;
    memset(&hdr, 0, sizeof(hdr));
    std::vector<uint32_t> idx(n), keep(n), pos(n), sidx(n), ct(16 * (size_t)n), lpar(n), bpar(n), lsz(n), bsmall(n), bsz(n),
        esz(n), nid(n3), order(n3), rank(n3);
    std::vector<uint64_t> skey((size_t)n * W), rlen8(n3), roff(n3), wk(n);
    std::vector<uint8_t> h(n), isrep(n), dkey(n3), ndepth(n3), dkey_s(n3);
    std::vector<uint8_t> val = k.val;
    if (val.empty()) val.push_back(0);
    TbCtx c{};
    c.keys = k.keys.data();
    c.val = val.data();
    c.voff = k.voff.data();
    c.key_len = k.key_len;
    c.n = n;
    c.wrap = k.wrap;
    c.W = W;
    c.hdr = &hdr;
    c.idx = idx.data();
    c.keep = keep.data();
    c.pos = pos.data();
    c.sidx = sidx.data();
    c.skey = skey.data();
    c.h = h.data();
    c.isrep = isrep.data();
    c.ct = ct.data();
    c.lpar = lpar.data();
    c.bpar = bpar.data();
    c.lsz = lsz.data();
    c.bsmall = bsmall.data();
    c.bsz = bsz.data();
    c.esz = esz.data();
    c.rlen8 = rlen8.data();
    c.roff = roff.data();
    c.dkey = dkey.data();
    c.ndepth = ndepth.data();
    c.nid = nid.data();
    c.dkey_s = dkey_s.data();
    c.order = order.data();
    c.rank = rank.data();

    for (uint32_t i = 0; i < n; i++) tb_init(c, i);
    if (hdr.err) {
        out.err = true;
        return out;
    }
    for (uint32_t w = (k.key_len + 3) / 4; w-- > 0;) {  // the LSD sort: distinct keys, so any sort serves
        for (uint32_t j = 0; j < n; j++) wk[j] = tb_sort_word(c, j, w);
        std::sort(wk.begin(), wk.end());
        std::vector<uint32_t> next(n);
        for (uint32_t j = 0; j < n; j++) next[j] = tb_gather(c, j, wk.data());
        idx.swap(next);
        c.idx = idx.data();
    }
    for (uint32_t j = 0; j < n; j++) tb_keep(c, j);
    for (uint32_t j = 0, s = 0; j < n; j++) {
        pos[j] = s;
        s += keep[j];
    }
    for (uint32_t j = 0; j < n; j++) tb_compact(c, j);
    for (uint32_t i = 0; i < n; i++) tb_lcp(c, i);
    for (uint32_t i = 0; i < n; i++) tb_branch(c, i);
    for (uint32_t i = 0; i < n; i++) tb_leaf_size(c, i);
    for (uint32_t i = 0; i < n; i++) tb_small(c, i);
    for (uint32_t i = 0; i < n; i++) tb_size(c, i);
    for (uint32_t t = 0; t < n3; t++) {
        const uint32_t f = tb_mark(c, t);
        hdr.n_branch += f & 1;
        hdr.n_ext += (f >> 1) & 1;
        hdr.max_depth = std::max(hdr.max_depth, f >> 8);
    }
    uint64_t s = 0;
    for (uint32_t t = 0; t < n3; t++) {
        roff[t] = s;
        s += rlen8[t];
    }
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return dkey[a] < dkey[b]; });
    for (uint32_t r = 0; r < n3; r++) dkey_s[r] = dkey[order[r]];
    for (uint32_t r = 0; r < n3; r++) tb_bounds(c, r);

    const uint64_t nr = hdr.dend[0];
    std::vector<uint64_t> arena(hdr.arena_bytes / 8 + 1);
    std::vector<PvTrieRec> recs(nr);
    for (PvTrieRec& r : recs) r.hole = 12345;  // every hole must be written
    c.arena = reinterpret_cast<uint8_t*>(arena.data());
    c.recs = recs.data();
    for (uint32_t r = 0; r < nr; r++) tb_emit(c, r);
    uint64_t holes = 0;
    for (const PvTrieRec& r : recs) holes += r.hole == 12345;
    if (holes || nr == 0) {
        out.err = true;
        return out;
    }
    std::vector<uint8_t> hashes(32 * nr);
    pv_trie_host_hash(c.arena, recs.data(), nr, hashes.data());
    memcpy(out.root, hashes.data() + 32 * (nr - 1), 32);
    out.n_keys = hdr.m;
    out.n_nodes = (uint64_t)hdr.m + hdr.n_branch + hdr.n_ext;
    out.n_records = nr;
    out.arena_bytes = hdr.arena_bytes;
    out.max_depth = hdr.max_depth;
    for (uint32_t d = 0; d < TB_DEPTHS; d++) out.depths += hdr.dend[d] > hdr.dstart[d];
    // the sizing bound: leaves inside a node below 32 bytes (a small branch, alone or under its extension)
    for (uint32_t i = 0; i + 1 < hdr.m; i++) {
        if (!isrep[i] || bsz[i] >= 32) continue;
        uint32_t leaves = 0;
        for (uint32_t sl = 0; sl < 16; sl++) {
            const uint32_t e = ct[16 * (size_t)i + sl];
            if (e == TB_NONE) continue;
            if (e & TB_IS_BRANCH) leaves = 99;  // a small branch holds leaves only
            else leaves++;
        }
        out.small_leaves = std::max(out.small_leaves, leaves);
    }
    return out;
}

// pv_trie_host_build + pv_trie_host_hash from the blank root on the same pairs
bool host(const Case& k, uint8_t* root, uint64_t* n_records, uint64_t* arena_bytes) {
    std::vector<uint64_t> key_off(k.n + 1), woff(k.n + 1);
    for (uint64_t i = 0; i <= k.n; i++) key_off[i] = i * k.key_len;
    std::vector<uint8_t> wrapped(k.val.size() + 8 * (size_t)k.n + 8);
    const uint8_t* vb = k.val.data();
    const uint64_t* vo = k.voff.data();
    if (k.wrap) {
        uint64_t at = 0;
        for (uint32_t i = 0; i < k.n; i++) {
            const uint8_t* p = k.val.data() + k.voff[i];
            const uint64_t len = k.voff[i + 1] - k.voff[i];
            woff[i] = at;
            at += tr_put_prefix(wrapped.data() + at, len ? tr_str_size(p, len) : 1, 0xc0);
            if (len) at += tr_put_str(wrapped.data() + at, p, len);
            else wrapped[at++] = 0x80;
        }
        woff[k.n] = at;
        vb = wrapped.data();
        vo = woff.data();
    }
    const PvTrieIn in{PV_TRIE_BLANK_ROOT, nullptr, nullptr, nullptr, 0, k.keys.data(), key_off.data(), vb, vo, k.n};
    PvTriePlan plan;
    std::string err;
    if (pv_trie_host_build(in, &plan, &err) != PV_OK || plan.recs.empty()) return false;
    const uint64_t nr = plan.recs.size();
    std::vector<uint8_t> hashes(32 * nr);
    pv_trie_host_hash(reinterpret_cast<uint8_t*>(plan.arena.data()), plan.recs.data(), nr, hashes.data());
    memcpy(root, hashes.data() + 32 * (nr - 1), 32);
    *n_records = nr;
    *arena_bytes = plan.arena_bytes;
    return true;
}

template <class T>
bool rd(FILE* f, T* p, size_t count) {
    return count == 0 || fread(p, sizeof(T), count, f) == count;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t cases;
    if (!rd(f, &cases, 1)) return 2;
    printf("[");
    for (uint32_t ci = 0; ci < cases; ci++) {
        Case k;
        uint64_t val_bytes;
        if (!rd(f, &k.key_len, 1) || !rd(f, &k.n, 1) || !rd(f, &k.wrap, 1) || !rd(f, &val_bytes, 1)) return 2;
        k.keys.resize((size_t)k.n * k.key_len);
        k.voff.resize(k.n + 1);
        k.val.resize(val_bytes);
        if (!rd(f, k.keys.data(), k.keys.size()) || !rd(f, k.voff.data(), k.voff.size()) || !rd(f, k.val.data(), k.val.size()))
            return 2;
        const Built b = build(k);
        uint8_t hroot[32] = {};
        uint64_t hrecs = 0, harena = 0;
        const bool hok = !b.err && host(k, hroot, &hrecs, &harena);
        printf("%s{\"err\": %d, \"root\": \"%s\", \"host_ok\": %d, \"host_root\": \"%s\", \"n_keys\": %llu, \"n_nodes\": %llu, "
               "\"n_records\": %llu, \"host_records\": %llu, \"arena_bytes\": %llu, \"host_arena_bytes\": %llu, "
               "\"max_depth\": %llu, \"depths\": %llu, \"small_leaves\": %u}",
               ci ? ",\n" : "", (int)b.err, hex(b.root, 32).c_str(), (int)hok, hex(hroot, 32).c_str(),
               (unsigned long long)b.n_keys, (unsigned long long)b.n_nodes, (unsigned long long)b.n_records,
               (unsigned long long)hrecs, (unsigned long long)b.arena_bytes, (unsigned long long)harena,
               (unsigned long long)b.max_depth, (unsigned long long)b.depths, b.small_leaves);
    }
    printf("]\n");
    fclose(f);
    return 0;
}
