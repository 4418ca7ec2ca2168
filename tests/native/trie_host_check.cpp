// Stand-alone check of the state trie's host code (csrc/trie_host.cpp over trie_core.h and keccak.h),
// built with -fsanitize=address,undefined by tests/test_trie_host.py and run as its own process: never
// loaded into Python, never run on a GPU. Input file (little-endian):
//   u32 cases; per case: u32 batches; per batch: u32 n; n x (u32 klen, key, u32 vlen, value); then the
//                        expected final root (32 bytes)
//   u32 malformed; per entry: u32 len, bytes: a node that must be rejected as the root of an update
// Every existing node handed to the update lives in a heap block of exactly its size, so a decoder that
// reads past a record reads past a block.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/plenum_verify.h"
#include "trie_core.h"
#include "trie_host.h"

namespace {

typedef std::vector<uint8_t> Bytes;

struct Reader {
    Bytes data;
    size_t at = 0;
    uint32_t u32() {
        uint32_t v;
        need(4);
        memcpy(&v, data.data() + at, 4);
        at += 4;
        return v;
    }
    Bytes bytes(size_t n) {
        need(n);
        Bytes b(data.begin() + at, data.begin() + at + n);
        at += n;
        return b;
    }
    void need(size_t n) {
        if (at + n > data.size()) {
            fprintf(stderr, "input truncated\n");
            exit(2);
        }
    }
};

// one update against `known` (exact-size blocks); rc of pv_trie_host_build, plan filled
int build(const Bytes& root, const std::vector<std::pair<Bytes, Bytes>>& known, const std::vector<Bytes>& keys,
          const std::vector<Bytes>& vals, PvTriePlan* plan, std::string* err) {
    std::vector<uint8_t> kh, kb{0}, keyb{0}, valb{0};
    std::vector<uint64_t> ko{0}, keyo{0}, valo{0};
    kb.clear();
    keyb.clear();
    valb.clear();
    for (auto& e : known) {
        kh.insert(kh.end(), e.first.begin(), e.first.end());
        kb.insert(kb.end(), e.second.begin(), e.second.end());
        ko.push_back(kb.size());
    }
    for (auto& k : keys) {
        keyb.insert(keyb.end(), k.begin(), k.end());
        keyo.push_back(keyb.size());
    }
    for (auto& v : vals) {
        valb.insert(valb.end(), v.begin(), v.end());
        valo.push_back(valb.size());
    }
    // exact-size heap copies: no slack behind the last record
    std::unique_ptr<uint8_t[]> kb_x(new uint8_t[kb.size() ? kb.size() : 1]), key_x(new uint8_t[keyb.size() ? keyb.size() : 1]),
        val_x(new uint8_t[valb.size() ? valb.size() : 1]);
    if (kb.size()) memcpy(kb_x.get(), kb.data(), kb.size());
    if (keyb.size()) memcpy(key_x.get(), keyb.data(), keyb.size());
    if (valb.size()) memcpy(val_x.get(), valb.data(), valb.size());
    const PvTrieIn in{root.data(), kh.data(), kb_x.get(), ko.data(), known.size(), key_x.get(), keyo.data(),
                      val_x.get(), valo.data(), keys.size()};
    return pv_trie_host_build(in, plan, err);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    Reader r;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) r.data.insert(r.data.end(), chunk, chunk + n);
    fclose(f);

    const uint32_t cases = r.u32();
    for (uint32_t c = 0; c < cases; c++) {
        std::map<Bytes, Bytes> store;
        Bytes root(PV_TRIE_BLANK_ROOT, PV_TRIE_BLANK_ROOT + 32);
        const uint32_t batches = r.u32();
        for (uint32_t b = 0; b < batches; b++) {
            const uint32_t n = r.u32();
            std::vector<Bytes> keys, vals;
            for (uint32_t i = 0; i < n; i++) {
                keys.push_back(r.bytes(r.u32()));
                vals.push_back(r.bytes(r.u32()));
            }
            if (n == 0) continue;
            std::vector<std::pair<Bytes, Bytes>> known;
            PvTriePlan plan;
            std::string err;
            for (int round = 0;; round++) {
                const int rc = build(root, known, keys, vals, &plan, &err);
                if (rc == PV_OK) break;
                if (rc != PV_TRIE_NEED_NODES || round > 100000) {
                    fprintf(stderr, "case %u batch %u: rc %d %s\n", c, b, rc, err.c_str());
                    return 1;
                }
                for (size_t m = 0; m < plan.missing.size(); m += 32) {
                    const Bytes h(plan.missing.begin() + m, plan.missing.begin() + m + 32);
                    auto it = store.find(h);
                    if (it == store.end()) {
                        fprintf(stderr, "case %u batch %u: a node the store never held is asked for\n", c, b);
                        return 1;
                    }
                    known.emplace_back(h, it->second);
                }
            }
            const size_t nr = plan.recs.size();
            Bytes hashes(32 * nr);
            uint8_t* arena = reinterpret_cast<uint8_t*>(plan.arena.data());
            pv_trie_host_hash(arena, plan.recs.data(), nr, hashes.data());
            for (size_t i = 0; i < nr; i++)
                store[Bytes(hashes.begin() + 32 * i, hashes.begin() + 32 * i + 32)] =
                    Bytes(arena + plan.recs[i].off, arena + plan.recs[i].off + plan.recs[i].len);
            root.assign(hashes.end() - 32, hashes.end());
        }
        const Bytes want = r.bytes(32);
        if (root != want) {
            fprintf(stderr, "case %u: final root differs\n", c);
            return 1;
        }
    }
    const uint32_t bad = r.u32();
    for (uint32_t i = 0; i < bad; i++) {
        const Bytes node = r.bytes(r.u32());
        std::unique_ptr<uint8_t[]> exact(new uint8_t[node.size() ? node.size() : 1]);
        if (node.size()) memcpy(exact.get(), node.data(), node.size());
        TrDecoded d;
        if (tr_decode_node(exact.get(), node.size(), &d)) {
            fprintf(stderr, "malformed node %u decoded\n", i);
            return 1;
        }
        const uint64_t off[2] = {0, node.size()};
        Bytes h(32);
        pv_sha3_host_batch(exact.get(), off, 1, h.data());
        PvTriePlan plan;
        std::string err;
        const int rc = build(h, {{h, node}}, {Bytes{0x12, 0x34}}, {Bytes{'v'}}, &plan, &err);
        if (rc != PV_ERR_DECODE) {
            fprintf(stderr, "malformed node %u: rc %d, not PV_ERR_DECODE\n", i, rc);
            return 1;
        }
    }
    printf("ok %u cases %u malformed\n", cases, bad);
    return 0;
}
