// Stand-alone check of the state-proof host code (csrc/trie_host.cpp: pv_proof_split_host,
// pv_proof_check_args, pv_proof_host over trie_core.h and keccak.h), built with -fsanitize=address,undefined by
// tests/test_state_proof_host.py and run as its own process: never loaded into Python, never run on a GPU.
// Input file (little-endian):
//   u32 cases; per case: u32 len, the serialized proof; the root (32 bytes); u32 klen, key; u32 vlen, value;
//                        u8 ok expected of the split; u8 status expected (ignored when ok is 0)
// All proofs are split in one call and all queries verified in one call, from heap blocks of exactly their
// size, so a read past a record, a key or a value is a read past a block.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/plenum_verify.h"
#include "trie_host.h"

namespace {

typedef std::vector<uint8_t> Bytes;

struct Reader {
    Bytes data;
    size_t at = 0;
    void need(size_t n) {
        if (at + n > data.size()) {
            fprintf(stderr, "input truncated\n");
            exit(2);
        }
    }
    uint32_t u32() {
        uint32_t v;
        need(4);
        memcpy(&v, data.data() + at, 4);
        at += 4;
        return v;
    }
    uint8_t u8() {
        need(1);
        return data[at++];
    }
    Bytes bytes(size_t n) {
        need(n);
        Bytes b(data.begin() + at, data.begin() + at + n);
        at += n;
        return b;
    }
};

std::unique_ptr<uint8_t[]> exact(const Bytes& b) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[b.size() ? b.size() : 1]);
    if (b.size()) memcpy(p.get(), b.data(), b.size());
    return p;
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
    Bytes ser, roots, keys, vals, want_ok, want_status;
    std::vector<uint64_t> ser_off{0}, key_off{0}, val_off{0};
    for (uint32_t c = 0; c < cases; c++) {
        const Bytes s = r.bytes(r.u32()), root = r.bytes(32), k = r.bytes(r.u32()), v = r.bytes(r.u32());
        ser.insert(ser.end(), s.begin(), s.end());
        ser_off.push_back(ser.size());
        roots.insert(roots.end(), root.begin(), root.end());
        keys.insert(keys.end(), k.begin(), k.end());
        key_off.push_back(keys.size());
        vals.insert(vals.end(), v.begin(), v.end());
        val_off.push_back(vals.size());
        want_ok.push_back(r.u8());
        want_status.push_back(r.u8());
    }
    const auto ser_x = exact(ser), key_x = exact(keys), val_x = exact(vals);

    // too little room first: the count alone comes back
    std::vector<uint64_t> first(cases + 1), off1(1), len1(1);
    Bytes ok(cases + 1);
    uint64_t n_nodes = 0;
    int rc = pv_proof_split_host(ser_x.get(), ser_off.data(), cases, first.data(), off1.data(), len1.data(), 0, &n_nodes, ok.data());
    if (n_nodes && rc != PV_TRIE_NEED_SPACE) {
        fprintf(stderr, "split without room: rc %d\n", rc);
        return 1;
    }
    std::vector<uint64_t> node_off(n_nodes + 1), node_len(n_nodes ? n_nodes : 1);
    rc = pv_proof_split_host(ser_x.get(), ser_off.data(), cases, first.data(), node_off.data(), node_len.data(), n_nodes, &n_nodes,
                             ok.data());
    if (rc != PV_OK) {
        fprintf(stderr, "split: rc %d\n", rc);
        return 1;
    }
    std::vector<uint32_t> qp;
    Bytes q_root, q_want;
    std::vector<uint64_t> q_koff{0}, q_voff{0};
    Bytes q_keys, q_vals;
    for (uint32_t c = 0; c < cases; c++) {
        if (ok[c] != want_ok[c]) {
            fprintf(stderr, "case %u: split ok %u, expected %u\n", c, ok[c], want_ok[c]);
            return 1;
        }
        if (!ok[c] || first[c + 1] - first[c] > PV_PROOF_MAX_NODES) continue;
        qp.push_back(c);
        q_root.insert(q_root.end(), roots.begin() + 32 * c, roots.begin() + 32 * c + 32);
        q_keys.insert(q_keys.end(), keys.begin() + key_off[c], keys.begin() + key_off[c + 1]);
        q_koff.push_back(q_keys.size());
        q_vals.insert(q_vals.end(), vals.begin() + val_off[c], vals.begin() + val_off[c + 1]);
        q_voff.push_back(q_vals.size());
        q_want.push_back(want_status[c]);
    }
    const auto qk_x = exact(q_keys), qv_x = exact(q_vals), qr_x = exact(q_root);
    PvProofIn in;
    in.node_blob = ser_x.get();
    in.node_off = node_off.data();
    in.n_nodes = n_nodes;
    in.proof_first = first.data();
    in.n_proofs = cases;
    in.query_proof = qp.data();
    in.root = qr_x.get();
    in.key_blob = qk_x.get();
    in.key_off = q_koff.data();
    in.val_blob = qv_x.get();
    in.val_off = q_voff.data();
    in.n_queries = qp.size();
    in.node_len = node_len.data();
    const char* why = nullptr;
    if (in.n_queries && pv_proof_check_args(in, &why) != PV_OK) {
        fprintf(stderr, "arguments refused: %s\n", why);
        return 1;
    }
    Bytes status(qp.size() + 1, 0xEE);
    if (in.n_queries) pv_proof_host(in, status.data());
    for (size_t i = 0; i < qp.size(); i++)
        if (status[i] != q_want[i]) {
            fprintf(stderr, "case %u: status %u, expected %u\n", qp[i], status[i], q_want[i]);
            return 1;
        }
    // what the argument check refuses
    PvProofIn bad = in;
    bad.query_proof = nullptr;
    int refused = pv_proof_check_args(bad, &why) == PV_ERR_ARG;
    if (in.n_queries) {
        std::vector<uint32_t> far(qp);
        far[0] = cases;
        bad = in;
        bad.query_proof = far.data();
        refused += pv_proof_check_args(bad, &why) == PV_ERR_ARG;
        std::vector<uint64_t> down(q_koff);
        down[0] = down.back() + 1;
        bad = in;
        bad.key_off = down.data();
        refused += pv_proof_check_args(bad, &why) == PV_ERR_ARG;
        if (refused != 3) {
            fprintf(stderr, "an argument error went through\n");
            return 1;
        }
    }
    printf("ok %u cases %zu queries %llu nodes\n", cases, qp.size(), (unsigned long long)n_nodes);
    return 0;
}
